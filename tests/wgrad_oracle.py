"""Plain fp64 reference of the weight gradient of a tap-grid convolution (include/disprcnn_hip.h: drc_tapconv_wgrad), the case tables of
tests/test_hip_wgrad_edges.py, a CPU model of what csrc/wgrad.hip and csrc/wgrad_slide.hip pick for a shape, and the "plausible mistakes"
tests/test_wgrad_host.py uses to show that every case is strong enough for its bound.

    gw[ca][cb][t] = sum_{n,o} a_pad[n, ca, in_mul*o + first + t*step] * b[n, cb, o]        t = (td*nh + th)*nw + tw

`launch_model` takes no part in deciding whether a result is right.  It serves two things: asserting that the case tables reach the
branches they are listed for (if the dispatch moves a case off its branch the host test fails, and the fix is another shape), and the
depth of the error bound -- the dependent fp32 additions behind one element of gw.
"""
import functools

import numpy as np
import torch

from disprcnn_amd.utils.synth import hash_uniform

F64 = np.float64
EPS32 = 2.0 ** -24
SENT = 7.25
NAN = float("nan")
POISON = 4096.0                     # finite integer fill of a's slack and of the pool units behind a prefix view
SLACK_FLOATS = 1 << 16              # engine.SLACK_FLOATS (asserted equal in tests/test_wgrad_host.py)
SCRATCH_FLOATS = (1024 + 3 * 64) * 49 * 256      # DRC_WGRAD_SCRATCH_FLOATS


# ------------------------------------------------------------------------------------------------ reference
def reference(a_pad, b, cls, in_mul, weight=None, shift_tap=None):
    """(gw, mag, terms): gw [Ca][Cb][T] in fp64 from the padded dense a_pad [N, Ca, Dp, Hp, Wp] and b [N, Cb, OD, OH, OW]; mag the same sum
    over |a||b|; terms the number of products per element.
    weight [N, OD, OH, OW] (mistakes only): every position o counts that many times.  shift_tap (mistakes only): tap t reads one voxel
    further along w."""
    a_pad, b = np.asarray(a_pad, F64), np.asarray(b, F64)
    N, Cb, OD, OH, OW = b.shape
    (nd, nh, nw), first, step = cls["n"], cls["first"], cls["step"]
    if weight is not None:
        b = b * np.asarray(weight, F64)[:, None]
    T = nd * nh * nw
    gw = np.zeros((a_pad.shape[1], Cb, T), F64)
    mag = np.zeros_like(gw)
    bf, baf = b.transpose(1, 0, 2, 3, 4).reshape(Cb, -1), np.abs(b).transpose(1, 0, 2, 3, 4).reshape(Cb, -1)
    for td in range(nd):
        for th in range(nh):
            for tw in range(nw):
                t = (td * nh + th) * nw + tw
                d0, h0, w0 = first[0] + td * step[0], first[1] + th * step[1], first[2] + tw * step[2] + (1 if t == shift_tap else 0)
                d1, h1, w1 = d0 + in_mul * (OD - 1) + 1, h0 + in_mul * (OH - 1) + 1, w0 + in_mul * (OW - 1) + 1
                assert d1 <= a_pad.shape[2] and h1 <= a_pad.shape[3] and w1 <= a_pad.shape[4], "a tap leaves the padded tensor"
                win = a_pad[:, :, d0:d1:in_mul, h0:h1:in_mul, w0:w1:in_mul].transpose(1, 0, 2, 3, 4).reshape(a_pad.shape[1], -1)
                gw[:, :, t] = win @ bf.T
                mag[:, :, t] = np.abs(win) @ baf.T
    return gw, mag, np.full(gw.shape, N * OD * OH * OW, np.int64)


# ------------------------------------------------------------------------------------------------ cases
def _ceil(a, b):
    return -(-a // b)


def conv_case(name, N, Ca, Cb, dims, k, stride=1, pad=None, dil=1, halo=None, **extra):
    """Conv3d / Conv2d (dims[0] == 1 and k[0] == 1): a = the layer input with halo `halo` >= pad, b = the gradient of the output."""
    k = (k,) * 3 if isinstance(k, int) else tuple(k)
    pad = tuple(dil * (kk - 1) // 2 for kk in k) if pad is None else tuple(pad)
    halo = pad if halo is None else tuple(halo)
    assert all(h >= p for h, p in zip(halo, pad)), "input halo too small for this convolution"
    sd = 1 if k[0] == 1 and dims[0] == 1 else stride
    strides = (sd, stride, stride)
    out = tuple((d + 2 * p - dil * (kk - 1) - 1) // s + 1 for d, p, kk, s in zip(dims, pad, k, strides))
    cls = dict(n=k, first=tuple(h - p for h, p in zip(halo, pad)), step=(dil if k[0] > 1 else 1, dil, dil))
    return dict(name=name, N=N, Ca=Ca, Cb=Cb, a_dims=tuple(dims), a_halo=halo, b_dims=out, b_halo=(1 if dims[0] > 1 else 0, 1, 1), cls=cls,
                in_mul=stride, conv=dict(kind="conv", k=k, stride=strides, pad=pad, dil=(dil if k[0] > 1 else 1, dil, dil)), **extra)


def deconv_case(name, N, Cin, Cout, dims, **extra):
    """ConvTranspose3d k3 s2 p1 op1 on an input of `dims`: a = the gradient of the output (halo 1, in_mul = 2), b = the input"""
    cls = dict(n=(3, 3, 3), first=(0, 0, 0), step=(1, 1, 1))
    return dict(name=name, N=N, Ca=Cout, Cb=Cin, a_dims=tuple(2 * d for d in dims), a_halo=(1, 1, 1), b_dims=tuple(dims), b_halo=(1, 1, 1),
                cls=cls, in_mul=2, conv=dict(kind="deconv"), **extra)


def raw_case(name, N, Ca, Cb, a_dims, a_halo, b_dims, n, first, step, in_mul, **extra):
    """a tap class no layer of the project has: parameters built by the test"""
    return dict(name=name, N=N, Ca=Ca, Cb=Cb, a_dims=tuple(a_dims), a_halo=tuple(a_halo), b_dims=tuple(b_dims), b_halo=(1 if b_dims[0] > 1 else 0, 1, 1),
                cls=dict(n=tuple(n), first=tuple(first), step=tuple(step)), in_mul=in_mul, conv=None, **extra)


def _s(name, N, Ca, Cb, D, H, W):
    return conv_case(name, N, Ca, Cb, (D, H, W), 3)


# slide path: 3x3x3, in_mul = 1
SLIDE_CASES = [
    _s("S1", 1, 16, 16, 2, 1, 1),        # one slot, NK = 0, nk = 1; one unit over four waves: three idle waves
    _s("S2", 2, 16, 16, 2, 3, 5),        # 15 slots, the last k-step partly masked
    _s("S3", 2, 32, 32, 3, 7, 7),        # NK = 13: 49 slots
    _s("S4", 2, 32, 32, 4, 14, 14),      # NK = 14, R = 4, ragged last row tile
    _s("S5", 2, 32, 32, 5, 8, 8),        # NK = 16, two segments of 3, the last ragged
    _s("S6", 2, 32, 32, 7, 5, 33),       # OW > 32: WT = 17, ragged column tile, ragged row tile, three segments, ragged last
    _s("S7", 2, 32, 32, 9, 9, 30),       # NK = 0 with nk = 15 (odd), ragged rows, three segments
    _s("S8", 2, 32, 32, 13, 4, 16),      # four segments of 4, the last holds one slice
    _s("S9", 3, 64, 64, 7, 28, 28),      # 126 units over 64 waves: a wave walks more than one unit
    _s("S10", 2, 40, 24, 4, 9, 30),      # channel padding on both sides (three a blocks, two b blocks)
    _s("S11", 2, 32, 32, 1, 40, 56),     # D = 1: falls through to wgrad_kernel<9> with nd = 3
]

# generic path through wgrad() with the tile search
GENERIC_CASES = [
    conv_case("G1odd", 2, 32, 48, (5, 7, 9), 3, stride=2),
    conv_case("G1even", 2, 32, 32, (8, 12, 16), 3, stride=2),
    deconv_case("G2a", 2, 32, 48, (3, 6, 8)),
    deconv_case("G2b", 2, 48, 32, (2, 5, 7)),
    conv_case("G3dil2", 2, 32, 32, (1, 9, 13), (1, 3, 3), dil=2),
    conv_case("G3dil4", 2, 32, 32, (1, 3, 13), (1, 3, 3), dil=4),            # 3 rows: smaller than the dilation span of 9
    conv_case("G3dil4b", 2, 32, 32, (1, 9, 13), (1, 3, 3), dil=4),
    conv_case("G3s2", 2, 32, 64, (1, 11, 15), (1, 3, 3), stride=2),
    conv_case("G3k1", 2, 64, 32, (1, 10, 14), (1, 1, 1), halo=(0, 1, 1)),
    conv_case("G3k1h0", 2, 64, 32, (1, 10, 14), (1, 1, 1), halo=(0, 0, 0)),
    conv_case("G3k1s2", 2, 32, 64, (1, 9, 13), (1, 1, 1), stride=2, halo=(0, 1, 1)),
    conv_case("G4", 3, 256, 256, (1, 14, 14), (1, 3, 3), units=6),           # the mask head's form, a = a prefix view of 6 units
    conv_case("G5", 2, 32, 32, (1, 17, 35), (1, 3, 3)),                      # the search itself picks a ragged column tile
]

# generic path with forced tiles
FORCED_CASES = [
    conv_case("G6", 2, 32, 32, (1, 11, 13), (1, 3, 3), R=4, WT=5),                       # ragged rows and columns together
    conv_case("G6s2", 2, 32, 32, (5, 7, 9), 3, stride=2, R=3, WT=2),
    conv_case("G7nm1a", 2, 16, 16, (1, 3, 5), (1, 3, 3), R=1, WT=1),                     # R*WT = 1: nm = 1
    conv_case("G7nm1b", 2, 16, 16, (1, 5, 7), (1, 3, 3), R=2, WT=2),                     # 4: nm = 1, full step
    conv_case("G7nm2", 2, 16, 16, (1, 3, 11), (1, 3, 3), R=1, WT=5),                     # 5: nm = 2, the "two steps left" epilogue at m = 0
    conv_case("G7nm2b", 1, 16, 16, (1, 5, 9), (1, 3, 3), R=2, WT=4),                     # 8: nm = 2; 6 groups: idle waves
    conv_case("G7nm3", 2, 16, 16, (1, 7, 4), (1, 3, 3), R=3, WT=3),                      # 9: nm = 3, loop once, one step left
    conv_case("G7nm4", 2, 16, 16, (1, 7, 9), (1, 3, 3), R=3, WT=5),                      # 15: nm = 4, loop once, two steps left
    conv_case("G4r", 3, 32, 32, (1, 14, 14), (1, 3, 3), R=4, WT=5, units=6),             # ragged tiles of a prefix view: the over-read meets the pool
    conv_case("G7k1", 2, 16, 32, (1, 5, 7), (1, 1, 1), halo=(0, 0, 0), R=2, WT=3),       # NT = 1, ragged, a without any halo
]
G8 = conv_case("G8", 2, 128, 128, (4, 7, 9), 3, stride=2, R=3, WT=2)                     # jobs = 192, 24 groups: the scratch step-down
G9 = conv_case("G9", 2, 32, 32, (3, 5, 7), 3, stride=2, R=2, WT=3)                       # overwrite = 0 on both flushes
G9S = _s("G9S", 2, 32, 32, 4, 5, 9)                                                      # and on the slide kernel

# instantiations no Python caller reaches
RAW_CASES = [
    raw_case("NT2", 2, 32, 32, (4, 6, 10), (1, 1, 1), (2, 3, 5), (1, 1, 2), (1, 1, 1), (1, 1, 1), 2),
    raw_case("NT4", 2, 32, 32, (6, 10, 14), (1, 1, 1), (3, 5, 7), (2, 2, 2), (1, 1, 1), (1, 1, 1), 2),
    raw_case("NT49", 2, 16, 32, (1, 14, 18), (0, 3, 3), (1, 7, 9), (1, 7, 7), (0, 0, 0), (1, 1, 1), 2),     # a stem-like 7x7 stride 2
]

ALL_CASES = SLIDE_CASES + GENERIC_CASES + FORCED_CASES + [G8, G9, G9S] + RAW_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def geometry(case, what):
    """the engine.Blocked strides of a case's `a` or `b` (floats)"""
    N = case["N"]
    C = case["Ca" if what == "a" else "Cb"]
    (D, H, W), (pd, ph, pw) = case[what + "_dims"], case[what + "_halo"]
    cb = _ceil(C, 16)
    h = (W + 2 * pw) * 16
    d = (H + 2 * ph) * h
    c = (D + 2 * pd) * d
    return dict(N=N, cb=cb, h_stride=h, d_stride=d, cb_stride=c, n_stride=cb * c, numel=N * cb * c, interior_off=pd * d + ph * h + pw * 16)


@functools.lru_cache(maxsize=4)
def data(name, kind):
    """the inputs and the reference of a case; kind "int": integers in -3..3, "real": uniform(-1, 1).  Never modified by a test."""
    c = BY_NAME[name]
    lo, hi = (-3.49, 3.49) if kind == "int" else (-1.0, 1.0)
    a = hash_uniform(f"wg:{name}:a", (c["N"], c["Ca"]) + c["a_dims"], lo, hi)
    b = hash_uniform(f"wg:{name}:b", (c["N"], c["Cb"]) + c["b_dims"], lo, hi)
    if kind == "int":
        a, b = torch.round(a), torch.round(b)
    a, b = a.numpy(), b.numpy()
    gw, mag, terms = reference(pad_a(c, a), b, c["cls"], c["in_mul"])
    for v in (a, b, gw, mag, terms):
        v.setflags(write=False)
    return dict(a=a, b=b, gw=gw, mag=mag, terms=terms)


def pad_a(case, a):
    pd, ph, pw = case["a_halo"]
    return np.pad(np.asarray(a, F64), ((0, 0), (0, 0), (pd, pd), (ph, ph), (pw, pw)))


def pad_gw(case, x):
    """[Ca, Cb, T] of the true channels -> the kernel's [cbA*16][cbB*16][T]: the padded channel rows are zero"""
    out = np.zeros((_ceil(case["Ca"], 16) * 16, _ceil(case["Cb"], 16) * 16, x.shape[2]), x.dtype)
    out[: case["Ca"], : case["Cb"]] = x
    return out


# ------------------------------------------------------------------------------------------------ launch model
def tile_search(H, W, in_mul, span_h, span_w):
    from disprcnn_amd.modeling.psmnet import train as T
    return T.wgrad_tile_search(H, W, in_mul, span_h, span_w)


def launch_model(N, cb_a, cb_b, out_dims, cls, in_mul, ga, gb, R=None, WT=None, scratch_floats=SCRATCH_FLOATS, a_off=0):
    """What drc_tapconv_wgrad does with a shape.  ga, gb: stride records (geometry()); R, WT: the forced tile; a_off: the float offset of
    p.a in its storage (a channel-block slice).  Returns a dict: path ("slide" / "generic"), R, WT, NK / nk / nseg / seglen or NT / nm,
    groups or units, grid, waves (what the reduce is told), workers (generic: before rounding to blocks), per_simd, partial, per_wave (the
    most work items one wave walks), idle (waves with no work), depth (dependent additions behind one element incl. the product),
    a_max / b_max (largest float offset read, + 1)."""
    OD, OH, OW = out_dims
    (nd, nh, nw), first, step = cls["n"], cls["first"], cls["step"]
    m = _slide_model(N, cb_a, cb_b, OD, OH, OW, cls, in_mul, ga, gb, scratch_floats)
    if m is not None:
        m["a_max"] += a_off
        return m
    span_h, span_w = (nh - 1) * step[1], (nw - 1) * step[2]
    if R is None:
        R, WT, need = tile_search(OH, OW, in_mul, span_h, span_w)
    NT = nh * nw
    assert NT in (1, 2, 4, 9, 49) and 0 < R * WT <= 112
    n_rt, n_wt = _ceil(OH, R), _ceil(OW, WT)
    groups = N * OD * n_rt * n_wt
    jobs = nd * cb_a * cb_b
    for per_simd in (3, 2, 1):
        workers = max(min(per_simd * 1024 // jobs, groups), 1)
        if per_simd == 1 or scratch_floats >= _ceil(workers, 4) * 4 * jobs * NT * 256:
            break
    grid = _ceil(workers, 4)
    waves = grid * 4
    partial = scratch_floats >= waves * jobs * NT * 256
    nm = _ceil(R * WT, 4)
    per_wave = _ceil(groups, waves)
    rows_in, seg_vox = in_mul * (R - 1) + span_h + 1, in_mul * (WT - 1) + span_w + 1
    oh0, ow0 = (n_rt - 1) * R, (n_wt - 1) * WT
    a_max = (a_off + (N - 1) * ga["n_stride"] + (cb_a - 1) * ga["cb_stride"] + (in_mul * (OD - 1) + first[0] + (nd - 1) * step[0]) * ga["d_stride"] +
             (in_mul * oh0 + first[1] + rows_in - 1) * ga["h_stride"] + (in_mul * ow0 + first[2] + seg_vox) * 16)
    b_max = (gb["interior_off"] + (N - 1) * gb["n_stride"] + (cb_b - 1) * gb["cb_stride"] + (OD - 1) * gb["d_stride"] +
             (oh0 + R - 1) * gb["h_stride"] + (ow0 + WT) * 16)
    depth = 4 * nm * per_wave + 1
    depth += (_ceil(waves, 4) + 3) if partial else waves
    return dict(path="generic", R=R, WT=WT, NT=NT, nm=nm, n_rt=n_rt, n_wt=n_wt, groups=groups, jobs=jobs, workers=workers, per_simd=per_simd,
                grid=grid, waves=waves, partial=partial, per_wave=per_wave, idle=max(waves - groups, 0), depth=depth, a_max=a_max, b_max=b_max,
                ragged_rows=OH % R != 0, ragged_cols=OW % WT != 0,
                need=[_ceil(max(min(k * 1024 // jobs, groups), 1), 4) * 4 * jobs * NT * 256 for k in (3, 2, 1)])


def _slide_model(N, cb_a, cb_b, OD, OH, OW, cls, in_mul, ga, gb, scratch_floats):
    if in_mul != 1 or tuple(cls["n"]) != (3, 3, 3) or tuple(cls["step"]) != (1, 1, 1) or OD < 2:
        return None
    parts = _ceil(OW, 32)
    WT = _ceil(OW, parts)
    R = min(64 // WT, OH)
    if R < 1:
        return None
    while R > 1 and OH % R and _ceil(OH, R) * R - OH > R // 2:
        R -= 1
    pieces_a, pieces_b = _ceil((R + 2) * (WT + 2) * 4, 64), _ceil(R * WT * 4, 64)
    if pieces_a > 10 or pieces_b > 6 or R * WT > 64 or 4 * (3 * pieces_a + 2 * pieces_b) * 1024 > 160 * 1024:
        return None
    n_rt, n_wt = _ceil(OH, R), _ceil(OW, WT)
    cols = N * n_rt * n_wt
    jobs = cb_a * cb_b
    workers = max(min(1024 // jobs, cols * 4), 1)
    grid = _ceil(workers, 4)
    waves = grid * 4
    partial = scratch_floats >= waves * jobs * 27 * 256
    nseg, seglen, best = 1, OD, 1e30
    for s in range(1, 5):
        ln = _ceil(OD, s)
        if s > 1 and ln < 3:
            break
        ns = _ceil(OD, ln)
        cost = _ceil(cols * ns, waves) * (ln + 0.75)
        if cost < best - 1e-9:
            best, nseg, seglen = cost, ns, ln
    nk = _ceil(R * WT, 4)
    units = cols * nseg
    per_wave = _ceil(units, waves)
    first = cls["first"]
    oh0, ow0 = (n_rt - 1) * R, (n_wt - 1) * WT
    nr, nc = min(OH - oh0, R), min(OW - ow0, WT)
    a_max = ((N - 1) * ga["n_stride"] + (cb_a - 1) * ga["cb_stride"] + (first[0] + OD + 1) * ga["d_stride"] +
             (oh0 + first[1] + nr + 1) * ga["h_stride"] + (ow0 + first[2] + nc + 1) * 16 + 16)
    b_max = (gb["interior_off"] + (N - 1) * gb["n_stride"] + (cb_b - 1) * gb["cb_stride"] + (OD - 1) * gb["d_stride"] +
             (oh0 + nr - 1) * gb["h_stride"] + (ow0 + nc - 1) * 16 + 16)
    depth = 4 * nk * seglen * per_wave + 1
    depth += (_ceil(waves, 4) + 3) if partial else waves
    return dict(path="slide", R=R, WT=WT, NT=27, NK=nk if nk in (13, 14, 16) else 0, nk=nk, n_rt=n_rt, n_wt=n_wt, nseg=nseg, seglen=seglen,
                last_seg=OD - (nseg - 1) * seglen, cols=cols, units=units, jobs=jobs, workers=workers, per_simd=1, grid=grid, waves=waves,
                partial=partial, per_wave=per_wave, idle=max(waves - units, 0), depth=depth, a_max=a_max, b_max=b_max,
                ragged_rows=OH % R != 0, ragged_cols=OW % WT != 0, need=[waves * jobs * 27 * 256])


def model_of(case, scratch_floats=SCRATCH_FLOATS):
    return launch_model(case["N"], _ceil(case["Ca"], 16), _ceil(case["Cb"], 16), case["b_dims"], case["cls"], case["in_mul"], geometry(case, "a"),
                        geometry(case, "b"), case.get("R"), case.get("WT"), scratch_floats)


def bound(case, model, mag, terms, extra=0):
    """depth * eps * mag + 1e-30 per element.  The atomicAdd flush adds in any order: the number of terms, if that is smaller."""
    depth = model["depth"] + extra
    if not model["partial"]:
        depth = np.minimum(depth, terms + extra)
    return depth * EPS32 * mag + 1e-30


# ------------------------------------------------------------------------------------------------ plausible mistakes
def position_worker(case, model):
    """[N, OD, OH, OW]: the wave that handles each position of b (all jobs share the map)"""
    N, (OD, OH, OW) = case["N"], case["b_dims"]
    n, od, oh, ow = np.meshgrid(np.arange(N), np.arange(OD), np.arange(OH), np.arange(OW), indexing="ij")
    rt, wt = oh // model["R"], ow // model["WT"]
    if model["path"] == "slide":
        col = (n * model["n_rt"] + rt) * model["n_wt"] + wt
        return (col * model["nseg"] + od // model["seglen"]) % model["waves"]
    return (((n * OD + od) * model["n_rt"] + rt) * model["n_wt"] + wt) % model["waves"]


def mistakes(case, model):
    """{name: keyword arguments of reference()} of the mistakes that apply to this case under this launch"""
    N, (OD, OH, OW) = case["N"], case["b_dims"]
    one = np.ones((N, OD, OH, OW))
    out = {}
    if model["ragged_rows"]:
        w = one.copy(); w[:, :, OH - 1] = 0
        out["drop the last row of the ragged tile"] = dict(weight=w)
    if model["ragged_cols"]:
        w = one.copy(); w[:, :, :, OW - 1] = 0
        out["drop the last column of the ragged tile"] = dict(weight=w)
    if model["path"] == "slide":
        w = one.copy(); w[:, OD - 1] = 0
        out["drop the last depth slice of the last segment"] = dict(weight=w)
        if model["nseg"] > 1:
            w = one.copy(); w[:, model["seglen"] - 1] = 0
            out["drop the last depth slice of the first segment"] = dict(weight=w)
    nw = case["cls"]["n"][2]
    mid = int(np.prod(case["cls"]["n"])) // 2                       # the centre tap: it reads the interior at every size
    w_last = case["cls"]["first"][2] + (mid % nw) * case["cls"]["step"][2] + case["in_mul"] * (OW - 1) + 1
    if w_last < case["a_dims"][2] + 2 * case["a_halo"][2]:          # room for it in the padded row
        out["shift the centre tap by one voxel"] = dict(shift_tap=mid)
    if model["partial"]:
        pos = position_worker(case, model)
        busy = int(pos.max())
        out["count one worker's partial twice"] = dict(weight=one + (pos == busy // 2))
        out["skip the last worker"] = dict(weight=one - (pos == busy))
    return out


# ------------------------------------------------------------------------------------------------ Config A / Config B layer geometries
def psmnet_layers():
    """[(label, case)]: every weight-gradient launch of one train step of Config A (112 x 112 ROI crops, disparities 0..48) and Config B
    (224 x 224 crops, -48..48), from modeling/psmnet/schedule.py"""
    from disprcnn_amd.modeling.psmnet.schedule import REGRESSOR_SITES, trunk_sites
    out = []
    for cfg, (D, H, W), (IH, IW) in (("A", (12, 28, 28), (112, 112)), ("B", (24, 56, 56), (224, 224))):
        for N in (1, 3):
            for s in REGRESSOR_SITES:
                dims = tuple(v >> s.level for v in (D, H, W))
                if s.kind == "up":
                    c = deconv_case(s.plan, N, s.cin, s.cout, dims)
                else:
                    c = conv_case(s.plan, N, s.cin, s.cout, dims, 3, stride=2 if s.kind == "s2" else 1)
                out.append((f"{cfg} N={N} {s.plan}", c))
            trunk = trunk_sites()
            halo = {"img": 1}
            for s in trunk.stem + trunk.blocks:
                halo[s.y] = 1 if s.y in (trunk.raw, trunk.skip) else s.halo                # the concat's slices carry the concat's halo
            for s in trunk.stem + trunk.blocks:
                oh, ow = IH >> s.level, IW >> s.level
                c = conv_case(s.wname, N, s.cin, s.cout, (1, oh * s.stride, ow * s.stride), (1, s.k, s.k), stride=s.stride, pad=(0, s.pad, s.pad),
                              dil=s.dilation, halo=(0, halo[s.x], halo[s.x]))
                c["b_halo"] = (0, 2, 2)                                                   # train.py: the 2D draw tensors
                c["a_cb_total"] = 20 if s.x == trunk.raw else None                        # a slice of the 320-channel concat
                out.append((f"{cfg} N={N} {s.wname}", c))
            H4, W4 = IH // 4, IW // 4
            for k in (64, 32, 16, 8):
                if H4 // k:
                    c = conv_case(f"branch{k}", N, 128, 32, (1, H4 // k, W4 // k), (1, 1, 1), halo=(0, 0, 0))
                    c["b_halo"] = (0, 2, 2)
                    out.append((f"{cfg} N={N} fe.branch pool {k}", c))
            c = conv_case("lastconv.0", N, 320, 128, (1, H4, W4), (1, 3, 3))
            c["b_halo"] = (0, 2, 2)
            out.append((f"{cfg} N={N} fe.lastconv.0", c))
            c = conv_case("lastconv.2", N, 128, 32, (1, H4, W4), (1, 1, 1), halo=(0, 0, 0))
            c["b_halo"] = (0, 2, 2)
            out.append((f"{cfg} N={N} fe.lastconv.2", c))
    return out


def model_of_layer(case):
    """launch_model of a psmnet_layers() entry; an `a` that is a slice of the concat keeps the concat's strides"""
    ga, gb = geometry(case, "a"), geometry(case, "b")
    cb_a = _ceil(case["Ca"], 16)
    if case.get("a_cb_total"):
        ga = dict(ga, n_stride=case["a_cb_total"] * ga["cb_stride"], numel=case["N"] * case["a_cb_total"] * ga["cb_stride"])
    return launch_model(case["N"], cb_a, _ceil(case["Cb"], 16), case["b_dims"], case["cls"], case["in_mul"], ga, gb), ga, gb

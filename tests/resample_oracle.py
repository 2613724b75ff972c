"""Plain fp64 references (numpy) of the train step's adjoint kernels and of the pool / resample kernels of the 2D stage, the inputs and
geometries of their GPU tests (tests/test_hip_train_adjoints.py, tests/test_hip_resample.py), mirrors of the launchers' grid arithmetic
and the "plausible mistakes" tests/test_resample_oracle.py uses to show that every case's input is strong enough for its bound.

Every reference returns, next to its value, the element-wise MAGNITUDE sum (the same sum with every term replaced by its absolute
value): the derived bounds are multiples of 2^-24 of it.

  cout1_bwd_data / cout1_bwd_weight   adjoints of Conv3d(C -> 1, k3, p1, no bias): dx[n,c,u] = sum_t w[t,c] gy[n,u-t+1],
                                      gw[t,c] = sum_{n,v} x[n,c,v+t-1] gy[n,v]            (t = (kd*3 + kh)*3 + kw, w as [27][C])
  cost_volume_fwd / _bwd              the concat-shift volume of stackhourglass.py:115-128 and its adjoint with (lo4, hi4, Dp) free
  avgpool / avgpool_bwd               AvgPool2d(k, k), floor mode
  bilinear / bilinear_bwd             both align_corners settings; source coordinates in numpy float32 with the expressions ATen and
                                      the kernels use, blend in fp64
  maxpool                             max_pool2d(k, s, pad 0, ceil_mode): windows clipped (exact)
"""
import functools
import zlib

import numpy as np
import torch

F64 = np.float64
EPS32 = 2.0 ** -24
SENT = 7.25
NAN = float("nan")
TAPS = [(kd, kh, kw) for kd in range(3) for kh in range(3) for kw in range(3)]


def uniform(tag, shape, lo=-1.0, hi=1.0):
    """Deterministic uniform [lo, hi) float32 array addressed by `tag` (PCG64: fast enough for the 34 M element case)."""
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return (np.float32(lo) + np.float32(hi - lo) * rng.random(shape, dtype=np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ classifier conv adjoints
def cout1_bwd_data(w, gy, flip=True):
    """w [27, C], gy [N, D, H, W] -> dx [N, C, D, H, W], sum_t |w||gy|.  flip=False is the mistake "taps not flipped" (u + t - 1)."""
    w, gy = np.asarray(w, F64), np.asarray(gy, F64)
    N, D, H, W = gy.shape
    C = w.shape[1]
    gp = np.pad(gy, ((0, 0), (1, 1), (1, 1), (1, 1)))
    cols = np.empty((27, N, D, H, W))                                                 # cols[t] = gy[u - t + 1], zero outside
    for t, (kd, kh, kw) in enumerate(TAPS):
        a, b, c = (kd, kh, kw) if flip else (2 - kd, 2 - kh, 2 - kw)
        cols[t] = gp[:, 2 - a:2 - a + D, 2 - b:2 - b + H, 2 - c:2 - c + W]
    cols = cols.reshape(27, -1)
    dx, mag = w.T @ cols, np.abs(w).T @ np.abs(cols)
    return [a.reshape(C, N, D, H, W).transpose(1, 0, 2, 3, 4) for a in (dx, mag)]


def cout1_bwd_weight(x, gy):
    """x [N, C, D, H, W], gy [N, D, H, W] -> gw [27, C], sum |x||gy|: 27 shifted dot products in fp64, one sample at a time (the three kw
    of a (kd, kh) pair share one product with gy laid out at its three column shifts)."""
    N, C, D, H, W = x.shape
    gw, mag = np.zeros((27, C)), np.zeros((27, C))
    positive = bool((np.asarray(x) >= 0).all() and (np.asarray(gy) >= 0).all())
    for n in range(N):
        xp = np.pad(np.asarray(x[n], F64), ((0, 0), (1, 1), (1, 1), (1, 1)))
        g3 = np.zeros((D, H, W + 2, 3))
        for kw in range(3):
            g3[:, :, kw:kw + W, kw] = gy[n]
        g3 = g3.reshape(-1, 3)
        for kd in range(3):
            for kh in range(3):
                slab = np.ascontiguousarray(xp[:, kd:kd + D, kh:kh + H, :]).reshape(C, -1)
                t0 = (kd * 3 + kh) * 3
                gw[t0:t0 + 3] += (slab @ g3).T
                if not positive:
                    mag[t0:t0 + 3] += (np.abs(slab) @ np.abs(g3)).T
    return gw, (gw.copy() if positive else mag)


def pack_cout1(w, cb_in):
    """w [27, C] -> the header's [27][cb_in][16] (channels past C are zero), by hand."""
    out = np.zeros((27, cb_in, 16), np.float32)
    for t in range(27):
        for c in range(w.shape[1]):
            out[t, c // 16, c % 16] = w[t, c]
    return out


def cout1_data_grid(N, cb_in, D, H, W):
    """(blocks, wraps) of drc_conv3d_cout1_bwd_data: 256 threads, one per (voxel, channel quad), at most 8192 blocks."""
    total = N * cb_in * D * H * W * 4
    blocks = min(max((total + 255) // 256, 1), 8192)
    return blocks, total > blocks * 256


def cout1_weight_grid(N, D, H, W):
    """(blocks, trips per thread, trips of the finish kernel's lane loop, depth of dependent fp32 additions) of drc_conv3d_cout1_bwd_weight:
    1024 voxels per block up to 1024 blocks; a block takes 64 voxels per trip; four xor-shuffle levels over the 16 voxel slots of a wave,
    four waves added from LDS; the finish wave takes blocks lane, lane + 64, ... and six shuffle levels."""
    nvox = N * D * H * W
    blocks = min((nvox + 1023) // 1024, 1024)
    trips = -(-nvox // (blocks * 64))
    finish = -(-blocks // 64)
    return blocks, trips, finish, trips + 4 + 4 + finish + 6


# (name, n, (D, H, W)) -- the last one has more than 8192 x 256 work items at cb_in = 2: the grid-stride loop wraps
DATA_SHAPES = [("1x1x1", 1, (1, 1, 1)), ("1x3x112", 1, (1, 3, 112)), ("3x30x7", 2, (3, 30, 7)), ("5x9x13", 2, (5, 9, 13)),
               ("12x28x28", 3, (12, 28, 28)), ("24x56x56", 4, (24, 56, 56))]
DATA_CASES = [(name, n, dims, cb) for name, n, dims in DATA_SHAPES for cb in ((1, 2, 3) if n * dims[0] * dims[1] * dims[2] < 5000 else (2,))]
CB_CHANNELS = {1: 16, 2: 32, 3: 40}                     # cb_in = 3 with a ragged last block


@functools.lru_cache(maxsize=2)
def data_case(name, cb_in):
    """inputs and the reference of one cout1_bwd_data case: w [27, C], gy, old (the values accumulate=1 adds onto), dx, mag"""
    _, n, dims = next(s for s in DATA_SHAPES if s[0] == name)
    C = CB_CHANNELS[cb_in]
    w = uniform(f"d:{name}:{cb_in}:w", (27, C))
    gy = uniform(f"d:{name}:{cb_in}:g", (n,) + dims)
    dx, mag = cout1_bwd_data(w, gy)
    return {"n": n, "dims": dims, "C": C, "w": w, "gy": gy, "dx": dx, "mag": mag}


def data_old(name, cb_in, shape):
    return uniform(f"d:{name}:{cb_in}:old", shape)


# (name, N, (D, H, W), blocks the case is meant to reach)
WEIGHT_CASES = [("5", 1, (1, 1, 5), 1), ("1024", 1, (4, 16, 16), 1), ("1025", 1, (1, 25, 41), 2), ("65k+3", 7, (1, 37, 257), 66),
                ("cap", 28, (12, 56, 56), 1024)]


@functools.lru_cache(maxsize=1)
def weight_case(name, C=32):
    """x [N, C, D, H, W] in [0.25, 1.25) and gy in [0.25, 1.25) scaled by a ramp along w (positive means: no sum cancels; the ramp
    makes the 27 taps differ by more than the boundary terms), gw, mag."""
    _, n, dims, _ = next(c for c in WEIGHT_CASES if c[0] == name)
    x = uniform(f"w:{name}:{C}:x", (n, C) + dims, 0.25, 1.25)
    x *= (1.0 + np.arange(dims[2], dtype=np.float32) / np.float32(dims[2]))
    gy = uniform(f"w:{name}:{C}:g", (n,) + dims, 0.25, 1.25)
    gw, mag = cout1_bwd_weight(x, gy)
    return {"n": n, "dims": dims, "x": x, "gy": gy, "gw": gw, "mag": mag}


# ------------------------------------------------------------------------------------------------ cost volume
def cost_volume_fwd(L, R, lo4, hi4, Dp):
    L, R = np.asarray(L), np.asarray(R)
    N, C, H, W = L.shape
    out = np.zeros((N, 2 * C, Dp, H, W), L.dtype)
    xs = np.arange(W)
    for j in range(Dp):
        i = lo4 + j
        if i >= hi4:
            break
        ok = (xs - i >= 0) & (xs - i < W)
        out[:, :C, j][..., ok] = L[..., ok]
        out[:, C:, j][..., ok] = R[..., (xs - i)[ok]]
    return out


def cost_volume_bwd(g, lo4, hi4, Dp, dead=False, swap=False, shift=0):
    """g [N, 2C, Dp', H, W] (Dp' >= Dp) -> gL, gR [N, C, H, W] and sum_j |g_j| of each.
    Mistakes: dead = slices with lo4 + j >= hi4 summed too, swap = the two halves of the channels exchanged, shift = disparity off by one."""
    g = np.asarray(g, F64)
    N, C2, _, H, W = g.shape
    C = C2 // 2
    gl, gr = (g[:, C:], g[:, :C]) if swap else (g[:, :C], g[:, C:])
    out = [np.zeros((N, C, H, W)) for _ in range(4)]
    xs = np.arange(W)
    for j in range(Dp):
        i = lo4 + j
        if i >= hi4 and not dead:
            break
        i += shift
        ok = (xs - i >= 0) & (xs - i < W)
        out[0][..., ok] += gl[:, :, j][..., ok]
        out[2][..., ok] += np.abs(gl[:, :, j][..., ok])
        out[1][..., (xs - i)[ok]] += gr[:, :, j][..., ok]
        out[3][..., (xs - i)[ok]] += np.abs(gr[:, :, j][..., ok])
    return tuple(out)


CV_RANGES = [(48, 0), (48, -48), (24, -24), (0, -48), (16, 8)]
CV_SHAPES = [(2, 32, 5, 13), (1, 3, 2, 7), (2, 4, 6, 20)]


def cv_args(mx, mn):
    """(lo4, hi4, Dp) as ops.cost_volume_backward passes them"""
    return mn // 4, mx // 4, (mx - mn) // 4


def cv_grad(mx, mn, shape, Dp, positive=False):
    N, C, H, W = shape
    return uniform(f"cv:{mx}:{mn}:{shape}:{Dp}", (N, 2 * C, Dp, H, W), 0.25 if positive else -1.0, 1.25 if positive else 1.0)


# ------------------------------------------------------------------------------------------------ AvgPool2d(k, k)
def avgpool(x, k, remainder=False, scale=True):
    """x [..., H, W] -> (mean over k x k windows, floor mode; sum |x| / k^2).  Mistakes: remainder = the last window of each axis also
    takes the remainder rows / columns, scale=False = 1 / k^2 missing."""
    x = np.asarray(x, F64)
    H, W = x.shape[-2:]
    OH, OW = H // k, W // k
    y, mag = np.zeros(x.shape[:-2] + (OH, OW)), np.zeros(x.shape[:-2] + (OH, OW))
    for oy in range(OH):
        y1 = H if remainder and oy == OH - 1 else (oy + 1) * k
        for ox in range(OW):
            x1 = W if remainder and ox == OW - 1 else (ox + 1) * k
            win = x[..., oy * k:y1, ox * k:x1]
            y[..., oy, ox] = win.sum((-2, -1))
            mag[..., oy, ox] = np.abs(win).sum((-2, -1))
    inv = 1.0 / (k * k) if scale else 1.0
    return y * inv, mag * inv


def avgpool_bwd(g, k, H, W, remainder=False, scale=True):
    """g [..., OH, OW] -> gx [..., H, W]: g / k^2 inside the pooled region, 0 on the remainder rows and columns"""
    g = np.asarray(g, F64)
    OH, OW = g.shape[-2:]
    gx = np.zeros(g.shape[:-2] + (H, W))
    ys, xs = np.arange(H) // k, np.arange(W) // k
    if remainder:
        ys, xs = np.minimum(ys, OH - 1), np.minimum(xs, OW - 1)
    oky, okx = ys < OH, xs < OW
    sub = g[..., ys[oky], :][..., xs[okx]]
    gx[..., :oky.sum(), :okx.sum()] = sub * (1.0 / (k * k) if scale else 1.0)
    return gx


def pool_input(tag, shape):
    """positive, growing 2 % per row and per column: a window moved by one column or a pooled remainder changes a mean by percents"""
    H, W = shape[-2:]
    ramp = np.float32(1.02) ** np.arange(H, dtype=np.float32)[:, None] * np.float32(1.02) ** np.arange(W, dtype=np.float32)[None, :]
    return (uniform(tag, shape, 0.5, 1.0) * ramp).astype(np.float32)


AVG_K = [1, 2, 8, 64]
AVG_HW = [(9, 7), (56, 72), (64, 64), (66, 130)]
AVG_CASES = [(k, hw) for k in AVG_K for hw in AVG_HW if hw[0] // k >= 1 and hw[1] // k >= 1]
AVG_BWD_CASES = [((9, 7), 2), ((9, 7), 4), ((8, 8), 8)]


def avgpool_bound(k, mag):
    """(k^2/16 + 8) 2^-24 sum|x|/k^2: a lane adds k^2/16 window positions in sequence, then four shuffle levels, the product with 1/k^2
    and the rounding of 1/k^2 itself (<= 6 more roundings; 8 taken)"""
    return (k * k / 16 + 8) * EPS32 * mag


# ------------------------------------------------------------------------------------------------ bilinear
def bilinear_axis(I, O, align):
    """(i0, i1, w0, w1) per output index, in float32 exactly as the kernels (and ATen) compute them"""
    o = np.arange(O, dtype=np.float32)
    if align:
        s = np.float32(I - 1) / np.float32(O - 1) if O > 1 else np.float32(0)
        f = s * o
    else:
        s = np.float32(I) / np.float32(O)
        f = np.maximum(s * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    assert f.dtype == np.float32
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < I - 1)
    t = f - i0.astype(np.float32)
    return i0, i1, np.float32(1) - t, t


def bilinear_matrix(I, O, align):
    """A [O, I] in fp64 (the float32 weights, exactly) and the 0/1 matrix of its non-zero entries"""
    i0, i1, w0, w1 = bilinear_axis(I, O, align)
    A = np.zeros((O, I))
    np.add.at(A, (np.arange(O), i0), w0.astype(F64))
    np.add.at(A, (np.arange(O), i1), w1.astype(F64))
    return A, (A != 0).astype(F64)


def bilinear(x, OH, OW, align):
    """x [..., IH, IW] -> y [..., OH, OW], sum w_i |v_i|"""
    x = np.asarray(x, F64)
    Ay, Ax = bilinear_matrix(x.shape[-2], OH, align)[0], bilinear_matrix(x.shape[-1], OW, align)[0]
    return Ay @ x @ Ax.T, Ay @ np.abs(x) @ Ax.T


def bilinear_bwd(g, IH, IW, align):
    """g [..., OH, OW] -> gx [..., IH, IW], sum w |g|, number of fine pixels that reach each coarse cell [IH, IW]"""
    g = np.asarray(g, F64)
    (Ay, Ny), (Ax, Nx) = bilinear_matrix(IH, g.shape[-2], align), bilinear_matrix(IW, g.shape[-1], align)
    return Ay.T @ g @ Ax, Ay.T @ np.abs(g) @ Ax, Ny.sum(0)[:, None] * Nx.sum(0)[None, :]


def up_bwd_takes_gather(IH, IW, OH, OW, cells):
    """drc_bilinear_up_blocked_bwd's branch: a block per coarse cell when the map grows at least four-fold"""
    return OH * OW >= 4 * IH * IW and cells < (1 << 31)


def up_bwd_gather_depth(IH, IW, OH, OW):
    """[IH, IW] depth of dependent fp32 additions of bilinear_up_bwd_gather_kernel per cell: 64 pixel slots walk the cell's conservative
    window of fine pixels (the kernel's own float32 bounds), four shuffle levels, three additions of the waves' sums from LDS."""
    one = np.float32(1)

    def span(I, O):
        s = np.float32(I - 1) / np.float32(O - 1) if O > 1 else np.float32(0)
        lo, hi = np.zeros(I, np.int64), np.full(I, O - 1, np.int64)
        if s > 0:
            c = np.arange(I, dtype=np.float32)
            lo = np.maximum(0, np.floor((c - one) / s).astype(np.int64) - 1)
            hi = np.minimum(O - 1, np.ceil((c + one) / s).astype(np.int64) + 1)
        return hi - lo + 1
    total = span(IH, OH)[:, None] * span(IW, OW)[None, :]
    return -(-total // 64) + 4 + 3


UP_BWD_SCATTER = [((7, 9), (10, 13)), ((7, 9), (7, 9)), ((12, 10), (5, 4)), ((1, 6), (1, 9))]
UP_BWD_GATHER = [((1, 1), (56, 72)), ((1, 2), (9, 40)), ((3, 4), (13, 31)), ((7, 9), (56, 72))]
UP_FWD = [((1, 1), (6, 5)), ((1, 2), (56, 72)), ((7, 9), (56, 72)), ((3, 4), (3, 4)), ((2, 2), (1, 1))]
RESIZE_FWD = [((12, 39), (24, 78)), ((24, 78), (47, 156)), ((47, 156), (94, 311)), ((5, 5), (5, 5)), ((9, 9), (4, 4))]


def bilinear_bound(mag):
    """8 2^-24 sum w_i |v_i|: two weight roundings (1 - t), four products and three additions per axis pair, nested (<= 7 roundings
    on any path from a v_i to the result)"""
    return 8 * EPS32 * mag


# ------------------------------------------------------------------------------------------------ max_pool2d
def maxpool_out(H, k, s):
    """ceil-mode output size with pad 0: the last window must start inside the input"""
    o = -(-(H - k) // s) + 1 if H >= k else 1
    if (o - 1) * s >= H:
        o -= 1
    return o


def maxpool(x, k, s, start=-np.inf, clip=True):
    """x [..., H, W] -> max over the clipped windows.  Mistakes: start = 0 (a zero start value), clip=False = floor mode: the ragged last
    row and column of windows are dropped (left at 0)."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    OH, OW = maxpool_out(H, k, s), maxpool_out(W, k, s)
    y = np.zeros(x.shape[:-2] + (OH, OW), x.dtype)
    for oy in range(OH):
        for ox in range(OW):
            if not clip and (oy * s + k > H or ox * s + k > W):
                continue
            win = x[..., oy * s:min(oy * s + k, H), ox * s:min(ox * s + k, W)]
            y[..., oy, ox] = np.maximum(win.max((-2, -1)), x.dtype.type(start))
    return y


MAXPOOL_CASES = [(3, 2, (5, 5)), (3, 2, (6, 7)), (3, 2, (188, 621)), (1, 2, (12, 39)), (1, 2, (1, 1))]


def up_bwd_inputs(ihw, ohw):
    """g [2, 32, OH, OW] and the nonzero grad_x [2, 32, IH, IW] it is accumulated onto"""
    return uniform(f"ub:{ihw}{ohw}:g", (2, 32) + ohw), uniform(f"ub:{ihw}{ohw}:old", (2, 32) + ihw)


def avg_bwd_inputs(hw, k):
    return uniform(f"ab:{hw}{k}:g", (2, 32, hw[0] // k, hw[1] // k)), uniform(f"ab:{hw}{k}:old", (2, 32) + hw)


def half(a):
    """rounded to fp16, as float32"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def f16_bound(ref, fp32_term):
    """the fp32 arithmetic's term, one rounding of the result to fp16 (2^-11 relative) and half the smallest subnormal"""
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + fp32_term


# ------------------------------------------------------------------------------------------------ generic mistakes on a result
def shift_col(a):
    out = np.zeros_like(a)
    out[..., 1:] = a[..., :-1]
    return out


def drop_last_col(a):
    out = a.copy()
    out[..., -1] = 0
    return out


def drop_last_row(a):
    out = a.copy()
    out[..., -1, :] = 0
    return out


def margin(ref, mutant, bound):
    """largest |mutant - ref| / bound over the elements (inf where the bound is 0 and the values differ)"""
    d = np.abs(np.asarray(mutant, F64) - np.asarray(ref, F64))
    b = np.broadcast_to(np.asarray(bound, F64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / b, 0.0)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ blocked storage without the pack kernels
def guarded(numel, fill, dev, dtype=torch.float32, guard=4096):
    """(whole, view): `numel` elements with `guard` elements in front and behind, all holding `fill`"""
    whole = torch.full((numel + 2 * guard,), fill, dtype=dtype, device=dev)
    return whole, whole[guard:guard + numel]


def guards_keep(whole, fill, guard=4096):
    return bool((whole[:guard] == fill).all()) and bool((whole[-guard:] == fill).all())


def interior(t, storage=None, off=0, cb=None):
    """the interior of a Blocked / Blocked16 tensor (channel blocks [off, off + cb)) as a view [N, cb, D, H, W, lanes] of its storage"""
    storage = t.storage if storage is None else storage
    lanes = 32 if storage.dtype == torch.float16 else 16
    v = storage[: t.numel].view(t.N, t.numel // (t.N * t.cb_stride) if t.N else 0, t.Dp, t.Hp, t.Wp, lanes)
    cb = v.shape[1] - off if cb is None else cb
    return v[:, off:off + cb, t.pd:t.pd + t.D, t.ph:t.ph + t.H, t.pw:t.pw + t.W]


def put(t, dense, off=0):
    """dense [N, C, D, H, W] (numpy or CPU tensor) -> the interior of channel blocks [off, ...) of t; padded channels become 0"""
    dense = torch.as_tensor(dense)
    lanes = 32 if t.storage.dtype == torch.float16 else 16
    N, C = dense.shape[:2]
    cb = (C + lanes - 1) // lanes
    full = torch.zeros(N, cb * lanes, *dense.shape[2:], dtype=t.storage.dtype)
    full[:, :C] = dense.to(t.storage.dtype)
    interior(t, off=off, cb=cb).copy_(full.view(N, cb, lanes, *dense.shape[2:]).permute(0, 1, 3, 4, 5, 2).to(t.storage.device))
    return t


def get(t, channels, off=0):
    """interior of channel blocks [off, ...) of t -> dense fp64 numpy [N, channels, D, H, W]"""
    lanes = 32 if t.storage.dtype == torch.float16 else 16
    cb = (channels + lanes - 1) // lanes
    v = interior(t, off=off, cb=cb)
    return v.permute(0, 1, 5, 2, 3, 4).reshape(t.N, cb * lanes, t.D, t.H, t.W)[:, :channels].cpu().double().numpy()


def outside_keeps(t, fill, off=0, cb=None):
    """True when everything but the interior of blocks [off, off + cb) of t -- halo, slack, the other channel blocks -- still holds `fill`"""
    s = t.storage.clone()
    interior(t, s, off, cb).fill_(fill)
    return bool((s == fill).all())

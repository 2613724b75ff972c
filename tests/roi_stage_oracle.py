"""Plain fp64 references (numpy) of the ROI stage -- csrc/roi_ops.hip (ROIAlign forward / backward, the FPN pooler, the ROI pairing, the
training targets) and the paste / depth kernels of csrc/post_ops.hip -- with the case tables of tests/test_hip_roi_stage.py, mirrors of
the launchers' grid arithmetic and the "plausible mistakes" tests/test_roi_stage_oracle.py uses to show that every case's input is strong
enough for its bound.

Every reference returns, next to its value, the element-wise MAGNITUDE sum (the same sum with every term replaced by its absolute
value).  Sample and source coordinates are numpy float32 with the reference's expressions (for ROIAlign the expression order of
oracle/roi_oracle.py, which is pinned bit for bit to the reference's kernel); weights, products and sums are fp64.

A mistake is a flag in `mis`:
  ROIAlign   "count_sq" count = gh*gh | "swap23" w2 and w3 swapped | "no_clamp0" the <= 0 clamp dropped | "max_before_scale" max(., 1)
             taken before the scale | "round_roi" the roi rounded to integers | "cg_off" the channel group read one group off (forward)
             | wrap_dropped_*: the stride step replaced by `total`, the second trip never taken
  targets    "keep_off" off not subtracted | "inv_scale" res/mw inverted | "half_pixel" align_corners=False coordinates | "no_pad" Masker
             padding ignored
  paste      "wd_left" wd = wl instead of max(wl, wr) | "no_offset" the x1 - x1p offset dropped
"""
import functools
import math

import numpy as np

from oracle import roi_oracle as RO
from tests.resample_oracle import EPS32, uniform

F32, F64 = np.float32, np.float64
CAP = 4096 * 256                                        # work items one trip of a capped grid covers


# ------------------------------------------------------------------------------------------------ grid mirrors
def grid_for(work):
    """roi_ops.hip: blocks of 256 threads, at least 1, at most 4096 -> (blocks, wraps)"""
    b = min(max((work + 255) // 256, 1), 4096)
    return b, work > b * 256


def blocks_for(n):
    """post_ops.hip: the same clamp, per plane (blockIdx.y walks the images / rois)"""
    b = min(max((n + 255) // 256, 1), 4096)
    return b, n > b * 256


def fwd_cc(C):
    """channels per thread of drc_roi_align_fwd"""
    return 4 if C % 4 == 0 else 3 if C % 3 == 0 else 1


def fpn_cc(C):
    return 4 if C % 4 == 0 else 1


# ------------------------------------------------------------------------------------------------ ROIAlign
def roi_geometry(roi, scale, ph, pw, sr, H, W, mis=()):
    """One roi -> dict: gh, gw, count, and per sample point [gh*gw, ph, pw]: yy, xx (float32 sample coordinates), dead, the corner rows /
    columns yl, yh, xl, xh and the four fp64 weights w1..w4 (zero where dead)."""
    f = F32
    r, s = np.asarray(roi, F32), f(scale)
    if "max_before_scale" in mis:
        rsw, rsh = f(r[1] * s), f(r[2] * s)
        rw, rh = f(max(f(r[3] - r[1]), f(1.0)) * s), f(max(f(r[4] - r[2]), f(1.0)) * s)
    else:
        rsw, rsh, rew, reh = f(r[1] * s), f(r[2] * s), f(r[3] * s), f(r[4] * s)
        if "round_roi" in mis:
            rsw, rsh, rew, reh = (f(np.round(v)) for v in (rsw, rsh, rew, reh))
        rw, rh = max(f(rew - rsw), f(1.0)), max(f(reh - rsh), f(1.0))
    bin_h, bin_w = f(rh / f(ph)), f(rw / f(pw))
    gh = sr if sr > 0 else int(math.ceil(rh / ph))
    gw = sr if sr > 0 else int(math.ceil(rw / pw))
    ii, jj = np.arange(ph, dtype=F32)[:, None], np.arange(pw, dtype=F32)[None, :]
    g = {k: [] for k in ("yy", "xx", "dead", "yl", "yh", "xl", "xh", "w1", "w2", "w3", "w4")}
    for iy in range(gh):
        yy = (rsh + ii * bin_h) + f(f(iy + 0.5) * bin_h) / f(gh)
        for ix in range(gw):
            xx = (rsw + jj * bin_w) + f(f(ix + 0.5) * bin_w) / f(gw)
            assert yy.dtype == F32 and xx.dtype == F32
            y, x = np.broadcast_to(yy, (ph, pw)).copy(), np.broadcast_to(xx, (ph, pw)).copy()
            g["yy"].append(y.copy()); g["xx"].append(x.copy())
            dead = (y < -1.0) | (y > H) | (x < -1.0) | (x > W)
            if "no_clamp0" not in mis:
                y[y <= 0] = 0; x[x <= 0] = 0
            y_low, x_low = np.maximum(y.astype(np.int64), 0), np.maximum(x.astype(np.int64), 0)     # (int): towards zero
            ycl, xcl = y_low >= H - 1, x_low >= W - 1
            y_low[ycl] = H - 1; x_low[xcl] = W - 1
            y_high, x_high = np.where(ycl, y_low, y_low + 1), np.where(xcl, x_low, x_low + 1)
            y = np.where(ycl, y_low.astype(F32), y); x = np.where(xcl, x_low.astype(F32), x)
            ly, lx = (y - y_low.astype(F32)).astype(F64), (x - x_low.astype(F32)).astype(F64)
            hy, hx = 1.0 - ly, 1.0 - lx
            w = [hy * hx, hy * lx, ly * hx, ly * lx]
            if "swap23" in mis:
                w[1], w[2] = w[2], w[1]
            for a in (y_low, y_high, x_low, x_high):
                a[dead] = 0
            for a in w:
                a[dead] = 0.0
            for k, a in zip(("dead", "yl", "yh", "xl", "xh", "w1", "w2", "w3", "w4"), (dead, y_low, y_high, x_low, x_high, *w)):
                g[k].append(a)
    out = {k: np.stack(v) for k, v in g.items()}
    out.update(gh=gh, gw=gw, count=float(gh * gh if "count_sq" in mis else gh * gw))
    return out


def roi_grids(rois, scale, ph, pw, sr):
    """[(gh, gw)] per roi"""
    return [(g["gh"], g["gw"]) for g in (roi_geometry(r, scale, ph, pw, sr, 8, 8) for r in rois)]


def _corners(g):
    return ((g["yl"], g["xl"], g["w1"]), (g["yl"], g["xh"], g["w2"]), (g["yh"], g["xl"], g["w3"]), (g["yh"], g["xh"], g["w4"]))


def roi_align_fwd64(inp, rois, scale, ph, pw, sr, mis=(), cc=None):
    """inp [B,C,H,W], rois [K,5] -> (out, mag) [K,C,ph,pw] fp64.  `cc` (channels per thread) only matters to the mistake "cg_off"."""
    inp = np.asarray(inp, F64)
    B, C, H, W = inp.shape
    K = len(rois)
    out, mag = np.zeros((K, C, ph, pw)), np.zeros((K, C, ph, pw))
    chan = np.arange(C)
    if "cg_off" in mis:
        cc = cc or fwd_cc(C)
        chan = ((chan // cc + 1) % (C // cc)) * cc + chan % cc
    for k in range(K):
        g = roi_geometry(rois[k], scale, ph, pw, sr, H, W, mis)
        img = inp[int(rois[k][0])][chan]
        for yi, xi, w in _corners(g):
            v = img[:, yi, xi]                                                        # [C, S, ph, pw]
            out[k] += (w * v).sum(1)
            mag[k] += (w * np.abs(v)).sum(1)
        out[k] /= g["count"]; mag[k] /= g["count"]
    return out, mag


def roi_align_bwd64(gout, rois, scale, ph, pw, sr, shape, init, mis=()):
    """gout [K,C,ph,pw] -> (gin, mag, contributors) [B,C,H,W]: init + sum of gout / count * w over every (roi, bin, sample, corner) that
    lands on the pixel; contributors counts those terms whose weight is not zero (a zero term changes nothing)."""
    B, C, H, W = shape
    gin = np.array(init, F64).reshape(shape).copy()
    mag = np.abs(gin)
    cnt = np.zeros(shape, np.int64)
    for k in range(len(rois)):
        g = roi_geometry(rois[k], scale, ph, pw, sr, H, W, mis)
        b = int(rois[k][0])
        gv = (np.asarray(gout[k], F64) / g["count"])[:, None]                          # [C, 1, ph, pw]
        for yi, xi, w in _corners(g):
            np.add.at(gin[b], (slice(None), yi, xi), gv * w)
            np.add.at(mag[b], (slice(None), yi, xi), np.abs(gv) * w)
            np.add.at(cnt[b], (slice(None), yi, xi), np.broadcast_to(w != 0, (C,) + w.shape).astype(np.int64))
    return gin, mag, cnt


def bwd_bound(mag, cnt):
    """(contributors + 4) 2^-24 mag: one rounding each for 1 - l, the weight product, gout / count and the term, one per addition"""
    return (cnt + 4) * EPS32 * mag


def fwd_tie_bound(mag, grids):
    """what the pinned float32 oracle may differ from fwd64 by: (4 gh gw + 2) 2^-24 mag per roi"""
    return np.stack([(4 * gh * gw + 2) * EPS32 * m for (gh, gw), m in zip(grids, mag)])


def wrap_dropped_fwd(out, cc, fill):
    """the forward with its second trip never taken: work items (k, cg, ph, pw) past the first CAP keep `fill`"""
    K, C, PH, PW = out.shape
    o = out.reshape(K, C // cc, cc, PH, PW).transpose(0, 1, 3, 4, 2).reshape(-1, cc).copy()
    o[CAP:] = fill
    return o.reshape(K, C // cc, PH, PW, cc).transpose(0, 1, 4, 2, 3).reshape(out.shape)


def wrap_dropped_flat(a, fill=0.0, per=None):
    """flat work items past the first CAP (per leading plane when `per`) replaced by `fill`"""
    o = np.array(a).copy()
    if per:
        o.reshape(-1, per)[:, CAP:] = fill
    else:
        o.reshape(-1)[CAP:] = fill
    return o


# (name, map shape, ph, pw, sampling ratio, scale, rois, mistakes that must clear 10x)
_ADAPTIVE = [(0, 2.3, 1.7, 7.1, 5.9), (1, 3.5, 2.25, 14.0, 11.0), (0, 10.2, 4.1, 27.9, 18.3), (1, 5.0, 6.0, 5.6, 20.5), (0, 12.0, 3.0, 23.5, 3.4),
             (1, 14.4, 8.8, 29.7, 12.9), (0, 1.0, 9.0, 8.5, 21.0), (1, 20.25, 1.5, 26.0, 9.75)]
_SCALED = [(0, 4.6, 3.4, 30.2, 25.8), (1, 20.0, 10.0, 55.5, 41.3), (0, 33.3, 7.7, 34.8, 30.1), (1, 2.2, 30.5, 44.4, 31.9), (0, 40.1, 20.9, 60.7, 44.2)]
_OUTSIDE = [(0, -5.6, 4.3, 5.2, 12.1), (0, 8.4, -5.5, 17.3, 6.0), (0, 22.7, 9.1, 36.0, 17.8), (0, 3.3, 15.2, 11.9, 28.0), (1, 40.0, 30.0, 50.0, 41.0)]
_MALFORMED = [(0, 12.5, 8.5, 7.0, 3.0), (1, 20.0, 5.2, 15.0, 12.7), (0, 5.3, 15.0, 9.9, 11.0)]
_WRAP = [(0, 1.5, 2.5, 58.0, 38.2), (1, 10.1, 0.3, 40.7, 39.0), (0, 20.0, 10.0, 31.0, 22.0), (1, 0.0, 0.0, 59.0, 39.0), (0, 30.3, 5.5, 55.5, 30.9),
         (1, 5.2, 12.8, 50.4, 33.3)]
BWD_CASES = [
    ("adaptive", (2, 5, 23, 31), 5, 6, 0, 1.0, _ADAPTIVE, ("count_sq", "swap23", "round_roi")),
    ("scaled.5", (2, 4, 23, 31), 7, 7, 2, 0.5, _SCALED, ("swap23", "max_before_scale", "round_roi")),
    ("scaled.25", (2, 4, 23, 31), 7, 7, 2, 0.25, _SCALED, ("swap23", "max_before_scale", "round_roi")),
    ("outside", (2, 3, 23, 31), 4, 4, 2, 1.0, _OUTSIDE, ("swap23", "no_clamp0", "round_roi")),
    ("malformed", (2, 3, 23, 31), 3, 3, 2, 1.0, _MALFORMED, ("swap23", "round_roi")),
    ("pileup", (2, 2, 23, 31), 7, 7, 2, 1.0, [(1, 10.2, 7.3, 12.9, 9.8)] * 64, ("swap23", "round_roi")),
    ("wrap", (2, 8, 40, 60), 150, 150, 1, 1.0, _WRAP, ("swap23", "round_roi", "wrap_dropped")),
    ("empty", (2, 3, 9, 11), 3, 3, 2, 1.0, [], ()),
]
ROI_MISTAKES = ("count_sq", "swap23", "no_clamp0", "max_before_scale", "round_roi")


def rois_of(rows):
    return np.asarray(rows, F32).reshape(-1, 5)


@functools.lru_cache(maxsize=2)
def bwd_case(name):
    """inputs and the reference of one backward case: rois, gout, init (nonzero: |init| in [0.25, 1.25)), gin, mag, cnt"""
    _, shape, ph, pw, sr, scale, rows, must = next(c for c in BWD_CASES if c[0] == name)
    rois = rois_of(rows)
    gout = uniform(f"rb:{name}:g", (len(rois), shape[1], ph, pw))
    init = uniform(f"rb:{name}:i", shape, 0.25, 1.25) * np.where(uniform(f"rb:{name}:s", shape) < 0, F32(-1), F32(1))
    gin, mag, cnt = roi_align_bwd64(gout, rois, scale, ph, pw, sr, shape, init)
    return dict(shape=shape, ph=ph, pw=pw, sr=sr, scale=scale, rois=rois, gout=gout, init=init, gin=gin, mag=mag, cnt=cnt, must=must)


# forward: channel groupings on the rois of tests/golden/roi_golden.npz (two of its settings), a 2 x C x 37 x 53 map
FWD_CHANNELS = [1, 2, 5, 6, 7, 9, 12]
FWD_NORM_CHANNELS = [4, 5, 6]
FWD_SETTINGS = [(6, 5, 0, 1.0), (14, 14, 0, 0.5)]
FWD_HW = (37, 53)
FWD_WRAP = dict(shape=(2, 8, 40, 60), ph=232, pw=232, sr=1, scale=1.0,
                rois=[(k % 2, 1.5 + 2.3 * k, 0.7 + 1.1 * k, 33.0 + 2.6 * k, 24.5 + 1.4 * k) for k in range(10)])


def fwd_input(C, hw=FWD_HW, B=2):
    return uniform(f"rf:{C}:{hw}", (B, C) + tuple(hw), 0.0, 1.0)


def norm_consts(C):
    return uniform(f"rf:mean{C}", (C,), 0.3, 0.6), uniform(f"rf:std{C}", (C,), 0.2, 0.3)


# FPN pooler: four levels of an 80 x 128 image, 24 rois in shuffled level order, level 2 empty, one roi larger than its level's map
FPN_LEVELS = [((20, 32), 0.25), ((10, 16), 0.125), ((5, 8), 0.0625), ((3, 4), 0.03125)]
FPN_SETTINGS = [(7, 7, 2), (3, 4, 0)]
FPN_CHANNELS = [8, 5]


def fpn_case(C):
    rng = np.random.default_rng(20 + C)
    levels = np.array([0] * 10 + [1] * 8 + [3] * 6, np.int32)
    rng.shuffle(levels)
    K = len(levels)
    x1, y1 = rng.uniform(-6, 100, K), rng.uniform(-6, 60, K)
    w, h = rng.uniform(3, 60, K), rng.uniform(3, 40, K)
    rois = np.stack([rng.integers(0, 2, K), x1, y1, x1 + w, y1 + h], 1).astype(F32)
    big = int(np.flatnonzero(levels == 3)[0])
    rois[big, 1:] = (-10.0, -12.0, 200.0, 150.0)                                      # 6.6 x 5.1 px on a 3 x 4 map
    feats = [uniform(f"fpn:{C}:{l}", (2, C) + hw, -1.0, 1.0) for l, (hw, _) in enumerate(FPN_LEVELS)]
    return feats, rois, levels, big


# ------------------------------------------------------------------------------------------------ ROI pairing
def align_pairs(lbox, rbox, img_idx, img_w, img_h):
    """[R,4] boxes (taken as float32 before floor / ceil, as the kernel sees them) -> rois_l, rois_r [R,5] f32, geom [R,4] int32 =
    (x1, x1p, x1 + mw, x1p + mw): oracle.roi_oracle.align_roi_pair per row"""
    lbox, rbox = np.asarray(lbox, F32).reshape(-1, 4), np.asarray(rbox, F32).reshape(-1, 4)
    R = len(lbox)
    rl, rr, geom = np.zeros((R, 5), F32), np.zeros((R, 5), F32), np.zeros((R, 4), np.int32)
    for i in range(R):
        x1, y1, x1p, y2, mw = RO.align_roi_pair([float(v) for v in lbox[i]], [float(v) for v in rbox[i]], img_w, img_h)
        rl[i] = (img_idx[i], x1, y1, x1 + mw, y2)
        rr[i] = (img_idx[i], x1p, y1, x1p + mw, y2)
        geom[i] = (x1, x1p, x1 + mw, x1p + mw)
    return rl, rr, geom


PAIR_W, PAIR_H = 1242, 375
PAIR_R = [1, 63, 64, 65, 129]
# (what it forces, left box, right box)
PAIR_SPECIALS = [
    ("integer", (100.0, 50.0, 200.0, 150.0), (80.0, 50.0, 180.0, 150.0)),
    ("negative", (-3.5, -2.25, 60.5, 40.5), (-10.0, -2.25, 50.2, 40.5)),
    ("beyond", (1100.3, 300.2, 1300.0, 400.0), (1050.1, 300.2, 1260.0, 400.0)),
    ("right wider", (500.2, 100.1, 540.7, 160.9), (450.3, 100.1, 520.8, 160.9)),
    ("cut by x1p", (1000.5, 10.0, 1241.5, 100.0), (1100.2, 10.0, 1241.9, 100.0)),
    ("cut by x1", (1150.3, 20.0, 1241.2, 90.0), (900.4, 20.0, 1241.7, 90.0)),
    ("x2 on the border", (700.5, 30.5, 1241.0, 200.0), (650.5, 30.5, 1200.0, 200.0)),
    ("just below an integer", (900.25, 40.0, 1240.9999, 300.5), (880.0001, 40.0, 1200.9999, 300.5)),
]


def pair_tables(R):
    """The box tables of one R: the specials sit at the END of the table (next to the block edge), the rows in front are random.  A table
    shorter than the specials is run once per rotation, so every R sees every special.  -> [(lbox, rbox, img_idx)]"""
    n = len(PAIR_SPECIALS)
    out = []
    for rot in (range(n) if R < n else (0,)):
        rng = np.random.default_rng(1000 * R + rot)
        m = max(R - n, 0)
        x1, y1 = rng.uniform(-20, 1200, m), rng.uniform(-10, 340, m)
        w, h = rng.uniform(2, 300, m), rng.uniform(2, 200, m)
        sh, dw = rng.uniform(0, 80, m), rng.uniform(-30, 30, m)
        lb = np.stack([x1, y1, x1 + w, y1 + h], 1)
        rb = np.stack([x1 - sh, y1, x1 - sh + np.maximum(w + dw, 1.5), y1 + h], 1)
        sp = [PAIR_SPECIALS[(i + rot) % n] for i in range(min(R, n))]
        lb = np.concatenate([lb, np.array([s[1] for s in sp]).reshape(-1, 4)]).astype(F32)
        rb = np.concatenate([rb, np.array([s[2] for s in sp]).reshape(-1, 4)]).astype(F32)
        out.append((lb, rb, (np.arange(R) % 3).astype(np.int32)))
    return out


# ------------------------------------------------------------------------------------------------ training targets
def _axis_ac(I, O, half_pixel=False):
    """align_corners=True source coordinates of O outputs over I inputs, float32 as the kernel (and ATen): i0, i1, fraction (float32)"""
    o = np.arange(O, dtype=F32)
    if half_pixel:
        fl = np.maximum(F32(I) / F32(O) * (o + F32(0.5)) - F32(0.5), F32(0))
    else:
        fl = (F32(I - 1) / F32(O - 1) if O > 1 else F32(0)) * o
    assert fl.dtype == F32
    i0 = np.minimum(fl.astype(np.int64), I - 1)
    return i0, i0 + (i0 < I - 1), (fl - i0.astype(F32)).astype(F32)


def paste_box(box, M, pad):
    """expand_boxes + .to(int32) of paste_mask_in_image, float32: -> bx0, by0, bw, bh"""
    b = np.asarray(box, F32)
    scale = F32((M + 2 * pad) / M)
    w_half, h_half = (b[2] - b[0]) * F32(0.5) * scale, (b[3] - b[1]) * F32(0.5) * scale
    xc, yc = (b[2] + b[0]) * F32(0.5), (b[3] + b[1]) * F32(0.5)
    x0, x1, y0, y1 = (int(np.trunc(v)) for v in (xc - w_half, xc + w_half, yc - h_half, yc + h_half))
    return x0, y0, max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)


def masker_blend64(prob, M, pad, box, H, W):
    """The Masker's interpolated probability over the image in fp64, NaN outside the pasted window: F.interpolate(padded mask, (bh, bw),
    bilinear, align_corners=False) with the source coordinate scale * (dst + 0.5) - 0.5 in float32, clamped at 0, as ATen does."""
    bx0, by0, bw, bh = paste_box(box, M, pad)
    P = M + 2 * pad
    padded = np.zeros((P, P))
    padded[pad:pad + M, pad:pad + M] = np.asarray(prob, F64).reshape(M, M)
    out = np.full((H, W), np.nan)
    ys, xs = np.arange(max(by0, 0), min(by0 + bh, H)), np.arange(max(bx0, 0), min(bx0 + bw, W))
    if len(ys) == 0 or len(xs) == 0:
        return out

    def axis(idx, o0, n):
        fl = np.maximum(F32(P) / F32(n) * ((idx - o0).astype(F32) + F32(0.5)) - F32(0.5), F32(0))
        assert fl.dtype == F32
        i0 = fl.astype(np.int64)
        return i0, i0 + (i0 < P - 1), (fl - i0.astype(F32)).astype(F64)
    (y0, y1, ly), (x0, x1, lx) = axis(ys, by0, bh), axis(xs, bx0, bw)
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * padded[y0][:, x0] + lx * padded[y0][:, x1]
    bot = (1 - lx) * padded[y1][:, x0] + lx * padded[y1][:, x1]
    out[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = (1 - ly) * top + ly * bot
    return out


def train_targets64(disp_maps, gt_masks, probs, M, pad, thresh, det_boxes, rois_l, geom, res, mis=()):
    """-> dict: target, mag [R,res,res] (mag includes res / mw); blend [R,H,W] (the Masker blend, NaN outside its window); src [R,H,W]
    uint8 = gt & (blend > thresh); and per roi the mask's source geometry rec[r] = None (empty slice: the mask is 0) or dict(Y [res,2],
    X [res,2] corner rows / columns in the image, wy, wx [res,2] their fp64 weights -- corner (a, b) of pixel (i, j) is (Y[i,a], X[j,b]) with
    weight wy[i,a] wx[j,b] --, ly, lx [res] the float32 fractions, box the clipped slice)."""
    disp_maps, probs = np.asarray(disp_maps, F64), np.asarray(probs, F64)
    R, (_, H, W) = len(rois_l), disp_maps.shape
    target, mag = np.zeros((R, res, res)), np.zeros((R, res, res))
    blend, src, rec = np.full((R, H, W), np.nan), np.zeros((R, H, W), np.uint8), []
    hp = "half_pixel" in mis
    for r in range(R):
        b = int(rois_l[r][0])
        x1, x1p, mw = int(geom[r][0]), int(geom[r][1]), int(geom[r][2] - geom[r][0])
        y1, y2 = int(rois_l[r][2]), int(rois_l[r][4])
        hc = y2 - y1
        if hc > 0 and mw > 0:
            off = 0.0 if "keep_off" in mis else float(x1 - x1p)
            crop, cab = np.full((hc, mw), -off), np.full((hc, mw), abs(off))
            ys, xs = np.arange(y1, y2), np.arange(x1, x1 + mw)
            oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            sub = disp_maps[b][ys[oky]][:, xs[okx]]
            crop[np.ix_(oky, okx)] += sub
            cab[np.ix_(oky, okx)] += np.abs(sub)
            (y0, ya, ly), (x0, xa, lx) = _axis_ac(hc, res, hp), _axis_ac(mw, res, hp)
            ly, lx = ly.astype(F64)[:, None], lx.astype(F64)[None, :]
            k = mw / res if "inv_scale" in mis else res / mw
            for dst, a in ((target, crop), (mag, cab)):
                top = (1 - lx) * a[y0][:, x0] + lx * a[y0][:, xa]
                bot = (1 - lx) * a[ya][:, x0] + lx * a[ya][:, xa]
                dst[r] = ((1 - ly) * top + ly * bot) * k
        blend[r] = masker_blend64(probs[r], M, 0 if "no_pad" in mis else pad, det_boxes[r], H, W)
        src[r] = (np.asarray(gt_masks[b]) != 0) & (np.nan_to_num(blend[r], nan=-np.inf) > thresh)
        ylo, xlo = max(y1, 0), max(x1, 0)
        mh, mwc = min(y2, H) - ylo, min(x1 + mw, W) - xlo
        if mh > 0 and mwc > 0:
            (y0, ya, ly), (x0, xa, lx) = _axis_ac(mh, res, hp), _axis_ac(mwc, res, hp)
            ly64, lx64 = ly.astype(F64), lx.astype(F64)
            rec.append(dict(Y=np.stack([ylo + y0, ylo + ya], 1), X=np.stack([xlo + x0, xlo + xa], 1), ly=ly, lx=lx, box=(ylo, xlo, mh, mwc),
                            wy=np.stack([1.0 - ly64, ly64], 1), wx=np.stack([1.0 - lx64, lx64], 1)))
        else:
            rec.append(None)
    return dict(target=target, mag=mag, blend=blend, src=src, rec=rec, thresh=thresh, res=res)


SKIP, ZERO, ONE, INTERP = -1, 0, 1, 2


def mask_expect(t):
    """The mask rules per output pixel -> (code [R,res,res], interp [R,res,res] uint8):
      1  a Masker blend within 16 2^-24 of the threshold at a contributing corner: SKIP
      2  float32 ly == 0 and lx == 0: the pixel equals gt & Masker at that source pixel (ZERO / ONE)
      3  a contributing corner of weight >= 2^-20 that is 0: ZERO          4  one of weight in (0, 2^-20) that is 0: SKIP
      5  every contributing corner 1, a fraction nonzero: INTERP -- compared with F.interpolate(align_corners=True).to(uint8) on the CPU of
         the same gt & Masker slice (`interp`), up to the share of mismatches the caller allows
    An empty slice is ZERO everywhere."""
    import torch
    import torch.nn.functional as F
    res, R = t["res"], len(t["rec"])
    code, interp = np.zeros((R, res, res), np.int8), np.zeros((R, res, res), np.uint8)
    for r, q in enumerate(t["rec"]):
        if q is None:
            continue
        near = np.abs(np.nan_to_num(t["blend"][r], nan=np.inf) - t["thresh"]) <= 16 * EPS32
        s = t["src"][r]
        wy, wx = q["wy"], q["wx"]                                                     # [res, 2]
        c = np.full((res, res), INTERP, np.int8)
        skip1, zero3, skip4 = (np.zeros((res, res), bool) for _ in range(3))
        for a in range(2):
            for b in range(2):
                w = wy[:, a][:, None] * wx[:, b][None, :]
                Y, X = q["Y"][:, a][:, None], q["X"][:, b][None, :]
                on = w > 0
                skip1 |= on & near[Y, X]
                zero3 |= (w >= 2.0 ** -20) & (s[Y, X] == 0)
                skip4 |= on & (w < 2.0 ** -20) & (s[Y, X] == 0)
        exact = (q["ly"] == 0)[:, None] & (q["lx"] == 0)[None, :]
        c[skip4] = SKIP
        c[zero3] = ZERO
        c[exact] = s[q["Y"][:, 0][:, None], q["X"][:, 0][None, :]][exact]
        c[skip1] = SKIP
        code[r] = c
        y, x, mh, mwc = q["box"]
        sl = torch.from_numpy(s[y:y + mh, x:x + mwc].astype(np.float32))[None, None]
        interp[r] = F.interpolate(sl, (res, res), mode="bilinear", align_corners=True)[0, 0].to(torch.uint8).numpy()
    return code, interp


def target_bound(mag):
    """12 2^-24 mag: the subtraction of off, two weight roundings, four products and three additions nested over the two axes, / mw, * res"""
    return 12 * EPS32 * mag


TGT_HW = (40, 64)


def _blob_probs(tag, R, M):
    """smooth mask probabilities: high in the middle, falling below the threshold towards the rim, a little noise"""
    g = (np.arange(M) + 0.5) / M * 2 - 1
    r4 = g[:, None] ** 4 + g[None, :] ** 4                                           # crosses the threshold next to the rim: the padding matters
    return np.clip(1.02 - 0.45 * r4[None] + uniform(tag, (R, M, M), -0.04, 0.04), 0.0, 1.0).astype(F32).reshape(R, M * M)


def _gt_masks(tag, B, H, W):
    """mostly 1, with a band of rows, a band of columns and a few single pixels off"""
    m = np.ones((B, H, W), np.uint8)
    for b in range(B):
        m[b, 5 + 7 * b:8 + 7 * b] = 0
        m[b, :, 20 + 9 * b:22 + 9 * b] = 0
    m[uniform(tag, (B, H, W), 0.0, 1.0) < 0.03] = 0
    return m


# (name, images, (H, W), res, M, pad, [(image, left box, right box)])
def _ibox(x1, y1, dw, dh, shift):
    """integer boxes whose mw - 1 = dw and hc - 1 = dh"""
    return (float(x1), float(y1), float(x1 + dw + 1), float(y1 + dh + 1)), (float(x1 - shift), float(y1), float(x1 - shift + dw + 1), float(y1 + dh + 1))


TGT_CASES = {
    "integer": dict(B=3, hw=TGT_HW, res=8, M=28, pad=1, rois=[(0,) + _ibox(5, 3, 7, 14, 2), (1,) + _ibox(30, 10, 21, 7, 4), (2,) + _ibox(12, 2, 14, 21, 0),
                                                                 (2,) + _ibox(40, 20, 7, 7, 6), (1,) + _ibox(3, 12, 14, 14, 1)]),
    # slice sizes (rows x columns) 22x19, 19x19, 25x37, 16x28, 28x9, 9x55: float32 F.interpolate on the CPU, which rule 5 compares with, is
    # itself exact on an all-ones neighbourhood at these sizes (at most sizes it truncates ~1 % of such pixels to 0; asserted on the CPU)
    "general": dict(B=2, hw=TGT_HW, res=28, M=28, pad=1, rois=[
        (0, (-3.2, -2.6, 18.4, 21.3), (-6.0, -2.6, 12.1, 21.3)),                      # paste window clipped at the left and the top
        (1, (45.3, 20.1, 66.7, 42.8), (38.9, 20.1, 60.2, 42.8)),                      # ... at the right and the bottom; mw cut by the image
        (0, (20.7, 8.2, 56.9, 32.6), (11.2, 8.2, 44.9, 32.6)), (1, (5.5, 4.5, 32.6, 19.8), (2.5, 4.5, 25.0, 19.8)),
        (0, (33.1, 10.9, 41.6, 38.0), (30.0, 10.9, 37.2, 38.0)), (1, (4.4, 22.3, 58.8, 30.7), (1.6, 22.3, 52.0, 30.7))]),
    "degenerate1": dict(B=2, hw=TGT_HW, res=1, M=28, pad=1, rois=None),
    "degenerate2": dict(B=2, hw=TGT_HW, res=2, M=28, pad=1, rois=None),
    "M14pad0": dict(B=2, hw=TGT_HW, res=12, M=14, pad=0, rois=None),
    "M14pad2": dict(B=2, hw=TGT_HW, res=12, M=14, pad=2, rois=None),
    "wrap": dict(B=2, hw=(24, 40), res=224, M=28, pad=1, rois=[
        (k % 2, (1.3 + 1.1 * k, 0.6 + 0.4 * k, 14.2 + 1.15 * k, 13.9 + 0.45 * k), (0.2 + 1.0 * k, 0.6 + 0.4 * k, 12.4 + 1.1 * k, 13.9 + 0.45 * k)) for k in range(22)]),
}
_DEGENERATE = [(0, (10.0, 6.3, 11.0, 20.8), (7.0, 6.3, 8.0, 20.8)),                 # mw = 1
               (1, (22.4, 17.0, 41.9, 18.0), (15.1, 17.0, 35.0, 18.0)),               # hc = 1
               (1, (33.2, 8.2, 33.6, 8.7), (30.1, 8.2, 30.5, 8.7)),                   # a 1 x 1 paste box (and mw = hc = 1)
               (0, (12.5, 9.5, 34.0, 31.5), (8.5, 9.5, 30.5, 31.5))]
for _n in ("degenerate1", "degenerate2"):
    TGT_CASES[_n]["rois"] = _DEGENERATE
_M14 = [(0, (-3.2, -2.6, 12.4, 21.3), (-6.0, -2.6, 8.1, 21.3)), (1, (50.3, 20.1, 66.7, 42.8), (44.9, 20.1, 60.2, 42.8)),     # 22x13, 19x14,
        (0, (20.7, 8.2, 49.9, 32.6), (11.2, 8.2, 38.9, 32.6)), (1, (5.5, 4.5, 33.6, 20.8), (2.5, 4.5, 27.0, 20.8)),          # 25x30, 17x29,
        (0, (33.1, 10.9, 40.6, 37.0), (30.0, 10.9, 36.2, 37.0)), (1, (4.4, 22.3, 53.8, 30.7), (1.6, 22.3, 47.0, 30.7))]      # 27x8, 9x50
for _n in ("M14pad0", "M14pad2"):                       # the general case's layout at slice sizes on which the CPU interpolation to 12x12 is exact
    TGT_CASES[_n]["rois"] = _M14
TGT_THRESH = 0.7


@functools.lru_cache(maxsize=2)
def tgt_case(name):
    c = TGT_CASES[name]
    B, (H, W), res, M, pad = c["B"], c["hw"], c["res"], c["M"], c["pad"]
    idx = np.array([r[0] for r in c["rois"]], np.int32)
    lbox, rbox = np.array([r[1] for r in c["rois"]], F32), np.array([r[2] for r in c["rois"]], F32)
    rois_l, _, geom = align_pairs(lbox, rbox, idx, W, H)
    disp = uniform(f"tt:{name}:d", (B, H, W), 1.0, 60.0)
    gt = _gt_masks(f"tt:{name}:m", B, H, W)
    probs = _blob_probs(f"tt:{name}:p", len(idx), M)
    ref = train_targets64(disp, gt, probs, M, pad, TGT_THRESH, lbox, rois_l, geom, res)
    code, interp = mask_expect(ref)
    return dict(B=B, H=H, W=W, res=res, M=M, pad=pad, idx=idx, lbox=lbox, rbox=rbox, rois_l=rois_l, geom=geom, disp=disp, gt=gt, probs=probs,
                ref=ref, code=code, interp=interp)


def mask_mismatch(code, interp, got):
    """(hard, soft): pixels that break rules 2 / 3, and rule-5 pixels that differ from the CPU interpolation"""
    got = np.asarray(got)
    hard = int((((code == ZERO) | (code == ONE)) & (got != code)).sum())
    soft = int(((code == INTERP) & (got != interp)).sum())
    return hard, soft


def mask_moved(code, interp, other_code, other_interp):
    """share of the case's pixels whose expected value another reference (a mistake) changes, among the pixels both check"""
    a = np.where(code == INTERP, interp.astype(np.int8), code)
    b = np.where(other_code == INTERP, other_interp.astype(np.int8), other_code)
    return float(((code != SKIP) & (other_code != SKIP) & (a != b)).mean())


# ------------------------------------------------------------------------------------------------ paste and depth maps
def roi_value64(d, S, box6, H, W, mis=()):
    """One roi's pasted values over its left box clipped to the image -> (ys, xs, value [len(ys), len(xs)], bound ingredients mag * wd / S
    and |x1 - x1p|) or None when the clipped box is empty.  upsample_bilinear2d(align_corners=True) to (y2 - y1) x max(wl, wr), times
    wd / S, plus x1 - x1p."""
    x1, y1, x2, y2, x1p, x2p = (int(v) for v in box6)
    ys, xs = np.arange(max(y1, 0), min(y2, H)), np.arange(max(x1, 0), min(x2, W))
    if len(ys) == 0 or len(xs) == 0:
        return None
    hr, wl, wr = y2 - y1, x2 - x1, x2p - x1p
    wd = wl if "wd_left" in mis else max(wl, wr)
    d = np.asarray(d, F64).reshape(S, S)

    def axis(idx, o0, n):
        fl = (F32(S - 1) / F32(n - 1) if n > 1 else F32(0)) * (idx - o0).astype(F32)
        assert fl.dtype == F32
        i0 = np.minimum(fl.astype(np.int64), S - 1)
        return i0, i0 + (i0 < S - 1), np.clip(fl - i0.astype(F32), F32(0), F32(1)).astype(F64)
    (y0, ya, ly), (x0, xa, lx) = axis(ys, y1, hr), axis(xs, x1, wd)
    ly, lx = ly[:, None], lx[None, :]
    off = 0.0 if "no_offset" in mis else float(x1 - x1p)
    vals = []
    for a in (d, np.abs(d)):
        top = (1 - lx) * a[y0][:, x0] + lx * a[y0][:, xa]
        bot = (1 - lx) * a[ya][:, x0] + lx * a[ya][:, xa]
        vals.append(((1 - ly) * top + ly * bot) / S * wd)
    return ys, xs, vals[0] + off, vals[1] + abs(off)


def paste_bound(mag):
    """10 2^-24 (mag wd / S + |x1 - x1p|): two weight roundings, four products, three additions, / S, * wd, + offset (<= 9 on a path)"""
    return 10 * EPS32 * mag


def paste64(disp, boxes6, counts, H, W, clamp0=False, masks=None, mis=()):
    """-> (out, bound, covered) [B,H,W]: the max over an image's rois of their pasted maps (0 outside a roi's box; clamp0: max(., 0);
    masks [R,H,W]: times the mask); the bound of a pixel is the largest bound among the rois that cover it"""
    B = len(counts)
    out, bound, covered = np.zeros((B, H, W)), np.zeros((B, H, W)), np.zeros((B, H, W), bool)
    r = 0
    for b, c in enumerate(counts):
        if c == 0:
            continue
        m = np.full((H, W), -np.inf)
        for _ in range(c):
            v = np.zeros((H, W))
            q = roi_value64(disp[r], disp.shape[-1], boxes6[r], H, W, mis)
            if q is not None:
                ys, xs, val, mg = q
                win = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
                v[win] = val
                bound[b][win] = np.maximum(bound[b][win], paste_bound(mg))
                covered[b][win] = True
            if clamp0:
                v = np.maximum(v, 0.0)
            if masks is not None:
                v = v * np.asarray(masks[r], F64)
            m = np.maximum(m, v)
            r += 1
        out[b] = m
    return out, bound, covered


def paste_surely_clamped(disp, boxes6, counts, H, W):
    """[B,H,W] bool: pixels some roi covers where every covering roi's value is negative by more than its bound -- with clamp0 the output
    there is exactly 0, whatever the masks hold"""
    B = len(counts)
    top = np.full((B, H, W), -np.inf)
    r = 0
    for b, c in enumerate(counts):
        for _ in range(c):
            q = roi_value64(disp[r], disp.shape[-1], boxes6[r], H, W)
            if q is not None:
                ys, xs, val, mg = q
                win = (b, slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
                top[win] = np.maximum(top[win], val + paste_bound(mg))
            r += 1
    return np.isfinite(top) & (top < 0)


def depth64(disp, boxes6, fuxb, H, W, mis=()):
    """-> (depth, bound, ok, inside) [R,H,W]: k / (d + 1e-6) inside the box, 0 outside; the paste bound carried through the division:
    k delta_d / d^2 + 2 2^-24 |k / d|; ok = inside and |d + 1e-6| >= 0.05"""
    R = len(boxes6)
    out, bound = np.zeros((R, H, W)), np.zeros((R, H, W))
    ok, inside = np.zeros((R, H, W), bool), np.zeros((R, H, W), bool)
    for r in range(R):
        q = roi_value64(disp[r], disp.shape[-1], boxes6[r], H, W, mis)
        if q is None:
            continue
        ys, xs, val, mg = q
        win = (r, slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
        den = val + 1e-6
        with np.errstate(divide="ignore", invalid="ignore"):
            out[win] = float(fuxb[r]) / den
            bound[win] = float(fuxb[r]) * paste_bound(mg) / den ** 2 + 2 * EPS32 * np.abs(float(fuxb[r]) / den)
        inside[win] = True
        ok[win] = np.abs(den) >= 0.05
    return out, bound, ok, inside


# boxes6 rows: (x1, y1, x2, y2, x1p, x2p)
_PASTE_DEGENERATE = [(3, 4, 4, 12, 1, 2), (6, 2, 15, 3, 2, 11), (18, 9, 19, 10, 15, 16), (22, 14, 24, 16, 20, 22), (8, 8, 14, 15, 2, 12),
                     (-3, 6, 5, 11, -6, 2), (25, 3, 33, 9, 21, 29), (10, -2, 17, 4, 7, 14), (12, 16, 20, 23, 9, 17)]
PASTE_CASES = {
    "degenerateS1": dict(S=1, hw=(20, 30), counts=[5, 4], boxes=_PASTE_DEGENERATE, clamp0=False, masks=False),
    "degenerateS2": dict(S=2, hw=(20, 30), counts=[5, 4], boxes=_PASTE_DEGENERATE, clamp0=False, masks=False),
    "gap": dict(S=6, hw=(20, 30), counts=[2, 0, 3], boxes=[(2, 3, 14, 12, 0, 13), (8, 6, 22, 18, 3, 15), (1, 1, 9, 9, 0, 8), (5, 4, 20, 15, 1, 19),
                                                             (15, 10, 29, 19, 9, 22)], clamp0=True, masks=True),
    "wrap": dict(S=8, hw=(1030, 1024), counts=[1, 2], boxes=[(100, 200, 1000, 1030, 60, 900), (0, 0, 600, 700, 0, 640), (500, 600, 1024, 1030, 380, 930)],
                 clamp0=False, masks=False),
}
DEPTH_CASES = {
    "degenerateS1": dict(S=1, hw=(20, 30), boxes=_PASTE_DEGENERATE),
    "degenerateS2": dict(S=2, hw=(20, 30), boxes=_PASTE_DEGENERATE),
    "gap": dict(S=6, hw=(20, 30), boxes=PASTE_CASES["gap"]["boxes"]),
    "wrap": dict(S=8, hw=(1030, 1024), boxes=PASTE_CASES["wrap"]["boxes"][:2]),
}
FUXB = 389.34


def paste_inputs(name, depth=False):
    c = (DEPTH_CASES if depth else PASTE_CASES)[name]
    R, (H, W) = len(c["boxes"]), c["hw"]
    signed = not depth and c.get("clamp0")
    disp = uniform(f"pp:{name}:d", (R, c["S"], c["S"]), -24.0 if signed else -8.0 if depth else 2.0, 48.0)
    masks = (uniform(f"pp:{name}:m", (R, H, W), 0.0, 1.0) > 0.3).astype(F32) if not depth and c["masks"] else None
    return disp, np.asarray(c["boxes"], np.int32), masks

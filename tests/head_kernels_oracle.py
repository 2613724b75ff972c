"""Plain numpy restatements of the 2D heads' training kernels (csrc/head_train.hip, csrc/srpn_train.hip, the two pack kernels of
csrc/linear.hip) and the cases the host test (tests/test_head_kernels_oracle_host.py) and the GPU tests
(tests/test_hip_head_train_edges.py, tests/test_hip_srpn_train_edges.py, tests/test_hip_srpn_train.py) share.  No GPU; nothing of the code
under test is imported but `hash_uniform`, for inputs.

Every case names the branch it is built for and carries the figures that show it gets there (partial counts, chunk, packed floats, active
count against cap); the host test asserts what is a property of the inputs, the GPU tests ask the library's size queries for the rest.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

F32, F64 = np.float32, np.float64
SENTINEL = np.float32(-1234.5)
SENTINEL_I32 = np.int32(-1234567)


def uniform(key, shape, lo=-1.0, hi=1.0):
    from disprcnn_amd.utils.synth import hash_uniform
    return hash_uniform(key, shape, lo, hi).numpy()


# ------------------------------------------------------------------------------------------------ packed GEMM operands
def pack_rows_np(a):
    """out[(rb * KC + kc) * 256 + (g * 16 + r) * 4 + e] = a[rb * 16 + r][kc * 16 + g * 4 + e], 0 outside R x K"""
    a = np.asarray(a)
    R, K = a.shape
    RB, KC = (R + 15) // 16, (K + 15) // 16
    p = np.zeros((RB * 16, KC * 16), a.dtype)
    p[:R, :K] = a
    return np.ascontiguousarray(p.reshape(RB, 16, KC, 4, 4).transpose(0, 2, 3, 1, 4)).reshape(-1)      # (rb, r, kc, g, e) -> (rb, kc, g, r, e)


def pack_cols_np(a):
    """out[(cb * RC + rc) * 256 + (g * 16 + c) * 4 + e] = a[rc * 16 + g * 4 + e][cb * 16 + c], 0 outside R x K"""
    a = np.asarray(a)
    R, K = a.shape
    RC, CB = (R + 15) // 16, (K + 15) // 16
    p = np.zeros((RC * 16, CB * 16), a.dtype)
    p[:R, :K] = a
    return np.ascontiguousarray(p.reshape(RC, 4, 4, CB, 16).transpose(3, 0, 1, 4, 2)).reshape(-1)      # (rc, g, e, cb, c) -> (cb, rc, g, c, e)


def packed_floats(R, K):
    return ((R + 15) // 16) * ((K + 15) // 16) * 256 if R > 0 and K > 0 else 0


PACK_SMALL = [(1, 1), (15, 17), (16, 16), (17, 15), (37, 72), (3, 5)]
PACK_GRID_FLOATS = 4096 * 256 * 4                          # one trip of the pack kernels' grid: 4096 blocks x 256 threads x one float4
PACK_WRAPPED = [(1030, 4100), (1031, 4099)]                # ragged last block in both axes; K % 4 != 0 is pack_rows' scalar path


@functools.lru_cache(maxsize=None)
def pack_case(R, K):
    a = uniform(f"hk:pack{R}x{K}", (R, K))
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ the engine's blocked layout
def blocked_np(dense, ph, pw, halo=0.0):
    """dense [units, C, H, W] -> float32 [units, CB, H + 2 ph, W + 2 pw, 16]: channel c at [c // 16][..][c % 16], padding channels 0, the
    halo filled with `halo`"""
    n, c, h, w = dense.shape
    cb = (c + 15) // 16
    out = np.full((n, cb, h + 2 * ph, w + 2 * pw, 16), halo, F32)
    p = np.zeros((n, cb * 16, h, w), F32)
    p[:, :c] = dense
    out[:, :, ph: ph + h, pw: pw + w, :] = p.reshape(n, cb, 16, h, w).transpose(0, 1, 3, 4, 2)
    return out


def interior_mask(shape5, ph, pw):
    m = np.zeros(shape5, bool)
    m[:, :, ph: shape5[2] - ph, pw: shape5[3] - pw, :] = True
    return m


# ------------------------------------------------------------------------------------------------ head_train.hip
def scale_of(p):
    """the fp32 1 / (1 - p) the entry hands to its kernels"""
    return F32(1.0) / (F32(1.0) - F32(p))


def relu_dropout_np(x, draws, p, relu):
    """y = max(x, 0) . [draws >= (float)p] / (1 - p): one fp32 product with the fp32 scale; p = 0 ignores draws"""
    v = np.asarray(x, F32)
    if relu:
        v = np.where(v > 0, v, F32(0))
    if p > 0:
        v = np.where(np.asarray(draws, F32) >= F32(p), (v * scale_of(p)).astype(F32), F32(0))
    return v.astype(F32)


def _dz(dy, y, draws, p, relu):
    dy = np.asarray(dy, F32)
    live = np.ones(dy.shape, bool)
    if relu:
        live &= np.asarray(y, F32) > 0                      # -0.0, 0.0 and NaN pass nothing; a positive denormal passes
    if p > 0:
        live &= np.asarray(draws, F32) >= F32(p)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = (dy * scale_of(p)).astype(F32) if p > 0 else dy
    return np.where(live, scaled, F32(0)).astype(F32)       # a select, as torch.where: a masked inf or NaN gives an exact 0


def act_bwd_np(dy, y, draws, p, relu):
    """row-major [M, N] -> (dz fp32, db = the fp64 column sums of that dz, sum |dz| per column in fp64)"""
    dz = _dz(dy, y, draws, p, relu)
    d = dz.astype(F64)
    return dz, d.sum(0), np.abs(d).sum(0)


def act_bwd_blocked_np(dy_b, y_b, relu, ph, pw):
    """blocked [units, CB, Hp, Wp, 16] -> (dz of the same shape, zero outside the interior; db [CB * 16] fp64; sum |dz| per channel).  The
    halo of dy and y is not read."""
    inside = interior_mask(dy_b.shape, ph, pw)
    dz = np.where(inside, _dz(dy_b, y_b, None, 0.0, relu), F32(0)).astype(F32)
    d = dz.astype(F64)
    return dz, d.sum((0, 2, 3)).reshape(-1), np.abs(d).sum((0, 2, 3)).reshape(-1)


def db_bound(ref64, sabs, addends):
    """|db - ref64| <= 2 (2^-24 |ref64| + addends 2^-53 sum|dz|): the kernels round ONE fp64 sum to fp32 (half an fp32 ulp of the result)
    and an fp64 sum of n addends in any order is within (n - 1) 2^-53 sum|.| of the exact one; the factor 2 is the margin"""
    return 2.0 * (2.0 ** -24 * np.abs(ref64) + addends * 2.0 ** -53 * sabs)


K_MAX_PARTS = 1024                                          # head_train.hip: kMaxParts


def rows_split(rows, lanes):
    """(rows per block, partials, rows of the last block) of head_train.hip's rows_per_block_for: the restatement the cases are built on;
    the GPU tests ask the library itself"""
    per = max(-(-rows // K_MAX_PARTS), 16 * lanes)
    per = -(-per // lanes) * lanes
    parts = -(-rows // per)
    return per, parts, rows - (parts - 1) * per


ACT_MODES = [(1, 0.2), (1, 0.0), (0, 0.0), (0, 0.5)]        # (relu, p), as tests/test_hip_roi_heads_train.py
# (M, N, folds, partials, rows of the last block): kMaxParts itself; rows_per_block past its floor of 64 (68, 72); a second column tile
# with one live column
ACT_ROWS_CASES = [(65536, 1, (1,), 1024, 64), (65537, 5, (1, 5), 964, 53), (69633, 1, (1,), 968, 9), (65537, 8, (4,), 964, 53),
                  (260, 65, (1,), 5, 4)]


def act_inputs(tag, shape, p, dy_range=(-2.0, 2.0)):
    dy = uniform(tag + ":dy", shape, *dy_range)
    y = np.maximum(uniform(tag + ":y", shape, -1.0, 1.0), F32(0))
    y.reshape(-1)[3::7] = 0.0                                # exact zeros: no gradient passes
    draws = uniform(tag + ":u", shape, 0.0, 1.0)
    draws.reshape(-1)[::5] = F32(p)                          # a draw exactly equal to p is kept
    return dy, y, draws


@functools.lru_cache(maxsize=None)
def act_rows_case(M, N, relu, p):
    """inputs and the oracle of one row-major case; M > 65536: dy in [0.5, 2], so every live element weighs at least 0.5 in its partial"""
    big = M >= 65536
    dy, y, draws = act_inputs(f"hk:ab{M}x{N}", (M, N), p, (0.5, 2.0) if big else (-2.0, 2.0))
    dz, db, sabs = act_bwd_np(dy, y, draws, p, relu)
    per, parts, last = rows_split(M, 4)
    for a in (dy, y, draws, dz, db, sabs):
        a.setflags(write=False)
    return NS(M=M, N=N, relu=relu, p=p, dy=dy, y=y, draws=draws, dz=dz, db=db, sabs=sabs, per=per, parts=parts, last=last, big=big)


def fold_cols(v, fold):
    return np.asarray(v, F64).reshape(-1, fold).sum(1)


def block_partials(dz, per):
    """the fp64 partial of every row block: [parts, columns]"""
    d = np.asarray(dz, F64)
    parts = -(-d.shape[0] // per)
    pad = np.zeros((parts * per,) + d.shape[1:], F64)
    pad[: d.shape[0]] = d
    return pad.reshape(parts, per, -1).sum(1)


@functools.lru_cache(maxsize=None)
def act_special_case():
    """y holds -0.0 (no gradient) and a positive denormal (gradient passes); dy is +-inf and NaN at masked elements: exact zeros"""
    M, N, p = 9, 7, 0.25
    dy, y, draws = act_inputs("hk:special", (M, N), p)
    y[0, 0], y[0, 1], y[1, 0], y[1, 1] = -0.0, 1e-40, 0.0, 1e-40
    draws[0, :2], draws[1, :2] = 0.9, 0.9                    # kept: the ReLU mask alone decides
    y[2, 0], dy[2, 0] = 0.0, np.inf                          # masked by the ReLU
    y[2, 1], dy[2, 1] = -0.0, -np.inf
    y[3, 0], draws[3, 0], dy[3, 0] = 0.7, 0.1, np.inf        # masked by the dropout
    y[3, 1], draws[3, 1], dy[3, 1] = 0.7, 0.0, -np.inf
    y[4, 0], dy[4, 0] = 0.0, np.nan
    assert np.signbit(y[0, 0]) and 0 < y[0, 1] < np.finfo(F32).tiny
    return NS(M=M, N=N, p=p, dy=dy, y=y, draws=draws, masked=([2, 2, 3, 3, 4], [0, 1, 0, 1, 0]))


# (units, C, H, W, ph, pw, partials): 16 410 rows in chunks of 17 whose edges cross unit edges; a single pixel; W not dividing 16 with a
# halo of 2; the mask head's own shape
ACT_BLOCKED_CASES = [(3, 24, 5470, 3, 0, 1, 966), (1, 16, 1, 1, 0, 0, 1), (5, 40, 7, 5, 2, 2, 3), (2, 16, 14, 14, 1, 1, 2)]


@functools.lru_cache(maxsize=None)
def act_blocked_case(units, C, H, W, ph, pw, relu):
    dy, y, _ = act_inputs(f"hk:abb{units}x{C}x{H}x{W}", (units, C, H, W), 0.0, (0.5, 2.0) if units * H > 16384 else (-2.0, 2.0))
    dy_b, y_b = blocked_np(dy, ph, pw, halo=SENTINEL), blocked_np(y, ph, pw, halo=F32(7.0))     # a halo the kernel must not read
    dz_b, db, sabs = act_bwd_blocked_np(dy_b, y_b, relu, ph, pw)
    per, parts, last = rows_split(units * H, 1)
    return NS(units=units, C=C, H=H, W=W, ph=ph, pw=pw, relu=relu, dy=dy, y=y, dy_b=dy_b, y_b=y_b, dz_b=dz_b, db=db, sabs=sabs, per=per, parts=parts,
              last=last)


RELU_DROPOUT_GRID = 8192 * 256                              # one trip of relu_dropout_fwd_kernel's grid
RELU_DROPOUT_TOTALS = [1, 255, 257, RELU_DROPOUT_GRID + 257]
RELU_DROPOUT_MODES = [(1, 0.2), (0, 0.5), (1, 0.0)]


@functools.lru_cache(maxsize=None)
def relu_dropout_case(total, p):
    x = uniform(f"hk:rd{total}:x", (1, total), -1.0, 1.0)
    draws = uniform(f"hk:rd{total}:u", (1, total), 0.0, 1.0)
    draws.reshape(-1)[::5] = F32(p)
    x.setflags(write=False), draws.setflags(write=False)
    return x, draws


# ------------------------------------------------------------------------------------------------ srpn_train.hip
SCAN_THREADS = 1024                                         # srpn_train.hip: kScanThreads


def pix_offsets(shapes):
    off = [0]
    for h, w in shapes:
        off.append(off[-1] + h * w)
    return off


def chunk_of(shapes):
    """pixels per thread of active_pixels_kernel"""
    return -(-pix_offsets(shapes)[-1] // SCAN_THREADS)


def level_of(shapes, q):
    off = pix_offsets(shapes)
    return max(k for k in range(len(shapes)) if q >= off[k])


def row_coords(row_pix, shapes, cap):
    """(row, image, level, y, x, flat pixel of the level) of every live row"""
    off = pix_offsets(shapes)
    for r, q in enumerate(np.asarray(row_pix).tolist()):
        if q >= 0:
            l = level_of(shapes, q)
            y, x = divmod(q - off[l], shapes[l][1])
            yield r, r // cap, l, y, x, q - off[l]


def active_pixels_np(pos, neg, N, A, shapes, cap):
    """drc_srpn_active_pixels: the first `cap` active pixels of every image in ascending (level, y, x) -> (row_pix [N * cap], -1 past the
    count; counts [N]; index, level-major [level][image][pixel], the row or -1)"""
    off = pix_offsets(shapes)
    P = off[-1]
    on = (np.asarray(pos).astype(bool) | np.asarray(neg).astype(bool)).reshape(N, P, A).any(2)
    row_pix, counts, index = -np.ones(N * cap, np.int32), np.zeros(N, np.int32), -np.ones((N, P), np.int32)
    for i in range(N):
        q = np.nonzero(on[i])[0][:cap]
        row_pix[i * cap: i * cap + len(q)], counts[i] = q, len(q)
        index[i, q] = i * cap + np.arange(len(q))
    flat = np.concatenate([index[:, a:b].reshape(-1) for a, b in zip(off[:-1], off[1:])])
    return row_pix, counts, flat


def gather_rows_np(row_pix, N, A, C, cap, shapes, hidden=None, feats=None, grads=None, s_obj=None, s_box=None):
    """drc_srpn_gather_rows on dense maps: hidden per level [N, 4C, H, W] -> T [N cap, 4C]; feats (left, right) per level [N, C, H, W] ->
    Xcol [2 N cap, 9C], (c, ky, kx) columns, zeros outside the map, the left rows then the right rows; grads (glogits [N, 2A, H, W],
    gbbox [N, 6A, H, W]) -> G [N cap, 8A], one fp32 product with s_obj / s_box (None: 0).  Rows past an image's count are zero rows."""
    R = N * cap
    T = np.zeros((R, 4 * C), F32) if hidden is not None else None
    X = np.zeros((2 * R, 9 * C), F32) if feats is not None else None
    G = np.zeros((R, 8 * A), F32) if grads is not None else None
    if feats is not None:
        padded = [[np.pad(np.asarray(f, F32), ((0, 0), (0, 0), (1, 1), (1, 1))) for f in side] for side in feats]
    so, sb = F32(0 if s_obj is None else s_obj), F32(0 if s_box is None else s_box)
    for r, img, l, y, x, _ in row_coords(row_pix, shapes, cap):
        if T is not None:
            T[r] = hidden[l][img, :, y, x]
        if X is not None:
            for view in range(2):
                X[view * R + r] = padded[view][l][img, :, y: y + 3, x: x + 3].reshape(-1)
        if G is not None:
            G[r, : 2 * A] = np.asarray(grads[0][l], F32)[img, :, y, x] * so
            G[r, 2 * A:] = np.asarray(grads[1][l], F32)[img, :, y, x] * sb
    return T, X, G


def col2im_np(dxcol, row_pix, N, C, cap, shapes, dtype):
    """drc_srpn_col2im in `dtype`: [view][level] maps [N, C, H, W]; every element adds its at most nine taps in ascending (ky, kx), one
    addition each"""
    R = N * cap
    dxcol = np.asarray(dxcol).reshape(2, R, C, 9)
    ref = [[np.zeros((N, C, h, w), dtype) for h, w in shapes] for _ in range(2)]
    rows = list(row_coords(row_pix, shapes, cap))
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        for r, img, l, y, x, _ in rows:
            h, w = shapes[l]
            yy, xx = y + ky - 1, x + kx - 1
            if 0 <= yy < h and 0 <= xx < w:
                for view in range(2):
                    ref[view][l][img, :, yy, xx] += dxcol[view, r, :, tap].astype(dtype)
    return ref


# ---- the masks of tests/test_hip_srpn_train.py
def set_anchor(mask, shapes, A, lvl, y, x, a):
    h, w = shapes[lvl]
    assert 0 <= y < h and 0 <= x < w and 0 <= a < A
    mask[(pix_offsets(shapes)[lvl] + y * w + x) * A + a] = 1


def image_a(shapes, A, cap):
    """a positive and a negative on one pixel, three anchors on the pixel to its right, the pixels below and diagonally below (horizontal,
    vertical and diagonal neighbours), then the four corners of every level from the last level down while `cap` distinct pixels hold
    them; the last level's bottom-right corner carries the LAST anchor of the last level"""
    P = pix_offsets(shapes)[-1]
    pos, neg = np.zeros(P * A, np.uint8), np.zeros(P * A, np.uint8)
    set_anchor(pos, shapes, A, 0, 1, 1, 0), set_anchor(neg, shapes, A, 0, 1, 1, A - 1)
    for a in range(A):
        set_anchor(neg if a % 2 else pos, shapes, A, 0, 1, 2, a)
    set_anchor(neg, shapes, A, 0, 2, 1, 1 % A), set_anchor(pos, shapes, A, 0, 2, 2, 0)
    used = 4
    for lvl in reversed(range(len(shapes))):
        h, w = shapes[lvl]
        if used + 4 > cap:
            break
        for k, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
            set_anchor(pos if k % 2 else neg, shapes, A, lvl, y, x, A - 1 if k == 3 else k % A)
        used += 4
    return pos, neg, used


def image_full(shapes, A, cap):
    """exactly `cap` anchors on `cap` distinct pixels"""
    P = pix_offsets(shapes)[-1]
    assert 3 * cap + 1 <= P
    pos, neg = np.zeros(P * A, np.uint8), np.zeros(P * A, np.uint8)
    for k in range(cap):
        (pos if k % 3 else neg)[(3 * k + 1) * A + k % A] = 1
    return pos, neg


def image_none(shapes, A):
    P = pix_offsets(shapes)[-1]
    return np.zeros(P * A, np.uint8), np.zeros(P * A, np.uint8)


def batch_masks(which, N, shapes, A, cap):
    """call 0: [image_a] or [image_a, none]; call 1 (other masks, the same buffers): [exactly cap] or [exactly cap, image_a]"""
    a = image_a(shapes, A, cap)[:2]
    imgs = ([a, image_none(shapes, A)] if which == 0 else [image_full(shapes, A, cap), a])[:N]
    return np.concatenate([p for p, _ in imgs]), np.concatenate([n for _, n in imgs])


# ---- active pixels: chunk 3 with level edges inside a thread's chunk, chunk 5 on one level, and the shape of the existing test (chunk 1)
ACTIVE_PYRAMIDS = {"five": [(40, 52), (20, 26), (10, 13), (5, 7), (3, 4)], "one": [(64, 65)], "small": [(24, 40)]}
ACTIVE_CASES = [(pyr, A, which) for pyr in ("five", "one") for A in (1, 3) for which in "abcde"] + [("small", 3, "f")]
ACTIVE_CAPS = dict(a=8, b=8, c=1, d=0, e=1100, f=8)
STRADDLE_THREAD = 700                                       # the thread whose chunk holds the 8th and the 9th active pixel of case (a)


def image_of_pixels(shapes, A, pixels):
    """one anchor on every pixel of `pixels`, positives and negatives in turn, the anchor walking over 0 .. A - 1; the first pixel carries a
    positive and a negative"""
    P = pix_offsets(shapes)[-1]
    pos, neg = np.zeros(P * A, np.uint8), np.zeros(P * A, np.uint8)
    for k, q in enumerate(pixels):
        (neg if k % 2 else pos)[q * A + k % A] = 1
    if len(pixels):
        neg[pixels[0] * A + A - 1] = 1
    return pos, neg


def pixels_a(shapes):
    """11 pixels: thread 0's first and last pixel, thread 1's first, both sides of a level edge (of a third of the map on one level), the
    8th and the 9th in the chunk of thread STRADDLE_THREAD, the last two pixels of the last level"""
    off, chunk = pix_offsets(shapes), chunk_of(shapes)
    P = off[-1]
    edge = off[1] if len(shapes) > 1 else P // 3
    b = STRADDLE_THREAD * chunk
    return [0, chunk - 1, chunk, 7 * chunk + 1, edge - 1, edge, edge + chunk, b, b + 1, P - 2, P - 1]


def active_case(pyr, A, which):
    """-> (shapes, cap, [first call's (pos, neg), second call's (pos, neg)]) for N = 2 images that differ"""
    shapes, cap = ACTIVE_PYRAMIDS[pyr], ACTIVE_CAPS[which]
    P = pix_offsets(shapes)[-1]
    if which == "f":
        return shapes, cap, [batch_masks(0, 2, shapes, A, cap), batch_masks(1, 2, shapes, A, cap)]
    if which in "acd":
        imgs = [image_of_pixels(shapes, A, pixels_a(shapes)), image_of_pixels(shapes, A, [3, P - 1])]
    elif which == "b":
        imgs = [image_of_pixels(shapes, A, list(range(P))), image_of_pixels(shapes, A, list(range(2, P)))]
    else:
        imgs = [image_of_pixels(shapes, A, [1, 2 * chunk_of(shapes), P // 2, P - 3, P - 1]), image_none(shapes, A)]
    cat = lambda two: (np.concatenate([two[0][0], two[1][0]]), np.concatenate([two[0][1], two[1][1]]))
    return shapes, cap, [cat(imgs), cat(imgs[::-1])]


def active_counts(pos, neg, N, A, shapes):
    P = pix_offsets(shapes)[-1]
    return (pos.astype(bool) | neg.astype(bool)).reshape(N, P, A).any(2).sum(1)


# ---- gather rows: all four corners of the first level, both ends of the one-pixel-high level, zero rows past the counts
GATHER_SHAPES, GATHER_N, GATHER_CAP = [(6, 10), (1, 7)], 2, 10
GATHER_PIXELS = [[0, 9, 23, 50, 59, 60, 66], [24, 66]]       # per image; 60 .. 66 are the second level
GATHER_C = [72, 32]                                         # 9C = 648, 4C = 288: both loops wrap, ragged; 9C = 288, 4C = 128: Xcol alone wraps
GATHER_A_WIDE = 33                                          # 8A = 264: G's loop wraps


def gather_row_pix(A):
    pos = np.concatenate([image_of_pixels(GATHER_SHAPES, A, px)[0] for px in GATHER_PIXELS])
    neg = np.concatenate([image_of_pixels(GATHER_SHAPES, A, px)[1] for px in GATHER_PIXELS])
    return active_pixels_np(pos, neg, GATHER_N, A, GATHER_SHAPES, GATHER_CAP)


@functools.lru_cache(maxsize=None)
def gather_case(C, A):
    N, shapes = GATHER_N, GATHER_SHAPES
    row_pix, counts, _ = gather_row_pix(A)
    mk = lambda what, ch: [uniform(f"hk:gr{C}x{A}:{what}{l}", (N, ch, h, w)) for l, (h, w) in enumerate(shapes)]
    return NS(C=C, A=A, row_pix=row_pix, counts=counts, hidden=mk("h", 4 * C), left=mk("l", C), right=mk("r", C), gz=mk("gz", 2 * A), gb=mk("gb", 6 * A),
              s_obj=F32(0.37), s_box=F32(-1.9))


# ---- col2im: hw on a 256-pixel block, one past it, a level one pixel wide, a single pixel
COL2IM_SHAPES, COL2IM_N, COL2IM_CAP = [(16, 16), (1, 257), (5, 1), (1, 1)], 2, 12
COL2IM_PIXELS = [[0, 119, 120, 135, 255, 256 + 255, 256 + 256, 513, 517, 518], [256 + 254, 518]]
COL2IM_C = [8, 40]


@functools.lru_cache(maxsize=None)
def col2im_case(C):
    N, shapes, cap, A = COL2IM_N, COL2IM_SHAPES, COL2IM_CAP, 1
    pos = np.concatenate([image_of_pixels(shapes, A, px)[0] for px in COL2IM_PIXELS])
    neg = np.concatenate([image_of_pixels(shapes, A, px)[1] for px in COL2IM_PIXELS])
    row_pix, counts, index = active_pixels_np(pos, neg, N, A, shapes, cap)
    dxcol = uniform(f"hk:c2i{C}", (2 * N * cap, 9 * C), -2.0, 2.0)
    ref64, ref32 = col2im_np(dxcol, row_pix, N, C, cap, shapes, F64), col2im_np(dxcol, row_pix, N, C, cap, shapes, F32)
    return NS(C=C, A=A, row_pix=row_pix, counts=counts, index=index, dxcol=dxcol, ref64=ref64, ref32=ref32)

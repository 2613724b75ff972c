"""NumPy restatement of PointRCNN's 3D box ops (point_rcnn/lib/utils/iou3d/src/iou3d_kernel.cu, iou3d.cpp, iou3d_utils.py,
roipool3d/src/roipool3d_kernel.cu), fp32 arithmetic in the kernels' order, vectorised over pairs (every element still sees the scalar
expression).  Plus an independent fp64 geometry check: a Sutherland-Hodgman clip of two rotated rectangles.

Shared by tests/test_box3d_host.py (hand-computed cases, the golden) and tests/test_hip_box3d.py (vs the HIP kernels)."""
import math

import numpy as np

F = np.float32
EPS = F(1e-8)
MARGIN = F(1e-5)


def _geom(b):
    """[N,5] boxes -> the per-box quantities box_overlap derives (fp32)."""
    b = np.asarray(b, F).reshape(-1, 5)
    x1, y1, x2, y2, ry = (b[:, k] for k in range(5))
    cx, cy = (x1 + x2) / F(2), (y1 + y2) / F(2)
    c, s = np.cos(ry), np.sin(ry)
    xs, ys = (x1, x2, x2, x1), (y1, y1, y2, y2)
    px = [(xs[k] - cx) * c + (ys[k] - cy) * s + cx for k in range(4)]
    py = [-(xs[k] - cx) * s + (ys[k] - cy) * c + cy for k in range(4)]
    return dict(x1=x1, y1=y1, x2=x2, y2=y2, cx=cx, cy=cy, cn=np.cos(-ry), sn=np.sin(-ry), px=px, py=py, area=(x2 - x1) * (y2 - y1))


def _take(g, idx):
    return {k: ([a[idx] for a in v] if isinstance(v, list) else v[idx]) for k, v in g.items()}


def _in_box(g, x, y):
    rx = (x - g["cx"]) * g["cn"] + (y - g["cy"]) * g["sn"] + g["cx"]
    ry = -(x - g["cx"]) * g["sn"] + (y - g["cy"]) * g["cn"] + g["cy"]
    return (rx > g["x1"] - MARGIN) & (rx < g["x2"] + MARGIN) & (ry > g["y1"] - MARGIN) & (ry < g["y2"] + MARGIN)


def _cross3(p1x, p1y, p2x, p2y, p0x, p0y):
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y)


def _intersection(p1x, p1y, p0x, p0y, q1x, q1y, q0x, q0y):
    ok = (np.minimum(p0x, p1x) <= np.maximum(q0x, q1x)) & (np.minimum(q0x, q1x) <= np.maximum(p0x, p1x)) & \
         (np.minimum(p0y, p1y) <= np.maximum(q0y, q1y)) & (np.minimum(q0y, q1y) <= np.maximum(p0y, p1y))
    s1 = _cross3(q0x, q0y, p1x, p1y, p0x, p0y)
    s2 = _cross3(p1x, p1y, q1x, q1y, p0x, p0y)
    s3 = _cross3(p0x, p0y, q1x, q1y, q0x, q0y)
    s4 = _cross3(q1x, q1y, p1x, p1y, q0x, q0y)
    ok &= (s1 * s2 > 0) & (s3 * s4 > 0)
    s5 = _cross3(q1x, q1y, p1x, p1y, p0x, p0y)
    a0, b0, c0 = p0y - p1y, p1x - p0x, p0x * p1y - p1x * p0y
    a1, b1, c1 = q0y - q1y, q1x - q0x, q0x * q1y - q1x * q0y
    D = a0 * b1 - a1 * b0
    far = np.abs(s5 - s1) > EPS
    ax = np.where(far, (s5 * q0x - s1 * q1x) / (s5 - s1), (b0 * c1 - b1 * c0) / D)
    ay = np.where(far, (s5 * q0y - s1 * q1y) / (s5 - s1), (a1 * c0 - a0 * c1) / D)
    return ok, ax.astype(F), ay.astype(F)


def _overlap_pairs(A, B):
    """box_overlap of pairs (A[p], B[p])."""
    P = A["x1"].shape[0]
    qx, qy = np.zeros((P, 24), F), np.zeros((P, 24), F)
    cnt = np.zeros(P, np.int64)
    sx, sy = np.zeros(P, F), np.zeros(P, F)
    rows = np.arange(P)

    def append(ok, x, y):
        nonlocal sx, sy
        r = rows[ok]
        qx[r, cnt[r]], qy[r, cnt[r]] = x[ok], y[ok]
        sx = np.where(ok, sx + x, sx).astype(F)
        sy = np.where(ok, sy + y, sy).astype(F)
        cnt[ok] += 1

    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                i1, j1 = (i + 1) % 4, (j + 1) % 4
                ok, x, y = _intersection(A["px"][i1], A["py"][i1], A["px"][i], A["py"][i], B["px"][j1], B["py"][j1], B["px"][j], B["py"][j])
                append(ok, x, y)
        for k in range(4):
            append(_in_box(A, B["px"][k], B["py"][k]), B["px"][k], B["py"][k])
            append(_in_box(B, A["px"][k], A["py"][k]), A["px"][k], A["py"][k])
        cf = cnt.astype(F)
        cx, cy = (sx / cf).astype(F), (sy / cf).astype(F)
        key = np.arctan2(qy - cy[:, None], qx - cx[:, None]).astype(F)
    for j in range(23):                                  # the reference's bubble sort, literally
        for i in range(23 - j):
            sw = (i < cnt - j - 1) & (key[:, i] > key[:, i + 1])
            if sw.any():
                for a in (qx, qy, key):
                    a[sw, i], a[sw, i + 1] = a[sw, i + 1].copy(), a[sw, i].copy()
    area = np.zeros(P, F)
    for k in range(23):
        live = k < cnt - 1
        if not live.any():
            break
        ax, ay = qx[:, k] - qx[:, 0], qy[:, k] - qy[:, 0]
        bx, by = qx[:, k + 1] - qx[:, 0], qy[:, k + 1] - qy[:, 0]
        area = np.where(live, area + (ax * by - ay * bx), area).astype(F)
    return (np.abs(area).astype(np.float64) / 2.0).astype(F)


def _pairwise(a, b, fn):
    a, b = np.asarray(a, F).reshape(-1, 5), np.asarray(b, F).reshape(-1, 5)
    na, nb = a.shape[0], b.shape[0]
    if na == 0 or nb == 0:
        return np.zeros((na, nb), F)
    ia, ib = np.repeat(np.arange(na), nb), np.tile(np.arange(nb), na)
    ga, gb = _geom(a), _geom(b)
    return fn(_take(ga, ia), _take(gb, ib)).reshape(na, nb)


def _iou_pairs(A, B):
    s = _overlap_pairs(A, B)
    return (s / np.maximum(A["area"] + B["area"] - s, EPS)).astype(F)


def _iou_normal_pairs(A, B):
    left, right = np.maximum(A["x1"], B["x1"]), np.minimum(A["x2"], B["x2"])
    top, bottom = np.maximum(A["y1"], B["y1"]), np.minimum(A["y2"], B["y2"])
    inter = np.maximum(right - left, F(0)) * np.maximum(bottom - top, F(0))
    return (inter / np.maximum(A["area"] + B["area"] - inter, EPS)).astype(F)


def box_overlap(a, b):
    """[Na,5], [Nb,5] [x1,y1,x2,y2,ry] -> [Na,Nb] rotated overlap areas (box_overlap(a_i, b_j))."""
    return _pairwise(a, b, _overlap_pairs)


def iou_bev(a, b):
    return _pairwise(a, b, _iou_pairs)


def iou_normal(a, b):
    return _pairwise(a, b, _iou_normal_pairs)


def boxes3d_to_bev(b7):
    b7 = np.asarray(b7, F).reshape(-1, 7)
    half_l, half_w = b7[:, 5] / F(2), b7[:, 4] / F(2)
    return np.stack([b7[:, 0] - half_l, b7[:, 2] - half_w, b7[:, 0] + half_l, b7[:, 2] + half_w, b7[:, 6]], 1).astype(F)


def iou3d(a7, b7):
    """boxes_iou3d_gpu: [Na,7], [Nb,7] [x,y,z,h,w,l,ry] -> [Na,Nb], the torch steps in their fp32 order."""
    a7, b7 = np.asarray(a7, F).reshape(-1, 7), np.asarray(b7, F).reshape(-1, 7)
    ov = box_overlap(boxes3d_to_bev(a7), boxes3d_to_bev(b7))
    amin, amax = (a7[:, 1] - a7[:, 3])[:, None], a7[:, 1][:, None]
    bmin, bmax = (b7[:, 1] - b7[:, 3])[None, :], b7[:, 1][None, :]
    oh = np.maximum(np.minimum(amax, bmax) - np.maximum(amin, bmin), F(0))
    o3 = ov * oh
    va, vb = (a7[:, 3] * a7[:, 4] * a7[:, 5])[:, None], (b7[:, 3] * b7[:, 4] * b7[:, 5])[None, :]
    return (o3 / np.maximum(va + vb - o3, F(1e-7))).astype(F)


def nms_sorted(boxes, thresh, normal=False, max_keep=-1):
    """iou3d.cpp's nms_gpu / nms_normal_gpu on boxes ALREADY in score order: the kept positions.  Row i's mask word compares box i
    (as box_a) with every later box j (as box_b) with `> thresh`; the greedy walk keeps i unless an earlier kept box removed it."""
    boxes = np.asarray(boxes, F).reshape(-1, 5)
    n = boxes.shape[0]
    thresh = F(thresh)
    g = _geom(boxes)
    fn = _iou_normal_pairs if normal else _iou_pairs
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if 0 < max_keep <= len(keep):
            break
        if i + 1 < n:
            j = np.arange(i + 1, n)
            removed[j] |= fn(_take(g, np.full(j.size, i)), _take(g, j)) > thresh
    return np.asarray(keep, np.int64)


def nms(boxes, scores, thresh, normal=False, max_keep=-1):
    """iou3d_utils.nms_gpu with a STABLE descending sort: original indices of the kept boxes, in score order."""
    order = np.argsort(-np.asarray(scores, F), kind="stable")
    return order[nms_sorted(np.asarray(boxes, F)[order], thresh, normal, max_keep)]


# ---- roipool3d
def pts_in_boxes3d(pts, boxes3d):
    """pt_in_box3d (max_dis 10, h/l/w halves in double, float cos/sin): pts [N,3], boxes [M,7] -> [M,N] bool."""
    p = np.asarray(pts, F).reshape(-1, 3)
    b = np.asarray(boxes3d, F).reshape(-1, 7)
    x, y, z = (p[None, :, k] for k in range(3))
    cx, by, cz, h, w, l, ang = (b[:, k:k + 1] for k in range(7))
    cy = (by.astype(np.float64) - h.astype(np.float64) / 2.0).astype(F)
    h2 = h.astype(np.float64) / 2.0
    near = ~((np.abs(x - cx) > F(10)) | (np.abs(y - cy).astype(np.float64) > h2) | (np.abs(z - cz) > F(10)))
    cosa, sina = np.cos(ang), np.sin(ang)
    x_rot = ((x - cx) * cosa + (z - cz) * (-sina)).astype(np.float64)
    z_rot = ((x - cx) * sina + (z - cz) * cosa).astype(np.float64)
    l64, w64 = l.astype(np.float64), w.astype(np.float64)
    inside = (x_rot >= -l64 / 2.0) & (x_rot <= l64 / 2.0) & (z_rot >= -w64 / 2.0) & (z_rot <= w64 / 2.0)
    return near & inside


def pooled_idx(flags, S):
    """get_pooled_idx of one box set: flags [M,N] -> idx [M,S] (first S in-box points, repeated cyclically), empty [M]."""
    M = flags.shape[0]
    idx = np.zeros((M, S), np.int64)
    empty = np.zeros(M, np.int32)
    for m in range(M):
        hit = np.nonzero(flags[m])[0][:S]
        if hit.size == 0:
            empty[m] = 1
        elif S:
            idx[m] = hit[np.arange(S) % hit.size]
    return idx, empty


def enlarge_box3d(boxes3d, extra_width):
    b = np.array(boxes3d, F, copy=True)
    b[:, 3:6] = b[:, 3:6] + F(extra_width * 2)
    b[:, 1] = b[:, 1] + F(extra_width)
    return b


def roipool3d(pts, feat, boxes3d, pool_extra_width, S=512):
    """roipool3d_gpu: pts [B,N,3], feat [B,N,C], boxes [B,M,7] -> pooled [B,M,S,3+C], empty [B,M] int32."""
    pts, feat, boxes3d = np.asarray(pts, F), np.asarray(feat, F), np.asarray(boxes3d, F)
    B, M, C = pts.shape[0], boxes3d.shape[1], feat.shape[2]
    pooled = np.zeros((B, M, S, 3 + C), F)
    empty = np.zeros((B, M), np.int32)
    for b in range(B):
        bx = enlarge_box3d(boxes3d[b], pool_extra_width)
        idx, empty[b] = pooled_idx(pts_in_boxes3d(pts[b], bx), S)
        rows = np.concatenate([pts[b], feat[b]], 1)
        for m in range(M):
            if not empty[b, m]:
                pooled[b, m] = rows[idx[m]]
    return pooled, empty


# ---- independent fp64 geometry
def rect_corners64(box):
    """[x1,y1,x2,y2,ry] -> its 4 corners rotated about the centre (fp64), counter-clockwise for ry = 0 in (x, y)."""
    x1, y1, x2, y2, ry = (float(v) for v in box)
    cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    c, s = math.cos(ry), math.sin(ry)
    return [((x - cx) * c + (y - cy) * s + cx, -(x - cx) * s + (y - cy) * c + cy) for x, y in ((x1, y1), (x2, y1), (x2, y2), (x1, y2))]


def _signed_area(poly):
    return 0.5 * sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1] for k in range(len(poly)))


def clip_overlap64(a, b):
    """Area of the intersection of two rotated rectangles: Sutherland-Hodgman clip of a by b, all in fp64."""
    subj, clip = rect_corners64(a), rect_corners64(b)
    if _signed_area(clip) < 0:
        clip = clip[::-1]
    if abs(_signed_area(clip)) == 0 or abs(_signed_area(subj)) == 0:
        return 0.0
    out = subj
    for k in range(4):
        (ex, ey), (fx, fy) = clip[k], clip[(k + 1) % 4]

        def side(p):
            return (fx - ex) * (p[1] - ey) - (fy - ey) * (p[0] - ex)
        inp, out = out, []
        for m in range(len(inp)):
            p, q = inp[m], inp[(m + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            return 0.0
    return abs(_signed_area(out)) if len(out) >= 3 else 0.0

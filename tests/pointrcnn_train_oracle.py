"""fp64 NumPy restatement of what PointRCNN.process_input does to the matched ground-truth boxes (reference point_rcnn.py:141-186): the
seven numbers scaled and flipped, Box3DList's corners, the rotation about y into the cloud frame and the mean subtracted, the way back,
the per-point regression labels, and each point's margin to the faces of its box; plus the loader of the golden scene
(tests/golden/pointrcnn_train_input_golden.npz) shared by the tests and tools.

Used by tests/golden/make_golden_pointrcnn_train_input.py (to place the boxes clear of every drawn point) and by the GPU tests, where
the reference's own fp32 error against these functions sets the bound.
"""
import os
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pointrcnn_train_input_golden.npz")


def augment_box7(box7, scale, flip):
    """(G,7) 'xyzhwl_ry' -> scaled ([:6] * scale; the reference multiplies fp32 by the scale rounded to fp32) and flipped (x = -x,
    ry = sign(ry) * pi - ry)"""
    b = np.asarray(box7, np.float64).copy()
    b[:, 0:6] *= float(np.float32(scale))
    if flip:
        b[:, 0] = -b[:, 0]
        b[:, 6] = np.sign(b[:, 6]) * float(np.float32(np.pi)) - b[:, 6]
    return b


def corners_of(box7):
    """(G,7) 'xyzhwl_ry' -> (G,8,3), Box3DList's corner order"""
    b = np.asarray(box7, np.float64)
    x, y, z, h, w, l, ry = (b[:, i] for i in range(7))
    xc = np.stack([-l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2], 1)
    yc = np.stack([0 * h, -h, -h, 0 * h, 0 * h, -h, -h, 0 * h], 1)
    zc = np.stack([w / 2, w / 2, w / 2, w / 2, -w / 2, -w / 2, -w / 2, -w / 2], 1)
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    return np.stack([c * xc + s * zc + x[:, None], yc + y[:, None], -s * xc + c * zc + z[:, None]], 2)


def box7_of(corners):
    """(G,8,3) -> (G,7) 'xyzhwl_ry' as Box3DList.convert does"""
    c = np.asarray(corners, np.float64)
    dif = c[:, 3] - c[:, 0]
    ry = -np.arctan2(dif[:, 2], dif[:, 0])
    xyz = (c[:, 7] + c[:, 0]) / 2
    l = np.linalg.norm(c[:, 0] - c[:, 3], axis=1)
    h = np.linalg.norm(c[:, 0] - c[:, 1], axis=1)
    w = np.linalg.norm(c[:, 0] - c[:, 4], axis=1)
    return np.concatenate([xyz, h[:, None], w[:, None], l[:, None], ry[:, None]], 1)


def rotate(p, ang):
    """rotate_pc_along_y: (R,K,3) by ang (R): x' = x cos - z sin, z' = x sin + z cos"""
    p = np.asarray(p, np.float64)
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    return np.stack([p[..., 0] * c - p[..., 2] * s, p[..., 1], p[..., 0] * s + p[..., 2] * c], -1)


def to_cloud_frame(box7, scale, flip, rot, mean):
    """the matched boxes (R,7) in the camera frame -> their corners (R,8,3) in the cloud frame; rot: the signed angle"""
    return rotate(corners_of(augment_box7(box7, scale, flip)), np.asarray(rot, np.float64)) - np.asarray(mean, np.float64)[:, None]


def to_camera_frame(corners, rot, mean):
    """the way back: (corners + mean) rotated by -rot"""
    return rotate(np.asarray(corners, np.float64) + np.asarray(mean, np.float64)[:, None], -np.asarray(rot, np.float64))


def enlarge(box7, extra):
    b = np.asarray(box7, np.float64).copy()
    b[:, 3:6] += 2 * extra
    b[:, 1] += extra
    return b


def face_coordinates(corners, pts):
    """filter_bbox_3d's three projections, normalised: (R,8,3), (R,N,3) -> (R,N,3) with a point inside iff all three lie in (0, 1)"""
    c = np.asarray(corners, np.float64)
    p = np.asarray(pts, np.float64) - c[:, None, 4]
    out = []
    for v in (c[:, 5] - c[:, 4], c[:, 0] - c[:, 4], c[:, 7] - c[:, 4]):
        out.append((p * v[:, None]).sum(2) / (v * v).sum(1)[:, None])
    return np.stack(out, 2)


def face_margin(corners, pts):
    """(R,N): the distance, in units of the box's size along that axis, of each point to the nearest face of the box; a face is the
    finite rectangle, so a point counts only where it lies within the box's extent (grown by the same margin) along the other two axes.
    A label can flip under rounding only where this is tiny."""
    t = face_coordinates(corners, pts)
    plane = np.minimum(np.abs(t), np.abs(t - 1))                        # to the two planes of each axis
    outside = np.maximum(np.maximum(-t, t - 1), 0)                      # how far outside the slab of each axis
    m = np.full(t.shape[:2], np.inf)
    for a in range(3):
        others = [b for b in range(3) if b != a]
        m = np.minimum(m, np.maximum(plane[..., a], np.maximum(outside[..., others[0]], outside[..., others[1]])))
    return m


def labels(corners, pts, cls_label):
    """reg_label (R,N,7) on the foreground points of cls_label: centre (at half height) - p, h, w, l, ry of the cloud-frame box"""
    b = box7_of(corners)
    p = np.asarray(pts, np.float64)
    reg = np.zeros(p.shape[:2] + (7,))
    centre = b[:, 0:3].copy()
    centre[:, 1] -= b[:, 3] / 2
    fg = np.asarray(cls_label) == 1
    reg[..., 0:3] = centre[:, None] - p
    reg[..., 3:7] = b[:, None, 3:7]
    reg[~fg] = 0
    return reg


def cls_labels(corners, corners_large, pts):
    t, tl = face_coordinates(corners, pts), face_coordinates(corners_large, pts)
    inside = ((t > 0) & (t < 1)).all(2)
    inside_large = ((tl > 0) & (tl < 1)).all(2)
    cls = np.zeros(inside.shape)
    cls[inside] = 1
    cls[inside_large != inside] = -1
    return cls


# ---- the golden scene as this package's structures
def scene(g, dev, with_empty_image=True):
    """-> left, right, targets (per-image BoxLists on `dev`; the targets carry box3d 'xyzhwl_ry' and calib)"""
    import torch

    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    from disprcnn_amd.structures.calib import Calib
    W, H = int(g["W"]), int(g["H"])
    left, right, targets, r, q = [], [], [], 0, 0
    n_img = len(g["rois_per_image"]) if with_empty_image else int((g["gts_per_image"] > 0).sum())
    for i in range(n_img):
        n, k = int(g["rois_per_image"][i]), int(g["gts_per_image"][i])
        lb = BoxList(torch.from_numpy(g["left_boxes"][r:r + n]).to(dev), (W, H))
        lb.add_field("disparity", torch.from_numpy(g["disparity"][r:r + n]).to(dev))
        lb.add_field("mask", torch.from_numpy(g["mask"][r:r + n]).to(dev))
        lb.add_field("scores", torch.ones(n, device=dev))
        left.append(lb)
        right.append(BoxList(torch.from_numpy(g["right_boxes"][r:r + n]).to(dev), (W, H)))
        t = BoxList(torch.from_numpy(g["gt_boxes"][q:q + k]).reshape(-1, 4).to(dev), (W, H))
        t.add_field("box3d", Box3DList(torch.from_numpy(g["gt_box3d"][q:q + k]).reshape(-1, 7).to(dev), (W, H), "xyzhwl_ry"))
        t.add_field("calib", Calib(SimpleNamespace(P2=g["P2s"][i], P3=g["P3s"][i]), (W, H)))
        targets.append(t)
        r += n
        q += k
    return left, right, targets


def matched_rows(g):
    """(R,7): the camera-frame box each kept cloud was matched to (the index clamped at 0), from the fixture's inputs and matched_idxs"""
    first = np.concatenate([[0], np.cumsum(g["gts_per_image"])])
    rows = []
    for img, m in zip(g["cloud_image"], g["matched_idxs"]):
        rows.append(g["gt_box3d"][first[img] + max(int(m), 0)])
    return np.stack(rows).astype(np.float64)


# ---- random cases of the 2D matching kernel
MATCH_SEED, MATCH_HIGH, MATCH_LOW = 3, 0.6, 0.3
MATCH_PROPOSALS, MATCH_GTS = (0, 65, 20), (3, 1, 2)         # an image without proposals, one ground truth, one more proposal than a wave


def matching_case(seed=MATCH_SEED):
    """-> per image (proposals (n,4), ground truths (g,4), rows (g,7)) fp32: ground truths over a 300 x 200 area, proposals that are
    shifted and resized copies of one of them (IoUs spread over [0, 1]) or unrelated boxes"""
    rs = np.random.RandomState(seed)
    out = []
    for n, g in zip(MATCH_PROPOSALS, MATCH_GTS):
        xy = rs.uniform(0, 200, (g, 2))
        wh = rs.uniform(20, 90, (g, 2))
        gt = np.concatenate([xy, xy + wh], 1)
        pick = rs.randint(0, g, n)
        shift = rs.uniform(-0.3, 0.3, (n, 2)) * wh[pick]
        size = wh[pick] * rs.uniform(0.75, 1.3, (n, 2))
        p1 = xy[pick] + shift
        pr = np.concatenate([p1, p1 + size], 1)
        far = rs.uniform(0, 1, n) < 0.15
        pr[far] = np.concatenate([rs.uniform(250, 300, (int(far.sum()), 2)), rs.uniform(310, 400, (int(far.sum()), 2))], 1)
        out.append((pr.astype(np.float32), gt.astype(np.float32), rs.uniform(-5, 5, (g, 7)).astype(np.float32)))
    return out


def matching_reference(case, high=MATCH_HIGH, low=MATCH_LOW):
    """The torch comparator on the CPU: Matcher(boxlist_iou(target, proposal)) per image -> matched (R) int64, rows (R,7), and the mask of
    the proposals whose best IoU is within 1e-6 of a threshold or tied with another ground truth's (left out of the comparison)"""
    import torch

    from disprcnn_amd.modeling.matcher import Matcher
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.boxlist_ops import boxlist_iou
    matcher = Matcher(high, low, allow_low_quality_matches=False)
    matched, rows, unsafe = [], [], []
    for pr, gt, r7 in case:
        if len(pr) == 0:
            continue
        iou = boxlist_iou(BoxList(torch.from_numpy(gt), (400, 400)), BoxList(torch.from_numpy(pr), (400, 400)))
        m = matcher(iou.clone())
        matched.append(m.numpy())
        rows.append(r7[m.clamp(min=0).numpy()])
        top = iou.sort(dim=0, descending=True)[0]
        tie = (top[0] - top[1]).abs() <= 1e-6 if iou.shape[0] > 1 else torch.zeros(iou.shape[1], dtype=torch.bool)
        unsafe.append((((top[0] - high).abs() <= 1e-6) | ((top[0] - low).abs() <= 1e-6) | (tie & (top[0] > 0))).numpy())
    return np.concatenate(matched), np.concatenate(rows), np.concatenate(unsafe)

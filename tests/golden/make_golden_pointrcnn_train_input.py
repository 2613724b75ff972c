#!/usr/bin/env python3
"""Golden fixture for PointRCNN's training input, recorded from the IMPORTED REFERENCE on torch-CPU (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointrcnn_train_input.py     -> pointrcnn_train_input_golden.npz

Reference code exercised (its own Python): PointRCNN.process_input + back_project (fix_seed=False) + match_targets_to_proposals +
generate_rpn_training_labels (pointnet_module/point_rcnn/lib/net/point_rcnn.py:37-187, 369-432), Matcher, boxlist_iou, Masker, Calib,
DisparityMap, Box3DList, rotate_pc_along_y (and its rotate_back for the targets' corners).  The unbound methods run on a stand-in `self`
(cfg.RPN.NPOINTS = 96, MASK_THRESH 0.7, Matcher(0.6, 0.3)); the stubs are make_golden_points.py's.  Each case calls
np.random.seed(k) first; the seeds are chosen so that there is a flipped case, an unflipped one and one with RPN.FIXED.

Scene: S = 16, M = 14, three 375 x 1242 images.  Images 0 and 1 have different intrinsics and ground truth; image 2 has ROIs but an empty
target list -- the reference skips such an image and then fails on the shape mismatch, so it is recorded on images 0 and 1 only and the
fixture carries image 2 as extra input that must change nothing.  ROIs (see SPEC): kept-point counts below, equal to and above 96, a box of
more than 1024 pixels, negative total disparity on part of a box, a right box wider than the left, a pair dropped by
remove_too_right_proposals, a left box with x1 == 0, one proposal below the low matcher threshold (-1) and one between the two (-2), and
an image with two ground truths where the second wins.

Conditions, asserted (boxes are jittered until they hold): no resampled mask value within 1e-3 of the threshold; no IoU within 1e-3 of a
matcher threshold and no IoU tie; |disp + 1e-6| >= 1e-2 on every box pixel; no drawn point within 1e-3 x box size of a face of its box or
of the enlarged box (tests/pointrcnn_train_oracle.face_margin), in any case.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_points as MP  # noqa: E402  (the stubs and the reference imports; P2, P3, calibration, resampled mask values)

sys.path.insert(0, MP.ROOT)
from tests import pointrcnn_train_oracle as TO  # noqa: E402

from disprcnn.modeling.matcher import Matcher  # noqa: E402  (the reference)
from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN  # noqa: E402
from disprcnn.modeling.roi_heads.mask_head.inference import expand_boxes, expand_masks  # noqa: E402
from disprcnn.structures.bounding_box import BoxList  # noqa: E402
from disprcnn.structures.bounding_box_3d import Box3DList  # noqa: E402
from disprcnn.structures.boxlist_ops import boxlist_iou  # noqa: E402
from disprcnn.structures.calib import Calib  # noqa: E402
from disprcnn.utils.utils_3d import rotate_pc_along_y  # noqa: E402

H, W, S, M, NPOINTS = 375, 1242, 16, 14, 96
MASK_THRESH, FG, BG = 0.7, 0.6, 0.3
CAMS = [(MP.P2, MP.P3), (MP.P2B, MP.P3B), (MP.P2, MP.P3)]
GT2D = [np.array([[400.0, 150.0, 470.0, 200.0]], np.float32),
        np.array([[700.0, 160.0, 760.0, 200.0], [200.0, 170.0, 290.0, 230.0]], np.float32),
        np.zeros((0, 4), np.float32)]
GT_DISP = [[30.0], [36.0, 24.0], []]                   # total disparity of each ground-truth object
# (image, x1, y1, w, h, x1 - x1p, right width - left width, mask kind, disparity (a ground truth's index or a kind), what)
SPEC = [
    (0, 402.3, 151.6, 66.2, 47.1, 30, 0, "rect", 0, "more than 1024 box pixels, count above 96"),
    (0, 398.4, 149.2, 70.3, 50.8, 30, 0, "small", 0, "count below 96"),
    (0, 425.2, 150.4, 70.1, 50.2, 30, 10, "rect", 0, "IoU between the thresholds (-2); right box 10 px wider"),
    (0, 900.0, 250.0, 12.0, 8.0, 25, 0, "empty", "other", "12 x 8 box, mask not applied: count equal to 96; below the low threshold (-1)"),
    (0, 0.0, 100.0, 40.3, 30.2, 0, 0, "rect", "other", "left x1 == 0 (and equal to the right x1); -1"),
    (0, 405.1, 152.3, 60.4, 45.5, -5, 0, "rect", 0, "left x1 < right x1: dropped by remove_too_right_proposals"),
    (0, 396.6, 152.9, 72.4, 46.3, 30, 0, "rect", "negative", "negative total disparity on the left part"),
    (1, 203.2, 172.1, 84.6, 56.3, 24, 0, "rect", 1, "two ground truths, the second wins"),
    (1, 197.5, 168.4, 90.2, 60.1, 24, 0, "rect", 1, "the second wins again"),
    (1, 701.7, 161.2, 57.3, 38.4, 36, 0, "rect", 0, "the first ground truth"),
    (2, 300.4, 180.2, 50.3, 40.6, 20, 0, "rect", "other", "image without ground truth"),
    (2, 600.8, 200.5, 30.2, 25.1, 15, 0, "rect", "other", "image without ground truth"),
]
CASES = [("flip", None, False, True), ("noflip", None, False, False), ("fixed", 5, True, False)]     # (name, seed or search, FIXED, flip)


def int_box(b):
    return int(np.floor(b[0])), int(np.floor(b[1])), int(np.ceil(b[2])), int(np.ceil(b[3]))


def total_disparity(d, lbox, rbox):
    from disprcnn.structures.disparity import DisparityMap
    x1, y1, x2, y2 = int_box(lbox.tolist())
    x1p, _, x2p, _ = int_box(rbox.tolist())
    return DisparityMap(d).resize((max(x2 - x1, x2p - x1p), y2 - y1)).crop((0, 0, x2 - x1, y2 - y1)).data + x1 - x1p


def resampled_mask(prob, box):
    padded, scale = expand_masks(prob[None], padding=1)
    b = expand_boxes(box[None], scale)[0].to(torch.int32)
    w, h = max(int(b[2] - b[0] + 1), 1), max(int(b[3] - b[1] + 1), 1)
    return torch.nn.functional.interpolate(padded[0, 0].expand(1, 1, -1, -1), size=(h, w), mode="bilinear", align_corners=False)[0, 0]


def make_rois():
    rng = np.random.RandomState(20261019)
    out = []
    for img, x1, y1, w, h, dx, dw, kind, dkind, what in SPEC:
        gt = BoxList(torch.from_numpy(GT2D[img]), (W, H))
        for _ in range(400):
            box = torch.tensor([x1, y1, x1 + w, y1 + h], dtype=torch.float32)
            rbox = torch.tensor([x1 - dx, y1, x1 - dx + w + dw, y1 + h], dtype=torch.float32)
            prob = torch.full((M, M), 0.02)
            if kind == "rect":
                r0, c0 = rng.randint(0, 3, size=2)
                r1, c1 = M - rng.randint(0, 3, size=2)
                prob[r0:r1, c0:c1] = 0.97
            elif kind == "small":
                prob[5:7, 5:7] = 0.97
            elif kind == "empty":
                prob[:] = 0.1
            v = resampled_mask(prob[None], box)
            lx1, _, lx2, _ = int_box(box.tolist())
            rx1, _, rx2, _ = int_box(rbox.tolist())
            wd = max(lx2 - lx1, rx2 - rx1)
            gy, gx = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
            if dkind == "negative":
                field = np.where(gx < -0.5, -3.0 + 0.5 * gy, GT_DISP[0][0] + 1.0 * gx + 0.6 * gy)
            else:
                target = GT_DISP[img][dkind] if isinstance(dkind, int) else rng.uniform(18.0, 40.0)
                field = target + 1.0 * gx + 0.6 * gy + 0.3 * np.sin(3 * gx) * np.cos(2 * gy)
            d = torch.from_numpy(((field - (lx1 - rx1)) * S / wd).astype(np.float32))
            disp = total_disparity(d, box, rbox)
            ok = (v - MASK_THRESH).abs().min().item() >= 1e-3 and (disp + 1e-6).abs().min().item() >= 1e-2
            if len(gt):
                iou = boxlist_iou(gt, BoxList(box[None], (W, H)))[:, 0]
                ok = ok and min((iou - FG).abs().min().item(), (iou - BG).abs().min().item()) >= 1e-3
                ok = ok and (len(iou) < 2 or (iou[0] - iou[1]).abs().item() >= 1e-3)
            if ok:
                break
            x1 += 0.137 if x1 != 0.0 else 0.0
            y1 += 0.071
        else:
            raise AssertionError(f"no box found for {what!r}")
        out.append(dict(img=img, box=box, rbox=rbox, disp=d, mask=prob[None], what=what, negative=dkind == "negative"))
    return out


def boxlists(rois, images):
    left, right = [], []
    for img in images:
        rs = [r for r in rois if r["img"] == img]
        lb = BoxList(torch.stack([r["box"] for r in rs]), (W, H))
        lb.add_field("disparity", torch.stack([r["disp"] for r in rs]))
        lb.add_field("mask", torch.stack([r["mask"] for r in rs]))
        left.append(lb)
        right.append(BoxList(torch.stack([r["rbox"] for r in rs]), (W, H)))
    return left, right


def targets_of(gt3d, images):
    out = []
    for img in images:
        t = BoxList(torch.from_numpy(GT2D[img]), (W, H))
        t.add_field("box3d", Box3DList(torch.from_numpy(gt3d[img].astype(np.float32)).reshape(-1, 7), (W, H), "xyzhwl_ry"))
        t.add_field("calib", Calib(MP.calibration(*CAMS[img]), (W, H)))
        out.append(t)
    return out


def run_reference(rois, gt3d, seed, fixed):
    """-> dict of the reference's outputs for np.random.seed(seed)"""
    me = types.SimpleNamespace(cfg=types.SimpleNamespace(RPN=types.SimpleNamespace(NPOINTS=NPOINTS, FIXED=fixed)),
                               proposal_matcher=Matcher(FG, BG, allow_low_quality_matches=False))
    me.match_targets_to_proposals = lambda p, t: PointRCNN.match_targets_to_proposals(me, p, t)
    cap = {}

    def back_project(depth_maps, mask_pred, targets, max_depth=160, fix_seed=False):
        cap["depth_maps"] = depth_maps
        return PointRCNN.back_project(me, depth_maps, mask_pred, targets, max_depth=max_depth, fix_seed=fix_seed)
    me.back_project = back_project
    left, right = boxlists(rois, (0, 1))
    targets = targets_of(gt3d, (0, 1))
    np.random.seed(seed)
    pts, cls_label, reg_label, matched = PointRCNN.process_input(me, left, right, targets, MASK_THRESH)
    # the draws again, as the reference made them, for the counts, the chosen pixels, the scale and the flip
    np.random.seed(seed)
    counts, src = [], []
    for dm in cap["depth_maps"]:
        for j in range(dm.shape[0]):
            flat = dm[j].t().reshape(-1)
            pos = torch.nonzero(flat > 0).squeeze(1)
            n = len(pos)
            if n > NPOINTS:
                choice = np.random.choice(n, NPOINTS, replace=False)
            else:
                choice = np.concatenate((np.arange(n), np.random.choice(n, NPOINTS - n, replace=True)))
            np.random.shuffle(choice)
            k = pos[choice]
            src.append(((k % H) * W + k // H).numpy().astype(np.int32))
            counts.append(n)
    scale, flip = 1.0, False
    if not fixed:
        scale = np.random.uniform(0.95, 1.05)
        flip = bool(np.random.random() < 0.5)
    corners = torch.cat([t.get_field("box3d").convert("corners").bbox_3d for t in matched]).view(-1, 8, 3)
    rot = me.rotator.rot_angle
    back = rotate_pc_along_y(None, None, rot_angle=rot).rotate_back((corners + me.pts_mean[:, None, :]).permute(0, 2, 1)).permute(0, 2, 1)
    large = torch.cat([t.get_field("box3d").enlarge_box3d(0.2).convert("corners").bbox_3d for t in matched]).view(-1, 8, 3)
    return dict(counts=np.array(counts, np.int64), src_pix=np.stack(src), scale=np.float64(scale), flip=np.bool_(flip), pts=pts.numpy(),
                pts_mean=me.pts_mean.numpy(), rot_angle=rot.numpy(), matched_idxs=torch.cat([t.get_field("matched_idxs") for t in matched]).numpy(),
                corners=corners.numpy(), corners_large=large.numpy(), cls_label=cls_label.numpy(), reg_label=reg_label.numpy(),
                corners_back=back.contiguous().numpy())


def main():
    rois = make_rois()
    # seeds: the first one that flips, the first one that does not
    cases = []
    for name, seed, fixed, flip in CASES:
        if seed is None:
            for k in range(100):
                probe = run_reference(rois, [np.array([[0, 1, 12, 1, 1, 2, 0.1]]), np.array([[0, 1, 12, 1, 1, 2, 0.1]] * 2), None], k, False)
                if bool(probe["flip"]) == flip and k not in [c[1] for c in cases]:
                    seed = k
                    break
        cases.append((name, seed, fixed))
    print("cases", cases)

    # the 3D ground truth: a box around the cloud of its home ROI, sized well inside the cloud so that each cloud has foreground, ignored
    # and background points; its numbers are jittered until every drawn point of every case is clear of every face
    home = {(0, 0): 0, (1, 1): 7, (1, 0): 9}                              # (image, gt) -> index into SPEC
    dummy = [np.array([[0, 1, 12, 1, 1, 2, 0.1]]), np.array([[0, 1, 12, 1, 1, 2, 0.1]] * 2), None]
    runs = [run_reference(rois, dummy, seed, fixed) for _, seed, fixed in cases]         # the clouds do not depend on the 3D boxes
    kept = [i for i, r in enumerate(rois) if r["img"] < 2 and "dropped" not in r["what"]]
    cloud_image = np.array([rois[i]["img"] for i in kept])
    first = [0, len(GT2D[0])]
    rng = np.random.RandomState(7)
    gt3d = [np.zeros((len(GT2D[0]), 7)), np.zeros((len(GT2D[1]), 7)), np.zeros((0, 7))]
    for (img, g), spec_i in home.items():
        c = kept.index(spec_i)
        r0 = runs[2]                                                      # the FIXED case: scale 1, no flip
        cam = TO.to_camera_frame(r0["pts"][c:c + 1], r0["rot_angle"][c:c + 1], r0["pts_mean"][c:c + 1])[0]
        lo, hi = np.percentile(cam, 10, axis=0), np.percentile(cam, 90, axis=0)
        ctr, ext = (lo + hi) / 2, hi - lo
        clouds = [k for k in range(len(kept)) if cloud_image[k] == img and max(int(runs[0]["matched_idxs"][k]), 0) == g]
        for attempt in range(4000):
            j = rng.uniform(-1, 1, 7)
            h, w, l = 0.7 * ext[1] * (1 + 0.1 * j[0]), 0.8 * ext[2] * (1 + 0.1 * j[1]) + 0.3, 0.7 * ext[0] * (1 + 0.1 * j[2])
            box = np.array([[ctr[0] + 0.05 * j[3], ctr[1] + h / 2, ctr[2] + 0.05 * j[4], h, w, l, 0.25 * j[5]]])
            box = box.astype(np.float32).astype(np.float64)
            worst = np.inf
            for r in runs:
                for k in clouds:
                    for b in (box, None):
                        aug = TO.augment_box7(box, r["scale"], bool(r["flip"]))
                        cr = TO.rotate(TO.corners_of(aug if b is not None else TO.enlarge(TO.box7_of(TO.corners_of(aug)), 0.2)),
                                       r["rot_angle"][k:k + 1]) - r["pts_mean"][k:k + 1, None]
                        worst = min(worst, TO.face_margin(cr, r["pts"][k:k + 1]).min())
            if worst >= 2e-3:
                break
        else:
            raise AssertionError(f"no 3D box found for ground truth {(img, g)}")
        print("gt", (img, g), "attempts", attempt + 1, "margin", worst)
        gt3d[img][g] = box[0]

    runs = [run_reference(rois, gt3d, seed, fixed) for _, seed, fixed in cases]
    out = {}
    for (name, seed, fixed), r in zip(cases, runs):
        # conditions on the reference's own outputs
        m = min(TO.face_margin(r["corners"], r["pts"]).min(), TO.face_margin(r["corners_large"], r["pts"]).min())
        assert m >= 1e-3, (name, m)
        assert np.array_equal(TO.cls_labels(r["corners"], r["corners_large"], r["pts"]), r["cls_label"]), name
        assert (r["cls_label"] == 1).any() and (r["cls_label"] == -1).any() and (r["cls_label"] == 0).any()
        assert bool(r["flip"]) == (name == "flip") and (fixed or r["scale"] != 1.0)
        assert np.array_equal(r["matched_idxs"], runs[0]["matched_idxs"]) and np.array_equal(r["counts"], runs[0]["counts"])
        print(name, "seed", seed, "scale", r["scale"], "flip", r["flip"], "fg", int((r["cls_label"] == 1).sum()), "ignored",
              int((r["cls_label"] == -1).sum()), "margin", m)
        for k, v in r.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_seed"], out[f"{name}_fixed"] = seed, fixed
    r = runs[0]
    counts, mi = r["counts"], r["matched_idxs"]
    print("counts", counts.tolist(), "matched", mi.tolist())
    assert (counts < NPOINTS).any() and (counts == NPOINTS).any() and (counts > NPOINTS).any()
    assert (mi == -1).any() and (mi == -2).any() and mi[cloud_image == 1].max() == 1 and (mi[cloud_image == 1] == 0).any()
    ib = np.array([int_box(x["box"].tolist()) for x in rois])
    ibr = np.array([int_box(x["rbox"].tolist()) for x in rois])
    assert ((ib[:, 2] - ib[:, 0]) * (ib[:, 3] - ib[:, 1]) > 1024).any() and (ib[:, 0] == 0).any()
    assert ((ibr[:, 2] - ibr[:, 0]) > (ib[:, 2] - ib[:, 0])).any()
    neg = next(x for x in rois if x["negative"])
    dn = total_disparity(neg["disp"], neg["box"], neg["rbox"])
    assert (dn < 0).any() and (dn > 0).any()
    assert len(kept) == len(counts) == len(rois) - 3

    np.savez_compressed(os.path.join(HERE, "pointrcnn_train_input_golden.npz"),
                        H=H, W=W, S=S, M=M, npoints=NPOINTS, mask_thresh=MASK_THRESH, fg_iou=FG, bg_iou=BG,
                        P2s=np.stack([c[0] for c in CAMS]), P3s=np.stack([c[1] for c in CAMS]),
                        rois_per_image=np.array([sum(1 for x in rois if x["img"] == i) for i in range(3)]),
                        gts_per_image=np.array([len(g) for g in GT2D]), gt_boxes=np.concatenate(GT2D),
                        gt_box3d=np.concatenate(gt3d).astype(np.float32), left_boxes=torch.stack([x["box"] for x in rois]).numpy(),
                        right_boxes=torch.stack([x["rbox"] for x in rois]).numpy(), disparity=torch.stack([x["disp"] for x in rois]).numpy(),
                        mask=torch.stack([x["mask"] for x in rois]).numpy(), kept_rois=np.array(kept), cloud_image=cloud_image,
                        matched_idxs=mi, cases=np.array([c[0] for c in cases]), **out)


if __name__ == "__main__":
    main()

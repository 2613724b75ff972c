#!/usr/bin/env python3
"""Golden fixture for the instance point clouds of the 3D stage, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_points.py            -> points_ref_golden.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_points.py --edges    -> points_ref_edges_golden.npz (see edges())

Reference code exercised (its own Python on torch-CPU):
  PointRCNN.process_input_eval + back_project (fix_seed=True)   pointnet_module/point_rcnn/lib/net/point_rcnn.py:37-83, 189-241
  Masker / paste_mask_in_image                                   modeling/roi_heads/mask_head/inference.py
  Calib / kitti_utils.Calibration, DisparityMap, rotate_pc_along_y
The unbound methods run on a stand-in `self` (cfg.RPN.NPOINTS = 768).  Harness-only stand-ins: the stubs of make_golden_det.py for
imports of neighbouring modules and CUDA extensions, numpy's removed aliases, `Tensor.cuda` = identity.
Inputs: two 375 x 1242 images, 12 ROIs: KITTI-like boxes, one of area < 768, one with an empty mask, one with x1 == x1p.  Masks are
rectangles of ones, boxes jittered until no resampled mask value lies within 1e-3 of the 0.5 threshold (asserted).
"""
import copy
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

for name in ("cv2", "pycocotools", "pycocotools.mask", "pointnet2_cuda", "iou3d_cuda", "roipool3d_cuda", "tensorboardX", "termcolor",
             "numba", "zarr", "fastai", "matplotlib", "matplotlib.pyplot", "dl_ext", "dl_ext.primitive", "dl_ext.vision_ext",
             "dl_ext.vision_ext.datasets", "dl_ext.vision_ext.datasets.kitti", "dl_ext.vision_ext.datasets.kitti.structures",
             "disprcnn._C", "PIL", "PIL.Image", "tqdm", "scipy", "scipy.spatial", "skimage", "shapely", "shapely.geometry"):
    sys.modules.setdefault(name, MagicMock())


class CfgNode(dict):
    def __init__(self, init=None, *a, **k):
        super().__init__(init or {})

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self):
        return copy.deepcopy(self)


yacs, yc = types.ModuleType("yacs"), types.ModuleType("yacs.config")
yc.CfgNode = CfgNode
yacs.config = yc
sys.modules["yacs"], sys.modules["yacs.config"] = yacs, yc
torch._six = types.SimpleNamespace(PY3=True, PY37=True, string_classes=(str,), int_classes=(int,),
                                   container_abcs=__import__("collections").abc)
sys.modules["torch._six"] = torch._six
np.float, np.int, np.bool = float, int, bool
torch.Tensor.cuda = lambda self, *a, **k: self

from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN  # noqa: E402  (the reference)
from disprcnn.modeling.roi_heads.mask_head.inference import expand_boxes, expand_masks  # noqa: E402
from disprcnn.structures.bounding_box import BoxList  # noqa: E402
from disprcnn.structures.calib import Calib  # noqa: E402
from disprcnn.utils.kitti_utils import Calibration  # noqa: E402

H, W, S, M, NPOINTS = 375, 1242, 64, 28, 768
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
P3 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]])
P2B = P2.copy()
P2B[0, 2] += 3.25                      # a second camera: the two images do not share intrinsics
P3B = P3.copy()
P3B[0, 2] += 3.25


def calibration(p2, p3):
    eye = np.eye(4)[:3]
    return Calibration({"P0": p2, "P1": p3, "P2": p2, "P3": p3, "R0_rect": np.eye(3), "Tr_velo_to_cam": eye, "Tr_imu_to_velo": eye}, (W, H))


def resampled_mask(prob, box):
    """paste_mask_in_image's values before the threshold (inference.py:119-150)."""
    padded, scale = expand_masks(prob[None], padding=1)
    b = expand_boxes(box[None], scale)[0].to(torch.int32)
    w, h = max(int(b[2] - b[0] + 1), 1), max(int(b[3] - b[1] + 1), 1)
    return F.interpolate(padded[0, 0].expand(1, 1, -1, -1), size=(h, w), mode="bilinear", align_corners=False)[0, 0]


def main():
    rng = np.random.RandomState(20261016)
    # (image, x1, y1, w, h, x1 - x1p, kind)
    spec = [(0, 100.3, 150.6, 180.2, 120.4, 38, "rect"), (0, 420.7, 170.2, 60.5, 45.8, 21, "rect"), (0, 700.1, 140.9, 295.6, 190.3, 61, "rect"),
            (0, 900.4, 180.3, 20.2, 30.1, 14, "full"), (0, 1000.2, 160.5, 120.7, 80.2, 0, "rect"), (0, 300.8, 200.1, 90.3, 60.6, 27, "empty"),
            (1, 50.5, 160.7, 240.4, 150.9, 45, "rect"), (1, 330.2, 175.4, 44.9, 33.3, 17, "full"), (1, 520.6, 150.2, 150.1, 100.7, 33, "rect"),
            (1, 760.3, 165.8, 75.4, 52.2, 24, "rect"), (1, 880.9, 140.3, 200.6, 170.5, 52, "rect"), (1, 1100.1, 170.6, 110.8, 70.4, 19, "rect")]
    lboxes, rboxes, disps, masks = [[], []], [[], []], [[], []], [[], []]
    for img, x1, y1, w, h, dx, kind in spec:
        for _ in range(200):
            box = torch.tensor([x1, y1, x1 + w, y1 + h], dtype=torch.float32)
            prob = torch.zeros(M, M)
            if kind == "rect":
                r0, c0 = rng.randint(0, 6, size=2)
                r1, c1 = M - rng.randint(0, 6, size=2)
                prob[r0:r1, c0:c1] = 0.97
                prob[prob == 0] = 0.02
            elif kind == "full":
                prob[:] = 0.97
            else:
                prob[:] = 0.1
            v = resampled_mask(prob[None], box)
            if (v - 0.5).abs().min().item() >= 1e-3:
                break
            x1 += 0.137
            y1 += 0.071
        else:
            raise AssertionError("no box found with mask values clear of the threshold")
        assert (v - 0.5).abs().min().item() >= 1e-3
        wd = max(int(np.ceil(x1 + w)) - int(np.floor(x1)), int(np.ceil(x1 + w)) - int(np.floor(x1 - dx)))
        # total disparity = v * wd / S + x1 - x1p: 15 .. 60 px on every pixel (depth 6.5 .. 26 m)
        target = rng.uniform(18.0, 50.0)
        gy, gx = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
        field = target + 4.0 * gx + 3.0 * gy + 1.5 * np.sin(3 * gx) * np.cos(2 * gy)
        d = (field - (int(np.floor(x1)) - int(np.floor(x1 - dx)))) * S / wd
        lboxes[img].append(box)
        rboxes[img].append(torch.tensor([x1 - dx, y1, x1 - dx + w, y1 + h], dtype=torch.float32))
        disps[img].append(torch.from_numpy(d.astype(np.float32)))
        masks[img].append(prob[None])

    left, right, targets = [], [], []
    calibs = [(P2, P3), (P2B, P3B)]
    for img in range(2):
        lb = BoxList(torch.stack(lboxes[img]), (W, H))
        lb.add_field("disparity", torch.stack(disps[img]))
        lb.add_field("mask", torch.stack(masks[img]))
        left.append(lb)
        right.append(BoxList(torch.stack(rboxes[img]), (W, H)))
        t = BoxList(torch.zeros(0, 4), (W, H))
        t.add_field("calib", Calib(calibration(*calibs[img]), (W, H)))
        targets.append(t)

    me = types.SimpleNamespace(cfg=types.SimpleNamespace(RPN=types.SimpleNamespace(NPOINTS=NPOINTS)))
    captured = {}

    def back_project(depth_maps, mask_pred, targets, max_depth=160, fix_seed=False):
        captured["depth_maps"] = depth_maps
        return PointRCNN.back_project(me, depth_maps, mask_pred, targets, max_depth=max_depth, fix_seed=fix_seed)
    me.back_project = back_project
    pts = PointRCNN.process_input_eval(me, left, right, targets, threshold=0.5)
    pts_mean, rot = me.pts_mean, me.rotator.rot_angle

    # counts and chosen source pixels (flat y * W + x) from the masked depth maps back_project left behind
    counts, src = [], []
    for dm in captured["depth_maps"]:
        for j in range(dm.shape[0]):
            flat = dm[j].t().reshape(-1)                                  # x-major, as meshgrid(x, y)
            pos = torch.nonzero(flat > 0).squeeze(1)
            n = len(pos)
            np.random.seed(0)
            if n > NPOINTS:
                choice = np.random.choice(n, NPOINTS, replace=False)
            else:
                choice = np.concatenate((np.arange(n), np.random.choice(n, NPOINTS - n, replace=True)))
            np.random.seed(0)
            np.random.shuffle(choice)
            k = pos[choice]
            src.append(((k % H) * W + k // H).numpy().astype(np.int32))
            counts.append(n)
    counts = np.array(counts, np.int64)
    print("counts", counts.tolist())
    assert (counts < NPOINTS).any() and (counts > NPOINTS).any()
    np.savez_compressed(os.path.join(HERE, "points_ref_golden.npz"),
                        H=H, W=W, S=S, M=M, npoints=NPOINTS, P2=P2, P3=P3, P2B=P2B, P3B=P3B,
                        rois_per_image=np.array([len(lboxes[0]), len(lboxes[1])]),
                        left_boxes=torch.cat([torch.stack(b) for b in lboxes]).numpy(),
                        right_boxes=torch.cat([torch.stack(b) for b in rboxes]).numpy(),
                        disparity=torch.cat([torch.stack(d) for d in disps]).numpy(),
                        mask=torch.cat([torch.stack(m) for m in masks]).numpy(),
                        fuxb=np.array([targets[0].get_field("calib").stereo_fuxbaseline, targets[1].get_field("calib").stereo_fuxbaseline]),
                        counts=counts, src_pix=np.stack(src), pts=pts.numpy(), pts_mean=pts_mean.numpy(), rot_angle=rot.numpy())


# ---- the edge scene: tests/golden/points_ref_edges_golden.npz (--edges)
#
# Three images; the middle one has no ROI.  Reference quirk: back_project takes targets[i] over the NON-EMPTY images only, so the ROIs
# of image 2 are back-projected with image 1's calibration.  InstancePointCloud pairs calibrations by image.  Images 1 and 2 therefore
# share a camera here, and both readings give the same points.
EDGE_CAMS = [(P2B, P3B), (P2, P3), (P2, P3)]
# (image, x1, y1, w, h, x1 - x1p, right width - left width, mask kind, disparity kind, jitter (dx, dy) per retry, edge)
EDGE_SPEC = [
    (0, 600.3, 170.2, 40.6, 20.4, 1, 0, "rect", "far", (0.137, 0.071), "depth > 160 m (disparity 1..2 px)"),
    (0, 200.4, 180.1, 90.3, 50.2, 10, 0, "rect", "negative", (0.137, 0.071), "negative disparity on the left part"),
    (0, 420.7, 150.9, 60.5, 45.8, 30, 25, "rect", "normal", (0.137, 0.071), "right box 25 px wider: crop branch"),
    (0, 800.6, 160.4, 110.2, 70.3, 20, -12, "rect", "normal", (0.137, 0.071), "right box 12 px narrower"),
    (0, 0.0, 0.0, 80.3, 60.2, 0, 0, "rect", "normal", (0.0, 0.0), "x1 = 0, y1 = 0"),
    (0, 1120.7, 253.8, 120.3, 120.2, 35, 0, "rect", "normal", (0.0, 0.0), "x2 = W-1, y2 = H-1"),
    (2, 300.2, 200.0, 50.5, 1.0, 20, 0, "full", "normal", (0.137, 0.0), "integer box of height 1"),
    (2, 500.0, 150.3, 2.0, 40.1, 15, 0, "miss", "normal", (0.0, 0.071), "width 2; mask pasted only left of the box"),
    (2, 650.4, 140.6, 140.2, 90.5, 40, 0, "soft", "normal", (0.137, 0.071), "graded (soft) mask"),
    (2, 0.0, 0.0, 1241.9, 374.9, 0, 0, "full", "normal", (0.0, 0.0), "full image"),
    (2, 0.0, 0.0, 1241.9, 374.9, 0, 0, "full", "normal", (0.0, 0.0), "full image"),
    (2, 0.0, 0.0, 1241.9, 374.9, 0, 0, "full", "normal", (0.0, 0.0), "full image"),
]


def _int_box(x1, y1, x2, y2):
    return int(np.floor(x1)), int(np.floor(y1)), int(np.ceil(x2)), int(np.ceil(y2))


def _total_disparity(d, lbox, rbox):
    """process_input_eval's disp_roi (point_rcnn.py:209-213) with the reference's own DisparityMap."""
    from disprcnn.structures.disparity import DisparityMap
    x1, y1, x2, y2 = _int_box(*lbox.tolist())
    x1p, _, x2p, _ = _int_box(*rbox.tolist())
    return DisparityMap(d).resize((max(x2 - x1, x2p - x1p), y2 - y1)).crop((0, 0, x2 - x1, y2 - y1)).data + x1 - x1p


def edges():
    rng = np.random.RandomState(20261017)
    n_img = 3
    lboxes, rboxes, disps, masks = [[] for _ in range(n_img)], [[] for _ in range(n_img)], [[] for _ in range(n_img)], [[] for _ in range(n_img)]
    for img, x1, y1, w, h, dx, dw, kind, dkind, (jx, jy), what in EDGE_SPEC:
        for _ in range(200):
            box = torch.tensor([x1, y1, min(x1 + w, W - 1.0), min(y1 + h, H - 1.0)], dtype=torch.float32)
            rbox = torch.tensor([x1 - dx, y1, x1 - dx + w + dw, y1 + h], dtype=torch.float32)
            prob = torch.full((M, M), 0.02)
            if kind == "rect":
                r0, c0 = rng.randint(0, 6, size=2)
                r1, c1 = M - rng.randint(0, 6, size=2)
                prob[r0:r1, c0:c1] = 0.97
            elif kind == "full":
                prob[:] = 0.97
            elif kind == "miss":
                prob[:, 1:5] = 0.97          # a 2-px box is pasted 4 px wide: mask columns 1..4 land only on pixel x1 - 1
            else:
                prob = torch.tensor([0.15, 0.35, 0.65, 0.85]).repeat_interleave(M // 4).expand(M, M).clone()   # graded in 4 bands
            v = resampled_mask(prob[None], box)
            lx1, ly1, lx2, ly2 = _int_box(*box.tolist())
            rx1, _, rx2, _ = _int_box(*rbox.tolist())
            wd = max(lx2 - lx1, rx2 - rx1)
            gy, gx = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
            if dkind == "far":
                field = 1.5 + 0.4 * gx + 0.1 * gy
            elif dkind == "negative":
                field = np.where(gx < -0.2, -3.0 + 0.5 * gy, 22.0 + 3.0 * gx)
            else:
                field = rng.uniform(18.0, 50.0) + 4.0 * gx + 3.0 * gy + 1.5 * np.sin(3 * gx) * np.cos(2 * gy)
            d = torch.from_numpy(((field - (lx1 - rx1)) * S / wd).astype(np.float32))
            disp = _total_disparity(d, box, rbox)
            if (v - 0.5).abs().min().item() >= 1e-3 and disp.abs().min().item() >= 0.5:
                break
            x1 += jx
            y1 += jy
        else:
            raise AssertionError(f"no box found for {what!r} with mask values clear of the threshold and |disparity| >= 0.5")
        lboxes[img].append(box)
        rboxes[img].append(rbox)
        disps[img].append(d)
        masks[img].append(prob[None])

    left, right, targets = [], [], []
    for img in range(n_img):
        bb = torch.stack(lboxes[img]) if lboxes[img] else torch.zeros(0, 4)
        lb = BoxList(bb, (W, H))
        lb.add_field("disparity", torch.stack(disps[img]) if disps[img] else torch.zeros(0, S, S))
        lb.add_field("mask", torch.stack(masks[img]) if masks[img] else torch.zeros(0, 1, M, M))
        left.append(lb)
        right.append(BoxList(torch.stack(rboxes[img]) if rboxes[img] else torch.zeros(0, 4), (W, H)))
        t = BoxList(torch.zeros(0, 4), (W, H))
        t.add_field("calib", Calib(calibration(*EDGE_CAMS[img]), (W, H)))
        targets.append(t)

    me = types.SimpleNamespace(cfg=types.SimpleNamespace(RPN=types.SimpleNamespace(NPOINTS=NPOINTS)))
    captured = {}

    def back_project(depth_maps, mask_pred, targets, max_depth=160, fix_seed=False):
        captured["depth_maps"] = depth_maps
        captured["unmasked"] = [dm.clone() for dm in depth_maps]
        captured["applied"] = [bool(mp[j].sum() != 0 and (dm[j] * mp[j].float()).max() > 0)
                               for dm, mp in zip(depth_maps, mask_pred) for j in range(dm.shape[0])]
        captured["mask_pixels"] = [int(mp[j].sum()) for mp in mask_pred for j in range(mp.shape[0])]
        out = PointRCNN.back_project(me, depth_maps, mask_pred, targets, max_depth=max_depth, fix_seed=fix_seed)
        captured["pre_rotation"] = out.clone()
        return out
    me.back_project = back_project
    pts = PointRCNN.process_input_eval(me, left, right, targets, threshold=0.5)
    pts_mean, rot = me.pts_mean, me.rotator.rot_angle

    counts, src = [], []
    for dm in captured["depth_maps"]:
        for j in range(dm.shape[0]):
            flat = dm[j].t().reshape(-1)
            pos = torch.nonzero(flat > 0).squeeze(1)
            n = len(pos)
            np.random.seed(0)
            if n > NPOINTS:
                choice = np.random.choice(n, NPOINTS, replace=False)
            else:
                choice = np.concatenate((np.arange(n), np.random.choice(n, NPOINTS - n, replace=True)))
            np.random.seed(0)
            np.random.shuffle(choice)
            k = pos[choice]
            src.append(((k % H) * W + k // H).numpy().astype(np.int32))
            counts.append(n)
    counts = np.array(counts, np.int64)
    applied = np.array(captured["applied"])
    lb_all = torch.cat([torch.stack(b) for b in lboxes if b]).numpy()
    rb_all = torch.cat([torch.stack(b) for b in rboxes if b]).numpy()
    unmasked = torch.cat(captured["unmasked"])
    pre = captured["pre_rotation"].numpy()
    print("counts", counts.tolist(), "applied", applied.tolist())

    # every edge really occurs
    whats = [e[-1] for e in EDGE_SPEC]
    ib = np.array([_int_box(*b) for b in lb_all.tolist()])
    ibr = np.array([_int_box(*b) for b in rb_all.tolist()])
    far = whats.index("depth > 160 m (disparity 1..2 px)")
    assert (unmasked[far][unmasked[far] > 0] > 160).all()                               # every point of this ROI is clamped
    assert (pre[far][:, 2] == 160).all()
    neg = whats.index("negative disparity on the left part")
    disp_neg = _total_disparity(torch.stack(disps[0])[neg], torch.from_numpy(lb_all[neg]), torch.from_numpy(rb_all[neg]))
    assert (disp_neg < 0).any() and (disp_neg > 0).any()
    assert (pre[neg][:, 2] == 1.0).any()                                               # negative disparity -> depth clamped to 1, kept
    wide, narrow = whats.index("right box 25 px wider: crop branch"), whats.index("right box 12 px narrower")
    assert (ibr[wide, 2] - ibr[wide, 0]) - (ib[wide, 2] - ib[wide, 0]) >= 10
    assert (ibr[narrow, 2] - ibr[narrow, 0]) < (ib[narrow, 2] - ib[narrow, 0])
    assert (ib[:, 0] == 0).any() and (ib[:, 1] == 0).any() and (ib[:, 2] == W - 1).any() and (ib[:, 3] == H - 1).any()
    assert ((ib[:, 3] - ib[:, 1]) == 1).any() and ((ib[:, 2] - ib[:, 0]) == 2).any()
    miss = whats.index("width 2; mask pasted only left of the box")
    assert captured["mask_pixels"][miss] > 0 and not applied[miss]                     # the "mask not applied" branch
    assert applied[[i for i in range(len(whats)) if i != miss]].all()
    assert ((ib[:, 2] - ib[:, 0]) * (ib[:, 3] - ib[:, 1])).sum() > 1 << 20
    assert [len(b) for b in lboxes][1] == 0 and (counts < NPOINTS).any() and (counts > NPOINTS).any()

    np.savez_compressed(os.path.join(HERE, "points_ref_edges_golden.npz"),
                        H=H, W=W, S=S, M=M, npoints=NPOINTS, P2s=np.stack([c[0] for c in EDGE_CAMS]), P3s=np.stack([c[1] for c in EDGE_CAMS]),
                        rois_per_image=np.array([len(b) for b in lboxes]), left_boxes=lb_all, right_boxes=rb_all,
                        disparity=torch.cat([torch.stack(d) for d in disps if d]).numpy(),
                        mask=torch.cat([torch.stack(m) for m in masks if m]).numpy(),
                        mask_applied=applied, counts=counts, src_pix=np.stack(src), pts=pts.numpy(), pts_mean=pts_mean.numpy(),
                        rot_angle=rot.numpy(), pts_pre_rotation=pre)


if __name__ == "__main__":
    edges() if "--edges" in sys.argv else main()

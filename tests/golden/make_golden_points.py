#!/usr/bin/env python3
"""Golden fixture for the instance point clouds of the 3D stage, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_points.py

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


if __name__ == "__main__":
    main()

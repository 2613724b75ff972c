#!/usr/bin/env python3
"""Time PointRCNN's training forward on one GPU: `process_input` (training clouds, 2D matching, targets into the cloud frame, point
labels) against a torch composition of the same steps, and the whole step (forward, backward, FusedSGD) for the rpn and the rcnn config.

    python tools/bench_pointrcnn_train.py [--iters 20] [--warmup 3] [--only input|rpn|rcnn]

Shapes: two 375 x 1242 images with 8 ROIs each -> 16 clouds of 768 points (car config), disparities 224 x 224, masks 28 x 28, one
ground truth per ROI.  Wall-clock microseconds around synchronised calls (process_input reads the host once, so HIP events alone would
miss its host part); medians with min / max; `input_share` is process_input's median over the step's.  The torch composition follows the
reference's flow per ROI (full-size depth map and Masker paste, back-projection of every pixel, nonzero, the draw, then the batched
augmentation, rotation, centring, per-image IoU matching, the boxes through Box3DList, the labels kernel) with the same draws; its
points are compared with process_input's before anything is timed.  One JSON line.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_rcnn as BC  # noqa: E402
import bench_rpn as BR  # noqa: E402
from bench_points import P2, P3  # noqa: E402
from disprcnn_amd.modeling.matcher import Matcher  # noqa: E402
from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN, generate_rpn_training_labels  # noqa: E402
from disprcnn_amd.solver.fused import FusedSGD  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.structures.bounding_box_3d import Box3DList  # noqa: E402
from disprcnn_amd.structures.boxlist_ops import boxlist_iou  # noqa: E402
from disprcnn_amd.structures.calib import Calib  # noqa: E402

W, H, S, M = 1242, 375, 224, 28


def scene(dev, images=2, per_image=8):
    """-> left, right, targets: per ROI a smooth disparity field around 30 px, a rectangular mask, and a ground truth (the box shifted by
    a few pixels, a car-sized 3D box at the cloud's place)"""
    g = torch.Generator().manual_seed(0)
    calib = Calib(SimpleNamespace(P2=P2, P3=P3), (W, H))
    k = calib.calib
    left, right, targets = [], [], []
    for _ in range(images):
        n = per_image
        x1 = 40 + torch.arange(n) * 140.0 + torch.rand(n, generator=g) * 20
        y1 = 140 + torch.rand(n, generator=g) * 30
        w, h = 60 + torch.rand(n, generator=g) * 60, 45 + torch.rand(n, generator=g) * 50
        lb = torch.stack([x1, y1, x1 + w, y1 + h], 1)
        total = 20 + torch.rand(n, generator=g) * 25                                   # total disparity, px
        dx = total.round()
        rb = lb - torch.stack([dx, torch.zeros(n), dx, torch.zeros(n)], 1)
        gy, gx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
        wd = (lb[:, 2].ceil() - lb[:, 0].floor())
        field = total[:, None, None] + 1.0 * gx + 0.6 * gy
        disp = (field - (lb[:, 0].floor() - rb[:, 0].floor())[:, None, None]) * S / wd[:, None, None]
        mask = torch.full((n, 1, M, M), 0.02)
        mask[:, :, 3:-3, 2:-2] = 0.97
        l = BoxList(lb.to(dev), (W, H))
        l.add_field("disparity", disp.to(dev))
        l.add_field("mask", mask.to(dev))
        l.add_field("scores", torch.ones(n, device=dev))
        left.append(l)
        right.append(BoxList(rb.to(dev), (W, H)))
        z = calib.stereo_fuxbaseline / total
        xc = ((lb[:, 0] + lb[:, 2]) / 2 - k.cu) * z / k.fu + k.tx
        yc = ((lb[:, 1] + lb[:, 3]) / 2 - k.cv) * z / k.fv + k.ty
        b7 = torch.stack([xc, yc + 0.4, z, torch.full((n,), 0.8), torch.full((n,), 0.9), torch.full((n,), 1.0),
                          torch.rand(n, generator=g) * 0.6 - 0.3], 1).float()
        t = BoxList((lb + 3.0).to(dev), (W, H))
        t.add_field("box3d", Box3DList(b7.to(dev), (W, H), "xyzhwl_ry"))
        t.add_field("calib", calib)
        targets.append(t)
    return left, right, targets


def torch_process_input(m, left, right, targets, rng):
    """process_input as a composition of torch ops, in the reference's flow"""
    dev = left[0].bbox.device
    npoints, thresh, pad = m.cfg.RPN.NPOINTS, m.masker_threshold, 1
    matcher = Matcher(m.fg_iou_threshold, m.bg_iou_threshold, allow_low_quality_matches=False)
    pts_list, fus, matched, rows = [], [], [], []
    for l, r, t in zip(left, right, targets):
        mi = matcher(boxlist_iou(t, l))
        matched.append(mi)
        rows.append(t.get_field("box3d").convert("xyzhwl_ry").bbox_3d[mi.clamp(min=0)])
        c = t.get_field("calib")
        probs = l.get_field("mask")
        scale = (M + 2 * pad) / M
        for lbox, rbox, d, prob in zip(l.bbox.tolist(), r.bbox.tolist(), l.get_field("disparity"), probs):
            x1, y1, x2, y2 = int(np.floor(lbox[0])), int(np.floor(lbox[1])), int(np.ceil(lbox[2])), int(np.ceil(lbox[3]))
            x1p, x2p = int(np.floor(rbox[0])), int(np.ceil(rbox[2]))
            wd = max(x2 - x1, x2p - x1p)
            dr = F.interpolate(d[None, None], size=(y2 - y1, wd), mode="bilinear", align_corners=True)[0, 0] / S * wd
            depth = torch.zeros(H, W, device=dev)
            depth[y1:y2, x1:x2] = c.stereo_fuxbaseline / (dr[:, :x2 - x1] + x1 - x1p + 1e-6)
            # Masker paste
            padded = F.pad(prob, (pad, pad, pad, pad))
            wh, hh = (lbox[2] - lbox[0]) * 0.5 * scale, (lbox[3] - lbox[1]) * 0.5 * scale
            xc, yc = (lbox[2] + lbox[0]) * 0.5, (lbox[3] + lbox[1]) * 0.5
            bx0, bx1, by0, by1 = int(xc - wh), int(xc + wh), int(yc - hh), int(yc + hh)
            bw, bh = max(bx1 - bx0 + 1, 1), max(by1 - by0 + 1, 1)
            pm = F.interpolate(padded[None], size=(bh, bw), mode="bilinear", align_corners=False)[0, 0] > thresh
            full = torch.zeros(H, W, dtype=torch.bool, device=dev)
            xa, xb, ya, yb = max(bx0, 0), min(bx1 + 1, W), max(by0, 0), min(by1 + 1, H)
            full[ya:yb, xa:xb] = pm[ya - by0:yb - by0, xa - bx0:xb - bx0]
            if full.sum() != 0 and (depth * full).max() > 0:
                depth = depth * full
            p = c.depthmap_to_rect(depth)[0]
            pos = torch.nonzero(p[:, 2] > 0).squeeze(1)
            n = len(pos)
            if n > npoints:
                choice = rng.choice(n, npoints, replace=False)
            else:
                choice = np.concatenate((np.arange(n), rng.choice(n, npoints - n, replace=True)))
            rng.shuffle(choice)
            pts_list.append(p[pos[torch.from_numpy(choice).to(dev)]])
            fus.append(c.calib.fu)
    pts = torch.stack(pts_list)
    pts[:, :, 2] = pts[:, :, 2].clamp(max=160.0)
    box7 = torch.cat(rows)
    flip = False
    if not m.cfg.RPN.FIXED:
        scale = rng.uniform(0.95, 1.05)
        pts = pts * scale
        box7 = torch.cat([box7[:, :6] * scale, box7[:, 6:]], 1)
        flip = rng.random() < 0.5
    bbox = torch.cat([l.bbox for l in left])
    rot = torch.atan2((bbox[:, 0] + bbox[:, 2]) / 2 - W / 2, torch.tensor(fus, dtype=torch.float64, device=dev))
    if flip:
        pts = torch.cat([-pts[:, :, :1], pts[:, :, 1:]], 2)
        box7 = torch.cat([-box7[:, :1], box7[:, 1:6], (torch.sign(box7[:, 6]) * np.pi - box7[:, 6])[:, None]], 1)
        rot = -rot
    cos, sin = torch.cos(rot).float()[:, None], torch.sin(rot).float()[:, None]

    def rotate(p):
        return torch.stack([p[..., 0] * cos - p[..., 2] * sin, p[..., 1], p[..., 0] * sin + p[..., 2] * cos], -1)
    pts = rotate(pts)
    mean = pts.mean(1)
    pts = pts - mean[:, None]
    corners = rotate(Box3DList(box7, (W, H), "xyzhwl_ry").convert("corners").bbox_3d.view(-1, 8, 3)) - mean[:, None]
    out = []
    for l, t, mi, c in zip(left, targets, matched, torch.split(corners, [len(a) for a in left])):
        b = BoxList(t.bbox[mi.clamp(min=0)], t.size)
        b.add_field("box3d", Box3DList(c.reshape(-1, 24), (W, H), "corners"))
        b.add_field("matched_idxs", mi)
        out.append(b)
    cls_label, reg_label = generate_rpn_training_labels(pts, out)
    return pts, cls_label, reg_label, out


def wall(fn, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e6)
    return BC.stats(ts)


def total_cfg(rcnn_step):
    c = BC.car_cfg().MODEL.POINTRCNN if rcnn_step else BR.car_cfg()
    c["RPN"]["FIXED"] = rcnn_step
    c["RPN"]["USE_BN"] = True
    if rcnn_step:
        c["RCNN"]["ENABLED"], c["RCNN"]["TRAIN"], c["RCNN"]["ROI_SAMPLE_JIT"], c["RCNN"]["LOSS_CLS"] = True, True, True, "SigmoidFocalLoss"
    else:
        c["RCNN"] = BR.make_cfg({"ENABLED": False})
    c["MASK_THRESH"] = 0.7
    return BR.make_cfg({"MODEL": {"POINTRCNN": c}})


def bench_input(dev, iters, warmup):
    m = PointRCNN(total_cfg(False)).to(dev).train()
    left, right, targets = scene(dev)
    a = m.process_input(left, right, targets, rng=np.random.RandomState(0))
    b = torch_process_input(m, left, right, targets, np.random.RandomState(0))
    diff = float((a[0] - b[0]).abs().max())
    same_cls = float((a[1] == b[1]).float().mean())
    rs = np.random.RandomState(1)
    hip = wall(lambda: m.process_input(left, right, targets, rng=rs), iters, warmup)
    comp = wall(lambda: torch_process_input(m, left, right, targets, rs), max(3, iters // 4), 1)
    return {"clouds": int(a[0].shape[0]), "process_input": hip, "torch_composition": comp,
            "speedup": round(comp["median"] / hip["median"], 1), "max_abs_point_diff": diff, "cls_label_agreement": same_cls}


def bench_step(dev, rcnn_step, iters, warmup):
    m = PointRCNN(total_cfg(rcnn_step)).to(dev).train()
    left, right, targets = scene(dev)
    opt = FusedSGD([p for p in (m.rcnn_net if rcnn_step else m.rpn).parameters()], lr=1e-4, momentum=0.9)
    rs = np.random.RandomState(0)
    last = {}

    def step():
        _, losses = m(left, right, targets, rng=rs)
        sum(losses.values()).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        last.update({k: float(v.detach()) for k, v in losses.items()})
    whole = wall(step, iters, warmup)
    inp = wall(lambda: m.process_input(left, right, targets, rng=rs), iters, warmup)
    return {"step": whole, "process_input": inp, "input_share": round(inp["median"] / whole["median"], 3), "losses": last}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["input", "rpn", "rcnn"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointrcnn_train: needs the GPU; there is no CPU path to time")
    dev = "cuda"
    out = {"bench": "pointrcnn_train", "clouds": 16, "points": 768, "device": torch.cuda.get_device_name(0)}
    if a.only in (None, "input"):
        out["input"] = bench_input(dev, a.iters, a.warmup)
    if a.only in (None, "rpn"):
        out["rpn_config"] = bench_step(dev, False, a.iters, a.warmup)
    if a.only in (None, "rcnn"):
        out["rcnn_config"] = bench_step(dev, True, a.iters, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the 3D stage's point ops on one GPU with HIP events: one KITTI pair with 16 ROIs -> InstancePointCloud, and one pass of the
PointRCNN RPN's SA / FP op sequence (ops only, no MLPs; configs/kitti/car/vob/rpn.yaml, config/defaults.py:201-208).

    python tools/bench_points.py [--iters 50] [--warmup 5]

Prints microseconds per stage (median over the timed iterations) as one JSON line.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from disprcnn_amd.layers import pointnet2 as P  # noqa: E402
from disprcnn_amd.modeling.pointcloud import InstancePointCloud  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.structures.calib import Calib  # noqa: E402

SA = [(768, (0.1, 0.5), (16, 32)), (512, (0.5, 1.0), (16, 32)), (256, (1.0, 2.0), (16, 32)), (64, (2.0, 4.0), (16, 32))]
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
P3 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]])


def kitti_pair(dev, R=16, W=1242, H=375, S=224, M=28):
    g = torch.Generator().manual_seed(0)
    x1 = torch.rand(R, generator=g) * (W - 320)
    y1 = 120 + torch.rand(R, generator=g) * 40
    w = 40 + torch.rand(R, generator=g) * 260
    h = 30 + torch.rand(R, generator=g) * 170
    lb = torch.stack([x1, y1, x1 + w, (y1 + h).clamp(max=H - 1)], 1)
    dx = 10 + torch.rand(R, 1, generator=g) * 40
    rb = lb - torch.cat([dx, torch.zeros(R, 1), dx, torch.zeros(R, 1)], 1)
    left = BoxList(lb.to(dev), (W, H))
    left.add_field("disparity", (torch.randn(R, S, S, generator=g) * 2).to(dev))
    left.add_field("mask", torch.rand(R, 1, M, M, generator=g).to(dev) * 0.4 + 0.4)
    return [left], [BoxList(rb.to(dev), (W, H))], [Calib(SimpleNamespace(P2=P2, P3=P3), (W, H))]


def rpn_ops(xyz, feats):
    cur, f = xyz, feats
    levels = [(xyz, feats)]
    for npoint, radii, nsamples in SA:
        idx = P.furthest_point_sample(cur, npoint)
        new = P.gather_operation(cur.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        outs = [P.QueryAndGroup(r, ns)(cur, new, f) for r, ns in zip(radii, nsamples)]
        f = torch.cat([o.max(dim=3)[0] for o in outs], 1).contiguous()
        cur = new
        levels.append((cur, f))
    for i in range(len(levels) - 1, 0, -1):
        (uk, _), (kn, kf) = levels[i - 1], levels[i]
        dist, idx = P.three_nn(uk, kn)
        w = 1.0 / (dist + 1e-8)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        P.three_interpolate(kf, idx, w)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ipc = InstancePointCloud()
    pair = kitti_pair(dev)
    pts, _, _ = ipc(*pair)
    xyz = pts.contiguous()
    feats = torch.randn(16, 8, 768, device=dev)
    out = {"instance_point_cloud_us": timed(lambda: ipc(*pair), a.iters, a.warmup),
           "rpn_sa_fp_ops_us": timed(lambda: rpn_ops(xyz, feats), a.iters, a.warmup),
           "fps_16x768_to_768_us": timed(lambda: P.furthest_point_sample(xyz, 768), a.iters, a.warmup),
           "rois": 16, "npoints": 768, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time PointRCNN's 3D box ops on cuda:0 with HIP events; one JSON line of median microseconds.

    python tools/bench_box3d.py [--iters 50] [--warmup 10]

  nms_batched_us      rotated NMS of 16 rows x 562 boxes (ProposalLayer: 9000 // 16 per ROI) in one nms_gpu_batched call, no sync
  nms_loop_us         the same work as the reference's form: a Python loop of 16 nms_gpu calls (one host sync each)
  iou3d_us            boxes_iou3d_gpu at 512 x 64
  roipool3d_us        roipool3d_gpu at B 16, N 768, M 6, S 512, C 130
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.layers import iou3d, roipool3d
    dev = torch.device("cuda:0")
    r = np.random.RandomState(0)
    B, N = 16, 562
    c = r.uniform(-20, 20, (B, 8, 2))
    k = r.randint(0, 8, (B, N))
    ctr = np.take_along_axis(c, k[..., None], 1) + r.normal(0, 0.5, (B, N, 2))
    sz = r.uniform(1.5, 4.5, (B, N, 2))
    boxes = torch.from_numpy(np.concatenate([ctr - sz / 2, ctr + sz / 2, r.uniform(-np.pi, np.pi, (B, N, 1))], 2).astype(np.float32)).to(dev)
    scores = torch.rand(B, N, device=dev)
    counts = torch.full((B,), N, dtype=torch.int32, device=dev)
    res = {"metric": "box3d_ops_median_us"}
    res["nms_batched_us"] = timed(lambda: iou3d.nms_gpu_batched(boxes, scores, counts, 0.8, max_keep=6), a.iters, a.warmup)
    res["nms_loop_us"] = timed(lambda: [iou3d.nms_gpu(boxes[b], scores[b], 0.8)[:6] for b in range(B)], a.iters, a.warmup)
    b7 = torch.from_numpy(np.stack([r.uniform(-30, 30, 512), r.uniform(1, 2, 512), r.uniform(2, 80, 512), r.uniform(1.2, 2.2, 512),
                                    r.uniform(1.4, 2, 512), r.uniform(3, 5, 512), r.uniform(-np.pi, np.pi, 512)], 1).astype(np.float32)).to(dev)
    gt = (b7[:64] + 0.3 * torch.randn(64, 7, device=dev)).contiguous()
    res["iou3d_us"] = timed(lambda: iou3d.boxes_iou3d_gpu(b7, gt), a.iters, a.warmup)
    pts = torch.stack([torch.rand(768, device=dev) * 6 - 3, torch.rand(768, device=dev) * 2, torch.rand(768, device=dev) * 6 + 17], 1)
    pts = pts.expand(16, 768, 3).contiguous()
    feat = torch.randn(16, 768, 130, device=dev)
    rb = torch.tensor([0.0, 1.8, 20.0, 2.0, 1.8, 4.2, 0.3], device=dev).repeat(16, 6, 1)
    rb[:, :, 0] += torch.linspace(-1, 1, 6, device=dev)
    res["roipool3d_us"] = timed(lambda: roipool3d.roipool3d_gpu(pts, feat, rb, 1.0, 512), a.iters, a.warmup)
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

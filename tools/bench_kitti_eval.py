#!/usr/bin/env python3
"""Time a full KITTI Car evaluation at 0.7 (2D, AOS, BEV and 3D over the three difficulties) on the GPU.

    python tools/bench_kitti_eval.py [--frames 3769] [--runs 5] [--seed 0]

The set is synthetic and has the size of the KITTI val split: 3,769 frames with about 8 ground-truth rows (cars, vans, pedestrians,
DontCare regions) and about 10 detections each, from a seeded generator.  After a warm-up run the evaluation is timed with HIP events; the
split shows the overlap kernel, the two passes, the reduction and the host part (packing the arrays, threshold selection, the curves).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_set(n_frames, seed):
    """-> gt_frames, det_frames in the (types, values) form of layers/kitti_eval.parse_label_lines"""
    rng = np.random.default_rng(seed)
    gt_frames, det_frames = [], []
    for _ in range(n_frames):
        n_obj, n_dc = int(rng.integers(5, 10)), int(rng.integers(0, 3))
        types = [str(t) for t in rng.choice(["Car", "Car", "Car", "Van", "Pedestrian", "Truck"], n_obj)]
        hgt = rng.uniform(18, 140, n_obj)
        x1, y1 = rng.uniform(0, 1100, n_obj), rng.uniform(100, 220, n_obj)
        box = np.stack([x1, y1, x1 + hgt * rng.uniform(0.5, 2.0, n_obj), y1 + hgt], 1)
        g = np.zeros((n_obj, 14))
        g[:, 0] = np.where(rng.random(n_obj) < 0.6, 0.0, rng.uniform(0, 0.6, n_obj))
        g[:, 1] = rng.choice([0, 0, 0, 1, 1, 2, 3], n_obj)
        g[:, 2] = rng.uniform(-3.1, 3.1, n_obj)
        g[:, 3:7] = box
        g[:, 7:10] = np.array([1.5, 1.6, 3.9]) * rng.uniform(0.9, 1.1, (n_obj, 3))
        g[:, 10:13] = np.stack([rng.uniform(-20, 20, n_obj), rng.uniform(1.2, 2.0, n_obj), rng.uniform(6, 60, n_obj)], 1)
        g[:, 13] = rng.uniform(-3.1, 3.1, n_obj)
        dc = np.tile(np.array([-1, -1, -10, 0, 0, 0, 0, -1, -1, -1, -1000, -1000, -1000, -10], np.float64), (n_dc, 1))
        dx, dy = rng.uniform(0, 1000, n_dc), rng.uniform(80, 200, n_dc)
        dc[:, 3:7] = np.stack([dx, dy, dx + rng.uniform(40, 200, n_dc), dy + rng.uniform(30, 100, n_dc)], 1)
        gt_frames.append((types + ["DontCare"] * n_dc, np.concatenate([g, dc])))
        # detections: most objects found, with noise at three levels, plus false positives
        found = np.flatnonzero(rng.random(n_obj) < 0.85)
        level = rng.choice([0.01, 0.04, 0.12], len(found))[:, None]
        d = np.zeros((len(found), 13))
        d[:, 0] = g[found, 2] + rng.normal(0, 0.3, len(found))
        wh = np.stack([box[found, 2] - box[found, 0], box[found, 3] - box[found, 1]] * 2, 1)
        d[:, 1:5] = box[found] + rng.normal(0, 1, (len(found), 4)) * level * wh
        d[:, 5:8] = g[found, 7:10] * (1 + rng.normal(0, 1, (len(found), 3)) * level)
        d[:, 8:11] = g[found, 10:13] + rng.normal(0, 1, (len(found), 3)) * level * 2
        d[:, 11] = g[found, 13] + rng.normal(0, 1, len(found)) * level[:, 0] * 2
        d[:, 12] = rng.uniform(0.05, 1.0, len(found))
        n_fp = int(rng.integers(2, 6))
        fp = np.zeros((n_fp, 13))
        fh = rng.uniform(18, 140, n_fp)
        fx, fy = rng.uniform(0, 1100, n_fp), rng.uniform(100, 220, n_fp)
        fp[:, 0] = rng.uniform(-3.1, 3.1, n_fp)
        fp[:, 1:5] = np.stack([fx, fy, fx + fh * rng.uniform(0.5, 2.0, n_fp), fy + fh], 1)
        fp[:, 5:8] = np.array([1.5, 1.6, 3.9]) * rng.uniform(0.9, 1.1, (n_fp, 3))
        fp[:, 8:11] = np.stack([rng.uniform(-20, 20, n_fp), rng.uniform(1.2, 2.0, n_fp), rng.uniform(6, 60, n_fp)], 1)
        fp[:, 11], fp[:, 12] = rng.uniform(-3.1, 3.1, n_fp), rng.uniform(0.05, 0.9, n_fp)
        det_frames.append((["Car"] * (len(found) + n_fp), np.concatenate([d, fp])))
    return gt_frames, det_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch

    from disprcnn_amd.layers.kitti_eval import kitti_eval_stats
    assert torch.cuda.is_available(), "bench_kitti_eval needs a GPU"
    gt_frames, det_frames = synthetic_set(args.frames, args.seed)
    n_gt, n_det = sum(len(t) for t, _ in gt_frames), sum(len(t) for t, _ in det_frames)
    stats = kitti_eval_stats(gt_frames, det_frames, "car", 0.7)                 # warm-up (loads the library, first launches)
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.runs):
        timings = {}
        t0 = time.perf_counter()
        again = kitti_eval_stats(gt_frames, det_frames, "car", 0.7, timings=timings)
        torch.cuda.synchronize()
        timings["total_ms"] = (time.perf_counter() - t0) * 1e3
        assert all(again[k].tobytes() == stats[k].tobytes() for k in stats)
        runs.append(timings)
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    ap11 = {k: (v[:, ::4].mean(1) * 100).round(2).tolist() for k, v in stats.items()}
    print(f"{args.frames} frames, {n_gt} ground-truth rows, {n_det} detections; median of {args.runs} runs after a warm-up")
    for k in ("overlaps_ms", "pass1_ms", "thresholds_ms", "pass2_ms", "reduce_ms", "host_ms", "total_ms"):
        print(f"  {k:14s} {med[k]:9.3f}")
    print(json.dumps({"tool": "bench_kitti_eval", "frames": args.frames, "gt_rows": n_gt, "detections": n_det, "runs": args.runs,
                      "median_ms": {k: round(v, 3) for k, v in med.items()}, "ap11": ap11}))


if __name__ == "__main__":
    main()

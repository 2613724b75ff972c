#!/usr/bin/env python3
"""Time the 3D detector behind DispRCNN3D (MODEL.DET3D_ON) on one GPU with HIP events.

    python tools/bench_det3d.py [--iters 30] [--warmup 5] [--parts frame,offline,online]

Parts (each may be run alone, so that a job can give every one its own time limit):
  frame    PointRCNN.proposals_to_camera (one kernel) against proposals_to_camera_unfused (the torch composition it replaced) on the RPN's
           real output, car config, B = 16 and B = 1 clouds, alternating in one process after a warm-up of both; medians with [min, max].
  offline  the DET3D_ON evaluation forward without the PSMNet (MODEL.DISPNET_ON false) on the golden instance-cloud scene (12 instances
           in 2 images, tests/golden/points_ref_golden.npz), split into InstancePointCloud, RPN, frame change, refine and the host copy
           of the fields, and the whole call.  InstancePointCloud reads its per-ROI counts on the host in the middle, so its span holds
           that wait.
  online   both flags on one KITTI-size pair (375 x 1242, 16 ROIs, masks of ones): the whole call, and the 3D stage run alone on what
           the disparity stage left on the results, as a share of it.
Event times in microseconds (`wall` entries: host clock around a synchronised call), one JSON line.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_rcnn as BC  # noqa: E402
import bench_rpn as BR  # noqa: E402
from disprcnn_amd.modeling.detector.disprcnn3d import DispRCNN3D, default_cfg  # noqa: E402
from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net import point_rcnn as PR  # noqa: E402
from disprcnn_amd.structures import BoxList, ImageList  # noqa: E402
from disprcnn_amd.structures.calib import Calib  # noqa: E402
from disprcnn_amd.utils import synth  # noqa: E402

KITTI_P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
KITTI_P3 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]])


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return BC.stats(out)


def frame_part(dev, iters, warmup):
    m = BC.build_model(dev)
    res = {}
    with torch.no_grad():
        for B in (16, 1):
            pts = BR.clouds(B, dev)
            out, _ = m.rpn(pts)
            mean = torch.tensor([1.5, 1.0, 20.0], device=dev).repeat(B, 1)
            rot = torch.full((B,), 0.1, dtype=torch.float64, device=dev)
            fused, unfused = BC.time_alternating(lambda: m.proposals_to_camera(out, mean, rot),
                                                 lambda: PR.proposals_to_camera_unfused(out, mean, rot), iters, warmup)
            res[f"B{B}"] = {"clouds": B, "points": out["backbone_xyz"].shape[1], "rois_per_cloud": out["roi_boxes3d"].shape[1], "fused": fused,
                            "unfused": unfused, "speedup": round(unfused["median"] / fused["median"], 2),
                            "ranges_apart": fused["max"] < unfused["min"]}
    return res


def golden_scene(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "points_ref_golden.npz"))
    W, H = int(g["W"]), int(g["H"])
    left, right, calibs, r = [], [], [], 0
    for n, cam in zip(g["rois_per_image"].tolist(), [(g["P2"], g["P3"]), (g["P2B"], g["P3B"])]):
        lb = BoxList(torch.from_numpy(g["left_boxes"][r:r + n]).to(dev), (W, H))
        lb.add_field("disparity", torch.from_numpy(g["disparity"][r:r + n]).to(dev))
        lb.add_field("mask", torch.from_numpy(g["mask"][r:r + n]).to(dev))
        left.append(lb)
        right.append(BoxList(torch.from_numpy(g["right_boxes"][r:r + n]).to(dev), (W, H)))
        calibs.append(Calib(SimpleNamespace(P2=cam[0], P3=cam[1]), (W, H)))
        r += n
    return left, right, calibs


def detector(dev, dispnet):
    cfg = default_cfg(48, -48, 224)
    cfg.MODEL.DET3D_ON, cfg.MODEL.DISPNET_ON, cfg.MODEL.POINTRCNN = True, dispnet, BC.car_cfg().MODEL.POINTRCNN
    model = DispRCNN3D(cfg)
    model.pcnet.load_state_dict(BC.build_model(dev).state_dict())
    if dispnet:
        sd = synth.synth_state_dict(model.dispnet.state_dict(), tempered=True)
        bn = os.path.join(ROOT, "tests", "golden", "bn_stats_At.npz")
        if os.path.exists(bn):
            synth.load_bn_stats(sd, bn)
        model.dispnet.load_state_dict(sd, strict=True)
    return model.to(dev).eval()


def split_3d(pc, left, right, calibs, st):
    """PointRCNN._forward_val restated with stage marks"""
    left, right = PR.remove_empty_proposals(left, right)
    with st("instance_point_cloud"):
        pts, mean, rot = pc.pointcloud(left, right, calibs)
    with st("rpn"):
        out, _ = pc.rpn(pts)
    with st("frame_change"):
        cam = pc.proposals_to_camera(out, mean, rot)
    with st("refine"):
        box, score, random = pc.rcnn_net.refine(cam)
    with st("host_copy"):
        PR.combine_2d_3d(left, box, score, random)


def offline_part(dev, iters, warmup):
    model = detector(dev, dispnet=False)
    left, right, calibs = golden_scene(dev)
    stages = {}
    with torch.no_grad():
        for it in range(warmup + iters):
            st = BR.Stages(it >= warmup)
            split_3d(model.pcnet, left, right, calibs, st)
            torch.cuda.synchronize()
            for k, v in st.totals().items():
                stages.setdefault(k, []).append(v)
        res = {"instances": sum(len(a) for a in left), "images": len(left), "stages": {k: BC.stats(v) for k, v in stages.items()}}
        res["stages_sum_of_medians"] = round(sum(v["median"] for v in res["stages"].values()), 1)
        res["forward_wall"] = wall(lambda: model(None, {"left": left, "right": right}, {"left": calibs}), iters, warmup)
    return res


def online_part(dev, iters, warmup):
    W, H, R = 1242, 375, 16
    model = detector(dev, dispnet=True)
    base = synth.hash_uniform("bench3d:L", (1, 3, H // 8, W // 8), 0.0, 1.0)
    limg = torch.nn.functional.interpolate(base, (H, W), mode="bilinear", align_corners=True)
    rimg = torch.roll(limg, -6, 3)
    x1 = torch.linspace(20.0, 1000.0, R)
    y1 = 120.0 + 10.0 * (torch.arange(R) % 4)
    lb = torch.stack([x1, y1, x1 + 150.0 + 5.0 * (torch.arange(R) % 5), y1 + 110.0 + 6.0 * (torch.arange(R) % 3)], 1)
    rb = lb - torch.tensor([6.0, 0.0, 6.0, 0.0])
    left = BoxList(lb.to(dev), (W, H))
    left.add_field("mask", torch.ones(R, 1, 28, 28, device=dev))
    results = {"left": [left], "right": [BoxList(rb.to(dev), (W, H))]}
    images = {"left": ImageList(limg.to(dev), [(H, W)]), "right": ImageList(rimg.to(dev), [(H, W)])}
    targets = {"left": [Calib(SimpleNamespace(P2=KITTI_P2, P3=KITTI_P3), (W, H))]}
    with torch.no_grad():
        out = model(images, results, targets)
        l2 = [lr.copy_with_fields(["disparity", "mask"]) for lr in out["left"]]
        r2 = [BoxList(rr.bbox, rr.size) for rr in out["right"]]
        total = wall(lambda: model(images, results, targets), iters, warmup)
        stage3d = wall(lambda: model.pcnet(l2, r2, targets["left"]), iters, warmup)
    return {"image": [H, W], "rois": R, "kept_points_min": min(model.pcnet.pointcloud.last_counts), "forward_wall": total, "stage_3d_wall": stage3d,
            "stage_3d_share": round(stage3d["median"] / total["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parts", default="frame,offline,online")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"iters": a.iters, "unit": "us"}
    parts = {"frame": frame_part, "offline": offline_part, "online": online_part}
    for name in a.parts.split(","):
        res[name] = parts[name](dev, a.iters, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

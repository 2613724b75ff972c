#!/usr/bin/env python3
"""Time PointRCNN's ProposalTargetLayer and the RCNN training step it completes (car config, RCNN.ROI_SAMPLE_JIT = True) on one GPU with
HIP events.

    python tools/bench_proposal_target.py [--iters 20] [--warmup 3] [--clouds 16] [--candidates 100] [--points 2048]

At the car config: B = 16 clouds of M = 100 candidates, P = ROI_PER_IMAGE = 16 slots, S = 512 pooled points, C = 128 feature channels,
T = ROI_FG_AUG_TIMES = 10, seeded (candidates scattered around one ground-truth box per cloud so that every class occurs):
  * layer: ProposalTargetLayer.sample alone (the draws' torch.rand, the sampling kernel, the pooling kernel), and its two kernels on
    their own;
  * step_jit: forward + loss + backward of RCNNNet.train()(proposals, targets) with ROI_SAMPLE_JIT = True;
  * step_presampled: the same network, loss and backward with ROI_SAMPLE_JIT = False on the layer's own outputs repacked as sampled
    ROIs, alternating with step_jit in one process after a warm-up of both.
Medians with min / max as the spread, microseconds, one JSON line.  No ratio here is a pass criterion.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_rpn as BR  # noqa: E402
from bench_rcnn import stats, time_alternating, timed  # noqa: E402
from disprcnn_amd.layers import proposal_target as PT  # noqa: E402
from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.structures.bounding_box_3d import Box3DList  # noqa: E402


def car_cfg(jit):
    with open(os.path.join(ROOT, "tests", "golden", "rcnn_cfg_car.json")) as f:
        c = json.load(f)
    c["RCNN"]["ROI_SAMPLE_JIT"] = jit
    c["RCNN"]["LOSS_CLS"] = "SigmoidFocalLoss"            # the sampled labels hold -1
    c["AUG_DATA"], c["AUG_ROT_RANGE"] = True, 18
    return BR.make_cfg(c)


def make_inputs(B, M, N, C, cfg, dev):
    rs = np.random.RandomState(B * 1000 + M)
    size = np.array(cfg.MEAN_SIZE[0])
    gt = np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(0.8, 1.8, (B, 1)), rs.uniform(14, 30, (B, 1)), size * rs.uniform(0.9, 1.1, (B, 3)),
                         rs.uniform(-np.pi, np.pi, (B, 1))], 1)
    spread = rs.choice([0.15, 0.6, 3.0], (B, M, 1))       # near, overlapping and far candidates: fg, hard and easy background
    cand = gt[:, None] + rs.normal(0, 1, (B, M, 7)) * spread * np.array([1.0, 0.15, 1.6, 0.1, 0.1, 0.2, 0.25])
    local = rs.uniform(-0.6, 0.6, (B, N, 3)) * gt[:, None, [5, 3, 4]]
    ca, sa = np.cos(gt[:, None, 6]), np.sin(gt[:, None, 6])
    xyz = np.stack([gt[:, None, 0] + local[..., 0] * ca + local[..., 2] * sa, gt[:, None, 1] - gt[:, None, 3] / 2 + local[..., 1],
                    gt[:, None, 2] - local[..., 0] * sa + local[..., 2] * ca], 2)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    prop = {"roi_boxes3d": f(cand), "rpn_xyz": f(xyz), "backbone_features": f(np.maximum(rs.normal(0, 0.6, (B, C, N)), 0)),
            "seg_mask": f(rs.uniform(size=(B, N)) < 0.7), "pts_depth": f(np.sqrt((xyz ** 2).sum(2)) + 20.0),
            "roi_scores_raw": torch.zeros(B, M, device=dev)}
    targets = []
    for b in range(B):
        bl = BoxList(torch.tensor([[0.0, 0.0, 10.0, 10.0]], device=dev), (1280, 384), "xyxy")
        bl.add_field("box3d", Box3DList(f(gt[b:b + 1]), (1280, 384), "xyzhwl_ry"))
        targets.append(bl)
    return prop, targets, f(gt[:, None])


def run_step(net, *args):
    for q in net.parameters():
        q.grad = None
    net(*args)[1]["loss_box3d"].backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--points", type=int, default=2048)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = car_cfg(True)
    rc = cfg.RCNN
    B, M, P, T = a.clouds, a.candidates, rc.ROI_PER_IMAGE, rc.ROI_FG_AUG_TIMES
    torch.manual_seed(0)
    net = RCNNNet(copy.deepcopy(cfg), None).to(dev).train()
    with torch.no_grad():
        net.reg_layer[-1].conv.weight.normal_(0, 0.05)
    other = RCNNNet(car_cfg(False), None).to(dev).train()
    other.load_state_dict(net.state_dict())
    prop, targets, gt = make_inputs(B, M, a.points, 128, cfg, dev)
    prop["draws"] = PT.proposal_draws(B, M, P, T, dev, generator=torch.Generator(device=dev).manual_seed(1))
    layer = net.proposal_target_layer
    s = layer.sample(prop, gt, draws=prop["draws"])
    counts = s["counts"].sum(0).tolist()
    pre = {"pts_input": torch.cat([s["pts"], s["feat"]], 1).transpose(1, 2).contiguous(), "roi_boxes3d": s["roi_boxes3d"],
           "cls_label": s["cls_label"].float(), "reg_valid_mask": s["reg_valid_mask"], "gt_boxes3d_ct": s["gt_of_rois"]}
    st = dict(P=P, fg=rc.FG_RATIO, reg=rc.REG_FG_THRESH, cls=rc.CLS_FG_THRESH, bg=rc.CLS_BG_THRESH, lo=rc.CLS_BG_THRESH_LO, hard=rc.HARD_BG_RATIO)

    def sampler():
        return PT.rcnn_sample_rois(prop["roi_boxes3d"], gt, prop["draws"], st["P"], st["fg"], st["reg"], st["cls"], st["bg"], st["lo"], st["hard"], T,
                                   rc.REG_AUG_METHOD)
    sampled = sampler()

    def pooling():
        return PT.rcnn_pool_target(prop["rpn_xyz"], prop["backbone_features"], prop["seg_mask"], prop["pts_depth"] if rc.USE_DEPTH else None, sampled,
                                   prop["draws"], rc.POOL_EXTRA_WIDTH, st["reg"], st["cls"], st["bg"], sampled_pt_num=rc.NUM_POINTS, aug_data=True,
                                   aug_rot_range=18, num_candidates=M, fg_aug_times=T)
    no_draws = {k: v for k, v in prop.items() if k != "draws"}
    res = {"iters": a.iters, "unit": "us", "clouds": B, "candidates": M, "slots": P, "points": a.points, "pooled_points": rc.NUM_POINTS,
           "candidate_counts_fg_hard_easy": counts[:3], "noise_iterations": int(s["n_iter"].sum()),
           "labels_fg_bg_ignored": [int((s["cls_label"] == v).sum()) for v in (1, 0, -1)],
           "layer": stats(timed(lambda: layer.sample(no_draws, gt), a.iters, a.warmup)),
           "sample_rois_kernel": stats(timed(sampler, a.iters, a.warmup)), "pool_target_kernel": stats(timed(pooling, a.iters, a.warmup))}
    jit, presampled = time_alternating(lambda: run_step(net, prop, targets), lambda: run_step(other, pre), a.iters, a.warmup)
    res["step_jit"], res["step_presampled"] = jit, presampled
    with torch.no_grad():
        res["loss_jit"], res["loss_presampled"] = net(prop, targets)[1]["loss_box3d"].item(), other(pre)[1]["loss_box3d"].item()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

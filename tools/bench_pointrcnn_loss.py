#!/usr/bin/env python3
"""Time PointRCNN's training losses, forward + backward, on one GPU with HIP events.

    python tools/bench_pointrcnn_loss.py [--iters 50] [--warmup 10] [--inner 20]

Two workloads: the RPN loss (PointRCNNLossComputation, BinaryCrossEntropy, 52 channels) at 16 clouds x 768 points, and the RCNN loss
(PointRCNNBox3dLossComputation, SigmoidFocalLoss, 46 channels) at 256 ROIs.  Each is timed against the same arithmetic composed from torch
ops on the GPU -- this tool's own unfused restatement, written without compaction or host reads (masks and torch.where), so it is the
fair comparator, not the reference's sync-bound code.  Both are checked against each other before anything is timed.

Method: every shape warmed up, then `iters` windows per variant, alternating; a window is `inner` forward + backward passes between two
events (a single pass is tens of microseconds: too short a window on its own).  Medians and the min-max spread, microseconds per pass, one JSON line.
A second JSON line gives the kernel launches per pass of both variants, counted by torch.profiler in a run of their own.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_loss import PointRCNNBox3dLossComputation  # noqa: E402
from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn_loss import PointRCNNLossComputation  # noqa: E402

MEAN_SIZE = [1.52563191462, 1.62856739989, 3.88311640418]


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def make_cfg(d):
    return Cfg({k: make_cfg(v) if isinstance(v, dict) else v for k, v in d.items()})


CFG = make_cfg({
    "MEAN_SIZE": [MEAN_SIZE],
    "RPN": {"LOSS_CLS": "BinaryCrossEntropy", "FOCAL_ALPHA": [0.25, 0.75], "FOCAL_GAMMA": 2.0, "FG_WEIGHT": 15.0, "NPOINTS": 768,
            "LOC_SCOPE": 3.0, "LOC_BIN_SIZE": 0.5, "NUM_HEAD_BIN": 12, "LOC_XZ_FINE": False, "LOSS_WEIGHT": [1.0, 1.0]},
    "RCNN": {"LOSS_CLS": "SigmoidFocalLoss", "FOCAL_ALPHA": [0.25, 0.75], "FOCAL_GAMMA": 2.0, "ROI_PER_IMAGE": 64, "SIZE_RES_ON_ROI": False,
             "LOC_SCOPE": 1.5, "LOC_BIN_SIZE": 0.5, "NUM_HEAD_BIN": 9, "LOC_Y_BY_BIN": False, "LOC_Y_SCOPE": 0.5, "LOC_Y_BIN_SIZE": 0.25},
})


# ---- the unfused restatement: all rows, weights instead of selections
def torch_reg_loss(pred, lab, w, scope, bs, H, anchor, xz_fine, ry_fine, masked):
    """-> loc, angle, size; w (rows) = selected (and loss-masked) rows as 0 / 1.  `masked`: the reference's loss_mask form (sum / count)."""
    P = int(scope / bs) * 2
    cnt = w.sum()
    dm = torch.where(cnt != 0, cnt, torch.ones_like(cnt))

    def red(v):
        return (v * w).sum() / dm

    def onehot_pick(block, label):
        return torch.gather(block, 1, label.view(-1, 1)).squeeze(1)

    xs = torch.clamp(lab[:, 0] + scope, 0, scope * 2 - 1e-3)
    zs = torch.clamp(lab[:, 2] + scope, 0, scope * 2 - 1e-3)
    xb, zb = (xs / bs).floor().long(), (zs / bs).floor().long()
    loc = red(F.cross_entropy(pred[:, 0:P], xb, reduction="none")) + red(F.cross_entropy(pred[:, P:2 * P], zb, reduction="none"))
    off = 2 * P
    if xz_fine:
        xr = (xs - (xb.float() * bs + bs / 2)) / bs
        zr = (zs - (zb.float() * bs + bs / 2)) / bs
        loc = loc + red(F.smooth_l1_loss(onehot_pick(pred[:, 2 * P:3 * P], xb), xr, reduction="none"))
        loc = loc + red(F.smooth_l1_loss(onehot_pick(pred[:, 3 * P:4 * P], zb), zr, reduction="none"))
        off = 4 * P
    loc = loc + red(F.smooth_l1_loss(pred[:, off], lab[:, 1], reduction="none"))
    off += 1
    ry = lab[:, 6]
    if ry_fine:
        apc = (math.pi / 2) / H
        ry = ry % (2 * math.pi)
        opp = (ry > math.pi * 0.5) & (ry < math.pi * 1.5)
        ry = torch.where(opp, (ry + math.pi) % (2 * math.pi), ry)
        shift = torch.clamp((ry + math.pi * 0.5) % (2 * math.pi) - math.pi * 0.25, min=1e-3, max=math.pi * 0.5 - 1e-3)
    else:
        apc = (2 * math.pi) / H
        shift = (ry % (2 * math.pi) + apc / 2) % (2 * math.pi)
    rb = (shift / apc).floor().long()
    rr = (shift - (rb.float() * apc + apc / 2)) / (apc / 2)
    angle = red(F.cross_entropy(pred[:, off:off + H], rb, reduction="none"))
    angle = angle + red(F.smooth_l1_loss(onehot_pick(pred[:, off + H:off + 2 * H], rb), rr, reduction="none"))
    off += 2 * H
    sz = F.smooth_l1_loss(pred[:, off:off + 3], (lab[:, 3:6] - anchor) / anchor, reduction="none")
    size = (sz * w[:, None]).sum() / (dm if masked else 3 * dm)
    return loc, angle, size


def torch_rpn_loss(cls, reg, cls_label, reg_label, matched, anchor):
    r = CFG.RPN
    m = (matched >= 0).unsqueeze(-1).repeat(1, r.NPOINTS).view(-1).float()
    lab = cls_label.view(-1)
    x = cls.view(-1)
    t = (lab > 0).float()
    wt = torch.where(lab > 0, torch.full_like(x, r.FG_WEIGHT), torch.ones_like(x))
    valid = (lab >= 0).float() * m
    loss_cls = (F.binary_cross_entropy_with_logits(x, t, weight=wt, reduction="none") * valid).sum() / torch.clamp(valid.sum(), min=1.0)
    n = reg.shape[0] * reg.shape[1]
    loc, angle, size = torch_reg_loss(reg.view(n, -1), reg_label.view(n, 7), t * m, r.LOC_SCOPE, r.LOC_BIN_SIZE, r.NUM_HEAD_BIN, anchor,
                                      r.LOC_XZ_FINE, False, True)
    return loss_cls * r.LOSS_WEIGHT[0] + (loc + angle + 3 * size) * r.LOSS_WEIGHT[1]


def torch_rcnn_loss(cls, reg, cls_label, reg_valid, gt, anchor):
    r = CFG.RCNN
    x, lab = cls.view(-1), cls_label.view(-1)
    pos, neg = (lab > 0).float(), (lab == 0).float()
    wts = (pos + neg) / torch.clamp(pos.sum(), min=1.0)
    ce = torch.clamp(x, min=0) - x * pos + torch.log1p(torch.exp(-torch.abs(x)))
    p = torch.sigmoid(x)
    pt = pos * p + (1 - pos) * (1 - p)
    loss_cls = (torch.pow(1.0 - pt, r.FOCAL_GAMMA) * (pos * r.FOCAL_ALPHA[0] + (1 - pos) * (1 - r.FOCAL_ALPHA[0])) * ce * wts).sum()
    loc, angle, size = torch_reg_loss(reg, gt, (reg_valid > 0).float(), r.LOC_SCOPE, r.LOC_BIN_SIZE, r.NUM_HEAD_BIN, anchor, True, True, False)
    return loss_cls + loc + angle + 3 * size


def reg_labels(rs, rows, scope):
    lab = np.empty((rows, 7), np.float32)
    lab[:, 0] = rs.uniform(-1.3 * scope, 1.3 * scope, rows)
    lab[:, 1] = rs.uniform(-0.8, 0.8, rows)
    lab[:, 2] = rs.uniform(-1.3 * scope, 1.3 * scope, rows)
    lab[:, 3:6] = np.array(MEAN_SIZE) * rs.uniform(0.8, 1.2, (rows, 3))
    lab[:, 6] = rs.uniform(-2 * math.pi, 3 * math.pi, rows)
    return lab


def workloads(dev):
    rs = np.random.RandomState(0)
    B, N, R = 16, 768, 256
    anchor = torch.tensor(MEAN_SIZE, dtype=torch.float32, device=dev)

    def t(a, grad=False):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)

    u = rs.uniform(size=(B, N))
    rpn = dict(cls=t(rs.uniform(-6, 6, (B, N, 1)).astype(np.float32), True), reg=t(rs.normal(0, 1.5, (B, N, 52)).astype(np.float32), True),
               cls_label=t(np.where(u < 0.3, 1.0, np.where(u < 0.4, -1.0, 0.0)).astype(np.float32)),
               reg_label=t(reg_labels(rs, B * N, 3.0).reshape(B, N, 7)), matched=t(np.where(np.arange(B) % 5 == 4, -1, 0).astype(np.int64)))
    u = rs.uniform(size=R)
    rcnn = dict(cls=t(rs.uniform(-6, 6, (R, 1)).astype(np.float32), True), reg=t(rs.normal(0, 1.5, (R, 46)).astype(np.float32), True),
                cls_label=t(np.where(u < 0.4, 1.0, np.where(u < 0.5, -1.0, 0.0)).astype(np.float32)),
                reg_valid=t((rs.uniform(size=R) < 0.5).astype(np.int64)), gt=t(reg_labels(rs, R, 1.5)),
                roi=t(np.concatenate([rs.uniform(-2, 2, (R, 3)), np.tile(MEAN_SIZE, (R, 1)), rs.uniform(-3, 3, (R, 1))], 1).astype(np.float32)))
    rpn_ev, rcnn_ev = PointRCNNLossComputation(CFG), PointRCNNBox3dLossComputation(CFG)

    def rpn_fused():
        o = rpn_ev(rpn["cls"], rpn["reg"], rpn["cls_label"], rpn["reg_label"], rpn["matched"])
        return o["rpn_loss_cls"] + o["rpn_loss_reg"]

    def rpn_unfused():
        return torch_rpn_loss(rpn["cls"], rpn["reg"], rpn["cls_label"], rpn["reg_label"], rpn["matched"], anchor)

    labels = {"cls_label": rcnn["cls_label"], "reg_valid_mask": rcnn["reg_valid"], "roi_boxes3d": rcnn["roi"], "gt_of_rois": rcnn["gt"],
              "pts_input": torch.zeros((R, 1), device=dev)}

    def rcnn_fused():
        return rcnn_ev({"rcnn_cls": rcnn["cls"], "rcnn_reg": rcnn["reg"]}, None, labels, None)

    def rcnn_unfused():
        return torch_rcnn_loss(rcnn["cls"], rcnn["reg"], rcnn["cls_label"], rcnn["reg_valid"], rcnn["gt"], anchor)

    return {"rpn_16x768": (rpn_fused, rpn_unfused, (rpn["cls"], rpn["reg"])), "rcnn_256": (rcnn_fused, rcnn_unfused, (rcnn["cls"], rcnn["reg"]))}


def step(fn, leaves):
    for p in leaves:
        p.grad = None
    fn().backward()


def agree(fused, unfused, leaves):
    out = []
    for fn in (fused, unfused):
        for p in leaves:
            p.grad = None
        loss = fn()
        loss.backward()
        out.append((loss.item(), [p.grad.clone() for p in leaves]))
    (la, ga), (lb, gb) = out
    assert abs(la - lb) <= 1e-4 * abs(lb), (la, lb)
    for a, b in zip(ga, gb):
        assert (a - b).abs().max().item() <= 1e-5 * max(b.abs().max().item(), 1e-30) + 1e-9, (a - b).abs().max().item()
    return la


def count_launches(fn, leaves):
    from torch.profiler import ProfilerActivity, profile
    step(fn, leaves)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(fn, leaves)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointrcnn_loss: no GPU; this tool measures on an MI355X only")
    dev = torch.device("cuda")
    res = {"iters": args.iters, "inner": args.inner}
    work = workloads(dev)
    for name, (fused, unfused, leaves) in work.items():
        loss = agree(fused, unfused, leaves)
        for _ in range(args.warmup):
            step(fused, leaves)
            step(unfused, leaves)
        torch.cuda.synchronize()
        evs = []
        for _ in range(args.iters):
            for tag, fn in (("fused", fused), ("unfused", unfused)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    step(fn, leaves)
                b.record()
                evs.append((tag, a, b))
        torch.cuda.synchronize()
        t = {"fused": [], "unfused": []}
        for tag, a, b in evs:
            t[tag].append(a.elapsed_time(b) * 1e3 / args.inner)
        res[name] = {"loss": loss}
        for tag, v in t.items():
            res[name][f"{tag}_us"] = float(np.median(v))
            res[name][f"{tag}_us_min_max"] = [float(np.min(v)), float(np.max(v))]
        res[name]["speedup"] = res[name]["unfused_us"] / res[name]["fused_us"]
    print(json.dumps(res), flush=True)
    if not args.no_launches:
        print(json.dumps({"launches_per_pass": {name: {"fused": count_launches(f, leaves), "unfused": count_launches(u, leaves)}
                                                for name, (f, u, leaves) in work.items()}}), flush=True)


if __name__ == "__main__":
    main()

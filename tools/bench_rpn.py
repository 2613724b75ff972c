#!/usr/bin/env python3
"""Time PointRCNN's RPN inference (car config: 768 points, SA_CONFIG.NPOINTS [768, 512, 256, 64]) on one GPU with HIP events.

    python tools/bench_rpn.py [--iters 30] [--warmup 5] [--batches 16,1]
    python tools/bench_rpn.py --levels [--iters 20]      # only the fused SA kernels of the two widest levels, for a kernel trace

Per batch size: the forward with the fused HIP shared MLPs and the same network with the MLPs done the materialising way
(grouping_operation -> torch conv2d / conv1d on a concatenated input -> max), timed in the same process, alternating, after a warm-up
of every shape; and the fused forward split per stage (index ops / SA MLPs / FP MLPs / heads / proposals).  Medians in microseconds,
one JSON line.  `flops` counts the shared-MLP multiply-adds (x2) from the shapes; `sa_level_tflops` is that count over the
event-timed fused kernels of SA levels 3 and 4 (for the fraction of the 157 TFLOP/s fp32-MFMA rate, take the kernel times of a
`rocprofv3 --kernel-trace --stats -- python tools/bench_rpn.py --levels` run: events include launch gaps).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from disprcnn_amd.layers import pn2_mlp  # noqa: E402
from disprcnn_amd.layers import pointnet2 as P  # noqa: E402
from disprcnn_amd.layers.rpn_proposals import points_depth  # noqa: E402
from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN  # noqa: E402

PEAK_TFLOPS = 157.0


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def make_cfg(d):
    return Cfg({k: make_cfg(v) if isinstance(v, dict) else v for k, v in d.items()})


def car_cfg():
    with open(os.path.join(ROOT, "tests", "golden", "rpn_cfg_car.json")) as f:
        return make_cfg(json.load(f))


def build_model(cfg, dev):
    torch.manual_seed(0)
    m = RPN(cfg, None)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.75, 1.25)
                mod.weight.uniform_(0.75, 1.25)
                mod.bias.normal_(0, 0.1)
        m.rpn_reg_layer[-1].conv.weight.normal_(0, 0.05)
        m.rpn_reg_layer[-1].conv.bias.normal_(0, 0.5)
    return m.to(dev).eval()


def clouds(B, dev, n=768):
    g = torch.Generator().manual_seed(1)
    p = (torch.rand(B, n, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.8, 2.1])
    p[:, :, 0] = torch.where(torch.rand(B, n, generator=g) < 0.7, torch.full((B, n), -1.0), p[:, :, 0]) + 0.03 * torch.randn(B, n, generator=g)
    return (p - p.mean(1, keepdim=True)).to(dev).contiguous()


class Stages:
    """HIP-event pairs per named stage; a stage may be entered many times in one forward"""

    def __init__(self, on):
        self.on, self.ev = on, []

    def __call__(self, name):
        return _Span(self, name)

    def totals(self):
        out = {}
        for name, a, b in self.ev:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e3
        return out


class _Span:
    def __init__(self, st, name):
        self.st, self.name = st, name

    def __enter__(self):
        if self.st.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.st.on:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.st.ev.append((self.name, self.a, b))


def forward(m, pts, fused, st):
    """RPN.forward restated with stage marks; fused=False does the shared MLPs with torch on materialised tensors"""
    bb = m.backbone_net
    l_xyz, l_feat = [pts], [None]
    for sa in bb.SA_modules:
        xyz, feats = l_xyz[-1], l_feat[-1]
        with st("index_ops"):
            fidx = P.furthest_point_sample(xyz, sa.npoint)
            new_xyz = P.gather_operation(xyz.transpose(1, 2).contiguous(), fidx).transpose(1, 2).contiguous()
            idxs = [P.ball_query(g.radius, g.nsample, xyz, new_xyz) for g in sa.groupers]
        with st("sa_mlp"):
            folded = [mlp.folded() for mlp in sa.mlps]
            if fused:
                out = torch.empty((xyz.shape[0], sum(f[-1].cout for f in folded), new_xyz.shape[1]), dtype=torch.float32, device=xyz.device)
                c = 0
                for idx, layers in zip(idxs, folded):
                    pn2_mlp.sa_mlp_max(xyz, new_xyz, feats, idx, layers, out=out, c_off=c)
                    c += layers[-1].cout
            else:
                out = torch.cat([pn2_mlp.sa_mlp_max_unfused(xyz, new_xyz, feats, idx, layers) for idx, layers in zip(idxs, folded)], 1)
        l_xyz.append(new_xyz)
        l_feat.append(out)
    for i in range(-1, -(len(bb.FP_modules) + 1), -1):
        with st("index_ops"):
            dist, idx = P.three_nn(l_xyz[i - 1], l_xyz[i])
            r = 1.0 / (dist + 1e-8)
            w = r / torch.sum(r, dim=2, keepdim=True)
            x = P.three_interpolate(l_feat[i].contiguous(), idx, w)
        with st("fp_mlp"):
            skip = l_feat[i - 1]
            for layer in bb.FP_modules[i].mlp:
                f = layer.folded()
                if fused:
                    x = pn2_mlp.pointwise_mlp(x, skip, f, None, True)
                else:
                    x = F.relu(F.conv1d(x if skip is None else torch.cat([x, skip], 1), f.wt.t().unsqueeze(2), f.bias))
                skip = None
            l_feat[i - 1] = x
    feats = l_feat[0]
    with st("heads"):
        outs = []
        for head in (m.rpn_cls_layer, m.rpn_reg_layer):
            x = feats
            for layer in head:
                if isinstance(layer, torch.nn.Dropout):
                    continue
                f = layer.folded()
                if fused:
                    x = pn2_mlp.pointwise_mlp(x, None, f, None, layer.relu)
                else:
                    x = F.conv1d(x, f.wt.t().unsqueeze(2), f.bias)
                    x = F.relu(x) if layer.relu else x
            outs.append(x.transpose(1, 2).contiguous())
    with st("proposals"):
        scores = outs[0][:, :, 0]
        seg = (torch.sigmoid(scores) > m.cfg.RPN.SCORE_THRESH).float()
        depth = points_depth(pts)
        rois, roi_scores = m.proposal_layer(scores, outs[1], pts)
    return outs, rois, roi_scores, seg, depth


def mlp_flops(cfg, B, n=768):
    """2 x multiply-adds of the shared MLPs, from the channel lists: per SA level, FP total, heads"""
    sa = cfg.RPN.SA_CONFIG
    cin, skip, per_level = 0, [0], []
    for k, npoint in enumerate(sa.NPOINTS):
        tot, cout = 0, 0
        for widths, ns in zip(sa.MLPS[k], sa.NSAMPLE[k]):
            c, macs = cin + 3, 0
            for w in widths:
                macs += c * w
                c = w
            tot += macs * npoint * ns
            cout += widths[-1]
        per_level.append(2 * B * tot)
        skip.append(cout)
        cin = cout
    fp, pts = 0, [n] + list(sa.NPOINTS)
    for k, widths in enumerate(cfg.RPN.FP_MLPS):
        c = (cfg.RPN.FP_MLPS[k + 1][-1] if k + 1 < len(cfg.RPN.FP_MLPS) else cin) + skip[k]
        for w in widths:
            fp += c * w * pts[k]
            c = w
    c0 = cfg.RPN.FP_MLPS[0][-1]
    reg_ch = int(cfg.RPN.LOC_SCOPE / cfg.RPN.LOC_BIN_SIZE) * 2 * (4 if cfg.RPN.LOC_XZ_FINE else 2) + cfg.RPN.NUM_HEAD_BIN * 2 + 4
    heads = sum(a * b for a, b in zip([c0] + list(cfg.RPN.CLS_FC), list(cfg.RPN.CLS_FC) + [1])) + \
        sum(a * b for a, b in zip([c0] + list(cfg.RPN.REG_FC), list(cfg.RPN.REG_FC) + [reg_ch]))
    return {"sa_levels": per_level, "fp": 2 * B * fp, "heads": 2 * B * heads * n}


def median(v):
    return float(np.median(v))


def time_pair(m, pts, iters, warmup):
    off = Stages(False)
    for _ in range(warmup):
        forward(m, pts, True, off)
        forward(m, pts, False, off)
    torch.cuda.synchronize()
    tot = {True: [], False: []}
    evs = []
    for _ in range(iters):
        for fused in (True, False):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            forward(m, pts, fused, off)
            b.record()
            evs.append((fused, a, b))
    torch.cuda.synchronize()
    for fused, a, b in evs:
        tot[fused].append(a.elapsed_time(b) * 1e3)
    stages = []
    for _ in range(iters):
        st = Stages(True)
        forward(m, pts, True, st)
        torch.cuda.synchronize()
        stages.append(st.totals())
    return {"fused_us": median(tot[True]), "unfused_us": median(tot[False]),
            "stages_us": {k: median([s[k] for s in stages]) for k in stages[0]}}


def level_case(m, cfg, B, k, dev):
    """inputs of SA level k (0-based) with random features of the right width"""
    sa = cfg.RPN.SA_CONFIG
    n_in = ([768] + list(sa.NPOINTS))[k]
    c_in = 0 if k == 0 else sum(w[-1] for w in sa.MLPS[k - 1])
    xyz = clouds(B, dev, n_in)
    feats = torch.randn(B, c_in, n_in, device=dev) if c_in else None
    mod = m.backbone_net.SA_modules[k]
    fidx = P.furthest_point_sample(xyz, mod.npoint)
    new_xyz = P.gather_operation(xyz.transpose(1, 2).contiguous(), fidx).transpose(1, 2).contiguous()
    idxs = [P.ball_query(g.radius, g.nsample, xyz, new_xyz) for g in mod.groupers]
    return xyz, new_xyz, feats, idxs, [mlp.folded() for mlp in mod.mlps]


def time_levels(m, cfg, B, iters, warmup, dev):
    out = {}
    fl = mlp_flops(cfg, B)["sa_levels"]
    for k in (2, 3):
        xyz, new_xyz, feats, idxs, folded = level_case(m, cfg, B, k, dev)
        buf = torch.empty((B, sum(f[-1].cout for f in folded), new_xyz.shape[1]), device=dev)

        def run():
            c = 0
            for idx, layers in zip(idxs, folded):
                pn2_mlp.sa_mlp_max(xyz, new_xyz, feats, idx, layers, out=buf, c_off=c)
                c += layers[-1].cout
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        us = median(ts)
        out[f"sa{k + 1}"] = {"us": us, "flops": fl[k], "tflops": fl[k] / us / 1e6, "fraction_of_peak": fl[k] / us / 1e6 / PEAK_TFLOPS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="16,1")
    ap.add_argument("--levels", action="store_true", help="run only the fused SA kernels of levels 3 and 4 (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = car_cfg()
    m = build_model(cfg, dev)
    out = {"tool": "bench_rpn", "iters": a.iters, "peak_tflops": PEAK_TFLOPS}
    with torch.no_grad():
        if a.levels:
            out["sa_level_tflops"] = {f"B{B}": time_levels(m, cfg, B, a.iters, a.warmup, dev) for B in (16,)}
        else:
            for B in [int(b) for b in a.batches.split(",")]:
                pts = clouds(B, dev)
                r = time_pair(m, pts, a.iters, a.warmup)
                fl = mlp_flops(cfg, B)
                r["flops"] = fl
                r["mlp_gflop"] = (sum(fl["sa_levels"]) + fl["fp"] + fl["heads"]) / 1e9
                out[f"B{B}"] = r
            out["sa_level_tflops"] = {"B16": time_levels(m, cfg, 16, a.iters, a.warmup, dev)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the FPN's training form (backbone/fpn_train.py: forward on the fp32 plans + the HIP backward) on one GPU with HIP events, against
the same FPN as F.conv2d / F.interpolate / F.max_pool2d autograd on the GPU, in the same run.

    python tools/bench_fpn_train.py [--windows 5] [--seconds 1.0] [--no-detector]

Shape: 2 stereo pairs of 384 x 1248 = four images, R-50 channels: C2..C5 = (256, 512, 1024, 2048) channels at 96 x 312, 48 x 156, 24 x 78,
12 x 39; 256 output channels; seeded random maps, parameters and incoming gradients.

What is timed, in windows of at least `--seconds` between two events, the variants alternating in the same run after a warm-up:
  hip / torch                forward and backward with the C maps NOT requiring grad (the frozen-body case: no 1x1 data gradients)
  hip_cgrad / torch_cgrad    the same with gradients to C2..C5
  split                      one instrumented set of passes of `hip_cgrad`: the time between events around each group of launches
                             (layout conversions, forward convs, resizes, channel sums, weight gradients, data gradients, resize adjoint)
  inner4_wgrad               fpn_inner4's weight gradient (2048 -> 256 over 1872 pixels) as drc_tapconv_wgrad with the 1x1 tap class and as
                             a drc_linear_fwd GEMM over packed pixel rows (packing included, the NCHW -> [pixels, C] transposes not)
  detector (unless --no-detector)  DispRCNN(R-50-FPN).train() on the same four images, 8 ground truths per pair: the whole step (forward,
                             backward, FusedSGD) with the backbone frozen and with the FPN trainable behind a frozen body, and the
                             losses of the first step of each
One JSON line: medians in milliseconds with the min-max spread and the ratios torch / HIP.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_roi_heads_train import ev, summarize, windows  # noqa: E402
from disprcnn_amd import engine as E  # noqa: E402
from disprcnn_amd.modeling.backbone import fpn_train as FT  # noqa: E402
from disprcnn_amd.modeling.backbone.fpn import FPN  # noqa: E402
from disprcnn_amd.modeling.backbone.runtime import FPNRuntime  # noqa: E402
from disprcnn_amd.utils import synth  # noqa: E402

IMG_H, IMG_W, PAIRS = 384, 1248, 2
CH, OCH = (256, 512, 1024, 2048), 256
HW = [(IMG_H // s, IMG_W // s) for s in (4, 8, 16, 32)]


def torch_fpn(feats, prm):
    conv = lambda x, name, pad: F.conv2d(x, prm[name + ".weight"], prm[name + ".bias"], padding=pad)
    last = conv(feats[3], "fpn_inner4", 0)
    res = [last]
    for i in (3, 2, 1):
        lat = conv(feats[i - 1], f"fpn_inner{i}", 0)
        last = conv(lat + F.interpolate(last, size=lat.shape[-2:], mode="bilinear", align_corners=False), f"fpn_layer{i}", 1)
        res.insert(0, last)
    res.append(F.max_pool2d(res[-1], 1, 2, 0))
    return res


class Split:
    """Events around the groups of launches of one pass: engine.TIMING for the convolution plans, wrappers for the rest."""

    def __init__(self):
        self.rows = []

    def wrap(self, owner, name, label):
        fn = getattr(owner, name)

        def timed(*a, **k):
            e0 = ev()
            out = fn(*a, **k)
            self.rows.append((label, e0, ev()))
            return out
        setattr(owner, name, timed)
        return lambda: setattr(owner, name, fn)

    def collect(self, run, passes):
        undo = [self.wrap(FT, "_conv_wgrad", "weight gradients (drc_tapconv_wgrad)"), self.wrap(FT, "channel_sums", "bias gradients (drc_channel_sums_blocked)"),
                self.wrap(FT, "resize_bwd", "resize adjoint (drc_bilinear_resize_blocked_bwd)"), self.wrap(E.Blocked, "from_dense", "dense -> blocked"),
                self.wrap(E.Blocked, "to_dense", "blocked -> dense")]
        E.TIMING = []
        try:
            for _ in range(passes):
                run()
            torch.cuda.synchronize()
            out = {}
            for label, e0, e1 in self.rows:
                out[label] = out.get(label, 0.0) + e0.elapsed_time(e1) / passes
            for kname, _, e0, e1 in E.TIMING:
                out["conv plans: " + kname] = out.get("conv plans: " + kname, 0.0) + e0.elapsed_time(e1) / passes
        finally:
            E.TIMING = None
            for u in undo:
                u()
        return {k: round(v, 4) for k, v in sorted(out.items(), key=lambda kv: -kv[1])}


def inner4_wgrad(dev, n):
    from disprcnn_amd.modeling.head_ops import _gemm_packed, _pack_cols
    h, w = HW[3]
    x = synth.hash_uniform("fpn:bench:w:x", (n, CH[3], h, w), -1.0, 1.0).to(dev)
    g = synth.hash_uniform("fpn:bench:w:g", (n, OCH, h, w), -1.0, 1.0).to(dev)
    xb = E.Blocked(n, CH[3], 1, h, w, 0, 0, 0, dev).from_dense(x)
    gb = E.Blocked(n, OCH, 1, h, w, 0, 1, 1, dev).from_dense(g)
    xr, gr = x.permute(0, 2, 3, 1).reshape(-1, CH[3]).contiguous(), g.permute(0, 2, 3, 1).reshape(-1, OCH).contiguous()
    M = xr.shape[0]

    def tap():
        a0 = ev()
        FT._conv_wgrad(xb, gb, 1, OCH, CH[3])
        return {"call": (a0, ev())}

    def gemm():
        a0 = ev()
        _gemm_packed(_pack_cols(gr), _pack_cols(xr), None, OCH, CH[3], M, False, dev)
        return {"call": (a0, ev())}
    a, b = FT._conv_wgrad(xb, gb, 1, OCH, CH[3]).reshape(OCH, CH[3]), _gemm_packed(_pack_cols(gr), _pack_cols(xr), None, OCH, CH[3], M, False, dev)
    agree = float((a - b).abs().max() / b.abs().max())
    return {"tapconv_wgrad": tap, "linear_gemm": gemm}, agree


def detector_steps(dev, n_windows, seconds):
    from bench_srpn_train import make_targets
    from disprcnn_amd.modeling.detector import DispRCNN, default_cfg_2d
    from disprcnn_amd.solver.fused import FusedSGD
    m = DispRCNN(default_cfg_2d("R-50-FPN"))
    sd = m.state_dict()
    w_rpn = synth.synth_det_state({k[4:]: v for k, v in sd.items() if k.startswith("rpn.")}, gain={"head.cls_logits.weight": 0.5, "head.bbox_pred.weight": 0.02})
    w_heads = synth.synth_det_state({k[10:]: v for k, v in sd.items() if k.startswith("roi_heads.")}, gain=synth.DET_GAIN)
    bb = synth.synth_backbone_state({k[9:]: v for k, v in sd.items() if k.startswith("backbone.")})
    m.load_state_dict({**{"backbone." + k: v for k, v in bb.items()}, **{"rpn." + k: v for k, v in w_rpn.items()},
                       **{"roi_heads." + k: v for k, v in w_heads.items()}}, strict=True)
    m = m.to(dev)
    left, right = synth.synth_images(PAIRS, IMG_H, IMG_W, tag="fpn:bench:det")
    lr = {"left": left.to(dev), "right": right.to(dev)}
    lt, rt = make_targets(dev)
    for boxes in (lt, rt):
        for b in boxes:
            b.add_field("labels", torch.ones(len(b), dtype=torch.int64, device=dev))
    for b in lt:
        masks = torch.zeros(len(b), IMG_H, IMG_W, dtype=torch.uint8, device=dev)
        for k, (x1, y1, x2, y2) in enumerate(b.bbox.round().long().tolist()):
            masks[k, y1: y2 + 1, x1: x2 + 1] = 1
        b.add_field("masks", masks)
    tg = {"left": lt, "right": rt}
    out, fns = {}, {}
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for mode in ("frozen", "fpn_trainable"):
        m.load_state_dict(state0, strict=True)
        m.backbone.requires_grad_(False)
        if mode == "fpn_trainable":
            m.backbone.fpn.requires_grad_(True)
            m.backbone.freeze_body()
        m.train()
        opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)

        def step(opt=opt):
            a0 = ev()
            losses = m(lr, tg)
            a1 = ev()
            opt.zero_grad(set_to_none=False)
            sum(losses.values()).backward()
            a2 = ev()
            opt.step()
            return {"forward": (a0, a1), "backward": (a1, a2), "sgd": (a2, ev())}, losses
        _, losses = step()
        out[mode + "_first_losses"] = {k: round(float(v), 6) for k, v in losses.items()}
        out[mode + "_step"] = summarize(windows({mode: lambda step=step: step()[0]}, n_windows, seconds, dev)[0][mode])
    out["ratio_fpn_trainable_over_frozen"] = round(out["fpn_trainable_step"]["total"]["median_ms"] / out["frozen_step"]["total"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-detector", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n = 2 * PAIRS
    fpn = FPN(CH, OCH)
    with torch.no_grad():
        for name, p in fpn.named_parameters():
            p.copy_(synth.hash_uniform("fpn:bench:" + name, tuple(p.shape), -1.0, 1.0) * (0.1 if name.endswith("bias") else (3.0 / p[0].numel()) ** 0.5))
    fpn = fpn.to(dev)
    prm = dict(fpn.named_parameters())
    rt = FPNRuntime(fpn, dev)
    hw5 = HW + [((HW[3][0] - 1) // 2 + 1, (HW[3][1] - 1) // 2 + 1)]
    feats = {g: [synth.hash_uniform(f"fpn:bench:C{i}", (n, c, h, w), -1.0, 1.0).to(dev).requires_grad_(g) for i, (c, (h, w)) in enumerate(zip(CH, HW))]
             for g in (False, True)}
    gouts = [synth.hash_uniform(f"fpn:bench:G{i}", (n, OCH, h, w), -1.0, 1.0).to(dev) for i, (h, w) in enumerate(hw5)]

    def zero(fs):
        for p in list(prm.values()) + list(fs):
            p.grad = None

    def variant(kind, cgrad):
        fs = feats[cgrad]

        def run():
            a0 = ev()
            outs = FT.fpn_train(fs, fpn, rt) if kind == "hip" else torch_fpn(fs, prm)
            a1 = ev()
            zero(fs)
            torch.autograd.backward(outs, gouts)
            return {"forward": (a0, a1), "backward": (a1, ev())}
        return run

    fns = {"hip": variant("hip", False), "torch": variant("torch", False), "hip_cgrad": variant("hip", True), "torch_cgrad": variant("torch", True)}
    # the two forms agree before they are timed against each other
    fns["hip_cgrad"]()
    got = {k: p.grad.clone() for k, p in prm.items() if p.grad is not None}
    fns["torch_cgrad"]()
    agree = max(float((got[k] - p.grad).abs().max() / p.grad.abs().max()) for k, p in prm.items() if p.grad is not None)
    rows, reps = windows(fns, a.windows, a.seconds, dev)
    res = {"tool": "bench_fpn_train", "device": torch.cuda.get_device_name(0), "images": n, "image_hw": [IMG_H, IMG_W], "stage_channels": list(CH),
           "out_channels": OCH, "passes_per_window": reps, "max_rel_param_grad_difference_hip_vs_torch": agree}
    for k, r in rows.items():
        res[k] = summarize(r)
    med = lambda k, p: res[k][p]["median_ms"]
    for tag in ("", "_cgrad"):
        res["ratio_torch_over_hip" + tag] = {p: round(med("torch" + tag, p) / med("hip" + tag, p), 3) for p in ("forward", "backward", "total")}
    res["split_ms_per_pass"] = Split().collect(fns["hip_cgrad"], 10)
    wfns, wagree = inner4_wgrad(dev, n)
    wrows, _ = windows(wfns, a.windows, min(a.seconds, 0.3), dev)
    res["inner4_wgrad"] = {"max_rel_difference": wagree, **{k: summarize(r)["call"] for k, r in wrows.items()}}
    if not a.no_detector:
        res["detector"] = detector_steps(dev, a.windows, a.seconds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

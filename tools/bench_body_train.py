#!/usr/bin/env python3
"""Time the ResNet body's training form (backbone/body_train.py: batch-statistics BatchNorm forward + the HIP backward) on one GPU with
HIP events, against the same body as F.conv2d / F.batch_norm autograd on the GPU, in the same run.

    python tools/bench_body_train.py [--windows 5] [--seconds 1.0] [--freeze-at 2] [--no-detector]

Shape: 2 stereo pairs of 384 x 1248 = four images, R-50 at full width; seeded random images, parameters and C-map gradients.

What is timed, in windows of at least `--seconds` between two events, the variants alternating in the same run after a warm-up:
  hip_gemm / hip_tap    body forward (stem .. C5, every BatchNorm on batch statistics) and backward from gradients on C2..C5 with
                        body_train.WGRAD_1X1 = "gemm" (drc_conv1x1_wgrad_blocked) and "tap" (drc_tapconv_wgrad)
  torch                 the same graph as F.conv2d / F.batch_norm(training=True) / relu / max_pool2d autograd on the GPU
  wgrad_1x1             the 1x1 weight gradients alone, per layer class of R-50 (input channels, output channels, map, stride), both forms
  detector (unless --no-detector)  DispRCNN(R-50-FPN).train() on the same four images, 8 ground truths per pair: the whole step (forward,
                        backward, FusedSGD) with the FPN trainable behind a frozen body and with the body opted in at --freeze-at
One JSON line: medians in milliseconds with the min-max spread and the ratios.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_roi_heads_train import ev, summarize, windows  # noqa: E402
from disprcnn_amd import engine as E  # noqa: E402
from disprcnn_amd.modeling.backbone import body_train as BT  # noqa: E402
from disprcnn_amd.modeling.backbone.backbone import ResNetFPNBackbone  # noqa: E402
from disprcnn_amd.modeling.backbone.runtime import BackboneRuntime  # noqa: E402
from disprcnn_amd.utils import synth  # noqa: E402

IMG_H, IMG_W, PAIRS = 384, 1248, 2
# (cin, cout, input map, stride) of R-50's 1x1 layers in layer2..4, one row per class
CLASSES_1X1 = [(256, 128, (96, 312), 2), (256, 512, (96, 312), 2), (128, 512, (48, 156), 1), (512, 128, (48, 156), 1),
               (512, 256, (48, 156), 2), (512, 1024, (48, 156), 2), (256, 1024, (24, 78), 1), (1024, 256, (24, 78), 1),
               (1024, 512, (24, 78), 2), (1024, 2048, (24, 78), 2), (512, 2048, (12, 39), 1), (2048, 512, (12, 39), 1)]


def torch_body(body, x):
    def cb(x, conv, bn, stride, pad, relu, res=None):
        y = F.batch_norm(F.conv2d(x, conv.weight, None, stride, pad), bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)
        y = y if res is None else y + res
        return F.relu(y) if relu else y
    with torch.no_grad():
        y = F.max_pool2d(cb(x, body.stem.conv1, body.stem.bn1, 2, 3, True), 3, 2, 0, ceil_mode=True)
    outs = []
    for li in range(1, 5):
        for u in getattr(body, f"layer{li}"):
            idn = y if u.downsample is None else cb(y, u.downsample[0], u.downsample[1], u.stride, 0, False)
            z = cb(cb(y, u.conv1, u.bn1, u.stride, 0, True), u.conv2, u.bn2, 1, 1, True)
            y = cb(z, u.conv3, u.bn3, 1, 0, True, idn)
        outs.append(y)
    return outs


def wgrad_classes(dev, n, n_windows, seconds):
    out = {}
    for cin, cout, (h, w), s in CLASSES_1X1:
        oh, ow = (h - 1) // s + 1, (w - 1) // s + 1
        a = E.Blocked(n, cin, 1, h, w, 0, 0, 0, dev).from_dense(synth.hash_uniform(f"body:bench:a{cin}", (n, cin, h, w), -1.0, 1.0).to(dev))
        b = E.Blocked(n, cout, 1, oh, ow, 0, 0, 0, dev).from_dense(synth.hash_uniform(f"body:bench:b{cout}", (n, cout, oh, ow), -1.0, 1.0).to(dev))

        def call(kernel, a=a, b=b, cin=cin, cout=cout, s=s):
            def run():
                e0 = ev()
                BT.conv1x1_wgrad(a, b, cin, cout, s, kernel=kernel)
                return {"call": (e0, ev())}
            return run
        g, t = BT.conv1x1_wgrad(a, b, cin, cout, s, kernel="gemm"), BT.conv1x1_wgrad(a, b, cin, cout, s, kernel="tap")
        rows, _ = windows({"gemm": call("gemm"), "tap": call("tap")}, n_windows, seconds, dev)
        out[f"{cin}->{cout} {h}x{w} s{s}"] = {"max_rel_difference": float((g - t).abs().max() / t.abs().max()),
                                              **{k: summarize(r)["call"] for k, r in rows.items()}}
    return out


def detector_steps(dev, n_windows, seconds, freeze_at):
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
    out = {}
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for mode in ("fpn_trainable", "body_trainable"):
        m.load_state_dict(state0, strict=True)
        m.backbone.requires_grad_(True)
        if mode == "fpn_trainable":
            m.backbone.freeze_body()
        else:
            m.backbone.enable_body_training(freeze_at)
        m.train()
        opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=1e-5, momentum=0.9)

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
    out["ratio_body_trainable_over_fpn_trainable"] = round(out["body_trainable_step"]["total"]["median_ms"] / out["fpn_trainable_step"]["total"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--freeze-at", type=int, default=2)
    ap.add_argument("--no-detector", action="store_true")
    ap.add_argument("--no-classes", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n = 2 * PAIRS
    bb = ResNetFPNBackbone("R-50")
    bb.load_state_dict(synth.synth_backbone_state(bb.state_dict()), strict=True)
    bb = bb.to(dev).enable_body_training(a.freeze_at).train()
    rt = BackboneRuntime(bb, dev)
    x = synth.synth_images(PAIRS, IMG_H, IMG_W, tag="body:bench")
    x = torch.cat(x, dim=0).to(dev)
    hw = [(IMG_H // s, IMG_W // s) for s in (4, 8, 16, 32)]
    gouts = [synth.hash_uniform(f"body:bench:G{i}", (n, c, h, w), -1.0, 1.0).to(dev) for i, (c, (h, w)) in enumerate(zip(bb.body.stage_channels, hw))]
    params = [p for p in bb.body.parameters() if p.requires_grad]

    def hip(kernel):
        def run():
            BT.WGRAD_1X1["kernel"] = kernel
            a0 = ev()
            _, _, cm = BT.forward_cmaps(rt, x)
            a1 = ev()
            for p in params:
                p.grad = None
            live = [(c, g) for c, g in zip(cm, gouts) if c is not None]
            torch.autograd.backward([c for c, _ in live], [g for _, g in live])
            return {"forward": (a0, a1), "backward": (a1, ev())}
        return run

    def torch_run():
        a0 = ev()
        outs = torch_body(bb.body, x)
        a1 = ev()
        for p in params:
            p.grad = None
        live = [(o, g) for o, g in zip(outs, gouts) if o.requires_grad]
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])
        return {"forward": (a0, a1), "backward": (a1, ev())}

    default = BT.WGRAD_1X1["kernel"]
    fns = {"hip_gemm": hip("gemm"), "hip_tap": hip("tap"), "torch": torch_run}
    fns["hip_gemm"]()
    got = {id(p): p.grad.clone() for p in params}
    fns["torch"]()
    agree = max(float((got[id(p)] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for p in params)
    rows, reps = windows(fns, a.windows, a.seconds, dev)
    BT.WGRAD_1X1["kernel"] = default
    res = {"tool": "bench_body_train", "device": torch.cuda.get_device_name(0), "images": n, "image_hw": [IMG_H, IMG_W], "freeze_at": a.freeze_at,
           "default_wgrad_1x1": default, "passes_per_window": reps, "max_rel_param_grad_difference_hip_vs_torch": agree}
    for k, r in rows.items():
        res[k] = summarize(r)
    med = lambda k, p: res[k][p]["median_ms"]
    res["ratio_torch_over_hip_gemm"] = {p: round(med("torch", p) / med("hip_gemm", p), 3) for p in ("forward", "backward", "total")}
    res["ratio_tap_over_gemm"] = {p: round(med("hip_tap", p) / med("hip_gemm", p), 3) for p in ("backward", "total")}
    if not a.no_classes:
        res["wgrad_1x1"] = wgrad_classes(dev, n, a.windows, min(a.seconds, 0.2))
    if not a.no_detector:
        res["detector"] = detector_steps(dev, a.windows, a.seconds, a.freeze_at)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

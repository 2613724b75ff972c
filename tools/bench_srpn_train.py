#!/usr/bin/env python3
"""Time the Stereo RPN's training step (StereoRPN.train(): head forward on the fp32 kernels, train-time proposal selection, targets +
balanced sample, the fused head + loss Function and its SPARSE backward) on one GPU with HIP events, against the same head as F.conv2d
autograd (dense backward) with the same srpn_loss on the same sample, in the same run.

    python tools/bench_srpn_train.py [--windows 5] [--seconds 1.0]

Shape: 2 image pairs of 384 x 1248, C = 256, the five FPN levels (39 900 pixels, 119 700 anchors per image), 8 ground truths per image,
RPN.BATCH_SIZE_PER_IMAGE 256, PRE_/POST_NMS_TOP_N_TRAIN 2000.

What is timed, in windows of at least `--seconds` between two events, the variants alternating in the same run after a warm-up:
  hip_step / hip_step_featgrad      head_forward, selection, targets_sample, loss_forward (drc_det2d_srpn_loss_fwd + active pixels + the
                                    gathers of T and Xcol), backward (G gather, four GEMMs, ReLU mask, bias sums; _featgrad: also dXcol
                                    and col2im to the ten feature maps)
  torch_dense / torch_dense_featgrad  forward = F.conv2d head (MIOpen) + the same srpn_loss kernel on its raw maps, backward = autograd
                                    through the dense head; selection and targets are not repeated (they are the same code)
One JSON line: medians in milliseconds with the min-max spread, the ratios torch / HIP of head forward + loss and of backward, and the
bytes of the dense hidden-map workspace.
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
from disprcnn_amd.layers import det2d_loss as D  # noqa: E402
from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d  # noqa: E402
from disprcnn_amd.modeling.rpn.srpn_train import srpn_head_loss  # noqa: E402
from disprcnn_amd.modeling.rpn.stereo_rpn import StereoRPN  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.structures.image_list import ImageList  # noqa: E402
from disprcnn_amd.utils import synth  # noqa: E402

IMG_H, IMG_W, N, G, C = 384, 1248, 2, 8, 256


def make_targets(dev):
    rng = np.random.default_rng(11)
    lt, rt = [], []
    for _ in range(N):
        w, h = rng.uniform(40, 260, G), rng.uniform(30, 160, G)
        x1, y1 = rng.uniform(0, IMG_W - w), rng.uniform(0, IMG_H - h)
        gl = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
        disp = rng.uniform(2, 40, G).astype(np.float32)
        gr = gl - np.stack([disp, 0 * disp, disp, 0 * disp], 1)
        lt.append(BoxList(torch.from_numpy(gl).to(dev), (IMG_W, IMG_H), mode="xyxy"))
        rt.append(BoxList(torch.from_numpy(gr).to(dev), (IMG_W, IMG_H), mode="xyxy"))
    return lt, rt


def torch_head(prm, fl, fr):
    logits, regs = [], []
    for a, b in zip(fl, fr):
        n = a.shape[0]
        t = F.relu(F.conv2d(torch.cat((a, b), 0), prm["head.conv.weight"], prm["head.conv.bias"], 1, 1))
        t = torch.cat((t[:n], t[n:]), 1)
        logits.append(F.conv2d(t, prm["head.cls_logits.weight"], prm["head.cls_logits.bias"]))
        regs.append(F.conv2d(t, prm["head.bbox_pred.weight"], prm["head.bbox_pred.bias"]))
    return logits, regs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rpn = StereoRPN(default_cfg_2d(), C)
    rpn.load_state_dict(synth.synth_det_state(rpn.state_dict(), gain=synth.DET_GAIN), strict=True)
    rpn = rpn.to(dev).train()
    prm = dict(rpn.named_parameters())
    fl0, fr0 = synth.synth_pyramid(N, IMG_H, IMG_W, c=C, tag="srpn:bench")
    images = ImageList(torch.zeros(N, 3, IMG_H, IMG_W), [(IMG_H, IMG_W)] * N)
    lt, rt = make_targets(dev)
    shapes = [tuple(f.shape[2:]) for f in fl0]
    total = sum(h * w for h, w in shapes) * 3
    draws = synth.hash_uniform("srpn:bench:sample", (N * total,), 0.0, 1.0).to(dev)
    ev_ = rpn.loss_evaluator
    cap = ev_.fg_bg_sampler.batch_size_per_image
    feats = {g: ([f.to(dev).requires_grad_(g) for f in fl0], [f.to(dev).requires_grad_(g) for f in fr0]) for g in (False, True)}

    def zero(fs):
        for p in list(prm.values()) + list(fs):
            p.grad = None

    def hip(featgrad):
        fl, fr = feats[featgrad]

        def run():
            a0 = ev()
            logits, regs, hidden = rpn.head_train(fl, fr)
            a1 = ev()
            rpn.proposals_from_maps(images, logits, regs, rpn.pre_nms_top_n_train, rpn.post_nms_top_n_train)
            a2 = ev()
            with torch.no_grad():
                _, labels, reg, counts = ev_.prepare_targets(rpn.anchor_generator(images, fl), lt, rt)
                pos, neg, n_sampled, _ = ev_.fg_bg_sampler.sample(labels, counts, draws)
            a3 = ev()
            lo, lb = srpn_head_loss(fl, fr, rpn.head, pos, neg, reg, n_sampled, logits, regs, hidden, cap)
            a4 = ev()
            zero(fl + fr)
            (lo + lb).backward()
            a5 = ev()
            return {"head_forward": (a0, a1), "selection": (a1, a2), "targets_sample": (a2, a3), "loss_forward": (a3, a4), "backward": (a4, a5)}
        return run

    with torch.no_grad():
        _, labels, reg, counts = ev_.prepare_targets(rpn.anchor_generator(images, feats[False][0]), lt, rt)
        pos, neg, n_sampled, _ = ev_.fg_bg_sampler.sample(labels, counts, draws)
    sampled = [int(v) for v in n_sampled.sum(1).cpu()]

    def dense(featgrad):
        fl, fr = feats[featgrad]

        def run():
            a0 = ev()
            logits, regs = torch_head(prm, fl, fr)
            lo, lb, _ = D.srpn_loss(logits, regs, pos, neg, reg, n_sampled, beta=1.0 / 9)
            a1 = ev()
            zero(fl + fr)
            (lo + lb).backward()
            a2 = ev()
            return {"forward": (a0, a1), "backward": (a1, a2)}
        return run

    fns = {"hip_step": hip(False), "torch_dense": dense(False), "hip_step_featgrad": hip(True), "torch_dense_featgrad": dense(True)}
    rows, reps = windows(fns, a.windows, a.seconds, dev)
    res = {"tool": "bench_srpn_train", "device": torch.cuda.get_device_name(0), "images": N, "image_hw": [IMG_H, IMG_W], "channels": C,
           "anchors_per_image": total, "sampled_per_image": sampled, "cap": cap, "passes_per_window": reps,
           "hidden_workspace_bytes": rpn.hidden_workspace_bytes()}
    for k, r in rows.items():
        res[k] = summarize(r)
    med = lambda k, p: res[k][p]["median_ms"]
    for tag in ("", "_featgrad"):
        h, t = "hip_step" + tag, "torch_dense" + tag
        res["ratio_torch_over_hip" + tag] = {
            "forward": round(med(t, "forward") / (med(h, "head_forward") + med(h, "loss_forward")), 3),
            "backward": round(med(t, "backward") / med(h, "backward"), 3),
            "forward_plus_backward": round((med(t, "forward") + med(t, "backward")) / (med(h, "head_forward") + med(h, "loss_forward") + med(h, "backward")), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the stereo ROI heads' training step (StereoCombinedROIHeads.train(): box head + mask head, forward, backward, FusedSGD step) on
one GPU with HIP events, against the same heads composed from torch layers.

    python tools/bench_roi_heads_train.py [--windows 5] [--seconds 1.0] [--rois 512]

Shape: 2 image pairs of 384 x 1248, 256-channel P2-P5 (+P6, unused), 8 ground truths per image with masks, ~2 000 proposals per image of
which `--rois` are sampled (a quarter positive), MLP_HEAD_DIM 2048; the mask head runs on the positives the sampler yields.

What is timed, in windows of at least `--seconds` between two events, HIP and torch alternating in the same run after a warm-up:
  hip_step            forward (sampling, both ROIAligns, the heads, the three losses), backward (parameter gradients only: the pyramids
                      need no gradient while the trunk's backward is not built) and FusedSGD.step().  The step bumps the parameter
                      versions, so the next forward re-packs W and W^T of every GEMM layer: that re-pack is inside `forward`/`backward`
                      and reported separately as `fc6_repack_W_and_WT` (the largest layer's).
  hip_on_pooled       the same heads from the POOLED features on (fc6 .. losses, mask convs .. loss_mask): the scope of the torch side
  torch_on_pooled     nn.Linear / F.conv2d / F.conv_transpose2d / F.dropout autograd + torch.optim.SGD on the same pooled features
                      (hipBLASLt / MIOpen), losses from F.cross_entropy / smooth L1 / BCE on precomputed mask targets
  pieces              fc6 forward, data gradient and weight gradient (kernel + operand packing of the activations; TFLOP/s from the
                      shapes), the mask head's conv chain forward and backward, the pyramid ROIAlign backward (14 x 14, the positives).
One JSON line: medians in milliseconds, min-max spread, ratios torch / HIP.
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

from disprcnn_amd.modeling import head_ops as HO  # noqa: E402
from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d  # noqa: E402
from disprcnn_amd.modeling.roi_heads.roi_heads import build_roi_heads  # noqa: E402
from disprcnn_amd.solver.fused import FusedSGD  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.utils import synth  # noqa: E402

IMG_H, IMG_W, N, G = 384, 1248, 2, 8


def make_inputs(dev):
    rng = np.random.default_rng(7)
    fl, fr = synth.synth_pyramid(N, IMG_H, IMG_W, tag="rht:bench")
    fl, fr = [f.to(dev) for f in fl], [f.to(dev) for f in fr]
    lp, rp, lt, rt = [], [], [], []
    for n in range(N):
        w, h = rng.uniform(40, 260, G), rng.uniform(30, 160, G)
        x1, y1 = rng.uniform(0, IMG_W - w), rng.uniform(0, IMG_H - h)
        gl = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
        disp = rng.uniform(2, 40, G).astype(np.float32)
        gr = gl - np.stack([disp, 0 * disp, disp, 0 * disp], 1)
        jit = rng.uniform(-0.08, 0.08, (40, G, 4)) * np.stack([w, h, w, h], 1)
        pos = (gl[None] + jit).reshape(-1, 4)
        far_wh = rng.uniform(16, 300, (1600, 2))
        far_xy = rng.uniform(0, 1, (1600, 2)) * (np.array([IMG_W, IMG_H]) - far_wh)
        far = np.concatenate([far_xy, far_xy + far_wh], 1)
        pl = np.concatenate([gl, pos, far]).astype(np.float32)
        pr = pl - np.concatenate([disp, np.tile(disp, 40), rng.uniform(2, 40, 1600)])[:, None].astype(np.float32) * np.array([1, 0, 1, 0], np.float32)
        masks = np.zeros((G, IMG_H, IMG_W), np.uint8)
        for g in range(G):
            masks[g, int(gl[g, 1]):int(gl[g, 3]), int(gl[g, 0]):int(gl[g, 2])] = 1
        mk = lambda b, **f: _boxlist(b, dev, **f)
        lp.append(mk(pl)); rp.append(mk(pr))
        lt.append(mk(gl, labels=np.ones(G, np.int64), masks=masks)); rt.append(mk(gr, labels=np.ones(G, np.int64)))
    return fl, fr, lp, rp, lt, rt


def _boxlist(b, dev, **fields):
    out = BoxList(torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev), (IMG_W, IMG_H), mode="xyxy")
    for k, v in fields.items():
        out.add_field(k, torch.from_numpy(v).to(dev))
    return out


class TorchHeads(torch.nn.Module):
    """the same layers as torch modules, on the pooled features"""

    def __init__(self, heads):
        super().__init__()
        sd = {k: v.detach().clone() for k, v in heads.state_dict().items()}
        w6 = sd["box.feature_extractor.RCNN_top.0.weight"]
        self.fc6, self.fc7 = torch.nn.Linear(w6[0].numel(), w6.shape[0]), torch.nn.Linear(w6.shape[0], w6.shape[0])
        self.cls, self.reg = torch.nn.Linear(w6.shape[0], 2), torch.nn.Linear(w6.shape[0], 12)
        self.convs = torch.nn.ModuleList([torch.nn.Conv2d(256, 256, 3, 1, 1) for _ in range(4)])
        self.deconv, self.logits = torch.nn.ConvTranspose2d(256, 256, 2, 2), torch.nn.Conv2d(256, 2, 1)
        with torch.no_grad():
            self.fc6.weight.copy_(w6.flatten(1)); self.fc6.bias.copy_(sd["box.feature_extractor.RCNN_top.0.bias"])
            self.fc7.weight.copy_(sd["box.feature_extractor.RCNN_top.3.weight"].flatten(1)); self.fc7.bias.copy_(sd["box.feature_extractor.RCNN_top.3.bias"])
            for lin, k in ((self.cls, "box.predictor.cls_score"), (self.reg, "box.predictor.bbox_pred"), (self.deconv, "mask.predictor.conv5_mask"),
                           (self.logits, "mask.predictor.mask_fcn_logits")):
                lin.weight.copy_(sd[k + ".weight"]); lin.bias.copy_(sd[k + ".bias"])
            for i, c in enumerate(self.convs, 1):
                c.weight.copy_(sd[f"mask.feature_extractor.mask_fcn{i}.weight"]); c.bias.copy_(sd[f"mask.feature_extractor.mask_fcn{i}.bias"])

    def forward(self, t, labels, reg, xm, mcls, mtgt):
        h = F.dropout(F.relu(self.fc6(t)), 0.2, True)
        h = F.dropout(F.relu(self.fc7(h)), 0.2, True)
        logits, deltas = self.cls(h), self.reg(h)
        loss_cls = F.cross_entropy(logits, labels)
        rows = torch.nonzero(labels > 0).squeeze(1)
        cols = 6 * labels[rows][:, None] + torch.arange(6, device=t.device)
        n = (deltas[rows[:, None], cols] - reg[rows]).abs()
        loss_box = torch.where(n < 1.0, 0.5 * n * n, n - 0.5).sum() / labels.numel()
        x = xm
        for c in self.convs:
            x = F.relu(c(x))
        lg = self.logits(F.relu(self.deconv(x)))
        loss_mask = F.binary_cross_entropy_with_logits(lg[torch.arange(len(mcls), device=t.device), mcls], mtgt)
        return loss_cls + loss_box + loss_mask


def windows(fns, n_windows, seconds, dev):
    """fns: name -> callable running ONE pass that returns a list of per-phase (start, stop) event pairs or None; alternating windows.
    -> name -> list of per-window dicts phase -> ms per pass"""
    out = {k: [] for k in fns}
    reps = {}
    for k, fn in fns.items():                                   # warm-up and the pass count of a window
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(dev)
        reps[k] = max(2, int(np.ceil(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    for _ in range(n_windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            phases = []
            e0.record()
            for _ in range(reps[k]):
                phases.append(fn())
            e1.record()
            torch.cuda.synchronize(dev)
            row = {"total": e0.elapsed_time(e1) / reps[k]}
            if phases[0]:
                for name in phases[0]:
                    row[name] = float(np.mean([p[name][0].elapsed_time(p[name][1]) for p in phases]))
            out[k].append(row)
    return out, reps


def summarize(rows):
    keys = rows[0].keys()
    return {k: {"median_ms": round(float(np.median([r[k] for r in rows])), 4), "min_ms": round(float(min(r[k] for r in rows)), 4),
                "max_ms": round(float(max(r[k] for r in rows)), 4)} for k in keys}


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rois", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = default_cfg_2d()
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = a.rois
    heads = build_roi_heads(cfg, 256)
    heads.load_state_dict(synth.synth_det_state(heads.state_dict(), gain=synth.DET_GAIN), strict=True)
    heads = heads.to(dev).train()
    fl, fr, lp, rp, lt, rt = make_inputs(dev)
    opt = FusedSGD(heads.parameters(), lr=1e-4, momentum=0.9)
    total_props = sum(len(p) for p in lp)
    sample_draws = synth.hash_uniform("rht:bench:sample", (total_props,), 0.0, 1.0).to(dev)

    def hip_step():
        a0 = ev()
        x, left, right, losses = heads(fl, fr, lp, rp, lt, rt, draws={"sample": sample_draws})
        a1 = ev()
        opt.zero_grad(set_to_none=False)
        sum(losses.values()).backward()
        a2 = ev()
        opt.step()
        a3 = ev()
        return {"forward": (a0, a1), "backward": (a1, a2), "sgd": (a2, a3)}

    # the pooled features and the sample of one step, for the two on-pooled variants
    with torch.no_grad():
        left, right = heads.box.loss_evaluator.subsample({"left": lp, "right": rp}, {"left": lt, "right": rt}, sample_draws)
        labels, reg = heads.box.loss_evaluator._labels.clone(), heads.box.loss_evaluator._regression_targets.clone()
        fe = heads.box.feature_extractor
        t = torch.cat([fe.pooler(fl, left), fe.pooler(fr, right)], 1).flatten(1)
        from disprcnn_amd.modeling.roi_heads.mask_head_loss import keep_only_positive_boxes
        pos, _ = keep_only_positive_boxes(left)
        xm = heads.mask.feature_extractor.pooler(fl, pos)
    R, P = t.shape[0], xm.shape[0]
    mcls = torch.cat([p.get_field("labels") for p in pos])

    def hip_on_pooled():
        a0 = ev()
        h = HO.linear_train(t, fe.RCNN_top[0], relu=True, p=0.2)
        h = HO.linear_train(h, fe.RCNN_top[3], relu=True, p=0.2)
        logits, deltas = heads.box.predictor(h)
        from disprcnn_amd.layers import det2d_loss as D
        lc, lb, _ = D.fastrcnn_loss(logits, deltas, labels, reg)
        lg = heads.mask.predictor(heads.mask.feature_extractor._forward_train(xm))
        lm = heads.mask.loss_evaluator(pos, lg, lt)
        a1 = ev()
        opt.zero_grad(set_to_none=False)
        (lc + lb + lm).backward()
        a2 = ev()
        opt.step()
        a3 = ev()
        return {"forward": (a0, a1), "backward": (a1, a2), "sgd": (a2, a3)}

    hip_on_pooled()
    mtgt = heads.mask.loss_evaluator.last_targets.float()
    th = TorchHeads(heads).to(dev).train()
    topt = torch.optim.SGD(th.parameters(), lr=1e-4, momentum=0.9)

    def torch_on_pooled():
        a0 = ev()
        loss = th(t, labels, reg, xm, mcls, mtgt)
        a1 = ev()
        topt.zero_grad(set_to_none=False)
        loss.backward()
        a2 = ev()
        topt.step()
        a3 = ev()
        return {"forward": (a0, a1), "backward": (a1, a2), "sgd": (a2, a3)}

    # ---- pieces
    w6 = fe.RCNN_top[0].weight.detach().flatten(1)
    Nn, K = w6.shape
    wp, wtp = HO._pack_rows(w6), HO._pack_cols(w6)
    dz = synth.hash_uniform("rht:bench:dz", (R, Nn)).to(dev)
    chain = heads.mask.feature_extractor._chain
    gm = synth.hash_uniform("rht:bench:gm", tuple(xm.shape)).to(dev)
    mp = heads.mask.feature_extractor.pooler

    def roi_bwd():
        feats = [f.detach().requires_grad_() for f in fl[:4]]
        out = mp(feats, pos)
        a0 = ev()
        out.backward(gm)
        return {"backward": (a0, ev())}

    def chain_fb():
        x = xm.detach().requires_grad_()
        a0 = ev()
        y = chain(x)
        a1 = ev()
        y.backward(gm)
        return {"forward": (a0, a1), "backward": (a1, ev())}

    def plain(f):
        def run():
            f()
            return None
        return run

    pieces = {
        "fc6_forward": plain(lambda: HO._gemm_packed(HO._pack_rows(t), wp, None, R, Nn, K, True, dev)),
        "fc6_dgrad": plain(lambda: HO._gemm_packed(HO._pack_rows(dz), wtp, None, R, K, Nn, False, dev)),
        "fc6_wgrad": plain(lambda: HO._gemm_packed(HO._pack_cols(dz), HO._pack_cols(t), None, Nn, K, R, False, dev)),
        "fc6_repack_W_and_WT": plain(lambda: (HO._pack_rows(w6), HO._pack_cols(w6))),
        "mask_conv_chain": chain_fb,
        "mask_roi_align_fpn_bwd": roi_bwd,
    }
    main_rows, reps = windows({"hip_step": hip_step, "hip_on_pooled": hip_on_pooled, "torch_on_pooled": torch_on_pooled}, a.windows, a.seconds, dev)
    piece_rows, _ = windows(pieces, max(3, a.windows // 2 + 1), min(a.seconds, 0.5), dev)
    res = {"tool": "bench_roi_heads_train", "device": torch.cuda.get_device_name(0), "images": N, "image_hw": [IMG_H, IMG_W], "sampled_rois": R,
           "mask_rois": P, "proposals": total_props, "passes_per_window": reps}
    for k, rows in {**main_rows, **piece_rows}.items():
        res[k] = summarize(rows)
    flops = 2.0 * R * Nn * K
    for k in ("fc6_forward", "fc6_dgrad", "fc6_wgrad"):
        res[k]["tflops"] = round(flops / (res[k]["total"]["median_ms"] * 1e-3) / 1e12, 1)
    res["ratio_torch_over_hip_on_pooled"] = {k: round(res["torch_on_pooled"][k]["median_ms"] / res["hip_on_pooled"][k]["median_ms"], 3)
                                             for k in ("total", "forward", "backward", "sgd")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

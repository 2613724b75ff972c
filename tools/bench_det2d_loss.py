#!/usr/bin/env python3
"""Time the 2D stage's training targets, sampling and losses on one GPU with HIP events, piece by piece, at the workload's shape.

    python tools/bench_det2d_loss.py [--iters 20] [--warmup 5] [--inner 10]

Shape: 2 images of 384 x 1248, the five-level pyramid (119 700 anchors per image, A = 3) with 8 ground truths each; 512 sampled ROIs per
image with C = 2 for the box head; 64 positive ROIs at M = 28 for the mask head.  Pieces: `rpn_targets` (match + label + encode),
`rpn_sample` (256 per image), `srpn_loss` (forward + backward to the raw maps), `box_targets` (2 x 2 000 joint proposals), `box_sample`,
`fastrcnn_loss` (forward + backward), `mask_loss` (targets + loss, forward + backward).

Each piece is timed against the same computation composed from torch ops on the GPU: the test oracle's code on device tensors, i.e. the
reference's per-image loops with their boolean-index compactions, the sampler as an argsort of the same draws, and for the mask targets
the reference's per-ROI crop + F.interpolate with the boxes read on the host.  Both sides are checked against each other before anything
is timed.  Method: every shape warmed up, then `iters` windows per variant, alternating; a window is `inner` passes between two events.
One JSON line: per piece the medians in microseconds per pass, the min-max spread and the ratio torch / HIP.
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

from disprcnn_amd.layers import det2d_loss as D, smooth_l1_loss  # noqa: E402
from disprcnn_amd.modeling.rpn.anchor_generator import pyramid_level_anchors  # noqa: E402

SIZES, STRIDES, RATIOS = (32, 64, 128, 256, 512), (4, 8, 16, 32, 64), (0.5, 1.0, 2.0)
IMG_H, IMG_W, N, A, G = 384, 1248, 2, 3, 8
PYR = [(-(-IMG_H // s), -(-IMG_W // s)) for s in STRIDES]


# ---- the torch-op composition (one image at a time, as the reference loops)
def t_iou(gt, cand):
    area1 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    area2 = (cand[:, 2] - cand[:, 0] + 1) * (cand[:, 3] - cand[:, 1] + 1)
    lt, rb = torch.max(gt[:, None, :2], cand[:, :2]), torch.min(gt[:, None, 2:], cand[:, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def t_match(iou, high, low, lq):
    vals, matches = iou.max(dim=0)
    allm = matches.clone()
    matches[vals < low] = -1
    matches[(vals >= low) & (vals < high)] = -2
    if lq:
        best, _ = iou.max(dim=1)
        upd = torch.nonzero(iou == best[:, None])[:, 1]
        matches[upd] = allm[upd]
    return matches


def t_expand(left, right):
    union = torch.cat((torch.min(left[:, :2], right[:, :2]), torch.max(left[:, 2:], right[:, 2:])), dim=1)
    return union, torch.stack((left[:, 0], union[:, 1], left[:, 2], union[:, 3], right[:, 0], right[:, 2]), dim=1)


def t_encode(ref, prop, w):
    ew, eh = prop[:, 2] - prop[:, 0] + 1, prop[:, 3] - prop[:, 1] + 1
    ex, ey = prop[:, 0] + 0.5 * ew, prop[:, 1] + 0.5 * eh
    ewp, exp = (prop[:, 5] - prop[:, 4] + 1, None) if prop.shape[1] == 6 else (ew, ex)
    if exp is None:
        exp = prop[:, 4] + 0.5 * ewp
    gw, gh, gwp = ref[:, 2] - ref[:, 0] + 1, ref[:, 3] - ref[:, 1] + 1, ref[:, 5] - ref[:, 4] + 1
    gx, gy, gxp = ref[:, 0] + 0.5 * gw, ref[:, 1] + 0.5 * gh, ref[:, 4] + 0.5 * gwp
    return torch.stack((w[0] * (gx - ex) / ew, w[1] * (gy - ey) / eh, w[2] * torch.log(gw / ew), w[3] * torch.log(gh / eh),
                        w[0] * (gxp - exp) / ewp, w[2] * torch.log(gwp / ewp)), dim=1)


def t_rpn_targets(anchors, vis, gl, gr):
    labels, regs = [], []
    for n in range(N):
        union, orig = t_expand(gl[n], gr[n])
        m = t_match(t_iou(union, anchors), 0.7, 0.3, True)
        lab = (m >= 0).float()
        lab[m == -1] = 0
        lab[~vis] = -1
        lab[m == -2] = -1
        labels.append(lab)
        regs.append(t_encode(orig[m.clamp(min=0)], anchors, (1.0, 1.0, 1.0, 1.0)))
    return torch.cat(labels), torch.cat(regs)


def t_box_targets(prop6, gt6, gt_labels):
    labels, regs = [], []
    for n in range(N):
        pu, po = t_expand(prop6[n][:, :4], prop6[n][:, [4, 1, 5, 3]])
        gu, go = t_expand(gt6[n][:, :4], gt6[n][:, [4, 1, 5, 3]])
        m = t_match(t_iou(gu, pu), 0.5, 0.5, False)
        lab = gt_labels[n][m.clamp(min=0)].clone()
        lab[m == -1] = 0
        lab[m == -2] = -1
        labels.append(lab)
        regs.append(t_encode(go[m.clamp(min=0)], po, (10.0, 10.0, 5.0, 5.0)))
    return torch.cat(labels), torch.cat(regs)


def t_sample(labels, draws, counts, batch, fraction):
    pos_masks, neg_masks, first = [], [], 0
    for c in counts:
        lab, dr = labels[first:first + c], draws[first:first + c]
        pos, neg = torch.nonzero(lab >= 1).squeeze(1), torch.nonzero(lab == 0).squeeze(1)
        num_pos = min(pos.numel(), int(batch * fraction))
        num_neg = min(neg.numel(), batch - num_pos)
        pm, nm = torch.zeros(c, dtype=torch.uint8, device=lab.device), torch.zeros(c, dtype=torch.uint8, device=lab.device)
        pm[pos[torch.argsort(dr[pos], stable=True)[:num_pos]]] = 1
        nm[neg[torch.argsort(dr[neg], stable=True)[:num_neg]]] = 1
        pos_masks.append(pm)
        neg_masks.append(nm)
        first += c
    return torch.cat(pos_masks), torch.cat(neg_masks)


def t_srpn_loss(zs, bs, labels, reg, pm, nm):
    obj, box = [], []
    for z, b in zip(zs, bs):
        n, _, H, W = z.shape
        p = z.view(n, 2, -1, W).softmax(1).view(*z.shape)
        obj.append(p.view(n, -1, 2, H, W).permute(0, 3, 4, 1, 2).reshape(n, -1, 2))
        box.append(b.view(n, -1, 6, H, W).permute(0, 3, 4, 1, 2).reshape(n, -1, 6))
    obj, box = torch.cat(obj, dim=1).reshape(-1, 2), torch.cat(box, dim=1).reshape(-1, 6)
    pos, neg = torch.nonzero(pm).squeeze(1), torch.nonzero(nm).squeeze(1)
    sampled = torch.cat([pos, neg])
    return (F.cross_entropy(obj[sampled], labels[sampled].long()),
            smooth_l1_loss(box[pos], reg[pos], beta=1.0 / 9, size_average=False) / sampled.numel())


def t_fastrcnn_loss(x, b, labels, reg):
    rows = torch.nonzero(labels > 0).squeeze(1)
    cols = 6 * labels[rows][:, None] + torch.arange(6, device=x.device)
    return F.cross_entropy(x, labels), smooth_l1_loss(b[rows[:, None], cols], reg[rows], size_average=False, beta=1) / labels.numel()


def t_mask_loss(x, boxes, inst_of, cls, masks, M):
    targets = []
    for (x1, y1, x2, y2), g in zip(boxes.tolist(), inst_of):           # the reference's loop: boxes read on the host
        m = masks[g]
        H, W = m.shape
        xmin, ymin, xmax, ymax = round(x1), round(y1), round(x2), round(y2)
        xmin, ymin = min(max(xmin, 0), W - 1), min(max(ymin, 0), H - 1)
        xmax, ymax = max(min(max(xmax, 0), W), xmin + 1), max(min(max(ymax, 0), H), ymin + 1)
        crop = m[ymin:ymax, xmin:xmax]
        targets.append(F.interpolate(crop[None, None].float(), size=(M, M), mode="bilinear", align_corners=False)[0, 0].byte())
    targets = torch.stack(targets).float()
    return F.binary_cross_entropy_with_logits(x[torch.arange(len(cls), device=x.device), cls], targets), targets


# ---- timing
def windows(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner


def compare(name, hip, ref, args, out):
    for _ in range(args.warmup):
        hip()
        ref()
    th, tr = [], []
    for _ in range(args.iters):
        th.append(windows(hip, args.inner))
        tr.append(windows(ref, args.inner))
    out[name] = {"hip_us": round(float(np.median(th)), 1), "hip_min_max": [round(min(th), 1), round(max(th), 1)],
                 "torch_us": round(float(np.median(tr)), 1), "torch_min_max": [round(min(tr), 1), round(max(tr), 1)],
                 "torch_over_hip": round(float(np.median(tr) / np.median(th)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det2d_loss: no GPU; this tool measures on an MI355X and has no CPU fallback")
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    anchors = torch.from_numpy(np.concatenate([pyramid_level_anchors(z, RATIOS, shp, st) for z, shp, st in zip(SIZES, PYR, STRIDES)])).float().to(dev)
    T = anchors.shape[0]
    vis = (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < IMG_W) & (anchors[:, 3] < IMG_H)
    x1, y1 = rng.uniform(0, IMG_W - 200, (N, G)), rng.uniform(0, IMG_H - 150, (N, G))
    left = np.stack([x1, y1, x1 + rng.uniform(30, 190, (N, G)), y1 + rng.uniform(30, 140, (N, G))], axis=2)
    disp = rng.uniform(2, 40, (N, G))
    right = left - np.stack([disp, np.zeros_like(disp), disp, np.zeros_like(disp)], axis=2)
    gl, gr = torch.from_numpy(left).float().to(dev), torch.from_numpy(right).float().to(dev)
    out = {"anchors_per_image": T, "images": N, "ground_truths": G}

    # RPN targets
    cand, visN = anchors.repeat(N, 1), vis.repeat(N)
    hip_t = lambda: D.match_label_encode(cand, [T] * N, gl.reshape(-1, 4), gr.reshape(-1, 4), [G] * N, 0.7, 0.3, True, visibility=visN)  # noqa: E731
    _, labels, reg = hip_t()
    lab_t, reg_t = t_rpn_targets(anchors, vis, gl, gr)
    assert torch.equal(labels, lab_t) and (reg - reg_t).abs().max() < 1e-4
    compare("rpn_targets", hip_t, lambda: t_rpn_targets(anchors, vis, gl, gr), args, out)

    # RPN sample
    draws = torch.rand(N * T, device=dev)
    pm, nm, counts, _ = D.balanced_sample(labels, [T] * N, 256, 0.5, draws)
    pm_t, nm_t = t_sample(labels, draws, [T] * N, 256, 0.5)
    assert torch.equal(pm, pm_t) and torch.equal(nm, nm_t)
    compare("rpn_sample", lambda: D.balanced_sample(labels, [T] * N, 256, 0.5, draws), lambda: t_sample(labels, draws, [T] * N, 256, 0.5), args, out)

    # RPN loss, forward + backward
    zs = [torch.randn(N, 2 * A, h, w, device=dev, requires_grad=True) for h, w in PYR]
    bs = [(0.3 * torch.randn(N, 6 * A, h, w, device=dev)).requires_grad_() for h, w in PYR]

    def hip_l():
        o, b, _ = D.srpn_loss(zs, bs, pm, nm, reg, counts)
        return torch.autograd.grad(o + b, zs + bs)

    def ref_l():
        o, b = t_srpn_loss(zs, bs, labels, reg, pm, nm)
        return torch.autograd.grad(o + b, zs + bs)
    for a, b in zip(hip_l(), ref_l()):
        assert (a - b).abs().max() < 1e-6
    compare("srpn_loss", hip_l, ref_l, args, out)

    # box head: targets, sample, loss
    P, C = 2000, 2
    prop6, gt6 = [], []
    for n in range(N):
        jit = torch.from_numpy(rng.normal(0, 12, (P, 4))).float().to(dev)
        base = gl[n][torch.from_numpy(rng.integers(0, G, P)).to(dev)] + jit
        base = torch.cat((torch.min(base[:, :2], base[:, 2:] - 4), base[:, 2:]), dim=1)
        d = torch.from_numpy(rng.uniform(2, 40, P)).float().to(dev)
        prop6.append(torch.cat((base, (base[:, 0] - d)[:, None], (base[:, 2] - d)[:, None]), dim=1))
        gt6.append(torch.cat((gl[n], gr[n][:, [0, 2]]), dim=1))
    gt_labels = [torch.ones(G, dtype=torch.int64, device=dev) for _ in range(N)]
    cand6, g6 = torch.cat(prop6), torch.cat(gt6)
    hip_b = lambda: D.match_label_encode(cand6, [P] * N, g6[:, :4], g6[:, [4, 1, 5, 3]], [G] * N, 0.5, 0.5, False, (10.0, 10.0, 5.0, 5.0),  # noqa: E731
                                         gt_labels=torch.cat(gt_labels))
    _, blab, breg = hip_b()
    blab_t, breg_t = t_box_targets(prop6, gt6, gt_labels)
    assert torch.equal(blab, blab_t) and (breg - breg_t).abs().max() < 1e-3
    compare("box_targets", hip_b, lambda: t_box_targets(prop6, gt6, gt_labels), args, out)
    bdraws = torch.rand(N * P, device=dev)
    bp, bn, _, bidx = D.balanced_sample(blab, [P] * N, 512, 0.25, bdraws, want_indices=True)
    bp_t, bn_t = t_sample(blab, bdraws, [P] * N, 512, 0.25)
    assert torch.equal(bp, bp_t) and torch.equal(bn, bn_t)
    compare("box_sample", lambda: D.balanced_sample(blab, [P] * N, 512, 0.25, bdraws, want_indices=True),
            lambda: [torch.nonzero(a | b).squeeze(1) for a, b in zip(*[m.split(P) for m in t_sample(blab, bdraws, [P] * N, 512, 0.25)])], args, out)
    keep = torch.nonzero(bp | bn).squeeze(1)
    R = keep.numel()
    slab, sreg = blab[keep].contiguous(), breg[keep].contiguous()
    x = torch.randn(R, C, device=dev, requires_grad=True)
    b = torch.randn(R, 6 * C, device=dev, requires_grad=True)

    def hip_f():
        lc, lb, _ = D.fastrcnn_loss(x, b, slab, sreg)
        return torch.autograd.grad(lc + lb, [x, b])

    def ref_f():
        lc, lb = t_fastrcnn_loss(x, b, slab, sreg)
        return torch.autograd.grad(lc + lb, [x, b])
    for u, v in zip(hip_f(), ref_f()):
        assert (u - v).abs().max() < 1e-6
    out["box_rois"] = R
    compare("fastrcnn_loss", hip_f, ref_f, args, out)

    # mask head: 64 positive ROIs at M = 28
    M, Pm = 28, 64
    yy, xx = torch.meshgrid(torch.arange(IMG_H, device=dev), torch.arange(IMG_W, device=dev), indexing="ij")
    masks = []
    for n in range(N):
        c = (gl[n][:, :2] + gl[n][:, 2:]) / 2
        r = (gl[n][:, 2:] - gl[n][:, :2]) / 2
        masks.append(((((xx[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((yy[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2) <= 1).to(torch.uint8))
    inst_of = torch.from_numpy(rng.integers(0, G, (N, Pm // N))).to(dev)
    mboxes = torch.cat([gl[n][inst_of[n]] + torch.from_numpy(rng.normal(0, 3, (Pm // N, 4))).float().to(dev) for n in range(N)])
    flat, table, inst_counts = D.pack_masks(masks)
    inst_labels = torch.ones(N * G, dtype=torch.int64, device=dev)
    matched = inst_of.reshape(-1).contiguous()
    mx = torch.randn(Pm, C, M, M, device=dev, requires_grad=True)
    all_masks = [m for n in range(N) for m in masks[n]]
    inst_global = (inst_of + torch.arange(N, device=dev)[:, None] * G).reshape(-1).tolist()
    cls = torch.ones(Pm, dtype=torch.int64, device=dev)

    def hip_m():
        loss, _, tg, _ = D.mask_loss(mx, mboxes, [Pm // N] * N, matched, inst_labels, flat, table, inst_counts)
        return torch.autograd.grad(loss, mx)[0], tg

    def ref_m():
        loss, tg = t_mask_loss(mx, mboxes, inst_global, cls, all_masks, M)
        return torch.autograd.grad(loss, mx)[0], tg
    (gh, th), (_, tt) = hip_m(), ref_m()
    # torch's GPU interpolate is not its CPU kernel, which the targets follow bit for bit (tests): a weight sum of 1 - ulp truncates to 0,
    # so the two sets of targets differ on some pixels.  Reported, not asserted; the gradient is checked on the HIP targets.
    out["mask_target_pixels"] = th.numel()
    out["mask_target_pixels_differing_from_torch_gpu"] = int((th.float() != tt).sum())
    want = torch.autograd.grad(F.binary_cross_entropy_with_logits(mx[torch.arange(Pm, device=dev), cls], th.float()), mx)[0]
    assert (gh - want).abs().max() < 1e-6
    compare("mask_loss", hip_m, ref_m, args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

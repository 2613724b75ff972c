"""The Stereo RPN's training step restated on torch-CPU, runnable in fp64 and fp32: the head in the reference's form (F.conv2d, ReLU,
channel concatenation, two 1x1 convolutions; srpn.py:30-50 without its softmax, which tests/det2d_loss_oracle.srpn_loss applies to the
raw maps itself), the loss through det2d_loss_oracle.srpn_loss, every gradient from autograd.  Targets and the balanced sample come from
det2d_loss_oracle (rpn_targets, sample) on the anchors of disprcnn_amd's generator.

    train_step(params, feats_left, feats_right, labels, reg, pos, neg, dtype) -> dict(loss_objectness, loss_rpn_box_reg, grads {name: array},
        gleft / gright [per level], logits / regs [per level], pre_lo, pre_hi)

pre_lo / pre_hi: the smallest and largest |pre-activation| of the hidden layer (both views) at the ACTIVE pixels -- those with a sampled
anchor -- which are the only ReLU inputs a gradient depends on.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import det2d_loss_oracle as DO

PARAMS = ("head.conv.weight", "head.conv.bias", "head.cls_logits.weight", "head.cls_logits.bias", "head.bbox_pred.weight", "head.bbox_pred.bias")
SIZES, RATIOS, STRIDES = (32, 64, 128, 256, 512), (0.5, 1.0, 2.0), (4, 8, 16, 32, 64)


def anchors_of(shapes, img_wh):
    """-> anchors [T,4] fp32 (level-major, then (y*W + x)*A + a) and their visibility (STRADDLE_THRESH 0) in an image of (width, height)"""
    from disprcnn_amd.modeling.rpn.anchor_generator import pyramid_level_anchors
    a = np.concatenate([pyramid_level_anchors(z, RATIOS, shp, st) for z, shp, st in zip(SIZES, shapes, STRIDES)]).astype(np.float32)
    w, h = img_wh
    vis = (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < w) & (a[:, 3] < h)
    return a, vis


def targets_and_sample(shapes, img_whs, gt_left, gt_right, draws, batch, fraction, high=0.7, low=0.3):
    """per image: labels, regression targets, and the sample of `draws` (the images' anchors concatenated) -> concatenated
    (labels [N*T], reg [N*T,6], pos, neg [N*T] uint8)"""
    labels, regs, pos, neg = [], [], [], []
    off = 0
    for wh, gl, gr in zip(img_whs, gt_left, gt_right):
        a, vis = anchors_of(shapes, wh)
        _, lab, reg = DO.rpn_targets(a, vis, gl, gr, high, low)
        p, n = DO.sample(lab, draws[off: off + len(a)], batch, fraction)
        off += len(a)
        labels.append(lab), regs.append(reg), pos.append(p), neg.append(n)
    return np.concatenate(labels), np.concatenate(regs), np.concatenate(pos), np.concatenate(neg)


def active_pixel_masks(pos, neg, N, A, shapes):
    """pos | neg [N*T] -> per level a bool [N,H,W]: a pixel with at least one sampled anchor"""
    m = (np.asarray(pos).astype(bool) | np.asarray(neg).astype(bool)).reshape(N, -1)
    out, off = [], 0
    for h, w in shapes:
        out.append(m[:, off: off + h * w * A].reshape(N, h, w, A).any(3))
        off += h * w * A
    return out


def head(params, feats_left, feats_right, dtype):
    """-> (logits, regs, pre): per level the raw [N,2A,H,W] / [N,6A,H,W] maps and the hidden pre-activation [N,4C,H,W] (left, then right)"""
    p = {k: v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)).to(dtype) for k, v in params.items()}
    logits, regs, pres = [], [], []
    for fl, fr in zip(feats_left, feats_right):
        pre = torch.cat((F.conv2d(fl, p[PARAMS[0]], p[PARAMS[1]], 1, 1), F.conv2d(fr, p[PARAMS[0]], p[PARAMS[1]], 1, 1)), 1)
        t = F.relu(pre)
        logits.append(F.conv2d(t, p[PARAMS[2]], p[PARAMS[3]]))
        regs.append(F.conv2d(t, p[PARAMS[4]], p[PARAMS[5]]))
        pres.append(pre)
    return logits, regs, pres


def train_step(params, feats_left, feats_right, labels, reg, pos, neg, dtype=torch.float64, feat_grad=True):
    prm = {k: torch.as_tensor(np.asarray(params[k])).to(dtype).clone().requires_grad_() for k in PARAMS}
    fl = [torch.as_tensor(np.asarray(f)).to(dtype).clone().requires_grad_(feat_grad) for f in feats_left]
    fr = [torch.as_tensor(np.asarray(f)).to(dtype).clone().requires_grad_(feat_grad) for f in feats_right]
    logits, regs, pres = head(prm, fl, fr, dtype)
    N, A = logits[0].shape[0], logits[0].shape[1] // 2
    shapes = [tuple(z.shape[2:]) for z in logits]
    lo, lb, gz, gb = DO.srpn_loss([z.detach() for z in logits], [b.detach() for b in regs], labels, reg, pos, neg, dtype)
    inputs = [prm[k] for k in PARAMS] + (fl + fr if feat_grad else [])
    outs = list(logits) + list(regs)
    gouts = [torch.as_tensor(g).to(dtype) for g in list(gz) + list(gb)]
    grads = torch.autograd.grad(outs, inputs, gouts, allow_unused=True)
    grads = [torch.zeros_like(i) if g is None else g for g, i in zip(grads, inputs)]
    act = active_pixel_masks(pos, neg, N, A, shapes)
    vals = [pre.detach().double().permute(0, 2, 3, 1)[torch.as_tensor(m)].abs().reshape(-1) for pre, m in zip(pres, act)]
    vals = torch.cat(vals) if vals else torch.zeros(0)
    L = len(shapes)
    out = dict(loss_objectness=float(lo), loss_rpn_box_reg=float(lb), grads={k: g.double().numpy() for k, g in zip(PARAMS, grads[:6])},
               logits=[z.detach().double().numpy() for z in logits], regs=[b.detach().double().numpy() for b in regs],
               pre_lo=float(vals.min()) if vals.numel() else float("inf"), pre_hi=float(vals.max()) if vals.numel() else 0.0,
               n_active=int(sum(m.sum() for m in act)))
    if feat_grad:
        out["gleft"] = [g.double().numpy() for g in grads[6: 6 + L]]
        out["gright"] = [g.double().numpy() for g in grads[6 + L:]]
    return out

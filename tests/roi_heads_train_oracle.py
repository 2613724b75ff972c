"""The training step of the stereo ROI heads restated with torch-CPU ops, runnable in fp64 and fp32: ROIAlign from
tests/roi_stage_oracle.py (roi_align_fwd64 / roi_align_bwd64 wrapped as an autograd Function, one level per ROI), plain matmuls,
F.conv2d / F.conv_transpose2d, dropout from the same draws as the kernels (kept iff draw >= (float32)p, scaled by 1 / (1 - p)), the
losses as tests/det2d_loss_oracle.py writes them.  Gradients by autograd.

Every step also returns the smallest and the largest |pre-activation| over all ReLU inputs of the case: where smallest >= 1e-4 * largest
in fp64, no ReLU mask can legitimately differ between an fp32 and an fp64 evaluation (an fp32 pre-activation of a dot product of a few
hundred to a few thousand O(1) terms is wrong by ~1e-6 of the largest), so a test may compare every gradient element.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import det2d_loss_oracle as DO
from . import roi_stage_oracle as RO

F32 = np.float32
BOX_PARAMS = ("feature_extractor.RCNN_top.0.weight", "feature_extractor.RCNN_top.0.bias", "feature_extractor.RCNN_top.3.weight",
              "feature_extractor.RCNN_top.3.bias", "predictor.cls_score.weight", "predictor.cls_score.bias", "predictor.bbox_pred.weight",
              "predictor.bbox_pred.bias")
MASK_PARAMS = tuple(f"feature_extractor.mask_fcn{i}.{k}" for i in range(1, 5) for k in ("weight", "bias")) + \
    ("predictor.conv5_mask.weight", "predictor.conv5_mask.bias", "predictor.mask_fcn_logits.weight", "predictor.mask_fcn_logits.bias")


class _RoiAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rois, scale, ph, pw, sr):
        ctx.cfg = (np.asarray(rois, F32), scale, ph, pw, sr, tuple(feat.shape))
        out, _ = RO.roi_align_fwd64(feat.detach().double().numpy(), ctx.cfg[0], scale, ph, pw, sr)
        return torch.from_numpy(out).to(feat.dtype)

    @staticmethod
    def backward(ctx, g):
        rois, scale, ph, pw, sr, shape = ctx.cfg
        gin, _, _ = RO.roi_align_bwd64(g.double().numpy(), rois, scale, ph, pw, sr, shape, np.zeros(shape))
        return torch.from_numpy(gin).to(g.dtype), None, None, None, None, None


def levels_of(boxes, k_min=2, k_max=5):
    """LevelMapper of modeling/poolers.py on fp32 numpy: round(4 + ln(sqrt(area) / 224)) clamped, minus k_min (area with the +1 convention)"""
    b = np.asarray(boxes, F32)
    area = (b[:, 2] - b[:, 0] + F32(1)) * (b[:, 3] - b[:, 1] + F32(1))
    lv = np.round(F32(4) + np.log(np.sqrt(area) / F32(224)))
    return (np.clip(lv, k_min, k_max) - k_min).astype(np.int64)


def level_margin(boxes):
    """distance of 4 + ln(sqrt(area) / 224) from the nearest rounding boundary (.5): cases keep it well above fp32 noise"""
    b = np.asarray(boxes, np.float64)
    v = 4 + np.log(np.sqrt((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)) / 224)
    return np.abs(v - np.floor(v) - 0.5).min(initial=1.0)


def pool(feats, rois, levels, img_h, ph, pw, sr):
    """feats: per-level torch [B,C,H,W]; rois [K,5] numpy; levels [K] -> [K,C,ph,pw]; the scale of a level is H / img_h (the fork's quirk)"""
    K, C = len(rois), feats[0].shape[1]
    out = torch.zeros(K, C, ph, pw, dtype=feats[0].dtype)
    for lv, f in enumerate(feats):
        idx = np.nonzero(np.asarray(levels) == lv)[0]
        if idx.size:
            out = out.index_copy(0, torch.from_numpy(idx), _RoiAlign.apply(f, np.asarray(rois, F32)[idx], f.shape[2] / img_h, ph, pw, sr))
    return out


def rois_of(boxes_per_image):
    return np.concatenate([np.concatenate([np.full((len(b), 1), i, F32), np.asarray(b, F32).reshape(-1, 4)], 1)
                           for i, b in enumerate(boxes_per_image)]).astype(F32)


class _Pre:
    """tracks the smallest and largest |pre-activation| of the ReLU inputs"""

    def __init__(self):
        self.lo, self.hi = np.inf, 0.0

    def relu(self, z):
        if z.numel():
            a = z.detach().abs()
            self.lo, self.hi = min(self.lo, float(a.min())), max(self.hi, float(a.max()))
        return F.relu(z)


def _leaves(arrays, dtype, grad=True):
    return [torch.as_tensor(np.asarray(a)).to(dtype).clone().requires_grad_(grad) for a in arrays]


def _np(t, like=None):
    if t is None:
        return np.zeros(tuple(like.shape))
    return t.detach().double().numpy()


def dropout_keep(draws, p):
    return np.asarray(draws, F32) >= F32(p)


def box_step(feats_left, feats_right, left_boxes, right_boxes, img_h, params, labels, reg, keep, p, dtype=torch.float64, feat_grad=False,
             resolution=7, sampling_ratio=0):
    """feats_*: per-level arrays [B,C,H,W]; left_boxes / right_boxes: per image [n,4]; params: dict BOX_PARAMS name -> array; labels [R],
    reg [R,6]; keep [2,R,D] bool dropout keep masks (dropout_keep of the draws), p the dropout probability.
    -> dict: loss_classifier, loss_box_reg, x, class_logits, box_regression, grads {name: array}, feat_grads (left, right) or None,
    pre_lo, pre_hi"""
    fl, fr = _leaves(feats_left, dtype, feat_grad), _leaves(feats_right, dtype, feat_grad)
    P = dict(zip(BOX_PARAMS, _leaves([params[k] for k in BOX_PARAMS], dtype)))
    rl, rr = rois_of(left_boxes), rois_of(right_boxes)
    ll, lr = levels_of(rl[:, 1:]), levels_of(rr[:, 1:])
    t = torch.cat([pool(fl, rl, ll, img_h, resolution, resolution, sampling_ratio),
                   pool(fr, rr, lr, img_h, resolution, resolution, sampling_ratio)], 1).flatten(1)
    pre = _Pre()
    keep = torch.as_tensor(np.asarray(keep)).to(dtype)
    w6 = P[BOX_PARAMS[0]]
    h = pre.relu(t @ w6.reshape(w6.shape[0], -1).t() + P[BOX_PARAMS[1]]) * keep[0] / (1 - p)
    w7 = P[BOX_PARAMS[2]]
    x = pre.relu(h @ w7.reshape(w7.shape[0], -1).t() + P[BOX_PARAMS[3]]) * keep[1] / (1 - p)
    logits = x @ P[BOX_PARAMS[4]].t() + P[BOX_PARAMS[5]]
    deltas = x @ P[BOX_PARAMS[6]].t() + P[BOX_PARAMS[7]]
    lab = torch.as_tensor(np.asarray(labels)).long()
    tgt = torch.as_tensor(np.asarray(reg)).to(dtype)
    loss_cls = F.cross_entropy(logits, lab)
    rows = torch.nonzero(lab > 0).squeeze(1)
    cols = 6 * lab[rows][:, None] + torch.arange(6)
    loss_box = DO.smooth_l1_sum(deltas[rows[:, None], cols], tgt[rows], 1.0) / lab.numel()
    (loss_cls + loss_box).backward()
    return dict(loss_classifier=float(loss_cls.detach().double()), loss_box_reg=float(loss_box.detach().double()), x=_np(x), class_logits=_np(logits),
                box_regression=_np(deltas), grads={k: _np(v.grad, v) for k, v in P.items()},
                feat_grads=([_np(f.grad, f) for f in fl], [_np(f.grad, f) for f in fr]) if feat_grad else None, pre_lo=pre.lo, pre_hi=pre.hi)


def mask_step(feats, boxes, img_h, params, cls, targets, dtype=torch.float64, feat_grad=False, resolution=14, sampling_ratio=2):
    """feats: the LEFT pyramid, per-level arrays; boxes: per image [n,4] positive proposals; params: dict MASK_PARAMS name -> array; cls [P]
    int64 labels of the proposals (> 0); targets [P,M,M] 0 / 1 -> dict: loss_mask, mask_logits, x, grads, feat_grads, pre_lo, pre_hi"""
    fl = _leaves(feats, dtype, feat_grad)
    P = dict(zip(MASK_PARAMS, _leaves([params[k] for k in MASK_PARAMS], dtype)))
    pre = _Pre()
    n = sum(len(b) for b in boxes)
    if n == 0:
        zeros = {k: np.zeros(tuple(v.shape)) for k, v in P.items()}
        return dict(loss_mask=0.0, mask_logits=None, x=None, grads=zeros, feat_grads=[np.zeros(tuple(f.shape)) for f in fl] if feat_grad else None,
                    pre_lo=np.inf, pre_hi=0.0)
    r = rois_of(boxes)
    x = pool(fl, r, levels_of(r[:, 1:]), img_h, resolution, resolution, sampling_ratio)
    for i in range(4):
        x = pre.relu(F.conv2d(x, P[MASK_PARAMS[2 * i]], P[MASK_PARAMS[2 * i + 1]], stride=1, padding=1))
    t = pre.relu(F.conv_transpose2d(x, P[MASK_PARAMS[8]], P[MASK_PARAMS[9]], stride=2))
    logits = F.conv2d(t, P[MASK_PARAMS[10]], P[MASK_PARAMS[11]])
    cls = torch.as_tensor(np.asarray(cls)).long()
    rows = torch.nonzero(cls > 0).squeeze(1)
    loss = F.binary_cross_entropy_with_logits(logits[rows, cls[rows]], torch.as_tensor(np.asarray(targets))[rows].to(dtype))
    loss.backward()
    return dict(loss_mask=float(loss.detach().double()), mask_logits=_np(logits), x=_np(x), grads={k: _np(v.grad, v) for k, v in P.items()},
                feat_grads=[_np(f.grad, f) for f in fl] if feat_grad else None, pre_lo=pre.lo, pre_hi=pre.hi)


def sampled(left_props, right_props, gt_left, gt_right, gt_labels, draws, batch, fraction, weights=(10.0, 10.0, 5.0, 5.0)):
    """the box head's subsample per image (fp32 decisions): -> per image (keep indices, labels [k], regression targets [k,6] fp32)"""
    out, first = [], 0
    for lp, rp, gl, gr, lab in zip(left_props, right_props, gt_left, gt_right, gt_labels):
        lp, rp, gl, gr = (np.asarray(a, F32) for a in (lp, rp, gl, gr))
        p6 = np.concatenate([lp, rp[:, [0, 2]]], 1)
        g6 = np.concatenate([gl, gr[:, [0, 2]]], 1)
        _, labels, enc = DO.box_targets(p6, g6, lab, 0.5, 0.5, weights)
        pm, nm = DO.sample(labels, np.asarray(draws, F32)[first:first + len(lp)], batch, fraction)
        keep = np.nonzero(pm | nm)[0]
        out.append((keep, labels[keep], enc[keep], p6[keep]))
        first += len(lp)
    return out


# ---- mask-head parameters whose ReLU inputs keep their distance from zero
def margin_mask_params(tag, feats, boxes, img_h, channels, ncls, resolution=14, sampling_ratio=2):
    """Five ROIs of the mask head make 250 000 ReLU inputs; with ordinary weights a few dozen of them land within 1e-4 of zero (relative to
    the largest) whatever the seed.  So the cases give every channel of every conv / deconv layer a bias of +B or -B (the sign by a hash of
    the channel) with B = 2 after scaling the layer's weights so that its largest |conv(x, W)| on the case's own ROIs is 1: a channel is wholly
    on or wholly off, every |pre-activation| lies in [1, 3], and the ReLU masks are still non-trivial (half the channels pass no gradient).  Masks that
    vary from pixel to pixel, exact zeros included, are the kernel-level test's business.  Weights: uniform, fan-in scaled."""
    from disprcnn_amd.utils.synth import hash_uniform
    n = sum(len(b) for b in boxes)
    out = {}
    x = None
    if n:
        r = rois_of(boxes)
        x = pool([torch.as_tensor(f).double() for f in feats], r, levels_of(r[:, 1:]), img_h, resolution, resolution, sampling_ratio)

    def signs(key, c):
        return np.where(hash_uniform(key, (c,), 0.0, 1.0).numpy() < 0.5, -1.0, 1.0)

    for i in range(1, 6):
        deconv = i == 5
        shape = (channels, channels, 2, 2) if deconv else (channels, channels, 3, 3)
        a = 2.0 * np.sqrt(3.0 / (channels if deconv else channels * 9))
        w = hash_uniform(f"{tag}:w{i}", shape, -a, a).numpy()
        sg = signs(f"{tag}:s{i}", channels)
        if x is None:
            b = 0.1 * sg
        else:
            wt = torch.as_tensor(w).double()
            z = F.conv_transpose2d(x, wt, stride=2) if deconv else F.conv2d(x, wt, padding=1)
            w = (w / float(z.abs().max())).astype(F32)                 # the layer's largest response becomes 1 (up to the fp32 rounding of w)
            wt = torch.as_tensor(w).double()
            z = F.conv_transpose2d(x, wt, stride=2) if deconv else F.conv2d(x, wt, padding=1)
            b = 2.0 * sg
            x = F.relu(z + torch.as_tensor(b).double().view(1, -1, 1, 1))
        name = "predictor.conv5_mask" if deconv else f"feature_extractor.mask_fcn{i}"
        out[name + ".weight"], out[name + ".bias"] = w.astype(F32), np.asarray(b, F32)
    out["predictor.mask_fcn_logits.weight"] = hash_uniform(f"{tag}:wl", (ncls, channels, 1, 1), -0.5, 0.5).numpy()
    out["predictor.mask_fcn_logits.bias"] = hash_uniform(f"{tag}:bl", (ncls,), -0.1, 0.1).numpy()
    return out

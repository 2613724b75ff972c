"""The 2D stage's training targets, sampling and losses restated with numpy / torch-CPU ops: fp32 wherever a decision is taken (IoU, maxima,
thresholds, box codes), any dtype for the loss sums (the tests evaluate them in fp64 and, for the tolerance, in fp32).  Written from the
algorithm of the reference's loss evaluators, one image at a time, the way the reference loops.  The sampler takes the same `draws` as the
kernels and selects by a stable argsort of (draw, index).
"""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


# ---- boxes
def expand_left_right(left, right):
    """left, right [G,4] fp32 -> union boxes [G,4], original_lr_bbox [G,6]"""
    left, right = np.asarray(left, F32), np.asarray(right, F32)
    union = np.stack([np.minimum(left[:, 0], right[:, 0]), np.minimum(left[:, 1], right[:, 1]),
                      np.maximum(left[:, 2], right[:, 2]), np.maximum(left[:, 3], right[:, 3])], axis=1)
    orig = np.stack([left[:, 0], union[:, 1], left[:, 2], union[:, 3], right[:, 0], right[:, 2]], axis=1)
    return union, orig


def box6_views(b6):
    b6 = np.asarray(b6, F32)
    return b6[:, 0:4], b6[:, [4, 1, 5, 3]]


def iou_matrix(gt, cand):
    """[G,4] x [R,4] -> [G,R] fp32, the legacy +1 convention"""
    gt, cand = np.asarray(gt, F32), np.asarray(cand, F32)
    one = F32(1)
    area1 = (gt[:, 2] - gt[:, 0] + one) * (gt[:, 3] - gt[:, 1] + one)
    area2 = (cand[:, 2] - cand[:, 0] + one) * (cand[:, 3] - cand[:, 1] + one)
    lt = np.maximum(gt[:, None, :2], cand[None, :, :2])
    rb = np.minimum(gt[:, None, 2:], cand[None, :, 2:])
    wh = np.maximum(rb - lt + one, F32(0))
    inter = wh[:, :, 0] * wh[:, :, 1]
    return (inter / (area1[:, None] + area2[None, :] - inter)).astype(F32)


def match(iou, high, low, allow_low_quality):
    vals, idx = iou.max(axis=0), iou.argmax(axis=0).astype(np.int64)          # argmax: the first (lowest) row of a tie
    out = idx.copy()
    out[vals < F32(low)] = -1
    out[(vals >= F32(low)) & (vals < F32(high))] = -2
    if allow_low_quality:
        best = iou.max(axis=1)
        cols = np.nonzero(iou == best[:, None])[1]
        out[cols] = idx[cols]
    return out


def encode(ref6, prop, weights, dtype=F32):
    """(dx, dy, dw, dh, dx', dw') of ref6 [R,6] against prop [R,4] (the right view coded against the same box) or [R,6]"""
    ref6, prop = np.asarray(ref6, F32).astype(dtype), np.asarray(prop, F32).astype(dtype)
    wx, wy, ww, wh = (dtype(w) for w in weights)
    one, half = dtype(1), dtype(0.5)
    ew, eh = prop[:, 2] - prop[:, 0] + one, prop[:, 3] - prop[:, 1] + one
    ex, ey = prop[:, 0] + half * ew, prop[:, 1] + half * eh
    ewp, exp = ew, ex
    if prop.shape[1] == 6:
        ewp = prop[:, 5] - prop[:, 4] + one
        exp = prop[:, 4] + half * ewp
    gw, gh, gwp = ref6[:, 2] - ref6[:, 0] + one, ref6[:, 3] - ref6[:, 1] + one, ref6[:, 5] - ref6[:, 4] + one
    gx, gy, gxp = ref6[:, 0] + half * gw, ref6[:, 1] + half * gh, ref6[:, 4] + half * gwp
    return np.stack([wx * (gx - ex) / ew, wy * (gy - ey) / eh, ww * np.log(gw / ew), wh * np.log(gh / eh),
                     wx * (gxp - exp) / ewp, ww * np.log(gwp / ewp)], axis=1).astype(dtype)


def rpn_targets(anchors, visibility, gt_left, gt_right, high, low, weights=(1.0, 1.0, 1.0, 1.0), dtype=F32):
    """one image -> matched [R] int64, labels [R] fp32 (1 / 0 / -1), regression targets [R,6]"""
    union, orig = expand_left_right(gt_left, gt_right)
    m = match(iou_matrix(union, anchors), high, low, True)
    labels = (m >= 0).astype(F32)
    labels[m == -1] = 0
    labels[~np.asarray(visibility, bool)] = -1
    labels[m == -2] = -1
    return m, labels, encode(orig[np.maximum(m, 0)], anchors, weights, dtype)


def box_targets(prop6, gt6, gt_labels, high, low, weights, dtype=F32):
    """one image, joint 6-boxes -> matched, labels [R] int64, regression targets [R,6]"""
    pu, po = expand_left_right(*box6_views(prop6))
    gu, go = expand_left_right(*box6_views(gt6))
    m = match(iou_matrix(gu, pu), high, low, False)
    labels = np.asarray(gt_labels, np.int64)[np.maximum(m, 0)].copy()
    labels[m == -1] = 0
    labels[m == -2] = -1
    return m, labels, encode(go[np.maximum(m, 0)], po, weights, dtype)


# ---- sampling
def sample(labels, draws, batch, fraction):
    """one image -> pos mask, neg mask (uint8): the num_pos / num_neg members with the smallest (draw, index) keys"""
    labels, draws = np.asarray(labels), np.asarray(draws, F32)
    pos, neg = np.nonzero(labels >= 1)[0], np.nonzero(labels == 0)[0]
    num_pos = min(pos.size, int(batch * fraction))
    num_neg = min(neg.size, batch - num_pos)
    pm, nm = np.zeros(labels.shape[0], np.uint8), np.zeros(labels.shape[0], np.uint8)
    pm[pos[np.argsort(draws[pos], kind="stable")[:num_pos]]] = 1
    nm[neg[np.argsort(draws[neg], kind="stable")[:num_neg]]] = 1
    return pm, nm


# ---- losses (torch CPU, any dtype; gradients by autograd)
def smooth_l1_sum(x, t, beta):
    n = (x - t).abs()
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum()


def flatten_level(layer, N, C, H, W):
    return layer.view(N, -1, C, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, C)


def srpn_loss(cls_logits, bbox_pred, labels, reg, pos_mask, neg_mask, dtype=torch.float64):
    """The reference's literal composition from the RAW maps: the head's softmax over view(N, 2, -1, W), the (A,2) / (A,6) flattening, then
    cross_entropy and smooth L1.  -> (loss_objectness, loss_box, [grad per cls map], [grad per bbox map]) as numpy fp64"""
    zs = [torch.as_tensor(z).to(dtype).clone().requires_grad_() for z in cls_logits]
    bs = [torch.as_tensor(b).to(dtype).clone().requires_grad_() for b in bbox_pred]
    obj, box = [], []
    for z, b in zip(zs, bs):
        N, _, H, W = z.shape
        p = z.view(N, 2, -1, W).softmax(1).view(*z.shape)
        obj.append(flatten_level(p, N, 2, H, W))
        box.append(flatten_level(b, N, 6, H, W))
    obj, box = torch.cat(obj, dim=1).reshape(-1, 2), torch.cat(box, dim=1).reshape(-1, 6)
    pos = torch.nonzero(torch.as_tensor(np.asarray(pos_mask))).squeeze(1)
    neg = torch.nonzero(torch.as_tensor(np.asarray(neg_mask))).squeeze(1)
    sampled = torch.cat([pos, neg])
    zero = [np.zeros(tuple(z.shape)) for z in zs], [np.zeros(tuple(b.shape)) for b in bs]
    if sampled.numel() == 0:
        return 0.0, 0.0, zero[0], zero[1]
    labels, reg = torch.as_tensor(np.asarray(labels)), torch.as_tensor(np.asarray(reg)).to(dtype)
    loss_box = smooth_l1_sum(box[pos], reg[pos], 1.0 / 9) / sampled.numel()
    loss_obj = F.cross_entropy(obj[sampled], labels[sampled].long())
    gz = torch.autograd.grad(loss_obj, zs, retain_graph=True)
    gb = torch.autograd.grad(loss_box, bs, allow_unused=True) if pos.numel() else [None] * len(bs)
    return (float(loss_obj.detach().double()), float(loss_box.detach().double()), [g.double().numpy() for g in gz],
            [np.zeros(tuple(b.shape)) if g is None else g.double().numpy() for g, b in zip(gb, bs)])


def fastrcnn_loss(class_logits, box_regression, labels, reg, dtype=torch.float64):
    x = torch.as_tensor(class_logits).to(dtype).clone().requires_grad_()
    b = torch.as_tensor(box_regression).to(dtype).clone().requires_grad_()
    labels, reg = torch.as_tensor(np.asarray(labels)).long(), torch.as_tensor(np.asarray(reg)).to(dtype)
    loss_cls = F.cross_entropy(x, labels)
    rows = torch.nonzero(labels > 0).squeeze(1)
    cols = 6 * labels[rows][:, None] + torch.arange(6)
    loss_box = smooth_l1_sum(b[rows[:, None], cols], reg[rows], 1.0) / labels.numel()
    gx, = torch.autograd.grad(loss_cls, x)
    gb = torch.autograd.grad(loss_box, b)[0] if rows.numel() else torch.zeros_like(b)
    return float(loss_cls.detach().double()), float(loss_box.detach().double()), gx.double().numpy(), gb.double().numpy()


# ---- mask targets
def crop_bounds(box, width, height):
    """BinaryMaskList.crop: Python's round (half to even) of each coordinate, the four clamps, at least one pixel -> x0, y0, w, h"""
    xmin, ymin, xmax, ymax = [round(float(b)) for b in box]
    xmin, ymin = min(max(xmin, 0), width - 1), min(max(ymin, 0), height - 1)
    xmax, ymax = min(max(xmax, 0), width), min(max(ymax, 0), height)
    xmax, ymax = max(xmax, xmin + 1), max(ymax, ymin + 1)
    return xmin, ymin, xmax - xmin, ymax - ymin


def resize_axis(in_size, out_size):
    """indices and weights of torch's CPU bilinear upsampling along one axis, align_corners=False, fp32.  The source index scale * (i + 0.5)
    - 0.5 has ONE rounding (the CPU kernel fuses it); both factors are short enough for the fp64 product and sum below to be exact."""
    if in_size == out_size:
        i = np.arange(out_size)
        return i, i, np.ones(out_size, F32), np.zeros(out_size, F32)
    scale = F32(in_size) / F32(out_size)
    src = (np.float64(scale) * (np.arange(out_size) + 0.5) - 0.5).astype(F32)
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    l1 = np.clip(src - i0.astype(F32), F32(0), F32(1)).astype(F32)
    return i0, i0 + (i0 < in_size - 1), F32(1) - l1, l1


def resize_crop(crop, M):
    """crop [h,w] of 0 / 1 -> the M x M bilinear resize as fp32 (the target is its truncation to uint8: 1 only where it reaches 1.0)"""
    c = np.asarray(crop).astype(F32)
    y0, y1, wy0, wy1 = resize_axis(c.shape[0], M)
    x0, x1, wx0, wx1 = resize_axis(c.shape[1], M)
    w00, w01, w10, w11 = wy0[:, None] * wx0[None, :], wy0[:, None] * wx1[None, :], wy1[:, None] * wx0[None, :], wy1[:, None] * wx1[None, :]
    return (((c[y0][:, x0] * w00 + c[y0][:, x1] * w01) + c[y1][:, x0] * w10) + c[y1][:, x1] * w11).astype(F32)   # weights first, left to right


def mask_target(mask, box, M):
    """mask [H,W] uint8, box xyxy -> [M,M] uint8"""
    x0, y0, w, h = crop_bounds(box, mask.shape[1], mask.shape[0])
    return resize_crop(mask[y0:y0 + h, x0:x0 + w], M).astype(np.uint8)


def mask_instances(H, W):
    """three instances of an H x W image: a filled rectangle, a one-pixel-wide line, a checkerboard"""
    rect, line = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    rect[H // 5:H - H // 4, W // 6:W - W // 3] = 1
    line[:, W // 2] = 1
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([rect, line, ((yy + xx) % 2).astype(np.uint8)])


def mask_rois(H, W, M):
    """coordinates ending in .5 (half to even both ways), partly and wholly outside, under one pixel, the whole image, exactly M x M (every
    lambda 0), and two ordinary ones"""
    return np.array([[2.5, 3.5, 20.5, 21.5], [1.5, 0.5, 30.5, 25.5], [-5.3, -4.2, 15.7, 12.1], [W + 60.0, H + 50.0, W + 80.0, H + 90.0],
                     [10.2, 10.3, 10.4, 10.45], [0.0, 0.0, float(W), float(H)], [5.0, 6.0, 5.0 + M, 6.0 + M],
                     [3.3, 2.2, W - 4.6, H - 7.9], [W / 3.0, H / 4.0, W / 3.0 + 9.7, H / 4.0 + 17.2]], F32)


def mask_loss(mask_logits, cls, targets, dtype=torch.float64):
    """mask_logits [P,C,M,M], cls [P] int64 (> 0 on the positive ROIs), targets [P,M,M] 0 / 1 -> (loss, grad [P,C,M,M]) over the positive ROIs"""
    x = torch.as_tensor(mask_logits).to(dtype).clone().requires_grad_()
    cls = torch.as_tensor(np.asarray(cls)).long()
    rows = torch.nonzero(cls > 0).squeeze(1)
    if rows.numel() == 0:
        return 0.0, np.zeros(tuple(x.shape))
    loss = F.binary_cross_entropy_with_logits(x[rows, cls[rows]], torch.as_tensor(np.asarray(targets))[rows].to(dtype))
    g, = torch.autograd.grad(loss, x)
    return float(loss.detach().double()), g.double().numpy()

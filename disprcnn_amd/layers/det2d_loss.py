"""The stereo 2D stage's training targets, balanced sampling and losses on HIP (pts/det_train.hip), with the gradients with respect to the
network outputs.  Reference: modeling/rpn/stereo_rpn/loss.py, roi_heads/box_head/loss.py, matcher.py,
balanced_positive_negative_sampler.py, box_coder.py (encode_*), utils/stereo_utils.py (expand_left_right_box).

    match_label_encode(cand, cand_counts, gt_left, gt_right, gt_counts, high, low, ...) -> (matched [R] int64, labels [R], reg_targets [R,6])
    balanced_sample(labels, cand_counts, batch, fraction, draws=None, ...)             -> (pos_mask, neg_mask [R] u8, counts [N,2] int32, idx)
    srpn_loss(cls_logits, bbox_pred, pos_mask, neg_mask, reg_targets, counts)           -> (loss_objectness, loss_rpn_box_reg, terms [3])
    fastrcnn_loss(class_logits, box_regression, labels, reg_targets)                    -> (loss_classifier, loss_box_reg, terms [3])
    mask_loss(mask_logits, boxes, roi_counts, matched, inst_labels, masks, table, ...)  -> (loss_mask, terms [2], targets [P,M,M] u8, count)

All images go in one launch; `cand_counts` / `gt_counts` are the per-image lengths (Python ints: the lists' lengths), from which an image
with no ground truth or no candidate raises ValueError on the host, as the reference's Matcher does.  At most MAX_GT ground truths per
image and MAX_IMAGES images.  Everything that decides a label, a match or a tie is fp32 in the reference's operation order; the loss sums
are fp64, per-block partials added in block order: two runs give the same bits and nothing reads back to the host, so a step with these
pieces can be captured in a graph.

balanced_sample takes its randomness as an input, like layers/proposal_target.py: every candidate reads one fp32 uniform in [0, 1) from
`draws` (one torch.rand call by default) and the num_pos positives / num_neg negatives with the smallest (draw, index) keys are taken.
That has the distribution of the reference's `randperm(n)[:k]` but NOT its generator stream: the same seed samples other candidates.

The losses are autograd Functions whose forward launch also writes the gradient; backward scales it by the incoming scalar.  They come
back as 0-dim fp32 device tensors (views of `terms`, the vector the kernel wrote: the two losses and their divisor).  Deviation: a batch
with no sampled anchor gives zero RPN losses and zero gradients where the reference gives NaN.
"""
import ctypes as C

import torch
from torch.autograd import Function

from .. import engine as E
from ..pts import _lib

MAX_GT = 128          # DRC_DET2D_MAX_GT
MAX_IMAGES = 64       # DRC_DET2D_MAX_IMAGES
MAX_LEVELS = 8        # DRC_DET2D_MAX_LEVELS


def _offsets(counts, what, name, allow_empty=False):
    counts = [int(c) for c in counts]
    if not 1 <= len(counts) <= MAX_IMAGES:
        raise ValueError(f"{what}: 1 .. {MAX_IMAGES} images expected, got {len(counts)}")
    off = [0]
    for c in counts:
        if c < 0 or (c == 0 and not allow_empty):
            raise ValueError(f"No {name} available for one of the images during training")
        off.append(off[-1] + c)
    return (C.c_int32 * len(off))(*off), off[-1]


def _host(arr):
    return C.cast(arr, C.c_void_p)


def _dev(t, what, dtype, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what}: expected a CUDA/HIP tensor on an MI355X; the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"{what}: {dtype} expected, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: shape {tuple(shape)} expected, got {tuple(t.shape)}")
    return t.contiguous()


def match_label_encode(cand, cand_counts, gt_left, gt_right, gt_counts, high, low, allow_low_quality=False, weights=(1.0, 1.0, 1.0, 1.0),
                       gt_labels=None, visibility=None):
    """cand [R,4] (anchors: the RPN form, targets coded ..._fromboxes4) or [R,6] (joint proposals x1 y1 x2 y2 x1' x2': the box head's form,
    matched by the union of their views, coded ..._fromboxes6); gt_left / gt_right [G,4], the two views of the ground truths, matched by
    their union.  labels: fp32 1 / 0 / -1 without gt_labels (generate_rpn_labels; -1 also where `visibility` is false), else int64
    gt_labels at the matched row / 0 / -1."""
    what = "match_label_encode"
    E.require_gpu(cand, what)
    if cand.dim() != 2 or cand.shape[1] not in (4, 6):
        raise RuntimeError(f"{what}: cand [R,4] or [R,6] expected, got {tuple(cand.shape)}")
    cand_off, R = _offsets(cand_counts, what, "proposal boxes")
    gt_off, G = _offsets(gt_counts, what, "ground-truth boxes")
    if len(cand_off) != len(gt_off):
        raise ValueError(f"{what}: {len(cand_off) - 1} images of candidates, {len(gt_off) - 1} of ground truths")
    if max(int(c) for c in gt_counts) > MAX_GT:
        raise ValueError(f"{what}: at most {MAX_GT} ground truths per image, got {max(int(c) for c in gt_counts)}")
    if cand.shape[0] != R:
        raise RuntimeError(f"{what}: {cand.shape[0]} candidates for counts that sum to {R}")
    dev = cand.device
    cand = cand.contiguous()
    gt_left = _dev(gt_left, what + " gt_left", torch.float32, (G, 4))
    gt_right = _dev(gt_right, what + " gt_right", torch.float32, (G, 4))
    if gt_labels is not None:
        gt_labels = _dev(gt_labels, what + " gt_labels", torch.int64, (G,))
    if visibility is not None:
        if visibility.dtype == torch.bool:
            visibility = visibility.view(torch.uint8)
        visibility = _dev(visibility, what + " visibility", torch.uint8, (R,))
    matched = torch.empty(R, dtype=torch.int64, device=dev)
    labels = torch.empty(R, dtype=torch.float32 if gt_labels is None else torch.int64, device=dev)
    reg = torch.empty((R, 6), dtype=torch.float32, device=dev)
    gt_max = torch.empty(G, dtype=torch.int32, device=dev) if allow_low_quality else None
    w = (C.c_float * 4)(*[float(v) for v in weights])
    st = _lib.lib().drc_det2d_match_fwd(len(cand_off) - 1, _host(cand_off), _host(gt_off), cand.shape[1], E._ptr(cand), E._ptr(gt_left),
                                        E._ptr(gt_right), E._ptr(gt_labels), E._ptr(visibility), float(high), float(low),
                                        1 if allow_low_quality else 0, _host(w), E._ptr(gt_max), E._ptr(matched),
                                        E._ptr(labels if gt_labels is None else None), E._ptr(None if gt_labels is None else labels),
                                        E._ptr(reg), E._stream_ptr(dev))
    _lib.check(st, "drc_det2d_match_fwd")
    return matched, labels, reg


def balanced_sample(labels, cand_counts, batch, fraction, draws=None, want_indices=False):
    """labels [R] fp32 or int64 (>= 1 positive, 0 negative, else ignored), concatenated over the images of `cand_counts`.
    -> pos_mask, neg_mask [R] uint8, counts [N,2] int32 (num_pos, num_neg per image, on the device), and with want_indices the [N,batch]
    int64 image-local indices of pos | neg in ascending order (-1 past an image's count), else None."""
    what = "balanced_sample"
    if not labels.is_cuda:
        raise RuntimeError(f"{what}: expected CUDA/HIP labels on an MI355X; the HIP path has no CPU fallback")
    if labels.dtype not in (torch.float32, torch.int64):
        raise RuntimeError(f"{what}: fp32 or int64 labels expected, got {labels.dtype}")
    off, R = _offsets(cand_counts, what, "candidates", allow_empty=True)
    if labels.shape != (R,):
        raise RuntimeError(f"{what}: labels [{R}] expected, got {tuple(labels.shape)}")
    batch = int(batch)
    cap_pos = int(batch * fraction)
    if batch < 0 or not 0 <= cap_pos <= batch:
        raise ValueError(f"{what}: batch >= 0 and a fraction in [0, 1] expected, got {batch}, {fraction}")
    dev = labels.device
    if draws is None:
        draws = torch.rand(R, dtype=torch.float32, device=dev)
    draws = _dev(draws, what + " draws", torch.float32, (R,))
    labels = labels.contiguous()
    N = len(off) - 1
    pos = torch.empty(R, dtype=torch.uint8, device=dev)
    neg = torch.empty(R, dtype=torch.uint8, device=dev)
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    idx = torch.empty((N, batch), dtype=torch.int64, device=dev) if want_indices else None
    st = _lib.lib().drc_det2d_sample_fwd(N, _host(off), E._ptr(labels), 0 if labels.dtype == torch.float32 else 1, E._ptr(draws), batch, cap_pos,
                                         E._ptr(pos), E._ptr(neg), E._ptr(counts), E._ptr(idx), E._stream_ptr(dev))
    _lib.check(st, "drc_det2d_sample_fwd")
    return pos, neg, counts, idx


def srpn_loss_launch(pos_mask, neg_mask, reg_targets, counts, beta, logits, bbox):
    """One drc_det2d_srpn_loss_fwd launch over contiguous per-level maps -> (terms [3], [gradient per cls map], [gradient per bbox map])."""
    L = len(logits)
    dev = logits[0].device
    N, A = logits[0].shape[0], logits[0].shape[1] // 2
    glogits, gbbox = [torch.empty_like(m) for m in logits], [torch.empty_like(m) for m in bbox]
    rows, off = [], 0
    for z, b, gz, gb in zip(logits, bbox, glogits, gbbox):
        H, W = z.shape[2:]
        rows += [z.data_ptr(), b.data_ptr(), gz.data_ptr(), gb.data_ptr(), H, W, off]
        off += H * W * A
    table = (C.c_int64 * len(rows))(*rows)
    lib = _lib.lib()
    n_part = lib.drc_det2d_srpn_loss_partials(N, A, L, _host(table))
    if n_part < 0:
        raise RuntimeError("srpn_loss: unsupported shape")
    partials = torch.empty(n_part, dtype=torch.float64, device=dev)
    terms = torch.empty(3, dtype=torch.float32, device=dev)
    st = lib.drc_det2d_srpn_loss_fwd(N, A, L, _host(table), off, E._ptr(pos_mask), E._ptr(neg_mask), E._ptr(reg_targets), E._ptr(counts),
                                     float(beta), E._ptr(partials), E._ptr(terms), E._stream_ptr(dev))
    _lib.check(st, "drc_det2d_srpn_loss_fwd")
    return terms, glogits, gbbox


class _SRPNLoss(Function):
    @staticmethod
    def forward(ctx, pos_mask, neg_mask, reg_targets, counts, beta, *maps):
        L = len(maps) // 2
        logits, bbox = [m.contiguous() for m in maps[:L]], [m.contiguous() for m in maps[L:]]
        terms, glogits, gbbox = srpn_loss_launch(pos_mask, neg_mask, reg_targets, counts, beta, logits, bbox)
        ctx.grads = (glogits, gbbox)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms)
        return terms[0], terms[1], terms

    @staticmethod
    def backward(ctx, g_obj, g_box, _g_terms):
        glogits, gbbox = ctx.grads
        out = [torch.zeros_like(g) if g_obj is None else g * g_obj.to(torch.float32) for g in glogits]
        out += [torch.zeros_like(g) if g_box is None else g * g_box.to(torch.float32) for g in gbbox]
        return (None,) * 5 + tuple(out)


def srpn_loss(cls_logits, bbox_pred, pos_mask, neg_mask, reg_targets, counts, beta=1.0 / 9):
    """cls_logits: per level the RAW [N,2A,H,W] map, bbox_pred: per level [N,6A,H,W], both read in place; pos_mask / neg_mask [N*total] and
    counts [N,2] as balanced_sample returned them for the images' concatenated anchors (level-major, then (y*W + x)*A + a), reg_targets
    [N*total,6].  The objective is the reference's: the head's softmax pairs raw channel c with c + A, the loss reads the probability map as
    (A,2) -- anchor a's vector is (p[2a], p[2a+1]) -- and takes cross_entropy of that vector.  -> (loss_objectness, loss_rpn_box_reg, terms)."""
    what = "srpn_loss"
    cls_logits, bbox_pred = list(cls_logits), list(bbox_pred)
    if not 1 <= len(cls_logits) <= MAX_LEVELS or len(cls_logits) != len(bbox_pred):
        raise RuntimeError(f"{what}: 1 .. {MAX_LEVELS} levels of cls_logits and as many of bbox_pred expected")
    N, A = cls_logits[0].shape[0], cls_logits[0].shape[1] // 2
    total = 0
    for z, b in zip(cls_logits, bbox_pred):
        E.require_gpu(z, what)
        E.require_gpu(b, what)
        if z.dim() != 4 or z.shape[:2] != (N, 2 * A) or b.shape != (N, 6 * A) + tuple(z.shape[2:]):
            raise RuntimeError(f"{what}: cls_logits [N,2A,H,W] and bbox_pred [N,6A,H,W] expected, got {tuple(z.shape)}, {tuple(b.shape)}")
        total += z.shape[2] * z.shape[3] * A
    if not 1 <= N <= MAX_IMAGES or A < 1:
        raise RuntimeError(f"{what}: 1 .. {MAX_IMAGES} images and at least one anchor per location expected")
    pos_mask = _dev(pos_mask, what + " pos_mask", torch.uint8, (N * total,))
    neg_mask = _dev(neg_mask, what + " neg_mask", torch.uint8, (N * total,))
    reg_targets = _dev(reg_targets, what + " reg_targets", torch.float32, (N * total, 6))
    counts = _dev(counts, what + " counts", torch.int32, (N, 2))
    return _SRPNLoss.apply(pos_mask, neg_mask, reg_targets, counts, float(beta), *cls_logits, *bbox_pred)


class _FastRCNNLoss(Function):
    @staticmethod
    def forward(ctx, class_logits, box_regression, labels, reg_targets):
        dev = class_logits.device
        x, b = class_logits.contiguous(), box_regression.contiguous()
        R, Cn = x.shape
        gx, gb = torch.empty_like(x), torch.empty_like(b)
        partials = torch.empty(2 * ((R + 255) // 256), dtype=torch.float64, device=dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        st = _lib.lib().drc_det2d_fastrcnn_loss_fwd(R, Cn, E._ptr(x), E._ptr(labels), E._ptr(b), E._ptr(reg_targets), E._ptr(gx), E._ptr(gb),
                                                    E._ptr(partials), E._ptr(terms), E._stream_ptr(dev))
        _lib.check(st, "drc_det2d_fastrcnn_loss_fwd")
        ctx.grads = (gx, gb)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms)
        return terms[0], terms[1], terms

    @staticmethod
    def backward(ctx, g_cls, g_box, _g_terms):
        gx, gb = ctx.grads
        return (torch.zeros_like(gx) if g_cls is None else gx * g_cls.to(torch.float32),
                torch.zeros_like(gb) if g_box is None else gb * g_box.to(torch.float32), None, None)


def fastrcnn_loss(class_logits, box_regression, labels, reg_targets):
    """class_logits [R,C], box_regression [R,6C], labels [R] int64 in [0, C), reg_targets [R,6] -> (cross_entropy, mean over R; smooth L1 with
    beta 1 over columns 6*label .. 6*label+5 of the rows with label > 0, summed, over R; terms)."""
    what = "fastrcnn_loss"
    E.require_gpu(class_logits, what)
    E.require_gpu(box_regression, what)
    if class_logits.dim() != 2 or class_logits.shape[0] < 1:
        raise RuntimeError(f"{what}: class_logits [R,C] with R >= 1 expected, got {tuple(class_logits.shape)}")
    R, Cn = class_logits.shape
    if box_regression.shape != (R, 6 * Cn):
        raise RuntimeError(f"{what}: box_regression [{R},{6 * Cn}] expected, got {tuple(box_regression.shape)}")
    labels = _dev(labels, what + " labels", torch.int64, (R,))
    reg_targets = _dev(reg_targets, what + " reg_targets", torch.float32, (R, 6))
    return _FastRCNNLoss.apply(class_logits, box_regression, labels, reg_targets)


class _MaskLoss(Function):
    @staticmethod
    def forward(ctx, mask_logits, boxes, matched, inst_labels, masks, table, roi_off, inst_off, n_images):
        dev = mask_logits.device
        x = mask_logits.contiguous()
        P, Cn, M = x.shape[0], x.shape[1], x.shape[2]
        grad = torch.empty_like(x)
        targets = torch.empty((P, M, M), dtype=torch.uint8, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        partials = torch.empty(max(P, 1), dtype=torch.float64, device=dev)
        terms = torch.empty(2, dtype=torch.float32, device=dev)
        st = _lib.lib().drc_det2d_mask_loss_fwd(n_images, _host(roi_off), _host(inst_off), Cn, M, E._ptr(boxes), E._ptr(matched),
                                                E._ptr(inst_labels), E._ptr(x), E._ptr(masks), E._ptr(table), E._ptr(count), E._ptr(targets),
                                                E._ptr(grad), E._ptr(partials), E._ptr(terms), E._stream_ptr(dev))
        _lib.check(st, "drc_det2d_mask_loss_fwd")
        ctx.grad = grad
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms, targets, count)
        return terms[0], terms, targets, count

    @staticmethod
    def backward(ctx, g, _g_terms, _g_targets, _g_count):
        return (torch.zeros_like(ctx.grad) if g is None else ctx.grad * g.to(torch.float32),) + (None,) * 8


def pack_masks(masks):
    """The instance masks of all images, per image a uint8 [G,H,W] device tensor -> (one flat uint8 buffer, table [I,3] int64 on the device =
    offset, H, W of each instance, the per-image instance counts)."""
    rows, off, counts = [], 0, []
    for m in masks:
        if not torch.is_tensor(m) or not m.is_cuda or m.dtype != torch.uint8 or m.dim() != 3:
            raise RuntimeError("pack_masks: per image a uint8 [G,H,W] CUDA/HIP tensor expected; the HIP path has no CPU fallback")
        G, H, W = m.shape
        rows += [(off + g * H * W, H, W) for g in range(G)]
        off += G * H * W
        counts.append(G)
    dev = masks[0].device
    flat = torch.cat([m.reshape(-1) for m in masks]) if off else torch.zeros(1, dtype=torch.uint8, device=dev)
    table = torch.tensor(rows if rows else [(0, 1, 1)], dtype=torch.int64).to(dev)
    return flat, table, counts


def mask_loss(mask_logits, boxes, roi_counts, matched, inst_labels, masks, table, inst_counts):
    """mask_logits [P,C,M,M]; boxes [P,4] the mask head's proposals, `roi_counts` per image; matched [P] int64 as match_label_encode
    returned it for them (no low-quality matches); inst_labels [I] int64, masks / table / inst_counts as pack_masks returned them.  A ROI is
    positive when its match is not -1 and the instance at the matched row (clamped at 0) has a label > 0; the others drop out on the
    device.  -> (loss, terms [2] = loss and the pixel count, targets [P,M,M] uint8, count [1] int32 of positive ROIs).  The loss is
    binary_cross_entropy_with_logits of the ROIs' class planes against the cropped, resized and truncated instance masks, the mean over the
    positive ROIs' pixels; 0 without a positive ROI."""
    what = "mask_loss"
    E.require_gpu(mask_logits, what)
    if mask_logits.dim() != 4 or mask_logits.shape[2] != mask_logits.shape[3]:
        raise RuntimeError(f"{what}: mask_logits [P,C,M,M] expected, got {tuple(mask_logits.shape)}")
    roi_off, P = _offsets(roi_counts, what, "proposal boxes", allow_empty=True)
    inst_off, I = _offsets(inst_counts, what, "ground-truth boxes", allow_empty=True)
    if len(roi_off) != len(inst_off) or mask_logits.shape[0] != P:
        raise RuntimeError(f"{what}: {mask_logits.shape[0]} rows of logits for {P} ROIs of {len(roi_off) - 1} images, {len(inst_off) - 1} images of instances")
    boxes = _dev(boxes, what + " boxes", torch.float32, (P, 4))
    matched = _dev(matched, what + " matched", torch.int64, (P,))
    inst_labels = _dev(inst_labels, what + " inst_labels", torch.int64, (I,))
    table = _dev(table, what + " table", torch.int64, (max(I, 1), 3))
    masks = _dev(masks, what + " masks", torch.uint8)
    return _MaskLoss.apply(mask_logits, boxes, matched, inst_labels, masks, table, roi_off, inst_off, len(roi_off) - 1)

"""PointRCNN's training labels and losses (point_rcnn/lib/net/point_rcnn.py:generate_rpn_training_labels, utils/loss_utils.py,
net/rpn_loss.py, net/rcnn_loss.py) on HIP, with the gradients with respect to the network outputs.

    rpn_point_labels(pts, boxes7, corners, corners_large)                     -> (cls_label [B,N], reg_label [B,N,7])
    reg_bin_targets(reg_label, loc_scope, ..., anchor_size, ...)              -> (bins [rows,4] int32, res [rows,7])
    bin_reg_loss(pred_reg, reg_label, row_mask, loc_scope, ..., loss_mask)    -> (loss_loc, loss_angle, loss_size, terms [16])
    point_cls_loss(kind, logits, labels, mask, ...)                           -> (loss, terms [8])
    focal_loss_elementwise(logits, targets, weights, alpha, gamma)            -> unreduced loss, logits' shape

bin_reg_loss is get_reg_loss over the rows `row_mask` selects: the reference's `pred_reg[fg_mask]` would need a compaction whose size
the host has to know, so the kernel takes every row and skips the unselected ones.  Labels are fp32 in the reference's expression order
(its Python-double constants are rounded to fp32 one at a time, here at the call, as decode_rpn_boxes documents), so a row lands in the
reference's bin; reg_bin_targets returns those labels from the same device function the loss calls.  Loss values are evaluated and summed
in fp64, per-block partials added in block order: two runs give the same bits, nothing synchronises with the host, and the reference's
`if count != 0: divide` is a select on the device, so a step with these losses can be captured in a graph.

The losses come back as 0-dim fp32 device tensors (views of `terms`, the vector the kernel wrote; its layout is REG_TERMS / CLS_TERMS).
"""
import ctypes as C
import math

import torch
from torch.autograd import Function

from .. import engine as E
from ..pts import _lib

REG_TERMS = ("loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res", "loss_y_offset|loss_y_bin", "loss_y_res", "loss_ry_bin", "loss_ry_res",
             "loss_size", "loss_loc", "loss_angle", "loss_size", "rows", "mask_rows", "", "")
CLS_TERMS = ("loss", "loss_pos", "loss_neg", "normalizer", "", "", "", "")
CLS_KINDS = {"BinaryCrossEntropy": 1, "SigmoidFocalLoss": 2, "DiceLoss": 3}


def _scratch(dev):
    """fp64 workspace of the two-launch reductions, as a float buffer of twice the length (engine.scratch hands out fp32)"""
    return E.scratch(dev, "pointrcnn_loss", 2 * _lib.lib().drc_train_scratch_doubles())


def _mask_u8(m, n, dev, what):
    if m is None:
        return None
    if not m.is_cuda:
        raise RuntimeError(f"{what}: expected a CUDA/HIP mask on an MI355X; the HIP path has no CPU fallback")
    if m.numel() != n:
        raise RuntimeError(f"{what}: mask of {m.numel()} elements for {n} rows")
    m = m.reshape(-1)
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    return (m != 0).view(torch.uint8)


# ---- labels
def rpn_point_labels(pts, boxes7, corners, corners_large):
    """pts (B,N,3); one ground-truth box per cloud: boxes7 (B,7) 'xyzhwl_ry', corners (B,8,3), corners of the enlarged box (B,8,3)
    -> cls_label (B,N) in {1, 0, -1}, reg_label (B,N,7).  One kernel, one thread per point."""
    what = "rpn_point_labels"
    for t in (pts, boxes7, corners, corners_large):
        E.require_gpu(t, what)
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise RuntimeError(f"{what}: pts [B,N,3] expected, got {tuple(pts.shape)}")
    B, N = pts.shape[:2]
    corners, corners_large = corners.reshape(-1, 8, 3), corners_large.reshape(-1, 8, 3)
    if boxes7.shape != (B, 7) or corners.shape[0] != B or corners_large.shape[0] != B:
        raise RuntimeError(f"{what}: one box per cloud expected (boxes7 [B,7], corners [B,8,3] twice), got {tuple(boxes7.shape)}, "
                           f"{tuple(corners.shape)}, {tuple(corners_large.shape)} for B = {B}")
    cls_label = torch.empty((B, N), dtype=torch.float32, device=pts.device)
    reg_label = torch.empty((B, N, 7), dtype=torch.float32, device=pts.device)
    if B * N:
        st = _lib.lib().drc_rpn_point_labels(B, N, E._ptr(pts.contiguous()), E._ptr(boxes7.contiguous()), E._ptr(corners.contiguous()),
                                             E._ptr(corners_large.contiguous()), E._ptr(cls_label), E._ptr(reg_label), E._stream_ptr(pts.device))
        _lib.check(st, "drc_rpn_point_labels")
    return cls_label, reg_label


# ---- regression
class _RegCfg:
    """The bin layout and the reference's constants as the kernel takes them: two small host arrays."""

    def __init__(self, loc_scope, loc_bin_size, num_head_bin, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size, get_ry_fine):
        self.P = int(loc_scope / loc_bin_size) * 2
        self.YB = int(loc_y_scope / loc_y_bin_size) * 2
        self.H = int(num_head_bin)
        self.xz_fine, self.y_by_bin, self.ry_fine = bool(get_xz_fine), bool(get_y_by_bin), bool(get_ry_fine)
        self.channels = self.P * (4 if self.xz_fine else 2) + (2 * self.YB if self.y_by_bin else 1) + 2 * self.H + 3
        apc = (math.pi / 2) / num_head_bin if self.ry_fine else (2 * math.pi) / num_head_bin
        self.cst = (C.c_float * 17)(loc_scope, loc_scope * 2 - 1e-3, loc_bin_size, loc_bin_size / 2,
                                    loc_y_scope, loc_y_scope * 2 - 1e-3, loc_y_bin_size, loc_y_bin_size / 2,
                                    apc, apc / 2, 2 * math.pi, math.pi, math.pi * 0.5, math.pi * 1.5, math.pi * 0.25, 1e-3, math.pi * 0.5 - 1e-3)

    def opt(self, anchor_per_row):
        return (C.c_int32 * 8)(self.P, self.YB, self.H, self.xz_fine, self.y_by_bin, self.ry_fine, 1 if anchor_per_row else 0, 0)


def _host(arr):
    return C.cast(arr, C.c_void_p)


def _reg_inputs(what, reg_label, anchor_size):
    E.require_gpu(reg_label, what)
    if reg_label.dim() != 2 or reg_label.shape[1] != 7:
        raise RuntimeError(f"{what}: reg_label [rows,7] expected, got {tuple(reg_label.shape)}")
    rows = reg_label.shape[0]
    if not isinstance(anchor_size, torch.Tensor):
        anchor_size = torch.tensor([float(v) for v in anchor_size], dtype=torch.float32, device=reg_label.device)
    E.require_gpu(anchor_size, what)
    if anchor_size.shape == (3,):
        per_row = False
    elif anchor_size.shape == (rows, 3):
        per_row = True
    else:
        raise RuntimeError(f"{what}: anchor_size (3) or ({rows},3) expected, got {tuple(anchor_size.shape)}")
    return rows, reg_label.contiguous(), anchor_size.contiguous(), per_row


def reg_bin_targets(reg_label, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
                    loc_y_bin_size=0.25, get_ry_fine=False):
    """The labels get_reg_loss derives from reg_label (rows,7): bins (rows,4) int32 = x, z, y (-1 when y is not binned), ry bin, and
    res (rows,7) = the normalised residual labels of x, z, y (the y offset itself when not binned), ry, and the three size residuals."""
    what = "reg_bin_targets"
    rows, reg_label, anchor, per_row = _reg_inputs(what, reg_label, anchor_size)
    cfg = _RegCfg(loc_scope, loc_bin_size, num_head_bin, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size, get_ry_fine)
    bins = torch.empty((rows, 4), dtype=torch.int32, device=reg_label.device)
    res = torch.empty((rows, 7), dtype=torch.float32, device=reg_label.device)
    st = _lib.lib().drc_bin_reg_targets(rows, cfg.channels, E._ptr(reg_label), E._ptr(anchor), _host(cfg.opt(per_row)), _host(cfg.cst),
                                        E._ptr(bins), E._ptr(res), E._stream_ptr(reg_label.device))
    _lib.check(st, "drc_bin_reg_targets")
    return bins, res


class _BinRegLoss(Function):
    @staticmethod
    def forward(ctx, pred_reg, reg_label, row_mask, loss_mask, anchor, cfg, per_row):
        dev = pred_reg.device
        rows, Cn = pred_reg.shape
        pred = pred_reg.contiguous()
        sums = torch.empty(16, dtype=torch.float64, device=dev)
        terms = torch.empty(16, dtype=torch.float32, device=dev)
        opt = cfg.opt(per_row)
        st = _lib.lib().drc_bin_reg_loss_fwd(rows, Cn, E._ptr(pred), E._ptr(reg_label), E._ptr(row_mask), E._ptr(loss_mask), E._ptr(anchor),
                                             _host(opt), _host(cfg.cst), E._ptr(sums), E._ptr(terms), E._ptr(_scratch(dev)), E._stream_ptr(dev))
        _lib.check(st, "drc_bin_reg_loss_fwd")
        ctx.save_for_backward(pred, reg_label, row_mask, loss_mask, anchor, sums)
        ctx.cfg, ctx.per_row = cfg, per_row
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms)
        return terms[9], terms[10], terms[11], terms

    @staticmethod
    def backward(ctx, g_loc, g_angle, g_size, _g_terms):
        pred, reg_label, row_mask, loss_mask, anchor, sums = ctx.saved_tensors
        rows, Cn = pred.shape
        gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_loc, g_angle, g_size)]
        grad = torch.empty_like(pred)
        st = _lib.lib().drc_bin_reg_loss_bwd(rows, Cn, E._ptr(pred), E._ptr(reg_label), E._ptr(row_mask), E._ptr(loss_mask), E._ptr(anchor),
                                             _host(ctx.cfg.opt(ctx.per_row)), _host(ctx.cfg.cst), E._ptr(sums), E._ptr(gs[0]), E._ptr(gs[1]),
                                             E._ptr(gs[2]), E._ptr(grad), E._stream_ptr(pred.device))
        _lib.check(st, "drc_bin_reg_loss_bwd")
        return grad, None, None, None, None, None, None


def bin_reg_loss(pred_reg, reg_label, row_mask, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True, get_y_by_bin=False,
                 loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False, loss_mask=None):
    """get_reg_loss over the rows of pred_reg (rows,C) / reg_label (rows,7) that row_mask (rows) selects (None: every row); loss_mask (rows)
    is the reference's argument of that name, in all-rows indexing.  -> (loss_loc, loss_angle, loss_size, terms); loss_size is NOT yet
    multiplied by 3.  With no selected row every loss is 0 and the gradient into pred_reg is a zero tensor."""
    what = "bin_reg_loss"
    E.require_gpu(pred_reg, what)
    rows, reg_label, anchor, per_row = _reg_inputs(what, reg_label, anchor_size)
    cfg = _RegCfg(loc_scope, loc_bin_size, num_head_bin, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size, get_ry_fine)
    if pred_reg.dim() != 2 or pred_reg.shape[0] != rows:
        raise RuntimeError(f"{what}: pred_reg [rows,C] with reg_label's {rows} rows expected, got {tuple(pred_reg.shape)}")
    if pred_reg.shape[1] != cfg.channels:
        raise RuntimeError(f"{what}: pred_reg has {pred_reg.shape[1]} channels, the bin layout needs {cfg.channels}")
    if row_mask is None:
        row_mask = torch.ones(rows, dtype=torch.uint8, device=pred_reg.device)
    row_mask = _mask_u8(row_mask, rows, pred_reg.device, what)
    loss_mask = _mask_u8(loss_mask, rows, pred_reg.device, what)
    return _BinRegLoss.apply(pred_reg, reg_label, row_mask, loss_mask, anchor, cfg, per_row)


# ---- classification
class _PointClsLoss(Function):
    @staticmethod
    def forward(ctx, logits, labels, mask, kind, fg_weight, alpha, gamma, ignore):
        dev = logits.device
        flat = logits.reshape(-1).contiguous()
        sums = torch.empty(16, dtype=torch.float64, device=dev)
        terms = torch.empty(8, dtype=torch.float32, device=dev)
        st = _lib.lib().drc_point_cls_loss_fwd(flat.numel(), kind, E._ptr(flat), E._ptr(labels), E._ptr(mask), fg_weight, alpha, gamma, ignore,
                                               E._ptr(sums), E._ptr(terms), E._ptr(_scratch(dev)), E._stream_ptr(dev))
        _lib.check(st, "drc_point_cls_loss_fwd")
        ctx.save_for_backward(flat, labels, mask, sums)
        ctx.args = (kind, fg_weight, alpha, gamma, ignore)
        ctx.shape = logits.shape
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        flat, labels, mask, sums = ctx.saved_tensors
        if g is None:
            return (torch.zeros(ctx.shape, dtype=torch.float32, device=flat.device),) + (None,) * 7
        kind, fg_weight, alpha, gamma, ignore = ctx.args
        g = g.to(torch.float32).contiguous()
        grad = torch.empty_like(flat)
        st = _lib.lib().drc_point_cls_loss_bwd(flat.numel(), kind, E._ptr(flat), E._ptr(labels), E._ptr(mask), fg_weight, alpha, gamma, ignore,
                                               E._ptr(sums), E._ptr(g), E._ptr(grad), E._stream_ptr(flat.device))
        _lib.check(st, "drc_point_cls_loss_bwd")
        return (grad.view(ctx.shape),) + (None,) * 7


def point_cls_loss(kind, logits, labels, mask=None, fg_weight=1.0, alpha=0.25, gamma=2.0, ignore_target=-1):
    """The RPN / RCNN classification losses over logits (any shape, M elements), labels (M; 1 foreground, 0 background, -1 ignored) and an
    optional validity mask (M).  kind: 'BinaryCrossEntropy' (fg_weight), 'SigmoidFocalLoss' (alpha, gamma) or 'DiceLoss' (ignore_target;
    takes no mask, as the reference's).  -> (loss, terms): terms[1], terms[2] are the focal loss's positive and negative parts."""
    what = "point_cls_loss"
    if kind not in CLS_KINDS:
        raise NotImplementedError(f"{what}: kind {kind!r}; one of {sorted(CLS_KINDS)}")
    E.require_gpu(logits, what)
    if not labels.is_cuda:
        raise RuntimeError(f"{what}: expected CUDA/HIP labels on an MI355X; the HIP path has no CPU fallback")
    n = logits.numel()
    if labels.numel() != n:
        raise RuntimeError(f"{what}: {labels.numel()} labels for {n} logits")
    if kind == "DiceLoss" and mask is not None:
        raise RuntimeError(f"{what}: DiceLoss takes no mask (the reference applies none)")
    labels = labels.reshape(-1).to(torch.float32).contiguous()
    mask = _mask_u8(mask, n, logits.device, what)
    return _PointClsLoss.apply(logits, labels, mask, CLS_KINDS[kind], float(fg_weight), float(alpha), float(gamma), float(ignore_target))


class _FocalElementwise(Function):
    @staticmethod
    def forward(ctx, logits, targets, weights, alpha, gamma):
        x = logits.contiguous()
        out = torch.empty_like(x)
        st = _lib.lib().drc_focal_elementwise(x.numel(), E._ptr(x), E._ptr(targets), E._ptr(weights), alpha, gamma, None, E._ptr(out),
                                              E._stream_ptr(x.device))
        _lib.check(st, "drc_focal_elementwise")
        ctx.save_for_backward(x, targets, weights)
        ctx.args = (alpha, gamma)
        return out

    @staticmethod
    def backward(ctx, g):
        x, targets, weights = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        grad = torch.empty_like(x)
        st = _lib.lib().drc_focal_elementwise(x.numel(), E._ptr(x), E._ptr(targets), E._ptr(weights), ctx.args[0], ctx.args[1], E._ptr(g),
                                              E._ptr(grad), E._stream_ptr(x.device))
        _lib.check(st, "drc_focal_elementwise")
        return grad, None, None, None, None


def focal_loss_elementwise(logits, targets, weights, alpha=0.25, gamma=2.0):
    """SigmoidFocalClassificationLoss.forward: the unreduced loss, in logits' shape; differentiable in logits."""
    what = "focal_loss_elementwise"
    for t in (logits, targets, weights):
        E.require_gpu(t, what)
    if targets.shape != logits.shape or weights.shape != logits.shape:
        raise RuntimeError(f"{what}: logits, targets and weights of one shape expected, got {tuple(logits.shape)}, {tuple(targets.shape)}, "
                           f"{tuple(weights.shape)}")
    return _FocalElementwise.apply(logits, targets.contiguous(), weights.contiguous(), float(alpha), float(gamma))

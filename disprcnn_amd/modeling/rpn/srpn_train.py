"""The Stereo RPN's head + loss as ONE autograd Function with a sparse backward (csrc/srpn_train.hip).

The RPN loss reads at most cap = RPN.BATCH_SIZE_PER_IMAGE anchors per image and its pair softmax couples raw channel c only with c + A of
the same pixel (layers/det2d_loss.srpn_loss), so the gradient of the head maps is exactly zero outside at most cap pixels per image.  The
backward therefore never touches a dense map of the head: it runs on N * cap rows gathered from the active pixels,

    G    [N*cap, 8A]    the loss's gradient maps at the rows, scaled by the incoming g_obj / g_box          (drc_srpn_gather_rows)
    T    [N*cap, 4C]    the hidden map (conv3x3 + ReLU of the left view, then of the right view)            (gathered in the forward)
    Xcol [2*N*cap, 9C]  the 3 x 3 x C patches of the left, then of the right feature map, (c, ky, kx) order  (gathered in the forward)

    dT = G . Wpred            dWpred = G^T . T  (rows 0..2A-1: cls_logits, the rest: bbox_pred)       db_pred = column sums of G
    dZ = dT . [T > 0]         dZ2 = dZ as [2*N*cap, 2C]: the left rows, then the right rows            db_conv = column sums of dZ2
    dWconv = dZ2^T . Xcol     dXcol = dZ2 . Wconv -> drc_srpn_col2im -> the dense feature-map gradients (only when a map requires grad)

on drc_linear_fwd with drc_linear_pack_rows / drc_linear_pack_cols and drc_act_bwd_rows (fp64 fixed-order column sums).  The active set
comes from pos | neg -- the contract is explicit, nothing relies on an incoming gradient happening to be sparse.  Every buffer has N * cap
rows, rows past an image's count are zero rows, nothing is read back to the host and nothing is added atomically: every gradient has the
same bits run to run.
"""
import ctypes as C

import torch
from torch.autograd import Function

from ... import _lib
from ... import engine as E
from ...layers import det2d_loss as D
from ..head_ops import _gemm_packed, _pack_cols, _pack_rows, act_bwd_rows

MAX_LEVELS = 8          # DRC_SRPN_MAX_LEVELS


def level_table(N, A, Cin, cap, shapes):
    """The geometry part of drc_srpn_levels for a pyramid of `shapes` = [(H, W), ...]."""
    if not 1 <= len(shapes) <= MAX_LEVELS:
        raise ValueError(f"srpn_train: 1 .. {MAX_LEVELS} levels expected, got {len(shapes)}")
    lv = _lib.DrcSrpnLevels()
    lv.n_levels, lv.N, lv.A, lv.C, lv.cap = len(shapes), int(N), int(A), int(Cin), int(cap)
    off = 0
    for l, (h, w) in enumerate(shapes):
        lv.H[l], lv.W[l], lv.pix_off[l] = int(h), int(w), off
        off += int(h) * int(w)
    lv.pix_off[len(shapes)] = off
    return lv


def pixels_per_image(shapes):
    return sum(int(h) * int(w) for h, w in shapes)


def index_maps(index, N, shapes):
    """The per-level [N,H,W] views of the flat index buffer drc_srpn_active_pixels wrote."""
    out, off = [], 0
    for h, w in shapes:
        out.append(index[N * off: N * (off + h * w)].view(N, h, w))
        off += h * w
    return out


def active_pixels(pos, neg, N, A, shapes, cap, out=None):
    """pos, neg [N * P * A] uint8 -> (row_pix [N*cap] int32, counts [N] int32, index [N*P] int32); `out` reuses these three buffers."""
    P = pixels_per_image(shapes)
    dev = pos.device
    for m in (pos, neg):
        if not m.is_cuda or m.dtype != torch.uint8 or tuple(m.shape) != (N * P * A,):
            raise RuntimeError(f"srpn active_pixels: uint8 CUDA/HIP masks [{N * P * A}] expected; the HIP path has no CPU fallback")
    if out is None:
        out = (torch.empty(N * cap, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
               torch.empty(N * P, dtype=torch.int32, device=dev))
    row_pix, counts, index = out
    lv = level_table(N, A, 1, cap, shapes)
    pos, neg = pos.contiguous(), neg.contiguous()
    st = _lib.lib().drc_srpn_active_pixels(C.byref(lv), E._ptr(pos), E._ptr(neg), E._ptr(row_pix), E._ptr(counts), E._ptr(index), E._stream_ptr(dev))
    _lib.check(st, "drc_srpn_active_pixels")
    return row_pix, counts, index


def gather_rows(row_pix, N, A, Cin, cap, shapes, hidden=None, feats=None, grads=None, g_obj=None, g_box=None):
    """hidden: per level (storage tensor, n_stride) of the blocked [N][4C/16][H][W][16] hidden map -> T [N*cap, 4C];
    feats: (left maps, right maps), dense [N,C,H,W] -> Xcol [2*N*cap, 9C]; grads: (glogits, gbbox) -> G [N*cap, 8A] scaled by the device
    scalars g_obj / g_box (None = 0).  -> (T, Xcol, G), None where not asked for."""
    dev = row_pix.device
    lv = level_table(N, A, Cin, cap, shapes)
    keep = []
    R = N * cap
    T = Xcol = G = None
    if hidden is not None:
        if (2 * Cin) % 16:
            raise NotImplementedError("srpn gather_rows: a view's 2C hidden channels must fill whole blocks of 16")
        for l, (st_, ns) in enumerate(hidden):
            lv.hidden[l], lv.hidden_n_stride[l] = st_.data_ptr(), int(ns)
        T = torch.empty(R, 4 * Cin, dtype=torch.float32, device=dev)
    if feats is not None:
        for l, (fl, fr) in enumerate(zip(*feats)):
            fl, fr = fl.detach().contiguous(), fr.detach().contiguous()
            if tuple(fl.shape) != (N, Cin) + tuple(shapes[l]) or fr.shape != fl.shape:
                raise RuntimeError(f"srpn gather_rows: feature maps [{N},{Cin},H,W] of the pyramid's shapes expected, got {tuple(fl.shape)}, {tuple(fr.shape)}")
            keep += [fl, fr]
            lv.left[l], lv.right[l] = fl.data_ptr(), fr.data_ptr()
        Xcol = torch.empty(2 * R, 9 * Cin, dtype=torch.float32, device=dev)
    if grads is not None:
        for l, (gz, gb) in enumerate(zip(*grads)):
            if tuple(gz.shape) != (N, 2 * A) + tuple(shapes[l]) or tuple(gb.shape) != (N, 6 * A) + tuple(shapes[l]) or not (gz.is_contiguous() and gb.is_contiguous()):
                raise RuntimeError("srpn gather_rows: contiguous gradient maps [N,2A,H,W] / [N,6A,H,W] expected")
            lv.glogits[l], lv.gbbox[l] = gz.data_ptr(), gb.data_ptr()
        G = torch.empty(R, 8 * A, dtype=torch.float32, device=dev)
    st = _lib.lib().drc_srpn_gather_rows(C.byref(lv), E._ptr(row_pix), E._ptr(g_obj), E._ptr(g_box), E._ptr(T), E._ptr(Xcol), E._ptr(G), E._stream_ptr(dev))
    _lib.check(st, "drc_srpn_gather_rows")
    return T, Xcol, G


def col2im(dxcol, index, N, A, Cin, cap, shapes, want_left=True, want_right=True):
    """dXcol [2*N*cap, 9C] + the index maps -> (per level dleft [N,C,H,W], per level dright), every element written; a view not asked
    for is None."""
    dev = index.device
    lv = level_table(N, A, Cin, cap, shapes)
    mk = lambda: [torch.empty(N, Cin, h, w, dtype=torch.float32, device=dev) for h, w in shapes]
    dl, dr = (mk() if want_left else None), (mk() if want_right else None)
    for l in range(len(shapes)):
        lv.left[l] = dl[l].data_ptr() if want_left else None
        lv.right[l] = dr[l].data_ptr() if want_right else None
    mask = (1 if want_left else 0) | (2 if want_right else 0)
    if mask:
        st = _lib.lib().drc_srpn_col2im(C.byref(lv), E._ptr(dxcol), E._ptr(index), mask, E._stream_ptr(dev))
        _lib.check(st, "drc_srpn_col2im")
    return dl, dr


class _SRPNHeadLoss(Function):
    """(loss_objectness, loss_rpn_box_reg) of the head at (features, parameters), given the raw maps and the hidden maps of THIS forward
    (computed under no_grad by StereoRPN.head_train) and the sample.  aux: dict(hidden=[(storage, n_stride)], cap, beta, shapes)."""

    @staticmethod
    def forward(ctx, aux, pos, neg, reg_targets, counts, w_conv, b_conv, w_cls, b_cls, w_box, b_box, *maps):
        L = len(aux["shapes"])
        left, right, logits, bbox = maps[:L], maps[L:2 * L], maps[2 * L:3 * L], maps[3 * L:]
        logits, bbox = [m.contiguous() for m in logits], [m.contiguous() for m in bbox]
        N, A, Cin, cap, shapes = logits[0].shape[0], logits[0].shape[1] // 2, w_conv.shape[1], aux["cap"], aux["shapes"]
        terms, glogits, gbbox = D.srpn_loss_launch(pos, neg, reg_targets, counts, aux["beta"], logits, bbox)
        row_pix, _, index = active_pixels(pos, neg, N, A, shapes, cap)
        T, Xcol, _ = gather_rows(row_pix, N, A, Cin, cap, shapes, hidden=aux["hidden"], feats=(left, right))
        ctx.save_for_backward(T, Xcol, row_pix, index, w_conv, w_cls, w_box, *glogits, *gbbox)
        ctx.geo = (N, A, Cin, cap, shapes)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms)
        return terms[0], terms[1], terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_obj, g_box, _g_terms):
        N, A, Cin, cap, shapes = ctx.geo
        L = len(shapes)
        T, Xcol, row_pix, index, w_conv, w_cls, w_box = ctx.saved_tensors[:7]
        glogits, gbbox = ctx.saved_tensors[7:7 + L], ctx.saved_tensors[7 + L:]
        dev = T.device
        R, C2, C4, C9 = N * cap, 2 * Cin, 4 * Cin, 9 * Cin
        scal = lambda g: None if g is None else g.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        g_obj, g_box = scal(g_obj), scal(g_box)
        _, _, G = gather_rows(row_pix, N, A, Cin, cap, shapes, grads=(glogits, gbbox), g_obj=g_obj, g_box=g_box)
        need = ctx.needs_input_grad
        need_feat_l, need_feat_r = any(need[11:11 + L]), any(need[11 + L:11 + 2 * L])
        wpred = torch.cat((w_cls.detach().reshape(2 * A, C4), w_box.detach().reshape(6 * A, C4)), 0).float().contiguous()
        _, db_pred = act_bwd_rows(G, None, None, 0.0, False)                                  # column sums of G (fp64, fixed order)
        gp = _pack_rows(G)
        dT = _gemm_packed(gp, _pack_cols(wpred), None, R, C4, 8 * A, False, dev)              # dT = G . Wpred
        dwpred = _gemm_packed(_pack_cols(G), _pack_cols(T), None, 8 * A, C4, R, False, dev)   # dWpred = G^T . T
        dZ, _ = act_bwd_rows(dT, T, None, 0.0, True, want_db=False)                           # dZ = dT . [T > 0]
        dZ2 = torch.cat((dZ[:, :C2], dZ[:, C2:]), 0).contiguous()                             # [2R, 2C]: left rows, then right rows
        _, db_conv = act_bwd_rows(dZ2, None, None, 0.0, False)                                # both views in one fixed-order fp64 sum
        dwconv = _gemm_packed(_pack_cols(dZ2), _pack_cols(Xcol), None, C2, C9, 2 * R, False, dev)     # dWconv = dZ2^T . Xcol
        dleft = dright = None
        if need_feat_l or need_feat_r:
            w2 = w_conv.detach().reshape(C2, C9).float().contiguous()
            dxcol = _gemm_packed(_pack_rows(dZ2), _pack_cols(w2), None, 2 * R, C9, C2, False, dev)    # dXcol = dZ2 . Wconv
            dleft, dright = col2im(dxcol, index, N, A, Cin, cap, shapes, need_feat_l, need_feat_r)
        none = [None] * L
        return (None, None, None, None, None, dwconv.view(w_conv.shape), db_conv, dwpred[:2 * A].reshape(w_cls.shape), db_pred[:2 * A],
                dwpred[2 * A:].reshape(w_box.shape), db_pred[2 * A:]) + tuple(dleft or none) + tuple(dright or none) + tuple(none) * 2


def srpn_head_loss(left_features, right_features, head, pos, neg, reg_targets, counts, logits, regs, hidden, cap, beta=1.0 / 9):
    """-> (loss_objectness, loss_rpn_box_reg), differentiable in the six parameters of `head` (SRPNHead) and in the feature maps.
    logits / regs: the RAW maps of this forward; hidden: per level the engine's blocked 4C-channel hidden map (halo 0)."""
    what = "srpn_head_loss"
    L = len(logits)
    N, A = logits[0].shape[0], logits[0].shape[1] // 2
    shapes = [tuple(int(v) for v in z.shape[2:]) for z in logits]
    total = pixels_per_image(shapes) * A
    for f in list(left_features) + list(right_features) + list(logits) + list(regs):
        E.require_gpu(f, what)
    if not (len(left_features) == len(right_features) == len(regs) == len(hidden) == L):
        raise RuntimeError(f"{what}: {L} levels of feature maps, raw maps and hidden maps expected")
    cap = int(cap)
    if cap < 1:
        raise ValueError(f"{what}: BATCH_SIZE_PER_IMAGE >= 1 expected, got {cap}")
    pos = D._dev(pos, what + " pos_mask", torch.uint8, (N * total,))
    neg = D._dev(neg, what + " neg_mask", torch.uint8, (N * total,))
    reg_targets = D._dev(reg_targets, what + " reg_targets", torch.float32, (N * total, 6))
    counts = D._dev(counts, what + " counts", torch.int32, (N, 2))
    hid = []
    for t, (h, w) in zip(hidden, shapes):
        if (t.N, t.C, t.D, t.H, t.W, t.pd, t.ph, t.pw) != (N, 4 * head.conv.in_channels, 1, h, w, 0, 0, 0):
            raise RuntimeError(f"{what}: the hidden map of a level does not have the head's geometry")
        hid.append((t.storage, t.n_stride))
    aux = dict(hidden=hid, cap=cap, beta=float(beta), shapes=shapes)
    lo, lb, _ = _SRPNHeadLoss.apply(aux, pos, neg, reg_targets, counts, head.conv.weight, head.conv.bias, head.cls_logits.weight,
                                    head.cls_logits.bias, head.bbox_pred.weight, head.bbox_pred.bias, *left_features, *right_features, *logits, *regs)
    return lo, lb

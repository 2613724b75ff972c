"""CPU restatement of the FPN's training step (reference: disprcnn/modeling/backbone/fpn.py:44-82 under torch autograd).

Two parts:
  * the bilinear resize (align_corners=False, upscaling) with its index and weight arithmetic in fp32 EXACTLY as the HIP kernels compute
    them (volume_ops.hip bilinear_up_blocked_kernel / fpn_train.hip) and every sum in fp64: forward, adjoint, and the per-element
    sum |w| * |g| that the adjoint's error bound is stated in;
  * the fork's FPN forward in torch on the CPU (any dtype; fp64 is the oracle, fp32 the yardstick of the tolerance rule), with
    gradients by autograd: F.conv2d, F.interpolate(size=..., mode='bilinear', align_corners=False), F.max_pool2d(x, 1, 2, 0), and the
    fork's `last_inner = layer_block(lateral + top_down)`; the top level is returned without its 3x3 block.
"""
import numpy as np
import torch
import torch.nn.functional as F

_f = np.float32


def axis_terms(I, O):
    """Per output position o: (i0, i1, w0, w1) with the forward's fp32 arithmetic: f = max(s * (o + 0.5) - 0.5, 0), s = I / O in fp32."""
    s = _f(I) / _f(O)
    o = np.arange(O, dtype=np.float32)
    f = np.maximum(s * (o + _f(0.5)) - _f(0.5), _f(0.0)).astype(np.float32)
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < I - 1)
    t = (f - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (_f(1.0) - t).astype(np.float32), t


def resize_matrix(IH, IW, OH, OW):
    """M [OH*OW, IH*IW] in fp64: entry = sum of the fp32 corner coefficients (h * w rounded to fp32, as the adjoint kernel forms them) with
    which output (oy, ox) reads input (iy, ix); a clamped neighbour contributes both of its corners to the same pixel."""
    y0, y1, h0, h1 = axis_terms(IH, OH)
    x0, x1, w0, w1 = axis_terms(IW, OW)
    M = np.zeros((OH * OW, IH * IW), dtype=np.float64)
    for oy in range(OH):
        for ox in range(OW):
            r = oy * OW + ox
            for yy, hh in ((y0[oy], h0[oy]), (y1[oy], h1[oy])):
                for xx, ww in ((x0[ox], w0[ox]), (x1[ox], w1[ox])):
                    M[r, yy * IW + xx] += np.float64(_f(hh * ww))
    return M


def resize_fwd(x, OH, OW):
    """x [N, C, IH, IW] -> fp64 [N, C, OH, OW]"""
    x = np.asarray(x, dtype=np.float64)
    N, C, IH, IW = x.shape
    M = resize_matrix(IH, IW, OH, OW)
    return (x.reshape(N * C, IH * IW) @ M.T).reshape(N, C, OH, OW)


def resize_bwd(g, IH, IW, gsub=None, old=None):
    """(resize^T(g) [+ subsample^T(gsub)] [+ old], the sum of |term| per element), both fp64 [N, C, IH, IW]; g [N, C, OH, OW] or None."""
    ref = np.zeros((0,))
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        N, C, OH, OW = g.shape
        M = resize_matrix(IH, IW, OH, OW)
        out = (g.reshape(N * C, OH * OW) @ M).reshape(N, C, IH, IW)
        mag = (np.abs(g).reshape(N * C, OH * OW) @ np.abs(M)).reshape(N, C, IH, IW)
    else:
        ref = np.asarray(gsub if gsub is not None else old)
        N, C = ref.shape[:2]
        out, mag = np.zeros((N, C, IH, IW)), np.zeros((N, C, IH, IW))
    if gsub is not None:
        gsub = np.asarray(gsub, dtype=np.float64)
        out[:, :, ::2, ::2] += gsub
        mag[:, :, ::2, ::2] += np.abs(gsub)
    if old is not None:
        old = np.asarray(old, dtype=np.float64)
        out, mag = out + old, mag + np.abs(old)
    return out, mag


PARAM_NAMES = tuple(f"fpn_{kind}{i}.{leaf}" for i in range(1, 5) for kind in ("inner", "layer") for leaf in ("weight", "bias"))


def fpn_forward(features, params):
    """The fork's FPN on torch CPU tensors: features (C2..C5), params {name: tensor} -> (P2, P3, P4, P5, P6)."""
    conv = lambda x, name, pad: F.conv2d(x, params[name + ".weight"], params[name + ".bias"], padding=pad)
    last = conv(features[3], "fpn_inner4", 0)
    results = [last]                                                    # (fpn.py:54-55: the top level skips fpn_layer4)
    for i in (3, 2, 1):
        lateral = conv(features[i - 1], f"fpn_inner{i}", 0)
        top_down = F.interpolate(last, size=lateral.shape[-2:], mode="bilinear", align_corners=False)
        last = conv(lateral + top_down, f"fpn_layer{i}", 1)             # the fork's last_inner = layer_block(...)
        results.insert(0, last)
    results.append(F.max_pool2d(results[-1], 1, 2, 0))
    return tuple(results)


def fpn_step(features, params, gouts, dtype, feature_grads=True):
    """Forward + autograd backward on the CPU in `dtype`.  -> (outputs, {param name: grad or None}, [C-map grads] or None)"""
    feats = [f.detach().cpu().to(dtype).requires_grad_(feature_grads) for f in features]
    ps = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params.items()}
    outs = fpn_forward(feats, ps)
    leaves = [ps[k] for k in PARAM_NAMES] + (feats if feature_grads else [])
    grads = torch.autograd.grad(outs, leaves, [g.detach().cpu().to(dtype) for g in gouts], allow_unused=True)
    pg = dict(zip(PARAM_NAMES, grads[:16]))
    return [o.detach() for o in outs], pg, (list(grads[16:]) if feature_grads else None)


def rel_err(x, ref):
    """max|x - ref| / max|ref| in fp64"""
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    return float((x - ref).abs().max() / ref.abs().max().clamp_min(1e-300))

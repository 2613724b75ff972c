"""Shared MLPs of PointNet++'s SA / FP modules on the fp32-MFMA kernels of libdisprcnn_pts.so (pts/pn2_mlp.hip).

    sa_mlp_max(xyz, new_xyz, feats, idx, layers, out=None, c_off=0)      group -> MLP -> max over the neighbourhood, one kernel
    pointwise_mlp(in0, in1, weight, bias, relu, out=None, c_off=0)       act(W . concat(in0, in1) + b), the concat never built

A layer is a pair (W [Cout,Cin], b [Cout]) with BatchNorm already folded in (`fold_bn`), or a `Packed` pair made once by `pack`: the
kernels read weights K-major, so a raw pair is transposed on the device at every call and a packed one is not.  GPU tensors, fp32,
no autograd; there is no torch fallback.  `sa_mlp_max_unfused` is the same arithmetic done the long way
(grouping_operation -> conv2d -> max) for tools/bench_rpn.py and the tests to compare against; the modules never call it.

Training forms (autograd, on the backward kernels of pts/pn2_mlp_bwd.hip and the BatchNorm kernels of pts/pn2_bn.hip):

    pointwise_mlp_train(in0, in1, weight, bias, relu)        one layer; gradients for in0, in1, weight (its own shape) and bias
    bn_act_train(y, bn_weight, bn_bias, running_mean, running_var, momentum, eps, relu)
                                                             act(BatchNorm(y)) on the statistics of the batch, running statistics updated
    pointwise_bn_train(in0, in1, weight, bn, relu)           conv without bias -> bn_act_train with the nn.BatchNorm module `bn`
    group_max(x)                                             (B,C,M,ns) -> (B,C,M), the max over ns; ties go to the lowest sample
    sa_mlp_max_train(xyz, new_xyz, feats, idx, layers)       group -> subtract the centre -> layers -> group_max, all in HBM

A training layer is (weight, bias), or (weight, None, bn) with an nn.BatchNorm1d / 2d module after a conv without bias.  The weight
gradient is summed in fp32 within a chunk of `WGRAD_CHUNK` columns and in fp64 across chunks, in chunk order; the BatchNorm sums are fp64
throughout, per chunk of `BN_CHUNK` columns and then across chunks in chunk order: bit-identical run to run, and the bits depend on the
chunk lengths.
"""
import torch
import torch.nn.functional as F

from .. import engine as E
from ..pts import _lib

WGRAD_CHUNK = 2048          # pts/pn2_mlp_bwd.hip:kWgradChunk (checked against the library when it is first used)
BN_CHUNK = 4096             # pts/pn2_bn.hip:kBnChunk (likewise)


class Packed:
    """One layer as the kernels read it: wt [Cin,Cout] (K-major), bias [Cout]."""

    __slots__ = ("wt", "bias", "cin", "cout")

    def __init__(self, wt, bias):
        self.wt, self.bias = wt, bias
        self.cin, self.cout = int(wt.shape[0]), int(wt.shape[1])


def pack(weight, bias):
    """(W [Cout,Cin] or [Cout,Cin,1(,1)], b [Cout]) on the GPU -> Packed."""
    w = weight.reshape(weight.shape[0], -1)
    E.require_gpu(w, "pn2_mlp.pack")
    E.require_gpu(bias, "pn2_mlp.pack")
    if bias.shape != (w.shape[0],):
        raise RuntimeError(f"pn2_mlp.pack: bias must be [{w.shape[0]}], got {tuple(bias.shape)}")
    return Packed(w.detach().t().contiguous(), bias.detach().contiguous())


def fold_bn(weight, bias, bn_weight, bn_bias, running_mean, running_var, eps):
    """Fold an eval-mode BatchNorm into the 1x1 conv before it, in fp64 on the host, rounded once to fp32:
    W' = W * g / sqrt(var + eps), b' = beta + (b - mean) * g / sqrt(var + eps)  (b = 0 when the conv has no bias).
    -> (W' [Cout,Cin], b' [Cout]) fp32 CPU tensors."""
    w = weight.detach().to("cpu", torch.float64).reshape(weight.shape[0], -1)
    b = bias.detach().to("cpu", torch.float64) if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    scale = bn_weight.detach().to("cpu", torch.float64) / torch.sqrt(running_var.detach().to("cpu", torch.float64) + eps)
    w = w * scale.unsqueeze(1)
    b = bn_bias.detach().to("cpu", torch.float64) + (b - running_mean.detach().to("cpu", torch.float64)) * scale
    return w.float(), b.float()


def _packed(layer):
    return layer if isinstance(layer, Packed) else pack(layer[0], layer[1])


def _out(out, shape, c_off, cout, dev, what):
    B, _, L = shape
    if out is None:
        if c_off != 0:
            raise RuntimeError(f"{what}: a channel offset needs the out buffer it points into")
        return torch.empty((B, cout, L), dtype=torch.float32, device=dev)
    E.require_gpu(out, what)
    if out.dim() != 3 or out.shape[0] != B or out.shape[2] != L or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be a contiguous [{B}, C_total, {L}] tensor, got {tuple(out.shape)}")
    if c_off < 0 or c_off + cout > out.shape[1]:
        raise RuntimeError(f"{what}: channels [{c_off}, {c_off + cout}) do not fit out's {out.shape[1]}")
    return out


def sa_mlp_max(xyz, new_xyz, feats, idx, layers, out=None, c_off=0):
    """xyz (B,N,3), new_xyz (B,M,3), feats (B,C,N) or None, idx (B,M,ns) int32 from ball_query, layers: 1..3 of (W, b) / Packed.
    -> out[b, c_off + c, m] = max_s MLP(concat(xyz[idx] - new_xyz, feats[:, idx]))[c], ReLU after every layer; out (B,C_total,M) is
    allocated (C_total = the last width) unless given.  The input channel order is QueryAndGroup's with use_xyz."""
    what = "sa_mlp_max"
    E.require_gpu(xyz, what)
    E.require_gpu(new_xyz, what)
    if xyz.dim() != 3 or xyz.shape[2] != 3 or new_xyz.dim() != 3 or new_xyz.shape[2] != 3 or new_xyz.shape[0] != xyz.shape[0]:
        raise RuntimeError(f"{what}: xyz [B,N,3] and new_xyz [B,M,3] expected, got {tuple(xyz.shape)} and {tuple(new_xyz.shape)}")
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    C = 0
    if feats is not None:
        E.require_gpu(feats, what)
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[2] != N:
            raise RuntimeError(f"{what}: feats must be [{B},C,{N}], got {tuple(feats.shape)}")
        C = feats.shape[1]
        feats = feats.contiguous() if C else None
    if not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 3 or idx.shape[:2] != (B, M):
        raise RuntimeError(f"{what}: idx must be an int32 GPU tensor [{B},{M},ns], got {idx.dtype} {tuple(idx.shape)}")
    ns = idx.shape[2]
    if not 1 <= ns <= 64:
        raise RuntimeError(f"{what}: nsample must be in 1..64, got {ns}")
    ls = [_packed(l) for l in layers]
    if not 1 <= len(ls) <= 3:
        raise RuntimeError(f"{what}: 1 to 3 layers, got {len(ls)}")
    cin = C + 3
    for i, l in enumerate(ls):
        if l.cin != cin:
            raise RuntimeError(f"{what}: layer {i} takes {l.cin} channels, its input has {cin}")
        cin = l.cout
    out = _out(out, (B, cin, M), c_off, cin, xyz.device, what)
    if B == 0 or M == 0:
        return out
    args = []
    for i in range(3):
        args += [E._ptr(ls[i].wt), E._ptr(ls[i].bias), ls[i].cout] if i < len(ls) else [E._ptr(None), E._ptr(None), 0]
    st = _lib.lib().drc_pn2_sa_mlp_max_fwd(B, N, M, C, ns, E._ptr(xyz.contiguous()), E._ptr(new_xyz.contiguous()), E._ptr(feats),
                                           E._ptr(idx.contiguous()), len(ls), *args, E._ptr(out), out.shape[1], c_off,
                                           E._stream_ptr(xyz.device))
    _lib.check(st, "drc_pn2_sa_mlp_max_fwd")
    return out


def pointwise_mlp(in0, in1, weight, bias, relu, out=None, c_off=0):
    """in0 (B,C0,N), in1 (B,C1,N) or None, weight [Cout,C0+C1] (or a Packed, bias then ignored), bias [Cout]
    -> out[b, c_off + c, n] = act(W . concat(in0, in1) + b), act = ReLU when `relu` else identity."""
    what = "pointwise_mlp"
    E.require_gpu(in0, what)
    if in0.dim() != 3:
        raise RuntimeError(f"{what}: in0 must be [B,C0,N], got {tuple(in0.shape)}")
    B, C0, N = in0.shape
    C1 = 0
    if in1 is not None:
        E.require_gpu(in1, what)
        if in1.dim() != 3 or in1.shape[0] != B or in1.shape[2] != N:
            raise RuntimeError(f"{what}: in1 must be [{B},C1,{N}], got {tuple(in1.shape)}")
        C1 = in1.shape[1]
        in1 = in1.contiguous() if C1 else None
    l = weight if isinstance(weight, Packed) else pack(weight, bias)
    if l.cin != C0 + C1 or C0 < 1:
        raise RuntimeError(f"{what}: the layer takes {l.cin} channels, the inputs have {C0} + {C1}")
    out = _out(out, (B, l.cout, N), c_off, l.cout, in0.device, what)
    if B == 0 or N == 0:
        return out
    st = _lib.lib().drc_pn2_pointwise_mlp_fwd(B, N, C0, C1, E._ptr(in0.contiguous()), E._ptr(in1), E._ptr(l.wt), E._ptr(l.bias), l.cout,
                                              1 if relu else 0, E._ptr(out), out.shape[1], c_off, E._stream_ptr(in0.device))
    _lib.check(st, "drc_pn2_pointwise_mlp_fwd")
    return out


def sa_mlp_max_unfused(xyz, new_xyz, feats, idx, layers):
    """The same result the materialising way: grouping_operation -> (B,C+3,M,ns) -> conv2d + ReLU per layer -> max.  For comparison
    (tools/bench_rpn.py, tests) only."""
    from .pointnet2 import grouping_operation
    g = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
    if feats is not None and feats.shape[1]:
        g = torch.cat([g, grouping_operation(feats.contiguous(), idx)], dim=1)
    for l in layers:
        w, b = (l.wt.t(), l.bias) if isinstance(l, Packed) else (l[0].reshape(l[0].shape[0], -1), l[1])
        g = F.relu(F.conv2d(g, w.reshape(w.shape[0], w.shape[1], 1, 1).contiguous(), b))
    return g.max(dim=3)[0]


# ---- training forms
def _check_chunk():
    got = _lib.lib().drc_pn2_wgrad_chunk()
    if got != WGRAD_CHUNK:
        raise RuntimeError(f"pn2_mlp: the library was built with a weight-gradient chunk of {got}, this module expects {WGRAD_CHUNK}")


def _dgrad(gout, out, w2, C0, C1, relu):
    B, cout, N = gout.shape
    gin = torch.empty((B, C0 + C1, N), dtype=torch.float32, device=gout.device)
    st = _lib.lib().drc_pn2_pointwise_mlp_dgrad(B, N, C0, C1, cout, 1 if relu else 0, E._ptr(gout), E._ptr(out if relu else None), E._ptr(w2),
                                                E._ptr(gin), E._stream_ptr(gout.device))
    _lib.check(st, "drc_pn2_pointwise_mlp_dgrad")
    return gin


def _wgrad(gout, out, in0, in1, relu, want_w, want_b):
    _check_chunk()
    B, cout, N = gout.shape
    C0, C1 = in0.shape[1], in1.shape[1] if in1 is not None else 0
    n_ws = _lib.lib().drc_pn2_wgrad_workspace_floats(B, N, C0, C1, cout)
    if n_ws < 0:
        raise RuntimeError(f"drc_pn2_wgrad_workspace_floats failed: status {n_ws}")
    ws = torch.empty(n_ws, dtype=torch.float32, device=gout.device)
    gw = torch.empty((cout, C0 + C1), dtype=torch.float32, device=gout.device) if want_w else None
    gb = torch.empty(cout, dtype=torch.float32, device=gout.device) if want_b else None
    st = _lib.lib().drc_pn2_pointwise_mlp_wgrad(B, N, C0, C1, cout, 1 if relu else 0, E._ptr(gout), E._ptr(out if relu else None), E._ptr(in0),
                                                E._ptr(in1), E._ptr(ws), E._ptr(gw), E._ptr(gb), E._stream_ptr(gout.device))
    _lib.check(st, "drc_pn2_pointwise_mlp_wgrad")
    return gw, gb


class _PointwiseMlpTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1, weight, bias, relu):
        out = pointwise_mlp(in0, in1, weight, bias, relu)
        ctx.relu = bool(relu)
        ctx.save_for_backward(in0, in1, weight, out)
        return out

    @staticmethod
    def backward(ctx, gout):
        in0, in1, weight, out = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, C0, N = in0.shape
        C1 = in1.shape[1] if in1 is not None else 0
        cout = weight.shape[0]
        g0 = g1 = gw = gb = None
        if B == 0 or N == 0:
            g0 = torch.zeros_like(in0) if need[0] else None
            g1 = torch.zeros_like(in1) if need[1] and in1 is not None else None
            gw = torch.zeros_like(weight) if need[2] else None
            gb = weight.new_zeros(cout) if need[3] else None
            return g0, g1, gw, gb, None
        E.require_gpu(gout, "pointwise_mlp_train (backward)")
        gout = gout.contiguous()
        in0c = in0.contiguous()
        in1c = in1.contiguous() if C1 else None
        if need[0] or (need[1] and C1):
            gin = _dgrad(gout, out, weight.detach().reshape(cout, -1).contiguous(), C0, C1, ctx.relu)
            if need[0]:
                g0 = gin[:, :C0]
            if need[1] and in1 is not None:
                g1 = gin[:, C0:]
        elif need[1] and in1 is not None:
            g1 = torch.zeros_like(in1)
        if need[2] or need[3]:
            gw, gb = _wgrad(gout, out, in0c, in1c, ctx.relu, need[2], need[3])
            if gw is not None:
                gw = gw.reshape(weight.shape)
        return g0, g1, gw, gb, None


def pointwise_mlp_train(in0, in1, weight, bias, relu):
    """pointwise_mlp with autograd: in0 (B,C0,N), in1 (B,C1,N) or None, weight [Cout,C0+C1] / [Cout,Cin,1] / [Cout,Cin,1,1], bias [Cout]
    -> act(W . concat(in0, in1) + b) (B,Cout,N).  The backward gives gradients for in0, in1, weight (in weight's shape) and bias, each only
    when it is needed."""
    what = "pointwise_mlp_train"
    E.require_gpu(in0, what)
    if in1 is not None:
        E.require_gpu(in1, what)
        if in1.dim() == 3 and in1.shape[1] == 0:
            in1 = None
    if isinstance(weight, Packed):
        raise RuntimeError(f"{what}: takes the raw conv weight, not a Packed")
    E.require_gpu(weight, what)
    if bias is None:
        raise RuntimeError(f"{what}: the layer needs a bias")
    E.require_gpu(bias, what)
    return _PointwiseMlpTrain.apply(in0, in1, weight, bias, bool(relu))


# ---- BatchNorm on the statistics of the batch
def _bn_workspace(B, C, N, dev):
    got = _lib.lib().drc_pn2_bn_chunk()
    if got != BN_CHUNK:
        raise RuntimeError(f"pn2_mlp: the library was built with a BatchNorm chunk of {got}, this module expects {BN_CHUNK}")
    n_ws = _lib.lib().drc_pn2_bn_workspace_doubles(B, C, N)
    if n_ws < 0:
        raise RuntimeError(f"drc_pn2_bn_workspace_doubles failed: status {n_ws}")
    return torch.empty(n_ws, dtype=torch.float64, device=dev)


class _BnActTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bn_weight, bn_bias, running_mean, running_var, momentum, eps, relu):
        B, C, N = y.shape
        dev = y.device
        y = y.contiguous()
        stats = torch.empty((2, C), dtype=torch.float32, device=dev)
        z = torch.empty_like(y)
        st = _lib.lib().drc_pn2_bn_stats(B, C, N, E._ptr(y), E._ptr(_bn_workspace(B, C, N, dev)), eps, momentum, E._ptr(stats),
                                         E._ptr(running_mean), E._ptr(running_var), E._stream_ptr(dev))
        _lib.check(st, "drc_pn2_bn_stats")
        st = _lib.lib().drc_pn2_bn_apply_fwd(B, C, N, 1 if relu else 0, E._ptr(y), E._ptr(stats), E._ptr(bn_weight), E._ptr(bn_bias),
                                             E._ptr(z), E._stream_ptr(dev))
        _lib.check(st, "drc_pn2_bn_apply_fwd")
        ctx.relu = bool(relu)
        ctx.save_for_backward(y, z, stats, bn_weight)
        ctx.mark_non_differentiable(stats)
        return z, stats

    @staticmethod
    def backward(ctx, gz, _gstats):
        y, z, stats, bn_weight = ctx.saved_tensors
        B, C, N = y.shape
        dev = y.device
        E.require_gpu(gz, "bn_act_train (backward)")
        gz = gz.contiguous()
        gy = torch.empty_like(y)
        gg = torch.empty(C, dtype=torch.float32, device=dev)
        gb = torch.empty(C, dtype=torch.float32, device=dev)
        st = _lib.lib().drc_pn2_bn_bwd(B, C, N, 1 if ctx.relu else 0, E._ptr(gz), E._ptr(z), E._ptr(y), E._ptr(stats), E._ptr(bn_weight),
                                       E._ptr(_bn_workspace(B, C, N, dev)), E._ptr(gy), E._ptr(gg), E._ptr(gb), E._stream_ptr(dev))
        _lib.check(st, "drc_pn2_bn_bwd")
        return gy, gg, gb, None, None, None, None, None


def bn_act_train(y, bn_weight, bn_bias, running_mean, running_var, momentum, eps, relu, return_stats=False):
    """torch.nn.BatchNorm1d / 2d in training mode, then ReLU when `relu`, with autograd: y (B,C,N), bn_weight / bn_bias [C] ->
    z = act(bn_weight * (y - mean) / sqrt(var + eps) + bn_bias) with the mean and the biased variance of each channel over its B * N
    values.  running_mean / running_var [C] (both None, or both given) are updated in place, r <- (1 - momentum) r + momentum * (mean |
    var * n / (n - 1)); through raw pointers, so their `_version` does not move.  Gradients go to y, bn_weight and bn_bias.
    return_stats: -> (z, stats [2,C]: mean, 1 / sqrt(var + eps))."""
    what = "bn_act_train"
    E.require_gpu(y, what)
    if y.dim() != 3:
        raise RuntimeError(f"{what}: y must be [B,C,N], got {tuple(y.shape)}")
    B, C, N = y.shape
    for name, t in (("bn_weight", bn_weight), ("bn_bias", bn_bias), ("running_mean", running_mean), ("running_var", running_var)):
        if t is None and name.startswith("running"):
            continue
        E.require_gpu(t, what)
        if t.shape != (C,) or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous [{C}] tensor, got {tuple(t.shape)}")
    if (running_mean is None) != (running_var is None):
        raise RuntimeError(f"{what}: running_mean and running_var come together")
    if momentum is None:
        raise NotImplementedError(f"{what}: momentum=None (the cumulative moving average) is not built")
    if C < 1:
        raise RuntimeError(f"{what}: y has no channel")
    if B * N < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
    rm = running_mean.detach() if running_mean is not None else None
    rv = running_var.detach() if running_var is not None else None
    z, stats = _BnActTrain.apply(y, bn_weight, bn_bias, rm, rv, float(momentum), float(eps), bool(relu))
    return (z, stats) if return_stats else z


_zero_bias = {}
_counters = None            # the num_batches_tracked tensors of the open batch_counters() block


def _zeros(cout, dev):
    key = (cout, dev)
    if key not in _zero_bias:
        _zero_bias[key] = torch.zeros(cout, dtype=torch.float32, device=dev)
    return _zero_bias[key]


class batch_counters:
    """with batch_counters(): every pointwise_bn_train inside adds its module's num_batches_tracked with one torch._foreach_add_ at the
    end of the block (one launch per step) instead of one op per layer."""

    def __enter__(self):
        global _counters
        self.outer, _counters = _counters, []
        return self

    def __exit__(self, exc_type, exc, tb):
        global _counters
        mine, _counters = _counters, self.outer
        if exc_type is None and mine:
            if self.outer is not None:
                self.outer.extend(mine)
            else:
                torch._foreach_add_(mine, 1)
        return False


def pointwise_bn_train(in0, in1, weight, bn, relu):
    """One conv -> BatchNorm (-> ReLU) layer in training mode: the conv is pointwise_mlp_train without activation, with a cached zero bias
    that needs no gradient (so no bias gradient is computed); `bn` is the nn.BatchNorm1d / 2d module, whose running statistics and
    num_batches_tracked are updated as its own training forward would."""
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm with momentum=None (the cumulative moving average) is not built on the HIP shared MLPs")
    if not bn.affine:
        raise NotImplementedError("BatchNorm without affine parameters is not built on the HIP shared MLPs")
    E.require_gpu(weight, "pointwise_bn_train")
    y = pointwise_mlp_train(in0, in1, weight, _zeros(weight.shape[0], weight.device), False)
    track = bn.track_running_stats and bn.running_mean is not None
    z = bn_act_train(y, bn.weight, bn.bias, bn.running_mean if track else None, bn.running_var if track else None, bn.momentum, bn.eps,
                     relu)
    if track and bn.num_batches_tracked is not None:
        if _counters is not None:
            _counters.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    return z


def train_layer_apply(in0, in1, layer, relu):
    """One training layer, (weight, bias) or (weight, None, bn), on in0 (B,C0,N) and in1 (B,C1,N) or None."""
    if len(layer) == 3:
        return pointwise_bn_train(in0, in1, layer[0], layer[2], relu)
    return pointwise_mlp_train(in0, in1, layer[0], layer[1], relu)


class _GroupMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, C, M, ns = x.shape
        out = torch.empty((B, C, M), dtype=torch.float32, device=x.device)
        arg = torch.empty((B, C, M), dtype=torch.int32, device=x.device)
        rows = B * C * M
        if rows:
            st = _lib.lib().drc_pn2_group_max_fwd(rows, ns, E._ptr(x), E._ptr(out), E._ptr(arg), E._stream_ptr(x.device))
            _lib.check(st, "drc_pn2_group_max_fwd")
        ctx.ns = ns
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, gout, _garg):
        (arg,) = ctx.saved_tensors
        B, C, M = arg.shape
        gin = torch.empty((B, C, M, ctx.ns), dtype=torch.float32, device=arg.device)
        rows = B * C * M
        if rows:
            E.require_gpu(gout, "group_max (backward)")
            st = _lib.lib().drc_pn2_group_max_bwd(rows, ctx.ns, E._ptr(gout.contiguous()), E._ptr(arg), E._ptr(gin), E._stream_ptr(arg.device))
            _lib.check(st, "drc_pn2_group_max_bwd")
        return gin


def group_max(x, return_arg=False):
    """x (B,C,M,ns), 1 <= ns <= 64 -> the max over ns (B,C,M), with autograd: the whole gradient goes to the winner, the lowest sample
    index among equal maxima.  return_arg: -> (out, arg int32 (B,C,M))."""
    what = "group_max"
    E.require_gpu(x, what)
    if x.dim() != 4 or not 1 <= x.shape[3] <= 64:
        raise RuntimeError(f"{what}: x must be [B,C,M,ns] with ns in 1..64, got {tuple(x.shape)}")
    out, arg = _GroupMax.apply(x.contiguous())
    return (out, arg) if return_arg else out


def sa_mlp_max_train(xyz, new_xyz, feats, idx, layers):
    """The training form of sa_mlp_max, with autograd through feats and the layers' parameters: xyz (B,N,3), new_xyz (B,M,3), feats (B,C,N)
    or None, idx (B,M,ns) int32, layers: 1..3 of (weight, bias) raw parameters or (weight, None, bn) with a BatchNorm module (batch
    statistics over all B * M * ns grouped columns, padded duplicates included), ReLU after every layer -> (B, Cout, M).  The grouped
    tensor and every layer's activation live in HBM: group (grouping_operation) -> subtract the centre -> pointwise_mlp_train over the
    M * ns columns -> group_max.  The coordinates are constants of the graph."""
    from .pointnet2 import grouping_operation
    what = "sa_mlp_max_train"
    E.require_gpu(xyz, what)
    E.require_gpu(new_xyz, what)
    if xyz.dim() != 3 or xyz.shape[2] != 3 or new_xyz.dim() != 3 or new_xyz.shape[2] != 3 or new_xyz.shape[0] != xyz.shape[0]:
        raise RuntimeError(f"{what}: xyz [B,N,3] and new_xyz [B,M,3] expected, got {tuple(xyz.shape)} and {tuple(new_xyz.shape)}")
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    C = 0
    if feats is not None:
        E.require_gpu(feats, what)
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[2] != N:
            raise RuntimeError(f"{what}: feats must be [{B},C,{N}], got {tuple(feats.shape)}")
        C = feats.shape[1]
    if not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 3 or idx.shape[:2] != (B, M):
        raise RuntimeError(f"{what}: idx must be an int32 GPU tensor [{B},{M},ns], got {idx.dtype} {tuple(idx.shape)}")
    ns = idx.shape[2]
    if not 1 <= ns <= 64:
        raise RuntimeError(f"{what}: nsample must be in 1..64, got {ns}")
    layers = list(layers)
    if not 1 <= len(layers) <= 3:
        raise RuntimeError(f"{what}: 1 to 3 layers, got {len(layers)}")
    cin = C + 3
    for i, l in enumerate(layers):
        w = l[0]
        if w.shape[0] < 1 or w.numel() != w.shape[0] * cin:
            raise RuntimeError(f"{what}: layer {i} has weight {tuple(w.shape)}, its input has {cin} channels")
        cin = w.shape[0]
    if B == 0 or M == 0:
        # nothing to launch: a correctly shaped result that still hangs on its inputs, so that backward gives them zero gradients
        out = torch.zeros((B, cin, M), dtype=torch.float32, device=xyz.device)
        for t in [feats] + [p for l in layers for p in (l[:2] if len(l) == 2 else (l[0], l[2].weight, l[2].bias))]:
            if t is not None and t.requires_grad:
                out = out + 0.0 * t.sum()
        return out
    idx = idx.contiguous()
    with torch.no_grad():
        g = grouping_operation(xyz.detach().transpose(1, 2).contiguous(), idx) - new_xyz.detach().transpose(1, 2).unsqueeze(-1)
    if C:
        g = torch.cat([g, grouping_operation(feats.contiguous(), idx)], dim=1)
    x = g.reshape(B, C + 3, M * ns)
    for l in layers:
        x = train_layer_apply(x, None, l, True)
    return group_max(x.reshape(B, cin, M, ns))

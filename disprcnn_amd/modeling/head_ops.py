"""Engine-backed layers of the 2D stage's heads: nn.Conv2d / nn.Linear parameter holders whose arithmetic runs on the HIP engine
(convolutions: the same MFMA kernels as the backbone, bias in the folded-BN epilogue slot) or, for the fully connected layers, on the
hand-written fp32-MFMA GEMM of csrc/linear.hip (round 3; rounds 1-2: torch.addmm -> hipBLASLt).  There is no CPU path.  The training
forms (gemm_bias_act_train / linear_train, ConvReluChainTrain) are autograd Functions whose backward runs on the same kernels plus
csrc/head_train.hip; the eval forms above them are untouched by training."""
from collections import OrderedDict

import torch

from .. import engine as E


class EngineConv2d:
    """y = act(conv2d(x, conv.weight) + conv.bias) on dense [N,C,H,W] tensors.  Packed weights are rebuilt when the parameters
    change (version counters).  Storage is owned ONCE per map geometry (h, w) -- a short LRU: FPN levels, ROI windows -- and sized for a
    capacity bucket of the unit count (engine.bucket_units, like the PSMNet runtime's WorkspacePool): the mask head sees a different
    detection count (0..100) on every image, and a workspace per exact count would allocate and zero-fill two blocked tensors per conv and
    image.  A smaller count runs on prefix views of the same storage (units are outermost, the zero halo is never written);
    launch plans (no memory) are cached per count."""

    MAX_SHAPES = 12
    MAX_PLANS = 32

    def __init__(self, conv, relu):
        if conv.groups != 1 or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] or conv.dilation[0] != conv.dilation[1]:
            raise NotImplementedError("EngineConv2d: square stride / padding / dilation, groups = 1")
        self.conv, self.relu = conv, bool(relu)
        self._ver, self._geo = None, OrderedDict()
        self._wp = self._sc = self._sh = None

    def _weights(self, dev):
        c = self.conv
        ver = (c.weight._version, c.weight.data_ptr(), None if c.bias is None else c.bias._version, dev)
        if ver != self._ver:
            w = c.weight.detach().to(device=dev, dtype=torch.float32)
            cp = E.cout_pad_of(w.shape[0])
            self._wp = E.pack_conv_weight(w)
            self._sc = torch.ones(cp, device=dev)
            self._sh = torch.zeros(cp, device=dev)
            if c.bias is not None:
                self._sh[: w.shape[0]] = c.bias.detach().to(device=dev, dtype=torch.float32)
            self._w32, self._ver = w, ver
            for geo in self._geo.values():
                geo["w16"] = {}
        return self._wp, self._sc, self._sh

    def nbytes(self):
        """HBM held by the cached workspaces (tests: flat over varying unit counts)."""
        return sum(4 * (g["x"].storage.numel() + g["y"].storage.numel()) for g in self._geo.values())

    def __call__(self, x):
        E.require_gpu(x, "EngineConv2d")
        c = self.conv
        n, cin, h, w = x.shape
        k, s, p, d = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
        cout = c.out_channels
        dev = x.device
        oh, ow = (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1
        if n == 0:
            return x.new_zeros(0, cout, oh, ow)
        wp, sc, sh = self._weights(dev)
        key = (h, w, dev)
        halo = max(p, 1)
        geo = self._geo.get(key)
        if geo is None or geo["cap"] < n:
            cap = E.bucket_units(n)
            geo = dict(cap=cap, x=E.Blocked(cap, cin, 1, h, w, 0, halo, halo, dev), y=E.Blocked(cap, cout, 1, oh, ow, 0, 1, 1, dev),
                       plans=OrderedDict(), w16={})
            self._geo[key] = geo
            while len(self._geo) > self.MAX_SHAPES:
                self._geo.popitem(last=False)
        self._geo.move_to_end(key)
        xb = E.Blocked(n, cin, 1, h, w, 0, halo, halo, dev, storage=geo["x"].storage)
        yb = E.Blocked(n, cout, 1, oh, ow, 0, 1, 1, dev, storage=geo["y"].storage)
        plan = geo["plans"].get(n)
        if plan is None:
            plan = geo["plans"][n] = E.plan_conv2d(xb, yb, k, s, p, d, cout, self.relu)
            while len(geo["plans"]) > self.MAX_PLANS:
                geo["plans"].popitem(last=False)
        else:
            geo["plans"].move_to_end(n)
        kind = plan.pack_kind                          # plans of different counts may read different packings (Winograd vs direct)
        if kind not in geo["w16"]:
            geo["w16"][kind] = plan.pack16(self._w32)
        xb.from_dense(x.float())
        plan.run(xb, wp, sc, sh, yb, None, w16=geo["w16"][kind])
        return yb.to_dense()[:, :, 0]


class BlockedConv2d:
    """A convolution of the heads that stays in the engine's blocked layout: y_blocked = act(conv2d(x_blocked) + bias).  The weight is
    the channel-wise (dim 0) concatenation of one or more nn.Conv2d layers of equal geometry -- sibling 1x1 predictors read their
    shared input once -- packed when a parameter's version changes; launch plans are cached per geometry (they hold no memory)."""

    MAX_PLANS = 16

    def __init__(self, convs, relu):
        self.convs = list(convs) if isinstance(convs, (list, tuple)) else [convs]
        c = self.convs[0]
        for o in self.convs:
            if (o.kernel_size, o.stride, o.padding, o.dilation, o.in_channels, o.groups) != \
                    (c.kernel_size, c.stride, c.padding, c.dilation, c.in_channels, 1):
                raise NotImplementedError("BlockedConv2d: sibling layers must share their geometry (groups = 1)")
        self.k, self.stride, self.pad, self.dil = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
        self.cout = sum(o.out_channels for o in self.convs)
        self.relu = bool(relu)
        self._ver, self._plans = None, OrderedDict()

    def _weights(self, dev):
        ver = tuple((o.weight._version, o.weight.data_ptr(), None if o.bias is None else o.bias._version) for o in self.convs) + (dev,)
        if ver != self._ver:
            w = torch.cat([o.weight.detach().to(device=dev, dtype=torch.float32) for o in self.convs], 0)
            cp = E.cout_pad_of(w.shape[0])
            self._wp = E.pack_conv_weight(w)
            self._sc = torch.ones(cp, device=dev)
            self._sh = torch.zeros(cp, device=dev)
            off = 0
            for o in self.convs:
                if o.bias is not None:
                    self._sh[off: off + o.out_channels] = o.bias.detach().to(device=dev, dtype=torch.float32)
                off += o.out_channels
            self._w32, self._ver, self._w16 = w, ver, {}
        return self._wp, self._sc, self._sh

    def out_hw(self, h, w):
        f = lambda n: (n + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        return f(h), f(w)

    def _bridge(self, xb, yb):
        """Large maps of a 3x3 stride-1 layer (the RPN head's 256 -> 512 convolution on P2..P4: 137 GFLOP of the 2D stage's heads) run on the
        split-f16 kernel between the same blocked tensors (engine.BridgedConv2dS16); None where that does not apply."""
        if (self.k, self.stride, self.pad, self.dil) != (3, 1, 1, 1) or type(xb) is not E.Blocked or type(yb) is not E.Blocked:
            return None
        if xb.n_stride != xb.cb * xb.cb_stride or yb.n_stride != yb.cb * yb.cb_stride or (yb.H, yb.W, xb.D, yb.D) != (xb.H, xb.W, 1, 1) or xb.N != yb.N:
            return None
        if not E.BridgedConv2dS16.worth(xb.N, xb.C, self.cout, xb.H, xb.W):
            return None
        if not hasattr(self, "_s16"):
            self._s16 = dict(cache={}, bridges=OrderedDict(), packs=None)
        key = (xb.N, xb.C, xb.H, xb.W)
        br = self._s16["bridges"].get(key)
        if br is None:
            br = self._s16["bridges"][key] = E.BridgedConv2dS16(xb.N, xb.C, self.cout, xb.H, xb.W, self.relu, xb.device, self._s16["cache"])
            while len(self._s16["bridges"]) > self.MAX_PLANS:
                (n_, c_, h_, w_), _ = self._s16["bridges"].popitem(last=False)
                for k in [k for k in self._s16["cache"] if (k[1], k[3], k[4]) == (n_, h_, w_)]:      # its RS16 maps (keyed (tag, N, ch, H, W)) go with it
                    del self._s16["cache"][k]
        return br

    def __call__(self, xb, yb):
        """(The split-f16 bridge reports to the range guard in scope -- the detector's, engine.guarded -- or, called on its own, to a guard
        of this layer: a value beyond +-65504 repeats the call on the fp32 kernel.)"""
        if E.guard_in_scope() is None and xb.device.type == "cuda":
            if getattr(self, "_guard", None) is None:
                self._guard = E.OverflowGuard(xb.device)
            return E.guarded(self._guard, lambda: self._call_once(xb, yb), what="BlockedConv2d (split-f16 3x3 layer)")
        return self._call_once(xb, yb)

    def fp32(self, xb, yb):
        """The same layer on the fp32 kernels only: no split-f16 bridge and no range guard (training: the backward differentiates
        exactly the arithmetic the forward ran)."""
        return self._call_once(xb, yb, bridge=False)

    def _call_once(self, xb, yb, bridge=True):
        wp, sc, sh = self._weights(xb.device)
        br = self._bridge(xb, yb) if bridge else None
        if br is not None:
            from .. import s16 as S
            pk = self._s16["packs"]
            if pk is None or pk[0] is not self._w32 or pk[1] != br.bounds:
                packs = [S.pack_weight_s16(self._w32[:, a:b].contiguous()) for a, b in br.bounds]
                pk = self._s16["packs"] = (self._w32, br.bounds, [(w16, (sc * (2.0 ** -wexp)).contiguous()) for w16, wexp in packs], torch.zeros_like(sh))
            br.run(xb, pk[2], sh, pk[3], yb)
            return yb
        key = (xb.N, xb.C, xb.H, xb.W, xb.ph, xb.pw, xb.n_stride, yb.H, yb.W, yb.ph, yb.pw, yb.n_stride)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = E.plan_conv2d(xb, yb, self.k, self.stride, self.pad, self.dil, self.cout, self.relu)
            while len(self._plans) > self.MAX_PLANS:
                self._plans.popitem(last=False)
        kind = plan.pack_kind
        if kind not in self._w16:
            self._w16[kind] = plan.pack16(self._w32)
        plan.run(xb, wp, sc, sh, yb, None, w16=self._w16[kind])
        return yb


_PACKED_W = {}     # id(parameter) -> (weakref to the parameter, {tag: (version key, packed tensor, 2D shape)}).  The weak reference is the
                   # identity check (ids and allocator addresses are reused once a model is freed) and its callback drops the entry -- and the
                   # packed GPU copies with it -- when the parameter dies; nothing is stored on the parameter, so pickling a model stays lean.


def _packed_cache(prm):
    import weakref
    k = id(prm)
    ent = _PACKED_W.get(k)
    if ent is None or ent[0]() is not prm:
        ent = _PACKED_W[k] = (weakref.ref(prm, lambda _r, k=k: _PACKED_W.pop(k, None)), {})
    return ent[1]


def clear_packed_weights(module):
    """Drop the packed GEMM operands cached for the parameters of `module`.  They are rebuilt on the next call; needed only after an edit
    the version counter cannot see (`param.data.copy_(...)`, `param.data[...] = ...`) -- `load_state_dict`, optimizers and every in-place
    operation on the parameter itself bump `_version` and are picked up automatically."""
    for prm in module.parameters():
        ent = _PACKED_W.get(id(prm))
        if ent is not None and ent[0]() is prm:
            ent[1].clear()


def _pack_rows(a):
    from .. import _lib
    lib = _lib.lib()
    R, K = a.shape
    out = torch.empty(lib.drc_linear_packed_floats(R, K), dtype=torch.float32, device=a.device)
    st = lib.drc_linear_pack_rows(E._ptr(a), R, K, E._ptr(out), E._stream_ptr(a.device))
    _lib.check(st, "drc_linear_pack_rows")
    return out


def gemm_bias_act(x, weight_param, w2d_fn, bias, relu, tag=""):
    """act(x [M,K] @ W^T + bias) with W = w2d_fn(weight_param) [N,K] on drc_linear_fwd.  The packed form of W is cached per
    live parameter object (and tag) and rebuilt when the parameter's version, storage, device or shape changes (see clear_packed_weights)."""
    from .. import _lib
    E.require_gpu(x, "gemm_bias_act")
    dev = x.device
    key = (weight_param._version, weight_param.data_ptr(), dev, tuple(weight_param.shape))
    cache = _packed_cache(weight_param)
    ent = cache.get(tag)
    if ent is None or ent[0] != key:
        w2 = w2d_fn(weight_param.detach().to(device=dev, dtype=torch.float32)).contiguous()
        ent = cache[tag] = (key, _pack_rows(w2), tuple(w2.shape))
    wp, (N, Kw) = ent[1], ent[2]
    x = x.float().contiguous()
    M, K = x.shape
    if Kw != K:
        raise ValueError(f"gemm_bias_act: input has {K} features, the layer expects {Kw}")
    y = torch.empty(M, N, dtype=torch.float32, device=dev)
    if M == 0:
        return y
    b = None if bias is None else bias.detach().to(device=dev, dtype=torch.float32).contiguous()
    lib = _lib.lib()
    xp = _pack_rows(x)
    nscr = lib.drc_linear_scratch_floats(M, N, K)
    scr = E.scratch(dev, "linear", nscr) if nscr else None
    st = lib.drc_linear_fwd(E._ptr(xp), E._ptr(wp), E._ptr(b), E._ptr(y), M, N, K, int(bool(relu)), E._ptr(scr), nscr, E._stream_ptr(dev))
    _lib.check(st, "drc_linear_fwd")
    return y


def linear(x, layer, relu=False):
    """act(x [R, in] @ layer.weight^T + bias) on the hand-written fp32-MFMA GEMM (csrc/linear.hip: drc_linear_fwd); layer is an nn.Linear
    or an nn.Conv2d that acts on a full window (its weight flattened to [out, in], K contiguous).  The weights are packed into the GEMM's
    operand layout once per parameter version, the activations per call.  GPU only."""
    return gemm_bias_act(x, layer.weight, lambda w: w.reshape(w.shape[0], -1), layer.bias, relu)


# ------------------------------------------------------------------------------------------------ training forms
def _pack_cols(a):
    """The packed operand of a^T from row-major a [R, K] (drc_linear_pack_cols): no transposed copy in HBM."""
    from .. import _lib
    lib = _lib.lib()
    R, K = a.shape
    out = torch.empty(lib.drc_linear_packed_floats(K, R), dtype=torch.float32, device=a.device)
    st = lib.drc_linear_pack_cols(E._ptr(a), R, K, E._ptr(out), E._stream_ptr(a.device))
    _lib.check(st, "drc_linear_pack_cols")
    return out


def _gemm_packed(xp, wp, bias, M, N, K, relu, dev):
    """drc_linear_fwd on operands that are packed already: y [M, N]."""
    from .. import _lib
    lib = _lib.lib()
    y = torch.empty(M, N, dtype=torch.float32, device=dev)
    if M == 0 or N == 0:
        return y
    nscr = lib.drc_linear_scratch_floats(M, N, K)
    scr = E.scratch(dev, "linear", nscr) if nscr else None
    st = lib.drc_linear_fwd(E._ptr(xp), E._ptr(wp), E._ptr(bias), E._ptr(y), M, N, K, int(bool(relu)), E._ptr(scr), nscr, E._stream_ptr(dev))
    _lib.check(st, "drc_linear_fwd")
    return y


def _cached_pack(weight_param, w2, tag, pack):
    """pack(w2) cached per live parameter object and tag, rebuilt when the parameter's version, storage, device or shape changes."""
    key = (weight_param._version, weight_param.data_ptr(), w2.device, tuple(weight_param.shape))
    cache = _packed_cache(weight_param)
    ent = cache.get(tag)
    if ent is None or ent[0] != key:
        ent = cache[tag] = (key, pack(w2.detach().to(torch.float32).contiguous()), tuple(w2.shape))
    return ent[1]


def relu_dropout(x, draws, p, relu=True):
    """max(x, 0) . [draws >= (float)p] / (1 - p) in place on row-major x (drc_relu_dropout_fwd); p = 0 ignores draws."""
    from .. import _lib
    st = _lib.lib().drc_relu_dropout_fwd(E._ptr(x), E._ptr(draws) if p > 0 else None, E._ptr(x), x.numel(), float(p), int(bool(relu)),
                                         E._stream_ptr(x.device))
    _lib.check(st, "drc_relu_dropout_fwd")
    return x


def act_bwd_rows(dy, y, draws, p, relu, want_db=True, fold=1):
    """dz = dy . [y > 0] . keep / (1 - p) and db = column sums of dz (fp64, fixed order; `fold` columns per entry) for row-major [M, N]."""
    from .. import _lib
    lib = _lib.lib()
    M, N = dy.shape
    dev = dy.device
    dz = torch.empty_like(dy)
    db = torch.empty(N // fold, dtype=torch.float32, device=dev) if want_db else None
    nd = lib.drc_act_bwd_rows_scratch_doubles(M, N) if want_db else 0
    scr = E.scratch(dev, "act_bwd", 2 * nd) if nd else None           # (float workspace: two floats per double)
    st = lib.drc_act_bwd_rows(E._ptr(dy), E._ptr(y) if relu else None, E._ptr(draws) if p > 0 else None, float(p), int(bool(relu)), M, N, int(fold),
                              E._ptr(dz), E._ptr(db), E._ptr(scr), nd, E._stream_ptr(dev))
    _lib.check(st, "drc_act_bwd_rows")
    return dz, db


def act_bwd_blocked(dy, y, relu, dz, want_db=True):
    """dz = dy . [y > 0] on Blocked tensors of one geometry (2D: D = 1) and the per-channel sums of dz over all units and pixels."""
    from .. import _lib
    lib = _lib.lib()
    for t in (y, dz):
        if (t.N, t.C, t.D, t.H, t.W, t.pd, t.ph, t.pw) != (dy.N, dy.C, dy.D, dy.H, dy.W, dy.pd, dy.ph, dy.pw):
            raise ValueError("act_bwd_blocked: dy, y and dz must share one geometry")
    if dy.D != 1 or dy.pd != 0:
        raise NotImplementedError("act_bwd_blocked: 2D blocked tensors")
    dev = dy.device
    db = torch.empty(dy.cb * 16, dtype=torch.float32, device=dev) if want_db else None
    nd = lib.drc_act_bwd_blocked_scratch_doubles(dy.N, dy.C, dy.H) if want_db else 0
    scr = E.scratch(dev, "act_bwd", 2 * nd) if nd else None
    st = lib.drc_act_bwd_blocked(E._ptr(dy.storage), E._ptr(y.storage), int(bool(relu)), dy.N, dy.C, dy.H, dy.W, dy.ph, dy.pw, E._ptr(dz.storage),
                                 E._ptr(db), E._ptr(scr), nd, E._stream_ptr(dev))
    _lib.check(st, "drc_act_bwd_blocked")
    return dz, (db[: dy.C] if want_db else None)


class _GemmBiasActTrain(torch.autograd.Function):
    """y = dropout_p(act(x @ w2^T + bias)) with its backward on the same GEMM.  w2 [N, K] is a (differentiable) 2D view of the layer's
    weight, `weight_param` the parameter it came from (the key of the packed-operand cache), bias [N / fold] is repeated `fold` times
    along N (the 2x2 transposed convolution's taps).  Saved: x, the OUTPUT y (its sign is the ReLU mask) and the draws."""

    @staticmethod
    def forward(ctx, x, w2, bias, weight_param, tag, relu, p, draws, fold):
        dev = x.device
        N, K = w2.shape
        M = x.shape[0]
        wp = _cached_pack(weight_param, w2, tag, _pack_rows)
        b = None
        if bias is not None:
            b = bias.detach().to(device=dev, dtype=torch.float32)
            b = (b.repeat_interleave(fold) if fold > 1 else b).contiguous()
        y = _gemm_packed(_pack_rows(x), wp, b, M, N, K, relu, dev) if M else torch.empty(0, N, dtype=torch.float32, device=dev)
        if p > 0 and M:
            relu_dropout(y, draws, p, relu)
        ctx.save_for_backward(x, y, draws if p > 0 else None, w2)
        ctx.cfg = (weight_param, tag, bool(relu), float(p), int(fold), bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, draws, w2 = ctx.saved_tensors
        weight_param, tag, relu, p, fold, has_bias = ctx.cfg
        dev = dy.device
        M, K = x.shape
        N = w2.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        if M == 0:
            return (x.new_zeros(0, K) if need_x else None, torch.zeros_like(w2) if need_w else None,
                    torch.zeros(N // fold, dtype=torch.float32, device=dev) if need_b else None, None, None, None, None, None, None)
        dy = dy.float().contiguous()
        if relu or p > 0 or need_b:
            dz, db = act_bwd_rows(dy, y, draws, p, relu, want_db=need_b, fold=fold)
        else:
            dz, db = dy, None
        dx = dw = None
        if need_x:                                             # dX [M, K] = dZ [M, N] . W [N, K]
            wtp = _cached_pack(weight_param, w2, tag + "^T", _pack_cols)
            dx = _gemm_packed(_pack_rows(dz), wtp, None, M, K, N, False, dev)
        if need_w:                                             # dW [N, K] = dZ^T . X, reduction over the M rows
            dw = _gemm_packed(_pack_cols(dz), _pack_cols(x), None, N, K, M, False, dev)
        return dx, dw, db, None, None, None, None, None, None


def gemm_bias_act_train(x, weight_param, w2d_fn, bias, relu, tag="", p=0.0, draws=None, bias_fold=1):
    """The training form of gemm_bias_act: dropout_p(act(x [M,K] @ W^T + bias)) as an autograd Function -- forward on drc_linear_fwd (+
    drc_relu_dropout_fwd where p > 0: element (m, n) is kept iff draws[m][n] >= (float)p and scaled by 1 / (1 - p)), backward =
    drc_act_bwd_rows (ReLU / dropout mask and the fp64 fixed-order bias gradient) + two more drc_linear_fwd calls on operands
    drc_linear_pack_cols transposes while packing.  The data-gradient GEMM is skipped when x needs no gradient.  Every result has the same
    bits run to run.  The packed W^T is cached per parameter version next to the packed W (tag + '^T'): for the box head's 25088 -> 2048
    layer that is a SECOND 205 MB copy of the weight on the device."""
    E.require_gpu(x, "gemm_bias_act_train")
    x = x.float().contiguous()
    w2 = w2d_fn(weight_param)
    if w2.shape[1] != x.shape[1]:
        raise ValueError(f"gemm_bias_act_train: input has {x.shape[1]} features, the layer expects {w2.shape[1]}")
    p = float(p)
    if p > 0:
        if draws is None:
            draws = torch.rand(x.shape[0], w2.shape[0], dtype=torch.float32, device=x.device)
        draws = draws.to(device=x.device, dtype=torch.float32).contiguous()
        if tuple(draws.shape) != (x.shape[0], w2.shape[0]):
            raise ValueError(f"gemm_bias_act_train: draws {tuple(draws.shape)} for an output of {(x.shape[0], w2.shape[0])}")
    else:
        draws = None
    return _GemmBiasActTrain.apply(x, w2, bias, weight_param, tag, relu, p, draws, int(bias_fold))


def linear_train(x, layer, relu=False, p=0.0, draws=None):
    """The training form of linear(): see gemm_bias_act_train."""
    return gemm_bias_act_train(x, layer.weight, lambda w: w.reshape(w.shape[0], -1), layer.bias, relu, p=p, draws=draws)


class ConvReluChainTrain:
    """The training form of a chain of conv3x3 + bias + ReLU layers (the mask head's feature extractor) on the engine's blocked layout.
    Forward: every layer's blocked activation is KEPT (no ping-pong), fp32 kernels only (BlockedConv2d.fp32).  Backward, per layer in
    reverse: drc_act_bwd_blocked (ReLU mask + the per-channel bias gradient, fp64 in a fixed order), the weight gradient on
    drc_tapconv_wgrad (psmnet.train.wgrad, fixed-order partials), the data gradient on the engine's stride-1 convolution plan with swapped
    and flipped weights -- as psmnet.train does for stride-1 2D layers.  Every parameter gradient has the same bits run to run.

    The activations live in storage this object owns, per map geometry and sized for a capacity bucket of the unit count; a later
    forward of the same geometry overwrites them, so backward() of an EARLIER forward raises instead of differentiating stale values."""

    def __init__(self, convs, engines):
        self.convs, self.engines = list(convs), list(engines)
        for c in self.convs:
            if (c.kernel_size, c.stride, c.padding, c.dilation, c.groups) != ((3, 3), (1, 1), (1, 1), (1, 1), 1) or c.bias is None:
                raise NotImplementedError("ConvReluChainTrain: conv3x3 / stride 1 / pad 1 layers with a bias")
        self._bufs, self._gen, self._dw = {}, 0, {}

    def _storage(self, n, h, w, dev):
        key = (h, w, dev)
        buf = self._bufs.get(key)
        chans = [self.convs[0].in_channels] + [c.out_channels for c in self.convs]
        if buf is None or buf["cap"] < n:
            cap = E.bucket_units(n)
            buf = self._bufs[key] = dict(cap=cap, acts=[E.Blocked(cap, ch, 1, h, w, 0, 1, 1, dev) for ch in chans],
                                         grads=[E.Blocked(cap, max(chans), 1, h, w, 0, 1, 1, dev) for _ in range(2)])
            while len(self._bufs) > 4:
                self._bufs.pop(next(iter(self._bufs)))
        if len(set(chans)) != 1:
            raise NotImplementedError("ConvReluChainTrain: layers of one width (the shipped CONV_LAYERS are 256 throughout)")
        view = lambda b, ch: E.Blocked(n, ch, 1, h, w, 0, 1, 1, dev, storage=b.storage)
        return [view(b, ch) for b, ch in zip(buf["acts"], chans)], [view(b, chans[0]) for b in buf["grads"]]

    def _dgrad_weights(self, conv, plan, dev):
        """swapped (in <-> out) and tap-flipped packings of conv.weight for the data-gradient plan, per parameter version"""
        key = (conv.weight._version, conv.weight.data_ptr(), dev, plan.pack_kind)
        ent = self._dw.get(id(conv))
        if ent is None or ent[0] != key:
            wt = conv.weight.detach().to(device=dev, dtype=torch.float32)
            if plan.pack_kind in ("tap", "t16"):
                wp, w16 = E.pack_layouts(wt, True, True, want_t16=plan.needs_t16)
            else:
                wp, w16 = E.pack_layouts(wt, True, True, want_t16=False)[0], plan.pack16(wt, True, True)
            cp = E.cout_pad_of(conv.in_channels)
            ent = self._dw[id(conv)] = (key, wp, w16, torch.ones(cp, device=dev), torch.zeros(cp, device=dev))
        return ent[1:]

    def __call__(self, x):
        """x dense [n, C, h, w] (n >= 1) -> dense [n, C_out, h, w], differentiable in x and in every layer's weight and bias."""
        params = [p for c in self.convs for p in (c.weight, c.bias)]
        return _ConvReluChainFn.apply(x, self, *params)


class _ConvReluChainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, chain, *params):
        E.require_gpu(x, "ConvReluChainTrain")
        n, _, h, w = x.shape
        acts, grads = chain._storage(n, h, w, x.device)
        acts[0].from_dense(x.float())
        for eng, src, dst in zip(chain.engines, acts[:-1], acts[1:]):
            eng.fp32(src, dst)
        chain._gen += 1
        ctx.chain, ctx.acts, ctx.gbuf, ctx.gen = chain, acts, grads, chain._gen
        return acts[-1].to_dense()[:, :, 0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        from .psmnet.train import wgrad
        chain, acts, (ga, gb) = ctx.chain, ctx.acts, ctx.gbuf
        if ctx.gen != chain._gen:
            raise RuntimeError("ConvReluChainTrain: a later forward has overwritten the activations this backward needs")
        dev = gout.device
        L = len(chain.convs)
        cls = dict(n=(1, 3, 3), first=(0, 0, 0), step=(1, 1, 1))            # taps of a 3x3 / pad 1 layer on a halo-1 input (engine.taps_conv)
        out = [None] * (2 * L)
        ga.from_dense(gout.float().contiguous())
        for i in reversed(range(L)):
            conv = chain.convs[i]
            dz, db = act_bwd_blocked(ga, acts[i + 1], True, gb)
            gw = wgrad(acts[i], dz, cls, 1)                                    # [ci][co][t]
            out[2 * i] = gw[: conv.in_channels, : conv.out_channels].permute(1, 0, 2).reshape(conv.weight.shape)
            out[2 * i + 1] = db
            if i > 0 or ctx.needs_input_grad[0]:
                plans = chain.__dict__.setdefault("_dplans", OrderedDict())
                key = (i, dz.N, dz.H, dz.W, dev)
                plan = plans.get(key)
                if plan is None:
                    plan = plans[key] = E.plan_conv2d(dz, ga, 3, 1, 1, 1, conv.in_channels, False)
                    while len(plans) > 32:
                        plans.popitem(last=False)
                wp, w16, ones, zeros = chain._dgrad_weights(conv, plan, dev)
                plan.run(dz, wp, ones, zeros, ga, None, w16=w16)
        gx = ga.to_dense()[:, :, 0] if ctx.needs_input_grad[0] else None
        return (gx, None) + tuple(out)

"""The ResNet body's training form on the HIP engine (reference: backbone/resnet.py:81-146,229-345 under torch autograd; the fork's
FrozenBatchNorm2d is a plain nn.BatchNorm2d, so in train() EVERY BatchNorm of the body -- the stem and the frozen stages included --
normalises with the statistics of the 2N-image batch and updates its running statistics).

  forward   per conv+BN site, as psmnet/runtime.py:_site: the fp32 plan with unit scale / zero shift writes a `raw` tensor (allocated on
            first use, geometry of the site's output), then drc_bn_stats_blocked, drc_bn_finalize (running statistics,
            num_batches_tracked) and drc_bn_apply_blocked (+ residual, + ReLU); (mean, invstd, M) are kept in the workspace.  A site whose
            BatchNorm module is in eval runs the folded form -- allowed in the frozen prefix only.  The frozen prefix (the stem, the
            max-pool, every unit in front of the first one with a trainable parameter) runs under no_grad with no tape.
  Function  ONE autograd Function from the first trainable unit to the last: inputs are the parameters of its sites (and, for a bare
            unit, the input map), outputs the dense maps asked for (C2..C5).  backward() walks the sites in reverse:
              drc_bn_bwd_reduce / _apply   ReLU mask and residual fan-out fused; gamma / beta gradients from `sums`
              weight gradient              3x3: drc_tapconv_wgrad.  1x1: WGRAD_1X1["kernel"] -- "gemm": drc_conv1x1_wgrad_blocked (a GEMM
                                           over pixels, pts/body_train.hip), "tap": drc_tapconv_wgrad with in_mul = stride
              data gradient                the engine's forward plans with swapped (3x3: and flipped) weights; a stride-2 1x1 runs the
                                           stride-1 plan on the half-resolution gradient and scatters it to the even positions
                                           (the subsample adjoint of drc_bilinear_resize_blocked_bwd: any parity, odd positions get 0)
            A tensor's gradient is ASSIGNED by its first contribution and accumulated by the later ones (a unit's input: conv1's data
            gradient plus the projection's, or the identity's dres; a stage output: its C-map gradient first).  No data gradient is
            computed into the frozen prefix.  No atomics: the same bits run to run.  backward() after a later forward of the runtime
            raises RuntimeError (fpn_train's rule).
"""
import torch

from ... import engine as E
from .runtime import _half, _Site, _w16_for

# The 1x1 layers' weight gradient: "gemm" = drc_conv1x1_wgrad_blocked, "tap" = drc_tapconv_wgrad, "auto" = per layer class what won the
# A/B of DESIGN.md (ResNet body training): the GEMM form, except for stride-1 layers on at most AUTO_TAP_PIXELS pixels (R-50's layer4 at
# 4 x 12 x 39, where the two tie inside the windows' spread and the tap form therefore stays).  Both forms pass the same tests.
WGRAD_1X1 = {"kernel": "auto"}
AUTO_TAP_PIXELS = 2048


# ------------------------------------------------------------------------------------------------ the 1x1 weight gradient
def _check_1x1(a, b, cin, cout, stride):
    if stride not in (1, 2):
        raise ValueError("conv1x1_wgrad: stride 1 or 2")
    for v in (a, b):
        if v.D != 1 or v.pd != 0:
            raise ValueError("conv1x1_wgrad: blocked 2D tensors")
    if a.N != b.N or a.cb != (cin + 15) // 16 or b.cb != (cout + 15) // 16 or cin < 1 or cout < 1:
        raise ValueError("conv1x1_wgrad: a / b do not fit (N, cin, cout)")
    if (b.H, b.W) != ((a.H - 1) // stride + 1, (a.W - 1) // stride + 1):
        raise ValueError("conv1x1_wgrad: b must have the shape of the stride-s 1x1 convolution of a")


def conv1x1_wgrad(a, b, cin, cout, stride=1, kernel=None, chunk=None):
    """gw [cout, cin] = sum_{n,y,x} b[n, :, y, x] (x) a[n, :, s*y, s*x] for Blocked 2D tensors a (the layer's input) and b (the gradient of
    its output).  kernel: "gemm" | "tap" | "auto" (default: WGRAD_1X1); chunk: the GEMM form's pixels per partial sum (default: the library's)."""
    from ...pts import _lib as P
    kernel = kernel or WGRAD_1X1["kernel"]
    _check_1x1(a, b, cin, cout, stride)
    if kernel == "auto":
        kernel = "tap" if stride == 1 and b.N * b.H * b.W <= AUTO_TAP_PIXELS else "gemm"
    dev = a.device
    if kernel == "tap":
        from ..psmnet.train import wgrad, wgrad_tile_search
        if b.N:
            # the tap kernel stages whole a tiles: a ragged last tile may read past the last unit, which only the slack behind a covers
            R, WT, _ = wgrad_tile_search(b.H, b.W, stride, 0, 0)
            last = (stride * (-(-b.H // R) * R - 1) + a.ph) * a.h_stride + (stride * (-(-b.W // WT) * WT - 1) + a.pw + 1) * 16
            if last > a.cb_stride + E.SLACK_FLOATS:
                raise ValueError("conv1x1_wgrad: the tap form's last tile would read past the input's slack")
        gw = wgrad(a, b, dict(n=(1, 1, 1), first=(0, a.ph, a.pw), step=(1, 1, 1)), stride)               # [ci][co][1]
        return gw[:cin, :cout, 0].t().contiguous()
    if kernel != "gemm":
        raise ValueError("WGRAD_1X1['kernel'] must be 'gemm' or 'tap' (or 'auto')")
    lib = P.lib()
    chunk = int(chunk) if chunk is not None else lib.drc_conv1x1_wgrad_default_chunk()
    if chunk < 1:
        raise ValueError("conv1x1_wgrad: chunk >= 1")
    gw = torch.empty(cout, cin, dtype=torch.float32, device=dev)
    need = lib.drc_conv1x1_wgrad_scratch_floats(b.N, b.H, b.W, cin, cout, chunk)
    scr = E.scratch(dev, "conv1x1_wgrad", max(need, 1))
    st = lib.drc_conv1x1_wgrad_blocked(E._ptr(a.storage), a.n_stride, a.cb_stride, a.h_stride, a.interior_off,
                                       E._ptr(b.storage), b.n_stride, b.cb_stride, b.h_stride, b.interior_off,
                                       b.N, b.H, b.W, cin, cout, stride, chunk, E._ptr(gw), E._ptr(scr), scr.numel(), E._stream_ptr(dev))
    P.check(st, "drc_conv1x1_wgrad_blocked")
    return gw


# ------------------------------------------------------------------------------------------------ the training form of a site
def _train_affine(c, dev):
    """(unit scale, zero shift, gamma, beta), all padded to the site's channel blocks; kept on the site, which its runtime rebuilds when
    one of its tensors changes"""
    ent = getattr(c, "_train", None)
    if ent is None:
        cp, bn = c.scale.numel(), c.bn
        gamma, beta = torch.zeros(cp, device=dev), torch.zeros(cp, device=dev)
        gamma[: bn.num_features] = bn.weight.detach().to(dev).float()
        beta[: bn.num_features] = bn.bias.detach().to(dev).float()
        ent = c._train = (torch.ones(cp, device=dev), torch.zeros(cp, device=dev), gamma, beta)
    return ent


def _site_forward(ws, W, dev, entry, taped):
    plan, x, y, res = entry
    t, pl, c = ws["t"], ws["p"][plan], W[plan]
    bn, rs = c.bn, (t[res] if res else None)
    if not bn.training:
        if taped:
            raise NotImplementedError(f"body training: the BatchNorm of {plan} is in eval mode behind a trainable parameter; the folded form "
                                      "has no backward here (it is allowed in the frozen prefix only)")
        pl.run(t[x], c.w, c.scale, c.shift, t[y], rs, w16=_w16_for(c, pl))
        return
    if (bn.momentum is None or not bn.track_running_stats or bn.running_mean.device.type != dev.type or bn.running_mean.dtype != torch.float32 or
            not bn.running_mean.is_contiguous() or not bn.running_var.is_contiguous()):
        raise NotImplementedError("body training: BatchNorm with fp32 running statistics on the device and a fixed momentum")
    yt = t[y]
    raw = ws.setdefault("raw", {}).get(plan)
    if raw is None:
        raw = ws["raw"][plan] = E.Blocked(yt.N, yt.C, 1, yt.H, yt.W, 0, yt.ph, yt.pw, dev)
    unit, zero, gamma, beta = _train_affine(c, dev)
    pl.run(t[x], c.w, unit, zero, raw, None, relu=False, w16=_w16_for(c, pl))
    stats, M = E.bn_batch_stats_raw(raw)
    invstd = E.bn_finalize(stats, M, bn, bn.num_features)
    E.bn_apply(raw, yt, rs, stats[0], invstd, gamma, beta, bool(pl.p.relu))
    ws.setdefault("saved", {})[plan] = (stats[0], invstd, M)


def _site_params(c):
    return [c.conv.weight, c.bn.weight, c.bn.bias]


class _Grads:
    """Gradient buffers (Blocked, halo 0, the forward tensors' shapes) of a workspace, with assign-or-accumulate bookkeeping per backward."""

    def __init__(self, ws, dev):
        self.ws, self.dev, self.buf, self.have = ws, dev, ws.setdefault("body_g", {}), set()

    def get(self, name):
        b = self.buf.get(name)
        if b is None:
            f = self.ws["t"][name]
            b = self.buf[name] = E.Blocked(f.N, f.C, 1, f.H, f.W, 0, 0, 0, self.dev)
        return b


def _site_backward(ws, W, dev, G, entry, need_w, need_dx, out):
    """One site of the reverse pass; out[0..2] = the gradients of (conv.weight, bn.weight, bn.bias)."""
    from ... import _lib
    from .fpn_train import _conv_wgrad, _dgrad_packs, resize_bwd
    plan, x, y, res = entry
    t, fwd, c = ws["t"], ws["p"][plan], W[plan]
    lib, sp = _lib.lib(), E._stream_ptr(dev)
    relu, stride = bool(fwd.p.relu), int(fwd.p.in_mul)
    xin, yt, raw = t[x], t[y], ws["raw"][plan]
    mean, invstd, M = ws["saved"][plan]
    cout, cin, k = c._weight.shape[0], c._weight.shape[1], c._weight.shape[2]
    if y not in G.have:
        raise RuntimeError(f"body training: no gradient reached {y}")
    dy = G.get(y)
    sums = torch.empty(2, raw.cb * 16, dtype=torch.float32, device=dev)
    st = lib.drc_bn_bwd_reduce(E._ptr(dy.storage), E._geom8(dy), E._ptr(yt.storage), E._geom8(yt), E._ptr(raw.storage), E._geom8(raw),
                               E._ptr(mean), E._ptr(invstd), int(relu), E._ptr(sums), E._ptr(E.bn_scratch(dev, raw.cb)), sp)
    _lib.check(st, "drc_bn_bwd_reduce")
    draw = ws.setdefault("draw", {}).get(plan)
    if draw is None:
        halo = 1 if k == 3 else 0                                       # the 3x3 data gradient reads its input with a halo
        draw = ws["draw"][plan] = E.Blocked(raw.N, raw.C, 1, raw.H, raw.W, 0, halo, halo, dev)
    dres, acc = None, 0
    if res is not None:
        dres, acc = G.get(res), int(res in G.have)
        G.have.add(res)
    gamma = _train_affine(c, dev)[2]
    st = lib.drc_bn_bwd_apply(E._ptr(dy.storage), E._geom8(dy), E._ptr(yt.storage), E._geom8(yt), E._ptr(raw.storage), E._geom8(raw),
                              E._ptr(mean), E._ptr(invstd), E._ptr(gamma), E._ptr(sums), 1.0 / M, int(relu), E._ptr(draw.storage),
                              E._geom8(draw), E._ptr(dres.storage) if dres is not None else None,
                              E._geom8(dres) if dres is not None else None, acc, sp)
    _lib.check(st, "drc_bn_bwd_apply")
    if need_w[1]:
        out[1] = sums[1, :cout]
    if need_w[2]:
        out[2] = sums[0, :cout]
    if need_w[0]:
        if k == 1:
            out[0] = conv1x1_wgrad(xin, draw, cin, cout, stride).view(cout, cin, 1, 1)
        else:
            out[0] = _conv_wgrad(xin, draw, 3, cout, cin)
    if not need_dx:
        return
    gx, first = G.get(x), x not in G.have
    plans = ws.setdefault("body_dplans", {})
    if k == 1 and stride == 2:
        ent = plans.get(plan)
        if ent is None:
            half = E.Blocked(draw.N, cin, 1, draw.H, draw.W, 0, 0, 0, dev)
            ent = plans[plan] = (E.plan_conv2d(draw, half, 1, 1, 0, 1, cin, False), half)
        pl, half = ent
        wp, w16, ones, zeros = _dgrad_packs(c, pl)
        pl.run(draw, wp, ones, zeros, half, None, w16=w16)
        resize_bwd(None, gx, not first, half)                           # even positions (=|+=) half, odd ones (=|+=) 0
    else:
        ent = plans.get(plan)
        if ent is None:
            ent = plans[plan] = (E.plan_conv2d(draw, gx, k, 1, k // 2, 1, cin, False), None)
        pl = ent[0]
        wp, w16, ones, zeros = _dgrad_packs(c, pl)
        pl.run(draw, wp, ones, zeros, gx, None if first else gx, w16=w16)
    G.have.add(x)


class _BodyTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, host, ws, W, entries, outs, x_name, x_dense, *params):
        dev = host.device
        for e in entries:
            _site_forward(ws, W, dev, e, True)
        host._pass = getattr(host, "_pass", 0) + 1
        ctx.host, ctx.ws, ctx.entries, ctx.outs, ctx.x_name, ctx.gen = host, ws, entries, outs, x_name, host._pass
        ctx.sites = {e[0]: W[e[0]] for e in entries}
        return tuple(ws["t"][o].to_dense()[:, :, 0] for o in outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        host, ws, entries = ctx.host, ctx.ws, ctx.entries
        if ctx.gen != getattr(host, "_pass", 0):
            raise RuntimeError("body_train: a later forward of this runtime has overwritten the maps this backward needs")
        dev = host.device
        G = _Grads(ws, dev)
        for name, g in zip(ctx.outs, gouts):
            G.get(name).from_dense(g.float())
            G.have.add(name)
        need_x, need_p = ctx.needs_input_grad[6], ctx.needs_input_grad[7:]
        made = {e[2] for e in entries}                                  # tensors the taped sites wrote: only they take a data gradient
        gp = [None] * (3 * len(entries))
        for i in reversed(range(len(entries))):
            e = entries[i]
            out = [None] * 3
            _site_backward(ws, ctx.sites, dev, G, e, need_p[3 * i: 3 * i + 3], e[1] in made or (need_x and e[1] == ctx.x_name), out)
            gp[3 * i: 3 * i + 3] = out
        gx = G.get(ctx.x_name).to_dense()[:, :, 0] if need_x else None
        return (None,) * 6 + (gx,) + tuple(gp)


def run(host, ws, W, entries, outs, x_name=None, x_dense=None):
    """The Function over the sites `entries` (schedule tuples (plan, x, y, res)) of a workspace whose input tensors are in place."""
    params = [p for e in entries for p in _site_params(W[e[0]])]
    return _BodyTrainFn.apply(host, ws, W, entries, outs, x_name, x_dense, *params)


def first_trainable(sched, W):
    """Index of the first site of the first UNIT with a trainable parameter (a unit's sites are adjacent and start at its projection or its
    conv1), or len(sched)."""
    for i, e in enumerate(sched):
        if any(p.requires_grad for p in _site_params(W[e[0]])):
            unit = e[0].rsplit(".", 1)[0]
            while i > 0 and sched[i - 1][0].rsplit(".", 1)[0] == unit:
                i -= 1
            return i
    return len(sched)


def forward_body(rt, x):
    """BackboneRuntime.forward_body_train: forward_cmaps, then the FPN's Function on the C maps.  -> the five dense maps."""
    from . import fpn_train
    ws, N, cmaps = forward_cmaps(rt, x)
    return fpn_train.run(rt, rt.model.fpn, ws, N, cmaps)


def forward_cmaps(rt, x):
    """The body of a BackboneRuntime in its training form: stem, max-pool and the frozen prefix under no_grad, the Function behind them.
    -> (workspace, N, [C2..C5]): a dense map that requires grad for every stage the Function produced, None for a stage of the frozen
    prefix (its blocked tensor is in the workspace all the same: ws["t"][ws["stage_out"][i][0]])."""
    from ... import _lib
    dev = rt.device
    N, _, H, W_ = x.shape
    Wt = rt._compile()
    ws = rt._workspace(N, H, W_)
    t = ws["t"]
    sched = ws["sched"]
    first = first_trainable(sched, Wt) if torch.is_grad_enabled() else len(sched)
    with torch.no_grad():
        if (H | W_) & 1:
            x = torch.nn.functional.pad(x, (0, W_ & 1, 0, H & 1))
        t["img"].from_dense(torch.nn.functional.pixel_unshuffle(x, 2))
        _site_forward(ws, Wt, dev, ("stem", "img", "stem", None), False)
        h1, w1, ph, pw = ws["pool"]
        _lib.check(_lib.lib().drc_maxpool2d_blocked(E._ptr(t["stem"].storage), E._ptr(t["pool"].storage), N, 4, h1, w1, 0, 3, 2, ph, pw, 0,
                                                    E._stream_ptr(dev)), "drc_maxpool2d_blocked")
        for e in sched[:first]:
            _site_forward(ws, Wt, dev, e, False)
    names = [s[0] for s in ws["stage_out"]]
    if first < len(sched):
        made = {e[2] for e in sched[first:]}
        cm = run(rt, ws, Wt, sched[first:], [n for n in names if n in made])
        cm = iter(cm)
        cmaps = [next(cm) if n in made else None for n in names]
    else:
        rt._pass = getattr(rt, "_pass", 0) + 1
        cmaps = [None] * 4
    return ws, N, cmaps


# ------------------------------------------------------------------------------------------------ one bare unit (tests, tools)
class UnitRuntime:
    """One Bottleneck unit (resnet.py:229-345: the stride on conv1) on the engine in its training form: the body's sites and plans behind a
    dense input.  forward_train(x) -> the dense output, differentiable in x and in the unit's parameters."""

    def __init__(self, unit, device):
        self.unit, self.device, self._ws, self._pass = unit, device, {}, 0

    def _compile(self):
        u, dev = self.unit, self.device
        W = {"u.c1": _Site(u.conv1, u.bn1, dev), "u.c2": _Site(u.conv2, u.bn2, dev), "u.c3": _Site(u.conv3, u.bn3, dev)}
        if u.downsample is not None:
            W["u.ds"] = _Site(u.downsample[0], u.downsample[1], dev)
        return W

    def _workspace(self, N, H, W_):
        key = (N, H, W_)
        if key not in self._ws:
            u, dev = self.unit, self.device
            B2 = lambda c, h, w, pad: E.Blocked(N, c, 1, h, w, 0, pad, pad, dev)
            s, mid, cout = u.stride, u.conv1.out_channels, u.conv3.out_channels
            oh, ow = (_half(H), _half(W_)) if s == 2 else (H, W_)
            t = {"in": B2(u.conv1.in_channels, H, W_, 0), "u.a": B2(mid, oh, ow, 1), "u.b": B2(mid, oh, ow, 0), "u.o": B2(cout, oh, ow, 0)}
            p = {"u.c1": E.plan_conv2d(t["in"], t["u.a"], 1, s, 0, 1, mid, True), "u.c2": E.plan_conv2d(t["u.a"], t["u.b"], 3, 1, 1, 1, mid, True),
                 "u.c3": E.plan_conv2d(t["u.b"], t["u.o"], 1, 1, 0, 1, cout, True)}
            sched, res = [], "in"
            if u.downsample is not None:
                t["u.s"] = B2(cout, oh, ow, 0)
                p["u.ds"] = E.plan_conv2d(t["in"], t["u.s"], 1, s, 0, 1, cout, False)
                sched.append(("u.ds", "in", "u.s", None))
                res = "u.s"
            sched += [("u.c1", "in", "u.a", None), ("u.c2", "u.a", "u.b", None), ("u.c3", "u.b", "u.o", res)]
            self._ws[key] = dict(t=t, p=p, sched=sched)
        return self._ws[key]

    def forward_train(self, x):
        E.require_gpu(x, "bottleneck input")
        if x.dim() != 4 or x.shape[1] != self.unit.conv1.in_channels:
            raise ValueError(f"expected [N,{self.unit.conv1.in_channels},H,W], got {tuple(x.shape)}")
        ws = self._workspace(*(int(v) for v in (x.shape[0], x.shape[2], x.shape[3])))
        ws["t"]["in"].from_dense(x.detach())
        return run(self, ws, self._compile(), ws["sched"], ["u.o"], "in", x)[0]

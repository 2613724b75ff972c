"""The FPN's training form on the HIP engine (reference: fpn.py:44-82 under torch autograd, behind a ResNet body in its eval form with
frozen parameters -- what the reference's fix_model helpers set up one level higher).

One autograd Function over (C2..C5, the 16 FPN parameters) -> the five dense maps.

  forward   the runtime's FPN schedule (runtime._run_fpn) on the fp32 plans only -- no split-f16 bridge, as in every training form here.
            Nothing is saved besides what the schedule leaves in the runtime's workspace: the C maps and sum1..3.  A later forward of the
            runtime overwrites them, so backward() of an EARLIER forward raises RuntimeError (ConvReluChainTrain's rule).
  backward  levels i = 1, 2, 3, then the top:
              out_i = fpn_layer{i}(sum_i)                 bias: drc_channel_sums_blocked; weight: drc_tapconv_wgrad, 3x3 tap class;
                                                          data: the engine's stride-1 3x3 plan with swapped and flipped weights
              sum_i = fpn_inner{i}(C_i) + resize(out_i+1) the same with the 1x1 tap class (the 1x1 data gradient only for a C map that
                                                          needs one); drc_bilinear_resize_blocked_bwd ACCUMULATES into the gradient of
                                                          out_{i+1} -- the fork's top-down path reads the layer block's output, not the
                                                          lateral sum -- and, for i = 3, into in4's together with P6's subsample adjoint
              in4   = fpn_inner4(C5)                      (out4 = in4: no 3x3 block)
            The incoming dense gradients go into halo-1 blocked buffers the workspace owns (per geometry, reused between steps).  No
            atomics anywhere: every parameter gradient and every C-map gradient has the same bits run to run.  fpn_layer4 is unused by the
            fork's forward (fpn.py:54-55): its gradients are zeros (torch autograd would leave them None).
"""
import torch

from ... import _lib
from ... import engine as E
from .runtime import FPNRuntime, _dense_outputs, _fp32_conv, _run_fpn

_CLS3 = dict(n=(1, 3, 3), first=(0, 0, 0), step=(1, 1, 1))        # taps of a 3x3 / pad 1 layer on a halo-1 input (engine.taps_conv)


def resize_bwd(grad_y, grad_x, accumulate, grad_sub=None):
    """grad_x (=|+=) resize^T(grad_y) + subsample^T(grad_sub) on Blocked 2D tensors (drc_bilinear_resize_blocked_bwd); grad_y or grad_sub
    may be None."""
    gy, gs = grad_y, grad_sub
    for g in (gy, gs):
        if g is not None and (g.N, g.cb, g.D, g.pd, g.ph == g.pw) != (grad_x.N, grad_x.cb, 1, 0, True):
            raise ValueError("resize_bwd: blocked 2D tensors of one unit and channel count, one halo per tensor")
    if gs is not None and (gs.H, gs.W) != ((grad_x.H - 1) // 2 + 1, (grad_x.W - 1) // 2 + 1):
        raise ValueError("resize_bwd: grad_sub must have the max_pool2d(1, 2, 0) shape of grad_x")
    st = _lib.lib().drc_bilinear_resize_blocked_bwd(E._ptr(gy.storage) if gy is not None else None, E._ptr(grad_x.storage), grad_x.N, grad_x.cb,
                                                    grad_x.H, grad_x.W, grad_x.ph, gy.H if gy is not None else 0, gy.W if gy is not None else 0,
                                                    gy.ph if gy is not None else 0, 0, int(bool(accumulate)),
                                                    E._ptr(gs.storage) if gs is not None else None, gs.ph if gs is not None else 0,
                                                    E._stream_ptr(grad_x.device))
    _lib.check(st, "drc_bilinear_resize_blocked_bwd")
    return grad_x


def channel_sums(x):
    """Per-channel sums [C] of a Blocked 2D tensor over all units and interior pixels (fp64, fixed order)."""
    lib = _lib.lib()
    sums = torch.empty(x.cb * 16, dtype=torch.float32, device=x.device)
    nd = lib.drc_channel_sums_blocked_scratch_doubles(x.N, x.C, x.H)
    scr = E.scratch(x.device, "channel_sums", 2 * max(nd, 1))            # (float workspace: two floats per double)
    st = lib.drc_channel_sums_blocked(E._ptr(x.storage), x.N, x.C, x.H, x.W, x.ph, x.pw, E._ptr(sums), E._ptr(scr), nd, E._stream_ptr(x.device))
    _lib.check(st, "drc_channel_sums_blocked")
    return sums[: x.C]


def _conv_wgrad(a, b, k, cout, cin):
    """weight gradient [cout, cin, k, k] of a stride-1 convolution (k = 3: pad 1 on a halo-1 input) with input a and output gradient b"""
    from ..psmnet.train import wgrad
    cls = _CLS3 if k == 3 else dict(n=(1, 1, 1), first=(0, a.ph, a.pw), step=(1, 1, 1))
    if k == 3 and (a.ph, a.pw) != (1, 1):
        raise ValueError("fpn_train: the 3x3 layers read halo-1 inputs")
    gw = wgrad(a, b, cls, 1)                                            # [ci][co][t]
    return gw[:cin, :cout].permute(1, 0, 2).reshape(cout, cin, k, k)


def _dgrad_packs(site, plan):
    """swapped (in <-> out) and, for 3x3, tap-flipped packings of a site's weight for its data-gradient plan; kept on the site, which the
    runtime rebuilds when the parameter changes"""
    ent = getattr(site, "_dgrad", None)
    if ent is None or ent[0] != plan.pack_kind:
        wt = site._weight
        if plan.pointwise:
            wp, w16 = E.pack_layouts(wt, True, False, want_tap=False)[1][0], None
        elif plan.pack_kind in ("tap", "t16"):
            wp, w16 = E.pack_layouts(wt, True, True, want_t16=plan.needs_t16)
        else:
            wp, w16 = E.pack_layouts(wt, True, True, want_t16=False)[0], plan.pack16(wt, True, True)
        cp = E.cout_pad_of(wt.shape[1])
        ent = site._dgrad = (plan.pack_kind, wp, w16, torch.ones(cp, device=wt.device), torch.zeros(cp, device=wt.device))
    return ent[1:]


def _grad_state(ws, N, dev):
    """The gradient buffers and data-gradient plans of a workspace: built once per geometry, reused between steps."""
    g = ws.get("fpn_g")
    if g is None:
        t = ws["t"]
        like = lambda b, pad: E.Blocked(N, b.C, 1, b.H, b.W, 0, pad, pad, dev)
        g = ws["fpn_g"] = dict(buf={}, plan={})
        for name in ws["outs"]:
            g["buf"][name] = like(t[name], 1)
        for i in (1, 2, 3):
            g["buf"][f"sum{i}"] = like(t[f"sum{i}"], 0)
            g["plan"][f"layer{i}"] = E.plan_conv2d(g["buf"][f"out{i}"], g["buf"][f"sum{i}"], 3, 1, 1, 1, t[f"sum{i}"].C, False)
    return g


def _cmap_grad(g, ws, i, dev):
    """(gradient buffer of C map i, the 1x1 data-gradient plan into it): allocated when a C map first needs a gradient"""
    name = f"c{i}"
    if name not in g["buf"]:
        src = ws["t"][ws["stage_out"][i - 1][0]]
        g["buf"][name] = E.Blocked(src.N, src.C, 1, src.H, src.W, 0, 0, 0, dev)
        g["plan"][f"inner{i}"] = E.plan_conv2d(g["buf"][f"sum{i}" if i < 4 else "in4"], g["buf"][name], 1, 1, 0, 1, src.C, False)
    return g["buf"][name], g["plan"][f"inner{i}"]


class _FPNTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rt, ws, N, *tensors):
        Wt = rt._compile()
        _run_fpn(ws, N, _fp32_conv(ws, Wt), rt.device)
        outs = _dense_outputs(rt, ws)                                  # (advances the runtime's generation)
        ctx.rt, ctx.ws, ctx.N, ctx.gen = rt, ws, N, rt._gen
        ctx.layer4_shapes = (tuple(tensors[18].shape), tuple(tensors[19].shape))
        ctx.sites = {k: Wt[k] for k in ("inner1", "inner2", "inner3", "inner4", "layer1", "layer2", "layer3")}
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        rt, ws, N, sites = ctx.rt, ctx.ws, ctx.N, ctx.sites
        if ctx.gen != rt._gen:
            raise RuntimeError("fpn_train: a later forward of this runtime has overwritten the maps this backward needs")
        dev = rt.device
        t = ws["t"]
        need_c, need_p = ctx.needs_input_grad[3:7], ctx.needs_input_grad[7:]
        g = _grad_state(ws, N, dev)
        buf = g["buf"]
        for name, go in zip(ws["outs"], gouts):
            buf[name].from_dense(go.float())
        gc, gp = [None] * 4, [None] * 16                              # parameters: (inner_i.weight, .bias, layer_i.weight, .bias) per level

        def lateral(i, gsum):
            feat = t[ws["stage_out"][i - 1][0]]
            s = sites[f"inner{i}"]
            if need_p[4 * (i - 1)]:
                gp[4 * (i - 1)] = _conv_wgrad(feat, gsum, 1, s._weight.shape[0], s._weight.shape[1])
            if need_p[4 * (i - 1) + 1]:
                gp[4 * (i - 1) + 1] = channel_sums(gsum)
            if need_c[i - 1]:
                gbuf, plan = _cmap_grad(g, ws, i, dev)
                wp, w16, ones, zeros = _dgrad_packs(s, plan)
                plan.run(gsum, wp, ones, zeros, gbuf, None, w16=w16)
                gc[i - 1] = gbuf.to_dense()[:, :, 0]

        for i in (1, 2, 3):
            gout, gsum = buf[f"out{i}"], buf[f"sum{i}"]
            s = sites[f"layer{i}"]
            if need_p[4 * (i - 1) + 2]:
                gp[4 * (i - 1) + 2] = _conv_wgrad(t[f"sum{i}"], gout, 3, s._weight.shape[0], s._weight.shape[1])
            if need_p[4 * (i - 1) + 3]:
                gp[4 * (i - 1) + 3] = channel_sums(gout)
            plan = g["plan"][f"layer{i}"]
            wp, w16, ones, zeros = _dgrad_packs(s, plan)
            plan.run(gout, wp, ones, zeros, gsum, None, w16=w16)
            lateral(i, gsum)
            if i < 3:
                resize_bwd(gsum, buf[f"out{i + 1}"], True)
            else:                                                       # g_in4 = g_P5 + resize^T(g_sum3) + subsample^T(g_P6)
                resize_bwd(gsum, buf["in4"], True, buf["p6"])
        lateral(4, buf["in4"])
        for j, shape in zip((14, 15), ctx.layer4_shapes):                # fpn_layer4: outside the graph, a zero gradient
            if need_p[j]:
                gp[j] = torch.zeros(shape, dtype=torch.float32, device=dev)
        return (None, None, None) + tuple(gc) + tuple(gp)


def _params(fpn):
    out = []
    for i in range(1, 5):
        for name in (f"fpn_inner{i}", f"fpn_layer{i}"):
            conv = getattr(fpn, name)
            out += [conv.weight, conv.bias]
    return out


def run(rt, fpn, ws, N, cmaps):
    """The Function on a workspace whose C maps are in place (cmaps: the dense maps as autograd inputs, or None each)."""
    outs = _FPNTrainFn.apply(rt, ws, N, *cmaps, *_params(fpn))
    for o in outs:
        o._drc_pyramid_gen = (id(rt), rt._gen)
    return tuple(outs)


def fpn_train(features, fpn, runtime=None):
    """The training form of a bare FPN module: features = (C2, C3, C4, C5) dense CUDA tensors -> (P2, P3, P4, P5, P6), differentiable in
    the features and in fpn's parameters.  runtime: the FPNRuntime to run on (default: one kept on the module per device)."""
    dev = features[0].device
    if runtime is None:
        rts = fpn.__dict__.setdefault("_drc_runtimes", {})
        runtime = rts.get(dev)
        if runtime is None:
            runtime = rts[dev] = FPNRuntime(fpn, dev)
    ws, N = runtime.load(features)
    return run(runtime, fpn, ws, N, list(features))

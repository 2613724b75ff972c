"""The FPN's training form on the MI355X: the resize adjoint and the channel sums against their fp64 restatements, the FPN backward of a
bare FPN module against torch-CPU fp64 autograd (with torch-CPU fp32 autograd as the yardstick), and DispRCNN's training step with the
FPN trainable behind a frozen ResNet body.

Tolerance rule of the FPN tests (per tensor): e = max|x - oracle| / max|oracle|; the HIP value must be <= max(4 * e(torch-CPU fp32), 1e-6).
The factor covers another summation order over at most 234 pixels x 3 images; a dropped tile or tap shows at 1e-2 and above."""
import itertools

import numpy as np
import pytest
import torch

from tests import fpn_train_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = np.float32(-1234.5)


def E():
    from disprcnn_amd import engine
    return engine


def LIB():
    from disprcnn_amd import _lib
    return _lib.lib()


def seeded(shape, *key, scale=1.0):
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return (np.random.default_rng(s).standard_normal(shape) * scale).astype(F32)


def blocked_with_halo(dense, pad, fill_interior=True):
    """A Blocked tensor whose every word is SENTINEL except (if fill_interior) the interior, which holds `dense` (padded lanes zero)."""
    n, c, h, w = dense.shape
    b = E().Blocked(n, c, 1, h, w, 0, pad, pad, torch.device("cuda"))
    b.storage.fill_(float(SENTINEL))
    if fill_interior and n:
        b.from_dense(torch.from_numpy(dense).cuda())
    return b


def words(b):
    return b.view6().cpu().numpy().view(np.uint32).copy()


def interior_mask(b):
    m = np.zeros((b.N, b.cb, b.Dp, b.Hp, b.Wp, 16), bool)
    m[:, :, :, b.ph: b.ph + b.H, b.pw: b.pw + b.W, :] = True
    return m


def call_resize_bwd(gy, gx, acc, gs=None, ac=0, oh=None, ow=None):
    e = E()
    return LIB().drc_bilinear_resize_blocked_bwd(e._ptr(gy.storage) if gy is not None else None, e._ptr(gx.storage), gx.N, gx.cb, gx.H, gx.W, gx.ph,
                                                 (gy.H if gy is not None else 0) if oh is None else oh,
                                                 (gy.W if gy is not None else 0) if ow is None else ow, gy.ph if gy is not None else 0, ac, acc,
                                                 e._ptr(gs.storage) if gs is not None else None, gs.ph if gs is not None else 0,
                                                 e._stream_ptr(torch.device("cuda")))


# ------------------------------------------------------------------------------------------------ 1. the resize adjoint
SHAPES = [((1, 1), (1, 1)), ((1, 1), (2, 2)), ((3, 5), (6, 10)), ((4, 3), (7, 5)), ((2, 7), (3, 13)), ((5, 4), (12, 9)), ((6, 6), (6, 6))]
# (C, N, px, py, accumulate, grad_sub and its halo): varied across the seven shapes so that every value of every knob meets odd and even maps
KNOBS = [(5, 1, 0, 0, 0, None), (24, 3, 1, 0, 1, 0), (5, 3, 0, 1, 1, 1), (24, 1, 1, 1, 0, 1), (5, 1, 1, 0, 0, 0), (24, 3, 0, 1, 1, None),
         (5, 3, 1, 1, 1, 0)]
RESIZE_CASES = [(s, KNOBS[(i + r) % 7]) for r in (0, 3) for i, s in enumerate(SHAPES)]


def resize_inputs(ihw, ohw, C, N, tag):
    (ih, iw), (oh, ow) = ihw, ohw
    g = seeded((N, C, oh, ow), "g", tag)
    old = seeded((N, C, ih, iw), "old", tag)
    sub = seeded((N, C, (ih - 1) // 2 + 1, (iw - 1) // 2 + 1), "sub", tag)
    return g, old, sub


@pytest.mark.parametrize("case", range(len(RESIZE_CASES)))
def test_resize_bwd_against_oracle(case):
    shape, knobs = RESIZE_CASES[case]
    (ih, iw), (oh, ow) = shape
    C, N, px, py, acc, ps = knobs
    g, old, sub = resize_inputs((ih, iw), (oh, ow), C, N, (shape, knobs))
    gy = blocked_with_halo(g, py)
    gs = blocked_with_halo(sub, ps) if ps is not None else None
    runs = []
    for _ in range(2):
        gx = blocked_with_halo(old, px, fill_interior=bool(acc))
        before = words(gx)
        assert call_resize_bwd(gy, gx, acc, gs) == 0
        torch.cuda.synchronize()
        runs.append((words(gx), gx.to_dense()[:, :, 0].cpu().numpy()))
    after, got = runs[0]
    assert np.array_equal(runs[0][0], runs[1][0])                                   # the same bits run to run
    inside = interior_mask(gx)
    assert np.array_equal(after[~inside], before[~inside])                          # halo words untouched
    lanes = after.view(F32)[:, :, 0, px: px + ih, px: px + iw, :].transpose(0, 1, 4, 2, 3).reshape(N, gx.cb * 16, ih, iw)
    assert not lanes[:, C:].any()                                                   # padded channel lanes: zero
    ref, mag = O.resize_bwd(g, ih, iw, sub if ps is not None else None, old if acc else None)
    err = np.abs(got.astype(np.float64) - ref)
    bound = 32 * 2.0 ** -24 * mag
    worst = float((err - bound).max())
    print(f"resize_bwd {shape} {knobs}: max err {err.max():.3e}, max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert worst <= 0


@pytest.mark.parametrize("ihw", [(3, 5), (4, 4), (1, 1), (2, 7)])
def test_resize_bwd_grad_sub_alone(ihw):
    ih, iw = ihw
    C, N = 24, 3
    _, old, sub = resize_inputs(ihw, ihw, C, N, ("alone", ihw))
    for acc, px, ps in ((0, 1, 0), (1, 0, 1)):
        gx = blocked_with_halo(old, px, fill_interior=bool(acc))
        before = words(gx)
        gs = blocked_with_halo(sub, ps)
        assert call_resize_bwd(None, gx, acc, gs) == 0
        torch.cuda.synchronize()
        want = old.copy() if acc else np.zeros_like(old)
        want[:, :, ::2, ::2] += sub                                                  # one fp32 add per element: exact
        assert np.array_equal(gx.to_dense()[:, :, 0].cpu().numpy(), want)
        inside = interior_mask(gx)
        assert np.array_equal(words(gx)[~inside], before[~inside])


def test_resize_bwd_adjoint_identity():
    """<resize(x), g> == <x, resize^T(g)> against the FORWARD kernel, summed in fp64"""
    e = E()
    dev = torch.device("cuda")
    for (ih, iw), (oh, ow) in SHAPES:
        N, C = 3, 24
        # positive values: the inner product is as large as the sum of its terms' magnitudes, so "relative" has no cancellation to hide behind
        x, g = np.abs(seeded((N, C, ih, iw), "adj:x", ih, iw, oh, ow)) + F32(0.5), np.abs(seeded((N, C, oh, ow), "adj:g", ih, iw, oh, ow)) + F32(0.5)
        xb, gb = blocked_with_halo(x, 1), blocked_with_halo(g, 0)
        yb, gxb = e.Blocked(N, C, 1, oh, ow, 0, 1, 1, dev), e.Blocked(N, C, 1, ih, iw, 0, 0, 0, dev)
        st = LIB().drc_bilinear_resize_blocked(e._ptr(xb.storage), e._ptr(yb.storage), N, xb.cb, ih, iw, 1, oh, ow, 1, xb.cb, 0, 0, e._stream_ptr(dev))
        assert st == 0 and call_resize_bwd(gb, gxb, 0) == 0
        y, gx = yb.to_dense()[:, :, 0].cpu().numpy().astype(np.float64), gxb.to_dense()[:, :, 0].cpu().numpy().astype(np.float64)
        lhs, rhs = float((y * g).sum()), float((x.astype(np.float64) * gx).sum())
        print(f"adjoint {(ih, iw)}->{(oh, ow)}: {lhs:.9e} vs {rhs:.9e}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_resize_bwd_refuses_bad_arguments():
    g, old, _ = resize_inputs((3, 5), (6, 10), 5, 1, "bad")
    gy, gx = blocked_with_halo(g, 0), blocked_with_halo(old, 0)
    before = words(gx)
    assert call_resize_bwd(gy, gx, 0, ac=1) == -2                                   # align_corners = 1
    assert call_resize_bwd(gy, gx, 0, oh=2) == -2                                   # OH < IH
    assert call_resize_bwd(gy, gx, 0, ow=4) == -2
    e = E()
    st = LIB().drc_bilinear_resize_blocked_bwd(e._ptr(gy.storage), e._ptr(gx.storage), 0, 1, 3, 5, 0, 6, 10, 0, 0, 0, None, 0,
                                               e._stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    assert st == 0 and np.array_equal(words(gx), before)                            # N = 0 touches nothing


# ------------------------------------------------------------------------------------------------ 2. channel sums
def ulp_diff(a, b):
    key = lambda v: np.where(v.view(np.int32) < 0, np.int32(-2 ** 31) - v.view(np.int32), v.view(np.int32)).astype(np.int64)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("units,C,hw,pad", [(u, c, hw, p) for (u, c, hw), p in zip(
    itertools.product((1, 3), (5, 16, 40), ((1, 1), (7, 9), (33, 65))), itertools.cycle((0, 1, 1, 0, 1)))])
def test_channel_sums(units, C, hw, pad):
    from disprcnn_amd.modeling.backbone.fpn_train import channel_sums
    h, w = hw
    x = seeded((units, C, h, w), "sums", units, C, h, w)
    b = blocked_with_halo(x, pad)                                                    # halo words hold the sentinel: they must not be summed
    got = [channel_sums(b).cpu().numpy() for _ in range(2)]
    assert got[0].shape == (C,) and np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    want = x.astype(np.float64).sum(axis=(0, 2, 3)).astype(F32)
    assert ulp_diff(got[0], want).max() <= 1


# ------------------------------------------------------------------------------------------------ 3. the FPN backward, bare module
STAGE_CH = (8, 24, 40, 72)
MAP_HW = ((13, 18), (7, 9), (4, 5), (2, 3))


def bare_fpn(och, tag):
    from disprcnn_amd.modeling.backbone.fpn import FPN
    fpn = FPN(STAGE_CH, och)
    with torch.no_grad():
        for name, p in fpn.named_parameters():
            p.copy_(torch.from_numpy(seeded(tuple(p.shape), "fpn", tag, name, scale=0.5 if name.endswith("bias") else (2.0 / p[0].numel()) ** 0.5)))
    return fpn.cuda()


def fpn_inputs(och, N, tag):
    feats = [torch.from_numpy(seeded((N, c, h, w), "C", tag, i)) for i, (c, (h, w)) in enumerate(zip(STAGE_CH, MAP_HW))]
    hws = MAP_HW + (((MAP_HW[3][0] - 1) // 2 + 1, (MAP_HW[3][1] - 1) // 2 + 1),)
    assert hws[4] == (1, 2)
    gouts = [torch.from_numpy(seeded((N, och, h, w), "G", tag, i)) for i, (h, w) in enumerate(hws)]
    return feats, gouts


def check_rule(what, hip, t32, ref, table):
    e_hip, e_32 = O.rel_err(hip, ref), O.rel_err(t32, ref)
    table.append((what, e_hip, e_32))
    print(f"  {what:24s} hip {e_hip:.3e}   torch-fp32 {e_32:.3e}")
    return e_hip <= max(4 * e_32, 1e-6)


@pytest.mark.parametrize("och,N", [(16, 2), (24, 3)])
def test_fpn_backward_against_fp64_autograd(och, N):
    from disprcnn_amd.modeling.backbone.fpn_train import fpn_train
    from disprcnn_amd.modeling.backbone.runtime import FPNRuntime
    fpn = bare_fpn(och, (och, N))
    feats, gouts = fpn_inputs(och, N, (och, N))
    params = {k: v for k, v in fpn.named_parameters()}
    ref_o, ref_p, ref_c = O.fpn_step(feats, params, gouts, torch.float64)
    t32_o, t32_p, t32_c = O.fpn_step(feats, params, gouts, torch.float32)
    rt = FPNRuntime(fpn, torch.device("cuda"))

    def step():
        fpn.zero_grad(set_to_none=True)
        cm = [f.cuda().requires_grad_(True) for f in feats]
        outs = fpn_train(cm, fpn, rt)
        torch.autograd.backward(outs, [g.cuda() for g in gouts])
        return outs, {k: (None if p.grad is None else p.grad.clone()) for k, p in fpn.named_parameters()}, [c.grad for c in cm]
    outs, pg, cg = step()
    table, ok = [], True
    print(f"FPN backward, out channels {och}, N {N}: max|x - oracle| / max|oracle|")
    for i, o in enumerate(outs):
        ok &= check_rule(f"P{i + 2}", o, t32_o[i], ref_o[i], table)
    with torch.no_grad():                                       # the eval runtime's FPN on the same C maps (no split-f16 bridge at this size)
        ev = FPNRuntime(fpn, torch.device("cuda")).forward([f.cuda() for f in feats])
    assert all(torch.equal(a, b) for a, b in zip(outs, ev))
    for k in O.PARAM_NAMES:
        if ref_p[k] is None:                                    # fpn_layer4: unused by the fork's forward -- a zero gradient
            assert k.startswith("fpn_layer4") and pg[k].shape == params[k].shape and not pg[k].any().item()
            continue
        assert pg[k] is not None and pg[k].shape == params[k].shape, k
        ok &= check_rule(k, pg[k], t32_p[k], ref_p[k], table)
    for i in range(4):
        ok &= check_rule(f"C{i + 2}", cg[i], t32_c[i], ref_c[i], table)
    assert ok
    # a second backward from the same inputs: the same bits
    outs2, pg2, cg2 = step()
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
    assert all(torch.equal(pg[k], pg2[k]) for k in pg)
    assert all(torch.equal(a, b) for a, b in zip(cg, cg2))


def test_fpn_backward_skips_cmap_gradients_and_refuses_a_stale_forward():
    from disprcnn_amd.modeling.backbone.fpn_train import fpn_train
    from disprcnn_amd.modeling.backbone.runtime import FPNRuntime
    och, N = 16, 2
    fpn = bare_fpn(och, "skip")
    feats, gouts = fpn_inputs(och, N, "skip")
    rt = FPNRuntime(fpn, torch.device("cuda"))
    cm = [f.cuda() for f in feats]
    outs = fpn_train(cm, fpn, rt)
    torch.autograd.backward(outs, [g.cuda() for g in gouts])
    ws = next(iter(rt._ws.values()))
    assert all(c.grad is None for c in cm)
    assert not any(k.startswith("c") for k in ws["fpn_g"]["buf"]) and not any(k.startswith("inner") for k in ws["fpn_g"]["plan"])
    ref_p = O.fpn_step(feats, dict(fpn.named_parameters()), gouts, torch.float64, feature_grads=False)[1]
    assert all(O.rel_err(p.grad, ref_p[k]) < 1e-4 for k, p in fpn.named_parameters() if ref_p[k] is not None)
    # a backward after a later forward on the same runtime
    first = fpn_train([f.cuda().requires_grad_(True) for f in feats], fpn, rt)
    fpn_train(cm, fpn, rt)
    with pytest.raises(RuntimeError, match="later forward"):
        torch.autograd.backward(first, [g.cuda() for g in gouts])


# ------------------------------------------------------------------------------------------------ 4. DispRCNN, FPN trainable
def test_disprcnn_trains_the_fpn_behind_a_frozen_body():
    import tests.test_hip_srpn_train as SR
    from tests import srpn_train_cases as CS
    from disprcnn_amd.modeling.detector import DispRCNN, default_cfg_2d
    from disprcnn_amd.solver.fused import FusedSGD
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.image_list import to_image_list
    from disprcnn_amd.utils import synth
    n, h, w = 2, 96, 160
    cfg = default_cfg_2d("R-50-FPN")
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TRAIN = 12000
    m = DispRCNN(cfg)
    sd = m.state_dict()
    w_rpn = synth.synth_det_state({k[4:]: v for k, v in sd.items() if k.startswith("rpn.")}, gain={"head.cls_logits.weight": 0.5, "head.bbox_pred.weight": 0.02})
    w_heads = synth.synth_det_state({k[10:]: v for k, v in sd.items() if k.startswith("roi_heads.")}, gain=synth.DET_GAIN)
    bb = synth.synth_backbone_state({k[9:]: v for k, v in sd.items() if k.startswith("backbone.")})
    m.load_state_dict({**{"backbone." + k: v for k, v in bb.items()}, **{"rpn." + k: v for k, v in w_rpn.items()},
                       **{"roi_heads." + k: v for k, v in w_heads.items()}}, strict=True)
    m = m.cuda()
    left, right = synth.synth_images(n, h, w, tag="srpn:det")
    lr = {"left": left.cuda(), "right": right.cuda()}
    lt, rt_ = [], []
    for g in SR.DET_GT:
        masks = np.zeros((len(g), h, w), np.uint8)
        for k, b in enumerate(g.astype(int)):
            masks[k, b[1]: b[3] + 1, b[0]: b[2] + 1] = 1
        l, r = BoxList(SR.cuda(g), (w, h), mode="xyxy"), BoxList(SR.cuda(g + np.array([-4, 0, -4, 0], F32)), (w, h), mode="xyxy")
        l.add_field("labels", torch.ones(len(g), dtype=torch.int64).cuda()), r.add_field("labels", torch.ones(len(g), dtype=torch.int64).cuda())
        l.add_field("masks", SR.cuda(masks))
        lt.append(l), rt_.append(r)
    tg = {"left": lt, "right": rt_}

    # the fully frozen step: the witness
    for p in m.backbone.parameters():
        p.requires_grad_(False)
    m.train()
    total = sum(hh * ww for hh, ww in CS.SHAPES) * CS.A
    d_rpn = SR.uniform("srpn:det:rpn", (n * total,), 0.0, 1.0).cuda()
    li, ri = to_image_list(lr["left"]), to_image_list(lr["right"])
    lf, rf, levels = m.frozen_features(li, ri)
    ws = m.backbone._rt._ws[(2 * n, h, w)]
    assert not ws["s16"]                                        # no layer is bridged to split-f16 at this size
    lp, rp, _ = m.rpn(li, ri, lf, rf, tg["left"], tg["right"], blocked_levels=levels, draws=d_rpn)
    d_sample = SR.uniform("srpn:det:sample", (sum(len(b) for b in lp),), 0.0, 1.0).cuda()
    x, _, _, _ = m.roi_heads.box({"left": lf, "right": rf}, {"left": lp, "right": rp}, tg, draws={"sample": d_sample})
    draws = {"rpn_sample": d_rpn, "sample": d_sample, "dropout": SR.uniform("srpn:det:drop", (2, x.shape[0], 64), 0.0, 1.0).cuda()}
    m.zero_grad(set_to_none=True)
    frozen = m(lr, tg, draws=draws)
    sum(frozen.values()).backward()
    frozen_grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert frozen_grads and not any(k.startswith("backbone.") for k in frozen_grads)

    # the FPN trainable behind the frozen body
    for p in m.backbone.fpn.parameters():
        p.requires_grad_(True)
    m.backbone.freeze_body()
    m.train()
    assert m.backbone.training and not m.backbone.body.training
    m.zero_grad(set_to_none=True)
    kept = {}

    def retain(module, args, outs):                             # the detector slices the five maps: their gradients are taken at the backbone
        for o in outs:
            o.retain_grad()
        kept["outs"] = outs
    hook = m.backbone.register_forward_hook(retain)
    try:
        losses = m(lr, tg, draws=draws)
    finally:
        hook.remove()
    keys = {"loss_classifier", "loss_box_reg", "loss_mask", "loss_objectness", "loss_rpn_box_reg"}
    assert set(losses) == keys
    for k in keys:
        print(k, losses[k].item())
        assert torch.equal(losses[k], frozen[k]), k             # the same maps, the same draws: the same bits
    assert all(o.requires_grad for o in kept["outs"])
    sum(losses.values()).backward()
    named = dict(m.named_parameters())
    for k, p in named.items():
        if k.startswith("backbone.body."):
            assert p.grad is None, k
        elif k.startswith("backbone.fpn."):
            assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
            if k.startswith("backbone.fpn.fpn_layer4"):         # unused by the fork's forward (fpn.py:54-55): outside the graph
                assert not p.grad.any().item(), k
        else:
            assert torch.equal(p.grad, frozen_grads[k]), k      # the RPN's and the heads' gradients: the frozen step's, bit for bit
    used_weights = [k for k in named if k.startswith("backbone.fpn.") and k.endswith(".weight") and "fpn_layer4" not in k]
    assert len(used_weights) == 7 and all(named[k].grad.any().item() for k in used_weights)

    # the FPN's parameter gradients against the fp64 oracle, from the gradients that reached the five maps and the workspace's C maps
    t = ws["t"]
    cmaps = [t[name].to_dense()[:, :, 0].cpu() for name, _, _ in ws["stage_out"]]
    gouts = [o.grad.cpu() for o in kept["outs"]]
    fp = {k: v for k, v in m.backbone.fpn.named_parameters()}
    ref_p = O.fpn_step(cmaps, fp, gouts, torch.float64, feature_grads=False)[1]
    t32_p = O.fpn_step(cmaps, fp, gouts, torch.float32, feature_grads=False)[1]
    table, ok = [], True
    print("DispRCNN step, FPN parameter gradients: max|x - oracle| / max|oracle|")
    for k in O.PARAM_NAMES:
        if ref_p[k] is not None:
            ok &= check_rule(k, fp[k].grad, t32_p[k], ref_p[k], table)
    assert ok

    before = {k: p.detach().clone() for k, p in named.items() if k.startswith("backbone.")}
    FusedSGD([p for p in m.parameters() if p.requires_grad], lr=0.02, momentum=0.9).step()
    for k, p in named.items():
        if k.startswith("backbone.body."):
            assert torch.equal(p, before[k]), k
        elif k.startswith("backbone.fpn.") and "fpn_layer4" not in k:
            assert not torch.equal(p, before[k]), k

"""The ResNet body's training form on the MI355X: the 1x1 weight-gradient GEMM against an fp64 einsum, one BottleneckUnit and the R-50
body against torch-CPU fp64 autograd (with torch-CPU fp32 autograd as the yardstick), DispRCNN's training step with the body opted in,
and the eval form of an opted-in backbone.

Tolerance rule of the unit / body tests (per tensor, from tests/test_hip_fpn_train.py): e = max|x - oracle| / max|oracle|; the HIP value
must be <= max(4 * e(torch-CPU fp32), 1e-6), and e(torch-CPU fp32) <= 1e-5 is asserted first: a ReLU mask that flips between fp32 and
fp64 shows as a large e_fp32 and must not widen the bound (tests/body_train_oracle.py says how the inputs were chosen, and why the body
case reads its e_fp32 from a record instead of running torch's fp32 step on whatever CPU the test runs on).

Bound of the kernel test (per element): the GEMM form adds at most `chunk` products in an fp32 fma chain -- one rounding of at most
2^-24 of the running magnitude per term -- then the partials in fp64, rounded once: |err| <= (min(chunk, P) + 2) * 2^-24 * sum|a*b|.
The tap form adds the P products of a tile walk in fp32 and its partials in fp64: (P + 2) * 2^-24 * sum|a*b|."""
import numpy as np
import pytest
import torch

from tests import body_train_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """The R-50 cases leave large free blocks in torch's caching allocator; a later test that measures its peak allocation would be served
    from them (an oversize block counts whole).  Hand them back when this module is done."""
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


F32 = np.float32
SENTINEL = np.float32(-1234.5)
DEV = "cuda"


def E():
    from disprcnn_amd import engine
    return engine


def BT():
    from disprcnn_amd.modeling.backbone import body_train
    return body_train


def blocked(dense, pad, lanes=None):
    """A Blocked tensor holding `dense`, every halo word SENTINEL; lanes: the value of the padded channel lanes of the interior."""
    n, c, h, w = dense.shape
    b = E().Blocked(n, c, 1, h, w, 0, pad, pad, torch.device(DEV))
    if n:
        b.storage[: b.numel].fill_(float(SENTINEL))
        b.from_dense(torch.from_numpy(dense).to(DEV))
        if lanes is not None and c % 16:
            b.view6()[:, -1, :, pad: pad + h, pad: pad + w, c % 16:] = lanes
    return b


def check_rule(what, hip, t32, ref, lines):
    """t32: the torch-CPU fp32 value, or its recorded e_fp32 (a float)"""
    e_hip, e_32 = O.rel_err(hip, ref), (t32 if isinstance(t32, float) else O.rel_err(t32, ref))
    lines.append(f"  {what:32s} hip {e_hip:.3e}   torch-fp32 {e_32:.3e}")
    return e_32 <= O.E32_MAX and e_hip <= max(4 * e_32, 1e-6)


def report(title, lines, ok):
    print(title)
    for ln in lines if not ok else lines[:8]:
        print(ln)


# ------------------------------------------------------------------------------------------------ 1. the 1x1 weight gradient
CHANNELS = [(24, 40), (16, 16), (80, 8), (33, 47)]                       # (cin, cout): one, odd and ragged block counts: a 32-wide tile half empty
MAPS = [(5, 7), (6, 6)]
N_UNITS = 3


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", MAPS)
def test_conv1x1_wgrad_against_fp64_einsum(cin, cout, stride, hw):
    bt = BT()
    h, w = hw
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    a = O.seeded((N_UNITS, cin, h, w), "k:a", cin, cout, stride, hw)
    b = O.seeded((N_UNITS, cout, oh, ow), "k:b", cin, cout, stride, hw)
    ref, mag = O.wgrad_1x1(a, b, stride)
    P = N_UNITS * oh * ow
    # one pixel below a chunk, exactly one chunk, one above; many chunks (P of them: more than the finishing launch has threads per
    # element to spare); the library's default
    chunks = [P + 1, P, P - 1, 4, 1, None]
    worst, got_default = 0.0, {}
    for pa, pb in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ab, bb = blocked(a, pa, lanes=7.0), blocked(b, pb, lanes=-3.0)   # halos hold the sentinel, padded lanes garbage: neither may reach gw
        for chunk in chunks:
            g1 = bt.conv1x1_wgrad(ab, bb, cin, cout, stride, kernel="gemm", chunk=chunk)
            g2 = bt.conv1x1_wgrad(ab, bb, cin, cout, stride, kernel="gemm", chunk=chunk)
            assert g1.shape == (cout, cin) and torch.equal(g1, g2)                               # the same bits run to run
            k = min(chunk or 512, P)
            err = np.abs(g1.cpu().numpy().astype(np.float64) - ref)
            bound = (k + 2) * 2.0 ** -24 * mag
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (pa, pb, chunk, float(err.max()))
            if chunk is None:
                got_default[(pa, pb)] = g1
        tap = bt.conv1x1_wgrad(ab, bb, cin, cout, stride, kernel="tap")
        assert tap.shape == (cout, cin) and torch.equal(tap, bt.conv1x1_wgrad(ab, bb, cin, cout, stride, kernel="tap"))
        err_t = np.abs(tap.cpu().numpy().astype(np.float64) - ref)
        assert (err_t <= (P + 2) * 2.0 ** -24 * mag).all(), (pa, pb, "tap", float(err_t.max()))
        # the two forms against each other: each within its own bound of the same oracle
        both = np.abs(tap.cpu().numpy().astype(np.float64) - got_default[(pa, pb)].cpu().numpy().astype(np.float64))
        assert (both <= (2 * P + 4) * 2.0 ** -24 * mag).all()
    vals = list(got_default.values())
    assert all(torch.equal(vals[0], v) for v in vals[1:])                                        # the halo does not change a bit
    print(f"conv1x1_wgrad cin {cin} cout {cout} stride {stride} map {hw}: worst err / bound {worst:.3f}")


def test_conv1x1_wgrad_empty_batch_and_bad_arguments():
    bt, e = BT(), E()
    dev = torch.device(DEV)
    for kernel in ("gemm", "tap"):
        a0, b0 = e.Blocked(0, 24, 1, 5, 7, 0, 0, 0, dev), e.Blocked(0, 40, 1, 3, 4, 0, 1, 1, dev)
        g = bt.conv1x1_wgrad(a0, b0, 24, 40, 2, kernel=kernel)
        assert g.shape == (40, 24) and not g.any().item()
    a = blocked(O.seeded((2, 24, 5, 7), "bad:a"), 0)
    b = blocked(O.seeded((2, 40, 5, 7), "bad:b"), 0)
    with pytest.raises(ValueError, match="shape of the stride-s"):
        bt.conv1x1_wgrad(a, b, 24, 40, 2)
    with pytest.raises(ValueError, match="do not fit"):
        bt.conv1x1_wgrad(a, b, 40, 40, 1)
    with pytest.raises(ValueError, match="stride"):
        bt.conv1x1_wgrad(a, b, 24, 40, 3)
    with pytest.raises(ValueError, match="chunk"):
        bt.conv1x1_wgrad(a, b, 24, 40, 1, kernel="gemm", chunk=0)
    with pytest.raises(ValueError, match="'gemm' or 'tap'"):
        bt.conv1x1_wgrad(a, b, 24, 40, 1, kernel="mfma")
    # the C entry itself: a scratch that is too small is refused before any launch
    from disprcnn_amd.pts import _lib as P
    gw = torch.full((40, 24), 5.0, device=DEV)
    scr = torch.zeros(40 * 24, device=DEV)
    st = P.lib().drc_conv1x1_wgrad_blocked(e._ptr(a.storage), a.n_stride, a.cb_stride, a.h_stride, a.interior_off, e._ptr(b.storage), b.n_stride,
                                           b.cb_stride, b.h_stride, b.interior_off, 2, 5, 7, 24, 40, 1, 36, e._ptr(gw), e._ptr(scr), scr.numel(),
                                           e._stream_ptr(dev))
    torch.cuda.synchronize()
    assert st == -3 and (gw == 5.0).all().item()
    st = P.lib().drc_conv1x1_wgrad_blocked(e._ptr(a.storage), a.n_stride, a.cb_stride, a.h_stride, a.interior_off, e._ptr(b.storage), b.n_stride,
                                           b.cb_stride, b.h_stride, b.interior_off, 2, 5, 7, 24, 40, 3, 36, e._ptr(gw), e._ptr(scr), scr.numel(),
                                           e._stream_ptr(dev))
    assert st == -2


# ------------------------------------------------------------------------------------------------ 2. one BottleneckUnit
@pytest.mark.parametrize("name", sorted(O.UNIT_CASES))
@pytest.mark.parametrize("kernel", ["gemm", "tap", "auto"])
def test_bottleneck_unit_against_fp64_autograd(name, kernel, monkeypatch):
    bt = BT()
    monkeypatch.setitem(bt.WGRAD_1X1, "kernel", kernel)
    r64, r32 = O.unit_reference(name)
    u, x, g = O.make_unit(name)
    u = u.to(DEV)
    rt = bt.UnitRuntime(u, torch.device(DEV))

    def step():
        u.zero_grad(set_to_none=True)
        xi = x.to(DEV).requires_grad_(True)
        y = rt.forward_train(xi)
        y.backward(g.to(DEV))
        return y.detach(), xi.grad, {k: p.grad.clone() for k, p in u.named_parameters()}
    y, gx, pg = step()
    bufs = {k: v.detach().cpu().clone() for k, v in u.named_buffers()}
    lines, ok = [], True
    ok &= check_rule("out", y, r32[0], r64[0], lines)
    ok &= check_rule("grad_in", gx, r32[1], r64[1], lines)
    for k in r64[2]:
        assert pg[k].shape == r64[2][k].shape, k
        ok &= check_rule(k, pg[k], r32[2][k], r64[2][k], lines)
    for k, v in r64[3].items():
        if v.is_floating_point():
            ok &= check_rule(k, bufs[k], r32[3][k], v, lines)
        else:
            assert int(bufs[k]) == 1, k                                                          # num_batches_tracked
    report(f"unit {name} ({kernel}): max|x - oracle| / max|oracle|", lines, ok)
    assert ok
    y2, gx2, pg2 = step()                                                                       # the same bits run to run
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and all(torch.equal(pg[k], pg2[k]) for k in pg)


# ------------------------------------------------------------------------------------------------ 3. the R-50 body
def make_backbone(freeze_at=None):
    from disprcnn_amd.modeling.backbone.backbone import ResNetFPNBackbone
    body, x, gouts = O.make_body()
    bb = ResNetFPNBackbone("R-50")
    bb.body.load_state_dict(body.state_dict(), strict=True)
    with torch.no_grad():
        for name, p in bb.fpn.named_parameters():
            p.copy_(torch.from_numpy(O.seeded(tuple(p.shape), "fpn", name, scale=0.5 if name.endswith("bias") else (2.0 / p[0].numel()) ** 0.5)))
    if freeze_at is not None:
        bb.enable_body_training(freeze_at)
    return bb.to(DEV), x, gouts


@pytest.mark.parametrize("freeze_at", [2, 4])
def test_body_against_fp64_autograd(freeze_at):
    from disprcnn_amd.modeling.backbone.runtime import BackboneRuntime
    bt = BT()
    r64, rec = O.body_reference()[0], O.recorded_e32()           # the yardstick: e_fp32 per tensor as recorded (body_train_oracle.py says why)
    bb, x, gouts = make_backbone(freeze_at)
    bb.train()
    rt = BackboneRuntime(bb, torch.device(DEV))
    first_stage = freeze_at - 1 if freeze_at > 1 else 0         # index of the first C map the Function produces

    def step():
        bb.zero_grad(set_to_none=True)
        ws, n, cmaps = bt.forward_cmaps(rt, x.to(DEV))
        assert n == O.BODY_N and [c is not None for c in cmaps] == [i >= first_stage for i in range(4)]
        dense = [ws["t"][name].to_dense()[:, :, 0] for name, _, _ in ws["stage_out"]]
        live = [(c, g) for c, g in zip(cmaps, gouts) if c is not None]
        assert all(c.requires_grad for c, _ in live) and all(torch.equal(c, d) for c, d in zip(cmaps, dense) if c is not None)
        return dense, live
    dense, live = step()
    bufs = {k: v.detach().cpu().clone() for k, v in bb.body.named_buffers()}
    torch.autograd.backward([c for c, _ in live], [g.to(DEV) for _, g in live])
    pg = {k: (None if p.grad is None else p.grad.clone()) for k, p in bb.body.named_parameters()}
    lines, ok = [], True
    for i in range(4):
        ok &= check_rule(f"C{i + 2}", dense[i], rec[f"C{i + 2}"], r64[0][i], lines)
    trainable = tuple(f"layer{li}." for li in range(freeze_at, 5))
    for k, ref in r64[1].items():
        if not k.startswith(trainable):
            assert pg[k] is None, k                             # frozen: no gradient
            continue
        assert pg[k] is not None and pg[k].shape == ref.shape, k
        ok &= check_rule(k, pg[k], rec[k], ref, lines)
    for k, v in r64[2].items():                                 # the running statistics of ALL BatchNorms, the stem's and layer1's included
        if v.is_floating_point():
            ok &= check_rule(k, bufs[k], rec[k], v, lines)
        else:
            assert int(bufs[k]) == 1, k
    report(f"R-50 body, freeze_at {freeze_at}: max|x - oracle| / max|oracle| over {len(lines)} tensors", lines, ok)
    assert ok
    # a second step from the same inputs: the same bits (the batch statistics do not read the running ones)
    dense2, live2 = step()
    torch.autograd.backward([c for c, _ in live2], [g.to(DEV) for _, g in live2])
    assert all(torch.equal(a, b) for a, b in zip(dense, dense2))
    assert all(pg[k] is None or torch.equal(pg[k], p.grad) for k, p in bb.body.named_parameters())
    assert all(int(v) == 2 for k, v in bb.body.named_buffers() if k.endswith("num_batches_tracked"))
    # a backward after a later forward on the same runtime
    _, stale = step()
    step()
    with pytest.raises(RuntimeError, match="later forward"):
        torch.autograd.backward([c for c, _ in stale], [g.to(DEV) for _, g in stale])


def test_backbone_forward_trains_body_and_fpn_and_refuses_an_eval_batchnorm():
    bb, x, _ = make_backbone(3)
    bb.train()
    outs = bb(x.to(DEV))
    assert len(outs) == 5 and all(o.requires_grad for o in outs)
    sum((o * o).sum() for o in outs).backward()
    for k, p in bb.named_parameters():
        frozen = k.startswith(("body.stem.", "body.layer1.", "body.layer2."))
        assert (p.grad is None) == frozen, k
        if not frozen and "fpn_layer4" not in k:
            assert torch.isfinite(p.grad).all().item() and p.grad.any().item(), k
    # a later eval forward of the runtime, then the stale backward
    outs = bb(x.to(DEV))
    with torch.no_grad():
        bb.eval()(x.to(DEV))
    bb.train()
    with pytest.raises(RuntimeError, match="later forward"):
        sum(o.sum() for o in outs).backward()
    # the folded form is allowed in the frozen prefix only
    bb.body.layer1.eval()
    outs = bb(x.to(DEV))
    assert all(torch.isfinite(o).all().item() for o in outs)
    bb.body.layer3[1].bn2.eval()
    with pytest.raises(NotImplementedError, match="eval mode behind a trainable parameter"):
        bb(x.to(DEV))
    # under no_grad nothing is taped
    bb.train()
    with torch.no_grad():
        assert not any(o.requires_grad for o in bb(x.to(DEV)))


def test_eval_forward_of_an_opted_in_backbone_is_unchanged():
    plain, x, _ = make_backbone(None)
    opted, _, _ = make_backbone(2)
    opted.train()
    plain.eval(), opted.eval()
    with torch.no_grad():
        a, b = plain(x.to(DEV)), opted(x.to(DEV))
    assert len(a) == 5 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert not any(o.requires_grad for o in b)


# ------------------------------------------------------------------------------------------------ 4. DispRCNN, body opted in
def test_disprcnn_trains_the_body_after_the_opt_in():
    import tests.test_hip_srpn_train as SR
    from tests import srpn_train_cases as CS
    from disprcnn_amd.modeling.detector import DispRCNN, default_cfg_2d
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
    state = {**{"backbone." + k: v for k, v in bb.items()}, **{"rpn." + k: v for k, v in w_rpn.items()},
             **{"roi_heads." + k: v for k, v in w_heads.items()}}
    state = {k: v.clone() for k, v in state.items()}
    m.load_state_dict(state, strict=True)
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

    # one step with the body opted in (the sizes of the draws depend on the proposals: the samplers draw for themselves)
    m.backbone.enable_body_training(2)
    m.train()
    assert m.backbone.body.training
    m.zero_grad(set_to_none=True)
    torch.manual_seed(0)
    losses = m(lr, tg)
    keys = {"loss_classifier", "loss_box_reg", "loss_mask", "loss_objectness", "loss_rpn_box_reg"}
    assert set(losses) == keys
    for k in keys:
        print(k, losses[k].item())
        assert torch.isfinite(losses[k]).item(), k
    sum(losses.values()).backward()
    for k, p in m.named_parameters():
        if k.startswith(("backbone.body.stem.", "backbone.body.layer1.")):
            assert p.grad is None, k
        elif k.startswith("backbone.fpn.fpn_layer4"):           # unused by the fork's forward (fpn.py:54-55): a zero gradient
            assert p.grad is not None and not p.grad.any().item(), k
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all().item() and p.grad.any().item(), k
    assert all(int(v) == 1 for k, v in m.backbone.body.named_buffers() if k.endswith("num_batches_tracked"))

    # the same model, reloaded and frozen again, against a model that was never opted in: today's FPN-training step, bit for bit
    def fpn_step(model, draws):
        model.load_state_dict(state, strict=True)
        model.backbone.freeze_body()
        model.train()
        model.zero_grad(set_to_none=True)
        out = model(lr, tg, draws=draws)
        sum(out.values()).backward()
        return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    witness = DispRCNN(cfg)
    witness.load_state_dict(state, strict=True)
    witness = witness.cuda()
    witness.backbone.freeze_body()
    witness.train()
    total = sum(hh * ww for hh, ww in CS.SHAPES) * CS.A
    d_rpn = SR.uniform("srpn:det:rpn", (n * total,), 0.0, 1.0).cuda()
    li, ri = to_image_list(lr["left"]), to_image_list(lr["right"])
    lf, rf, levels = witness.frozen_features(li, ri)
    lp, rp, _ = witness.rpn(li, ri, lf, rf, tg["left"], tg["right"], blocked_levels=levels, draws=d_rpn)
    d_sample = SR.uniform("srpn:det:sample", (sum(len(b) for b in lp),), 0.0, 1.0).cuda()
    x, _, _, _ = witness.roi_heads.box({"left": lf, "right": rf}, {"left": lp, "right": rp}, tg, draws={"sample": d_sample})
    draws = {"rpn_sample": d_rpn, "sample": d_sample, "dropout": SR.uniform("srpn:det:drop", (2, x.shape[0], 64), 0.0, 1.0).cuda()}
    want, want_g = fpn_step(witness, draws)
    got, got_g = fpn_step(m, draws)
    assert not m.backbone._body_training and not m.backbone.body.training
    assert all(torch.equal(got[k], want[k]) for k in keys)
    assert set(got_g) == set(want_g) and not any(k.startswith("backbone.body.") for k in got_g)
    # the losses and the RPN's / the heads' gradients: the same bits.  The gradients that reach the five maps come out of ROIAlign's
    # adjoint, an atomicAdd scatter whose order changes run to run, so the FPN's parameter gradients repeat to rounding only -- today as
    # well (tests/test_hip_fpn_train.py compares them to an oracle, not to a second run): 1e-4 of the largest entry, as its skip test asks
    differ = [k for k in want_g if not torch.equal(got_g[k], want_g[k])]
    print("gradients that differ in bits from the never-opted-in model's:", differ)
    assert all(k.startswith("backbone.fpn.") for k in differ)
    for k in differ:
        assert O.rel_err(got_g[k], want_g[k]) < 1e-4, k

"""The stereo ROI heads' training step on the GPU: the new kernels at their edges (drc_linear_pack_cols, drc_relu_dropout_fwd,
drc_act_bwd_rows, drc_act_bwd_blocked, drc_roi_align_fpn_bwd), the linear training Function, and the box head, the mask head and
StereoCombinedROIHeads end to end against tests/roi_heads_train_oracle.py (held to the reference's recorded step and to torch's layers
by tests/test_roi_heads_train_host.py, which also holds every case here to its ReLU margin, so no gradient element is excluded).

Bounds.  Elementwise results (pack_cols, dz): bit-exact.  Bias gradients: 2 e32 + 1e-6 max|ref64|, e32 the oracle's own fp32-vs-fp64
error.  One pass through the GEMM: 2e-5 max|ref| + 1e-6, the bound tests/test_hip_detector2d.py grants this kernel.  End-to-end losses and
gradients: 2 e32 + 2e-5 max|ref64| -- the chain's fp32 conditioning plus one GEMM pass.  Everything but the feature-map gradients
(atomicAdd) must have the same bits on a second run.
"""
import numpy as np
import pytest
import torch

from tests import roi_heads_train_cases as CS
from tests import roi_heads_train_oracle as TO
from tests import roi_stage_oracle as RO
from tests.helpers import golden_npz

pytestmark = pytest.mark.gpu
F32 = np.float32


def H():
    from disprcnn_amd.modeling import head_ops
    return head_ops


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def uniform(key, shape, lo=-1.0, hi=1.0):
    from disprcnn_amd.utils.synth import hash_uniform
    return hash_uniform(key, shape, lo, hi)


def check(got, ref64, ref32, what, rel=2e-5):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    e32 = np.abs(np.asarray(ref32, np.float64) - ref64).max(initial=0.0)
    err, mag = np.abs(got - ref64).max(initial=0.0), np.abs(ref64).max(initial=0.0)
    bound = 2 * e32 + rel * mag
    print(f"{what}: err {err:.3g} e32 {e32:.3g} bound {bound:.3g} (|ref| <= {mag:.3g})")
    assert np.isfinite(got).all() and err <= bound, what


# ------------------------------------------------------------------------------------------------ 1. pack_cols
@pytest.mark.parametrize("R,K", [(1, 1), (37, 72), (130, 784), (16, 16), (0, 8)])
def test_pack_cols_is_pack_rows_of_the_transpose(R, K):
    a = uniform(f"pc{R}x{K}", (R, K)).cuda()
    got = H()._pack_cols(a)
    if R == 0:
        assert got.numel() == 0
        return
    want = H()._pack_rows(a.t().contiguous())
    assert got.shape == want.shape and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 2. activation backward
def act_inputs(tag, shape, p):
    dy = uniform(tag + ":dy", shape, -2.0, 2.0)
    y = torch.relu(uniform(tag + ":y", shape, -1.0, 1.0))
    y.view(-1)[3::7] = 0.0                                                      # exact zeros: no gradient passes
    draws = uniform(tag + ":u", shape, 0.0, 1.0)
    draws.view(-1)[::5] = float(np.float32(p))                                  # a draw exactly equal to p is kept
    return dy, y, draws


@pytest.mark.parametrize("relu,p", [(1, 0.2), (1, 0.0), (0, 0.0), (0, 0.5)])
@pytest.mark.parametrize("N", [5, 72, 128])
@pytest.mark.parametrize("M", [1, 37, 130, 260])
def test_act_bwd_rows(M, N, relu, p):
    dy, y, draws = act_inputs(f"ab{M}x{N}", (M, N), p)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    mask = torch.ones(M, N, dtype=torch.bool)
    if relu:
        mask &= y > 0
    if p > 0:
        mask &= draws >= float(np.float32(p))
    scaled = torch.from_numpy((dy.numpy() * scale).astype(F32)) if p > 0 else dy          # one fp32 product with the fp32 1 / (1 - p)
    want = torch.where(mask, scaled, torch.zeros(()))
    dz, db = H().act_bwd_rows(dy.cuda(), y.cuda(), draws.cuda(), p, relu)
    assert torch.equal(dz.cpu(), want), "dz differs from the fp32 formula"
    assert p == 0 or M * N < 37 or (draws == float(np.float32(p)))[mask].any()       # kept draws that equal p exist
    ref64, ref32 = want.double().sum(0).numpy(), want.sum(0).numpy()
    e32 = np.abs(ref32 - ref64).max()
    err = np.abs(host(db).astype(np.float64) - ref64).max()
    print(f"db: err {err:.3g} e32 {e32:.3g}")
    assert err <= 2 * e32 + 1e-6 * np.abs(ref64).max()
    dz2, db2 = H().act_bwd_rows(dy.cuda(), y.cuda(), draws.cuda(), p, relu)
    assert torch.equal(db, db2) and torch.equal(dz, dz2)
    if N % 4 == 0:                                                              # the 2x2 deconvolution's fold: 4 columns per bias entry
        _, dbf = H().act_bwd_rows(dy.cuda(), y.cuda(), draws.cuda(), p, relu, fold=4)
        r64 = ref64.reshape(-1, 4).sum(1)
        assert np.abs(host(dbf).astype(np.float64) - r64).max() <= 2 * np.abs(want.sum(0).view(-1, 4).sum(1).numpy() - r64).max() + 1e-6 * np.abs(r64).max()


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("units", [1, 5])
@pytest.mark.parametrize("C", [16, 24, 32])
def test_act_bwd_blocked(C, units, relu):
    from disprcnn_amd import engine as E
    dy, y, _ = act_inputs(f"abb{C}x{units}", (units, C, 14, 14), 0.0)
    dev = torch.device("cuda")
    mk = lambda: E.Blocked(units, C, 1, 14, 14, 0, 1, 1, dev)
    bdy, by, bdz = mk().from_dense(dy.cuda()), mk().from_dense(y.cuda()), mk()
    _, db = H().act_bwd_blocked(bdy, by, relu, bdz)
    want = torch.where(y > 0, dy, torch.zeros(())) if relu else dy
    assert torch.equal(bdz.to_dense()[:, :, 0].cpu(), want), "dz differs from the fp32 formula"
    full = bdz.storage[: bdz.numel].view(units, bdz.cb, 16, 16, 16)
    assert not full[:, :, 0].any() and not full[:, :, -1].any() and not full[:, :, :, 0].any() and not full[:, :, :, -1].any(), "halo written"
    ref64, ref32 = want.double().sum((0, 2, 3)).numpy(), want.sum((0, 2, 3)).numpy()
    err, e32 = np.abs(host(db).astype(np.float64) - ref64).max(), np.abs(ref32 - ref64).max()
    print(f"db: err {err:.3g} e32 {e32:.3g}")
    assert db.shape == (C,) and err <= 2 * e32 + 1e-6 * np.abs(ref64).max()
    _, db2 = H().act_bwd_blocked(bdy, by, relu, mk())
    assert torch.equal(db, db2)


@pytest.mark.parametrize("relu,p", [(1, 0.2), (1, 0.0), (0, 0.5)])
def test_relu_dropout_forward(relu, p):
    x = uniform("rd:x", (37, 72), -1.0, 1.0)
    draws = uniform("rd:u", (37, 72), 0.0, 1.0)
    draws.view(-1)[::5] = float(np.float32(p))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    v = torch.relu(x) if relu else x
    want = torch.where(draws >= float(np.float32(p)), torch.from_numpy((v.numpy() * scale).astype(F32)), torch.zeros(())) if p > 0 else v
    got = H().relu_dropout(x.cuda().clone(), draws.cuda(), p, relu)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ 3. the linear training Function
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N,K", [(130, 70, 36), (37, 72, 784), (260, 72, 72), (1, 5, 20), (0, 8, 16)])
def test_linear_train_function(M, N, K, bias):
    lin = torch.nn.Linear(K, N, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(uniform(f"lt{M}{N}{K}:w", (N, K)) / K ** 0.5)
        if bias:
            lin.bias.copy_(uniform(f"lt{N}:b", (N,), -0.5, 0.5))
    lin = lin.cuda()
    x0, g0 = uniform(f"lt{M}{K}:x", (M, K)), uniform(f"lt{M}{N}:g", (M, N))

    def run(need_x=True):
        lin.zero_grad()
        x = x0.cuda().requires_grad_(need_x)
        y = H().linear_train(x, lin, relu=True)
        y.backward(g0.cuda())
        return y.detach().cpu(), x.grad, lin.weight.grad.cpu().clone(), lin.bias.grad.cpu().clone() if bias else None

    y, dx, dw, db = run()
    xd = x0.double().requires_grad_()
    wd = lin.weight.detach().cpu().double().requires_grad_()
    bd = lin.bias.detach().cpu().double().requires_grad_() if bias else None
    z = xd @ wd.t() + (bd if bias else 0.0)
    yd = torch.relu(z)
    yd.backward(g0.double())
    assert y.shape == (M, N) and dw.shape == (N, K) and dx.shape == (M, K)
    if M == 0:
        assert not dw.any() and (db is None or not db.any())
        return
    assert float(z.detach().abs().min()) > 1e-6 * float(z.detach().abs().max()), "a ReLU input of this case sits on zero"
    close = lambda got, ref: (got.double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-6
    assert close(y, yd.detach()) and close(dx.cpu(), xd.grad) and close(dw, wd.grad)
    if bias:
        dz32 = torch.where(yd.detach() > 0, g0, torch.zeros(()))
        e32 = (dz32.sum(0).double() - bd.grad).abs().max().item()
        assert (db.double() - bd.grad).abs().max().item() <= 2 * e32 + 1e-6 * bd.grad.abs().max().item()
    y2, dx2, dw2, db2 = run()
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))
    _, dx3, dw3, _ = run(need_x=False)
    assert dx3 is None and torch.equal(dw, dw3)


def test_linear_train_skips_the_data_gradient_gemm(monkeypatch):
    """x.requires_grad = False: no dX is produced -- the backward makes two pack_cols calls (dZ^T, X^T) and none of W^T"""
    lin = torch.nn.Linear(36, 70).cuda()
    calls = []
    real = H()._pack_cols
    monkeypatch.setattr(H(), "_pack_cols", lambda a: (calls.append(tuple(a.shape)), real(a))[1])
    for need in (False, True):
        calls.clear()
        H().clear_packed_weights(lin)
        x = uniform("skip:x", (130, 36)).cuda().requires_grad_(need)
        H().linear_train(x, lin, relu=True).sum().backward()
        assert ((70, 36) in calls) == need and (130, 70) in calls and (130, 36) in calls


def test_dropout_draws_default_to_one_rand_call():
    lin = torch.nn.Linear(36, 72).cuda()
    x = uniform("dd:x", (130, 36)).cuda()
    y = H().linear_train(x, lin, relu=True, p=0.2)
    dead = ((y == 0) & (H().linear(x, lin, relu=True) > 0)).float().sum().item() / max(1.0, (H().linear(x, lin, relu=True) > 0).float().sum().item())
    assert 0.15 < dead < 0.25                                                   # nn.Dropout's distribution (4 700 trials at p = 0.2: sigma 0.006)


# ------------------------------------------------------------------------------------------------ 4. ROIAlign pyramid backward
FPN_SHAPES, FPN_C, FPN_IMG_H = [(24, 40), (12, 20), (6, 10), (3, 5)], 8, 96
FPN_BOXES = [np.array([[10, 12, 40, 44], [60, 20, 150, 90], [-30, -20, 200, 180], [-150, -180, 330, 290],     # levels 0, 1, 2, 3
                       [140, 80, 190, 120],                                                                    # sample points beyond the map
                       [50, 50, 40, 45]], F32),                                                                # malformed: forced to 1 x 1
             np.array([[30, 30, 75, 70], [20, 5, 130, 95], [100, 60, 530, 460], [0, 0, 159, 95]], F32)]


def boxlists(boxes, size, **fields):
    from disprcnn_amd.structures.bounding_box import BoxList
    out = []
    for i, b in enumerate(boxes):
        bl = BoxList(cuda(np.asarray(b, F32).reshape(-1, 4)), size, mode="xyxy")
        for k, v in fields.items():
            bl.add_field(k, cuda(v[i]))
        out.append(bl)
    return out


@pytest.mark.parametrize("single_launch", [True, False])
@pytest.mark.parametrize("res,sr", [(7, 0), (14, 2)])
def test_fpn_roi_align_backward(res, sr, single_launch, monkeypatch):
    from disprcnn_amd.modeling.poolers import Pooler
    feats = [uniform(f"fpnb:L{l}", (2, FPN_C, h, w), -1.7, 1.7) for l, (h, w) in enumerate(FPN_SHAPES)]
    rois = TO.rois_of(FPN_BOXES)
    levels = TO.levels_of(rois[:, 1:])
    assert set(levels) == {0, 1, 2, 3} and set(rois[:, 0]) == {0.0, 1.0}
    gout = uniform(f"fpnb:g{res}", (len(rois), FPN_C, res, res), -1.0, 1.0)
    pooler = Pooler((res, res), (0.25, 0.125, 0.0625, 0.03125), sr)
    pooler.single_launch = single_launch
    fdev = [f.cuda().requires_grad_() for f in feats]
    syncs = []
    real = torch.nonzero
    monkeypatch.setattr(torch, "nonzero", lambda *a, **k: (syncs.append(1), real(*a, **k))[1])
    out = pooler(fdev, boxlists(FPN_BOXES, (160, 96)))
    out.backward(gout.cuda())
    monkeypatch.undo()
    # the code path, not a timer: the one-launch path goes through the autograd Function and never asks for nonzero (the host read of the loop)
    assert pooler.last_path == ("fpn_autograd" if single_launch else "per_level") and (len(syncs) == 0) == single_launch
    for lv, f in enumerate(feats):
        idx = np.nonzero(levels == lv)[0]
        scale = f.shape[2] / FPN_IMG_H
        fwd, _ = RO.roi_align_fwd64(f.numpy(), rois[idx], scale, res, res, sr)
        ref, mag, cnt = RO.roi_align_bwd64(gout.numpy()[idx], rois[idx], scale, res, res, sr, tuple(f.shape), np.zeros(tuple(f.shape)))
        err = np.abs(host(fdev[lv].grad).astype(np.float64) - ref)
        bound = RO.bwd_bound(mag, cnt)
        assert np.abs(ref).max() > 0 and (err <= bound).all(), (lv, float((err - bound).max()))
        assert np.abs(host(out)[idx] - fwd).max() <= 1e-5
    g = RO.roi_geometry(rois[4], 0.25, res, res, sr, 24, 40)
    assert g["dead"].any() and not g["dead"].all()                              # the roi that reaches beyond its map
    assert rois[5][3] < rois[5][1] and rois[5][4] < rois[5][2]


# ------------------------------------------------------------------------------------------------ 5. the box head
def box_cfg(dim=CS.BOX_DIM, batch=CS.BOX_BATCH, channels=(CS.MASK_C,) * 4):
    from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d
    cfg = default_cfg_2d()
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = dim
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = batch
    cfg.MODEL.ROI_MASK_HEAD.CONV_LAYERS = channels
    return cfg


def load(module, params, prefix=""):
    module.load_state_dict({prefix + k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return module.cuda().train()


def param_grads(module, names, prefix=""):
    named = dict(module.named_parameters())
    return {k: named[prefix + k].grad.detach().cpu().clone() for k in names}


def golden_case():
    from tests.test_roi_heads_train_host import golden_case as g
    return g()


def test_box_head_on_the_recorded_samples():
    from disprcnn_amd.modeling.roi_heads.box_head import ROIBoxHead
    z, args = golden_case()
    r64, r32 = TO.box_step(**args, dtype=torch.float64), TO.box_step(**args, dtype=torch.float32)
    head = load(ROIBoxHead(box_cfg(), CS.BOX_C), args["params"])
    feats = {"left": [cuda(f) for f in args["feats_left"]], "right": [cuda(f) for f in args["feats_right"]]}
    left, right = boxlists(args["left_boxes"], CS.BOX_IMG), boxlists(args["right_boxes"], CS.BOX_IMG)
    x, logits, deltas, losses = head.losses_on_sampled(feats, left, right, cuda(z["labels"]), cuda(z["regression_targets"]),
                                                       cuda(z["keep"].astype(F32)))
    assert set(losses) == {"loss_classifier", "loss_box_reg"}
    (losses["loss_classifier"] + losses["loss_box_reg"]).backward()
    check(host(x), r64["x"], r32["x"], "x")
    check(host(logits), r64["class_logits"], r32["class_logits"], "class_logits")
    check(host(deltas), r64["box_regression"], r32["box_regression"], "box_regression")
    for k in ("loss_classifier", "loss_box_reg"):
        check(host(losses[k]), r64[k], r32[k], k)
    got = param_grads(head, TO.BOX_PARAMS)
    for k in TO.BOX_PARAMS:
        check(got[k].numpy(), r64["grads"][k], r32["grads"][k], "d/d " + k)


@pytest.mark.parametrize("name", ["box_full_case", "box_one_case"])
def test_box_head_forward_with_draws(name):
    from disprcnn_amd.modeling.roi_heads.box_head import ROIBoxHead
    c = CS.cached(name)
    r64, r32 = CS.box_oracle(c, 64), CS.box_oracle(c, 32)
    head = load(ROIBoxHead(box_cfg(), CS.BOX_C), c.params)
    props = {"left": boxlists(c.left_props, c.img), "right": boxlists(c.right_props, c.img)}
    tgts = {"left": boxlists(c.gt_left, c.img, labels=c.gt_labels), "right": boxlists(c.gt_right, c.img, labels=c.gt_labels)}
    draws = {"sample": cuda(c.sample_draws), "dropout": cuda(c.dropout)}

    def run():
        head.zero_grad()
        fl, fr = [cuda(f).requires_grad_() for f in c.feats_left], [cuda(f).requires_grad_() for f in c.feats_right]
        x, left, right, losses = head({"left": fl, "right": fr}, props, tgts, draws)
        (losses["loss_classifier"] + losses["loss_box_reg"]).backward()
        return x, left, right, losses, fl, fr, param_grads(head, TO.BOX_PARAMS)

    x, left, right, losses, fl, fr, grads = run()
    assert head.feature_extractor.pooler.last_path == "fpn_autograd"
    for n, (keep, lab, enc, p6) in enumerate(c.sampled):
        assert np.array_equal(host(left[n].bbox), p6[:, :4]) and np.array_equal(host(right[n].bbox), p6[:, [4, 1, 5, 3]])
        assert np.array_equal(host(left[n].get_field("labels")), lab) and np.array_equal(host(right[n].get_field("labels")), lab)
    assert x.shape == (c.R, CS.BOX_DIM)
    for k in ("loss_classifier", "loss_box_reg"):
        check(host(losses[k]), r64[k], r32[k], k)
    for k in TO.BOX_PARAMS:
        check(grads[k].numpy(), r64["grads"][k], r32["grads"][k], "d/d " + k)
    for side, got, i in (("left", fl, 0), ("right", fr, 1)):
        for lv in range(4):
            check(host(got[lv].grad), r64["feat_grads"][i][lv], r32["feat_grads"][i][lv], f"d/d {side} P{lv + 2}")
    *_, grads2 = run()
    for k in TO.BOX_PARAMS:
        assert torch.equal(grads[k], grads2[k]), k + ": two runs differ"


# ------------------------------------------------------------------------------------------------ 6. the mask head
def mask_lists(c):
    props = [np.concatenate([b, n]) for b, n in zip(c.boxes, c.negatives)]
    labels = [np.concatenate([np.ones(len(b), np.int64), np.zeros(len(n), np.int64)]) for b, n in zip(c.boxes, c.negatives)]
    return boxlists(props, c.img, labels=labels), boxlists(c.gt, c.img, labels=c.gt_labels, masks=c.masks)


@pytest.mark.parametrize("which", [5, 1, 0])
def test_mask_head_training_step(which):
    from disprcnn_amd.modeling.roi_heads.mask_head import ROIMaskHead
    c = CS.cached("mask_case", which)
    r64, r32 = CS.mask_oracle(c, 64), CS.mask_oracle(c, 32)
    head = load(ROIMaskHead(box_cfg(), CS.MASK_C), c.params)
    props, tgts = mask_lists(c)

    def run():
        head.zero_grad()
        feats = [cuda(f).requires_grad_() for f in c.feats]
        x, out, losses = head(feats, props, tgts)
        losses["loss_mask"].backward()
        return x, out, losses["loss_mask"], feats, param_grads(head, TO.MASK_PARAMS)

    x, out, loss, feats, grads = run()
    assert [len(o) for o in out] == [len(b) for b in c.boxes] and x.shape[0] == which
    assert all(tuple(o.get_field("mask").shape) == (len(o), 1, CS.MASK_M, CS.MASK_M) and not o.get_field("mask").requires_grad for o in out)
    if which == 0:
        assert float(loss.detach()) == 0.0
        for k in TO.MASK_PARAMS:
            assert grads[k].shape == r64["grads"][k].shape and not grads[k].any(), k
        return
    assert np.array_equal(host(head.loss_evaluator.last_targets), c.targets)
    check(host(loss), r64["loss_mask"], r32["loss_mask"], "loss_mask")
    for k in TO.MASK_PARAMS:
        check(grads[k].numpy(), r64["grads"][k], r32["grads"][k], "d/d " + k)
    for lv in range(4):
        check(host(feats[lv].grad), r64["feat_grads"][lv], r32["feat_grads"][lv], f"d/d left P{lv + 2}")
    *_, grads2 = run()
    for k in TO.MASK_PARAMS:
        assert torch.equal(grads[k], grads2[k]), k + ": two runs differ"


def test_mask_head_without_target_masks_gives_a_zero_loss():
    from disprcnn_amd.modeling.roi_heads.mask_head import ROIMaskHead
    c = CS.cached("mask_case", 1)
    head = load(ROIMaskHead(box_cfg(), CS.MASK_C), c.params)
    props, _ = mask_lists(c)
    x, out, losses = head([cuda(f) for f in c.feats], props, boxlists(c.gt, c.img, labels=c.gt_labels))
    losses["loss_mask"].backward()
    assert losses["loss_mask"].item() == 0.0 and all(p.grad is not None and not p.grad.any() for p in head.parameters())


# ------------------------------------------------------------------------------------------------ 7. both heads
def test_combined_heads_train_step_and_eval_after():
    from disprcnn_amd.modeling.roi_heads.roi_heads import build_roi_heads
    from disprcnn_amd.solver.fused import FusedSGD
    c = CS.cached("combined_case")
    state = {**{"box." + k: v for k, v in c.box_params.items()}, **{"mask." + k: v for k, v in c.mask_params.items()}}
    heads = load(build_roi_heads(box_cfg(), CS.MASK_C), state)
    fl, fr = [cuda(f) for f in c.feats_left], [cuda(f) for f in c.feats_right]
    lp, rp = boxlists(c.left_props, c.img), boxlists(c.right_props, c.img)
    lt = boxlists(c.gt_left, c.img, labels=c.gt_labels, masks=c.masks)
    rt = boxlists(c.gt_right, c.img, labels=c.gt_labels)
    draws = {"sample": cuda(c.sample_draws), "dropout": cuda(c.dropout)}
    keys = ("loss_classifier", "loss_box_reg", "loss_mask")

    def compare(losses, box_params, mask_params, what):
        b64, m64 = CS.combined_oracle(c, 64, box_params, mask_params)
        b32, m32 = CS.combined_oracle(c, 32, box_params, mask_params)
        for k, r64, r32 in (("loss_classifier", b64, b32), ("loss_box_reg", b64, b32), ("loss_mask", m64, m32)):
            check(host(losses[k]), r64[k], r32[k], f"{what} {k}")
        return b64, b32, m64, m32

    x, left, right, losses = heads(fl, fr, lp, rp, lt, rt, draws=draws)
    assert set(losses) == set(keys) and [len(b) for b in left] == [len(p) for p in c.pos_boxes]
    b64, b32, m64, m32 = compare(losses, None, None, "step 0")
    opt = FusedSGD(heads.parameters(), lr=0.05, momentum=0.9)
    sum(losses.values()).backward()
    gb, gm = param_grads(heads, TO.BOX_PARAMS, "box."), param_grads(heads, TO.MASK_PARAMS, "mask.")
    for k in TO.BOX_PARAMS:
        check(gb[k].numpy(), b64["grads"][k], b32["grads"][k], "d/d box." + k)
    for k in TO.MASK_PARAMS:
        check(gm[k].numpy(), m64["grads"][k], m32["grads"][k], "d/d mask." + k)
    before = {k: v.detach().cpu().clone() for k, v in heads.state_dict().items()}
    opt.step()
    after = {k: v.detach().cpu().clone() for k, v in heads.state_dict().items()}
    assert all(not torch.equal(before[k], after[k]) for k in before)
    # the next forward reads the UPDATED weights (packed W and W^T are rebuilt from the bumped versions).  Forward values only: a ReLU input
    # that crosses zero between fp32 and fp64 moves a loss continuously, so this comparison needs no margin.
    _, _, _, losses1 = heads(fl, fr, lp, rp, lt, rt, draws=draws)
    compare(losses1, {k: after["box." + k].numpy() for k in TO.BOX_PARAMS}, {k: after["mask." + k].numpy() for k in TO.MASK_PARAMS}, "step 1")
    assert all(losses1[k].item() != losses[k].item() for k in keys)
    # .eval() afterwards: the outputs of a freshly built model with the same weights, bit for bit
    fresh = build_roi_heads(box_cfg(), CS.MASK_C)
    fresh.load_state_dict(after, strict=True)
    fresh = fresh.cuda().eval()
    heads.eval()
    with torch.no_grad():
        a, b = heads(fl, fr, lp, rp), fresh(fl, fr, lp, rp)
    assert torch.equal(a[0], b[0])
    for la, lb in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(la.bbox, lb.bbox) and sorted(la.fields()) == sorted(lb.fields())
        for f in la.fields():
            assert torch.equal(la.get_field(f), lb.get_field(f)), f
    heads.train()
    with pytest.raises(RuntimeError):
        heads([f.cpu() for f in fl], [f.cpu() for f in fr], lp, rp, lt, rt, draws=draws)

"""The RPN's training step on the MI355X against tests/rpn_train_oracle.py in fp64: a small RPN (3 clouds of 96 points, three SA levels of
two scales, three FP levels, BatchNorm everywhere, widths that are no multiple of 16), labels from the label oracle with one cloud
unmatched, one test per LOSS_CLS.

Tolerance, per tensor, the rule of tests/test_hip_rcnn_train.py: max error <= 4 x and mean error <= 2 x the oracle's own fp32-vs-fp64
error on that tensor, plus the floor 1e-6 * max|ref|.  It covers the two losses, every parameter's gradient and the updated running_mean
/ running_var of every BatchNorm.

Condition on the inputs (not a tolerance): the oracle counts, in fp64, the pre-ReLU values and the max-winner gaps (equal columns of
padded neighbourhoods excepted) within 1e-5 of their tensor's scale; the weight seed was chosen on the CPU so that both counts are zero
(rpn_train_oracle.find_seed), and the test asserts it.  A flipped mask or winner therefore cannot explain, or hide, an error.
"""
import functools

import numpy as np
import pytest
import torch

from tests import rpn_oracle as RO
from tests import rpn_train_oracle as TO

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def fixture(kind):
    """-> cfg, state dict, inputs, the oracle's fp64 step and its fp32 step, computed once per loss"""
    cfg = TO.small_cfg(kind)
    sd, inp = TO.state(cfg), TO.make_inputs()
    return cfg, sd, inp, TO.train_step(sd, cfg, inp, torch.float64), TO.train_step(sd, cfg, inp, torch.float32)


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def new_rpn(cfg, sd):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN
    m = RPN(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


def targets(matched):
    """one target per cloud, one instance each; a cloud matched to instance 0 carries no field: the default is zeros"""
    from disprcnn_amd.structures.bounding_box import BoxList
    out = []
    for m in matched:
        b = BoxList(torch.tensor([[0.0, 0.0, 10.0, 10.0]]), (1242, 375), mode="xyxy")
        if m != 0:
            b.add_field("matched_idxs", torch.tensor([int(m)], dtype=torch.long))
        out.append(b)
    return out


def step(model, inp):
    ret, losses = model(t(inp["pts"]), t(inp["cls_label"]), t(inp["reg_label"]), targets(inp["matched"]))
    assert sorted(ret) == ["backbone_features", "backbone_xyz", "rpn_cls", "rpn_reg"]
    assert sorted(losses) == ["rpn_loss_cls", "rpn_loss_reg"]
    (losses["rpn_loss_cls"] + losses["rpn_loss_reg"]).backward()
    return ret, losses


def within(name, got, ref, r32):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    e32 = np.abs(np.asarray(r32, np.float64) - ref)
    floor = 1e-6 * np.abs(ref).max()
    r_max, r_mean = err.max() / (4 * e32.max() + floor), err.mean() / (2 * e32.mean() + floor)
    print(f"{name}: max err {err.max():.3g} (oracle fp32 {e32.max():.3g}), mean err {err.mean():.3g} (oracle fp32 {e32.mean():.3g}), "
          f"floor {floor:.3g}; ratio to the bound: max {r_max:.3f} mean {r_mean:.3f}")
    return r_max <= 1.0 and r_mean <= 1.0


@pytest.mark.parametrize("kind", TO.LOSS_KINDS)
def test_loss_gradients_and_running_statistics_match_fp64(kind):
    cfg, sd, inp, ref, r32 = fixture(kind)
    assert ref["near_zero"] == 0 and ref["near_tie"] == 0, "the fixture must stay clear of every ReLU edge and winner tie"
    assert sorted(set(inp["cls_label"].reshape(-1).tolist())) == [-1.0, 0.0, 1.0] and list(inp["matched"]) == [0, -1, 0]
    model = new_rpn(cfg, sd).train()
    _, losses = step(model, inp)
    bad = []
    for name, key in (("rpn_loss_cls", "loss_cls"), ("rpn_loss_reg", "loss_reg")):
        got = losses[name].item()
        e32 = abs(r32[key] - ref[key])
        print(f"{name} {got:.9g}, oracle fp64 {ref[key]:.9g} (its fp32 error {e32:.3g})")
        if abs(got - ref[key]) > 4 * e32 + 1e-6 * abs(ref[key]):
            bad.append(name)
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(ref["grads"])
    for name in sorted(params):
        grad = params[name].grad
        assert grad is not None and grad.shape == params[name].shape, name
        assert np.abs(ref["grads"][name]).max() > 0, name
        if not within(name, grad.cpu().numpy().reshape(-1), ref["grads"][name].reshape(-1), r32["grads"][name].reshape(-1)):
            bad.append(name)
    state = model.state_dict()
    assert len(ref["bn_layers"]) == 26 and sorted(ref["stats"]) == sorted(k for k in state if "running_" in k)
    for name in sorted(ref["stats"]):
        assert not np.array_equal(state[name].cpu().numpy(), sd[name]), name
        if not within(name, state[name].cpu().numpy(), ref["stats"][name], r32["stats"][name]):
            bad.append(name)
    for name in state:
        if name.endswith("num_batches_tracked"):
            assert int(state[name]) == 1, name
    assert not bad, bad


def test_eval_uses_the_new_weights_and_statistics_after_a_fused_sgd_step():
    from disprcnn_amd.solver.fused import FusedSGD
    cfg, sd, inp, _, _ = fixture("BinaryCrossEntropy")
    model = new_rpn(cfg, sd)
    pts = t(inp["pts"])
    model.eval()
    before, _ = model(pts)                                   # fills the folded cache
    model.train()
    opt = FusedSGD(model.parameters(), lr=1e-2)
    step(model, inp)
    opt.step()
    model.eval()
    after, _ = model(pts)
    assert not torch.equal(before["rpn_reg"], after["rpn_reg"])
    new_sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    assert not np.array_equal(new_sd["rpn_reg_layer.0.conv.weight"], sd["rpn_reg_layer.0.conv.weight"])
    out = {}
    for dtype in (np.float64, np.float32):
        _, feats, _ = RO.backbone(new_sd, cfg, inp["pts"], dtype)
        out[dtype] = (feats,) + tuple(RO.heads(new_sd, feats, dtype))
    for i, name in enumerate(("backbone_features", "rpn_cls", "rpn_reg")):
        ref = out[np.float64][i]
        e32 = np.abs(out[np.float32][i].astype(np.float64) - ref)
        err = np.abs(after[name].cpu().numpy().astype(np.float64) - ref)
        print(f"{name} after the step: max err {err.max():.3g} (bound {4 * e32.max():.3g}), mean err {err.mean():.3g} (bound {2 * e32.mean():.3g})")
        assert err.max() <= 4 * e32.max() and err.mean() <= 2 * e32.mean()


def test_a_model_that_went_through_train_mode_evaluates_bit_for_bit():
    cfg, sd, inp, _, _ = fixture("BinaryCrossEntropy")
    pts = t(inp["pts"])
    ref, _ = new_rpn(cfg, sd).eval()(pts)
    m = new_rpn(cfg, sd)
    m.train()
    m.eval()
    got, _ = m(pts)
    for name in ("rpn_cls", "rpn_reg", "backbone_features", "roi_boxes3d", "roi_scores_raw"):
        assert torch.equal(ref[name], got[name]), name


def test_two_training_steps_from_the_same_state_give_the_same_bits():
    cfg, sd, inp, _, _ = fixture("SigmoidFocalLoss")
    runs = []
    for _ in range(2):
        m = new_rpn(cfg, sd).train()
        ret, losses = step(m, inp)
        runs.append((ret, losses, {k: p.grad for k, p in m.named_parameters()}, m.state_dict()))
    a, b = runs
    for i in range(4):
        assert sorted(a[i]) == sorted(b[i])
        for k in a[i]:
            assert torch.equal(a[i][k], b[i][k]), k


def test_dropout_is_torch_dropout():
    cfg, sd, inp, _, _ = fixture("BinaryCrossEntropy")
    drop = TO.small_cfg("BinaryCrossEntropy", dp_ratio=0.5)

    def loss(c, seed):
        torch.manual_seed(seed)
        _, losses = step(new_rpn(c, sd).train(), inp)
        return (losses["rpn_loss_cls"] + losses["rpn_loss_reg"]).item()
    plain, a, b = loss(cfg, 5), loss(drop, 5), loss(drop, 5)
    assert a == b and a != plain


def test_training_raises_where_it_is_not_built():
    cfg, sd, inp, _, _ = fixture("BinaryCrossEntropy")
    with pytest.raises(NotImplementedError):
        new_rpn(cfg, sd).train()(t(inp["pts"]))
    with pytest.raises(NotImplementedError):
        new_rpn(cfg, sd).train()(t(inp["pts"]), t(inp["cls_label"]), None, targets(inp["matched"]))
    fixed = TO.small_cfg("BinaryCrossEntropy", fixed=True)
    with pytest.raises(NotImplementedError, match="FIXED"):
        step(new_rpn(fixed, sd).train(), inp)

"""RCNNNet's training step on the MI355X against the imported reference's recording (tests/golden/rcnn_train_golden.npz): the loss, every
parameter's gradient and the gradient with respect to pts_input's feature channels; the folded eval cache after an optimiser step; and
the eval outputs, which must not move.

Tolerance, per tensor, the rule tests/test_hip_rcnn.py applies to the forward: max error <= 4 x and mean error <= 2 x the reference's
own fp32-vs-fp64 error on exactly the stored entries (err32_max_* / err32_mean_*), plus the kernel bound's floor 1e-6 * max|ref| so that a
tensor the reference happened to get exact cannot fail on an ulp.  The stored sums (whole-tensor sum and absolute sum of the large
gradients) are checked against their own recorded fp32 error the same way; their floor is 1e-6 * sum|ref|, the scale of the sum (no
larger than the per-entry floor times the number of entries).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import rcnn_oracle as CO
from tests import rcnn_train_oracle as TO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "rcnn_train_golden.npz"))
GE = np.load(os.path.join(HERE, "golden", "rcnn_ref_golden.npz"))
with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as _f:
    CFG_JSON = json.load(_f)
CFG = TO.train_cfg(CFG_JSON)
DEV = "cuda"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()
    yield
    import gc
    gc.collect()                        # autograd's graphs die with the garbage collector; hand their blocks back to the driver, so that
    torch.cuda.synchronize()            # later modules that count allocated bytes are not served from this module's split-up blocks
    torch.cuda.empty_cache()


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def state():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    shapes = {k: tuple(v.shape) for k, v in RCNNNet(CFG, None).state_dict().items()}
    return CO.random_state(shapes, int(G["weight_seed"]))


def new_net(sd=None):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    m = RCNNNet(CFG, None)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in (sd or state()).items()}, strict=True)
    return m.to(DEV)


def train_inputs():
    return TO.make_train_inputs(CFG, int(G["input_bump"]), int(G["gt_seed"]))


def proposals(prop, grad=False):
    p = {"pts_input": t(prop["pts_input"]), "roi_boxes3d": t(prop["roi_boxes3d"]), "cls_label": t(prop["cls_label"]),
         "reg_valid_mask": t(prop["reg_valid_mask"], torch.int64), "gt_boxes3d_ct": t(prop["gt_boxes3d_ct"])}
    if grad:
        p["pts_input"].requires_grad_()
    return p


def within(name, got, ref, emax, emean, floor):
    err = np.abs(np.asarray(got, np.float64) - ref)
    r_max, r_mean = err.max() / (4 * emax + floor), err.mean() / (2 * emean + floor)
    print(f"{name}: max err {err.max():.3g} (reference fp32 {emax:.3g}), mean err {err.mean():.3g} (reference fp32 {emean:.3g}), floor {floor:.3g}; "
          f"ratio to the bound: max {r_max:.3f} mean {r_mean:.3f}")
    return r_max <= 1.0 and r_mean <= 1.0


def test_loss_and_gradients_match_the_reference_recording():
    net = new_net().train()
    p = proposals(train_inputs(), grad=True)
    ret, losses = net(p)
    assert ret is p and sorted(losses) == ["loss_box3d"]
    loss = losses["loss_box3d"]
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    l64 = float(G["loss64"])
    print(f"loss {loss.item():.9g}, reference fp64 {l64:.9g} (its fp32 error {float(G['err32_loss']):.3g})")
    assert abs(loss.item() - l64) <= 4 * float(G["err32_loss"]) + 1e-6 * abs(l64)
    bad = []
    params = dict(net.named_parameters())
    assert sorted(params) == [str(k) for k in G["param_names"]]
    for name in sorted(params):
        grad = params[name].grad
        assert grad is not None and grad.shape == params[name].shape, name
        g = grad.detach().cpu().numpy().reshape(-1).astype(np.float64)
        ref = G[f"g_{name}"]
        sel = G[f"gi_{name}"] if f"gi_{name}" in G.files else np.arange(g.size)
        if not within(name, g[sel], ref, float(G[f"err32_max_{name}"]), float(G[f"err32_mean_{name}"]), 1e-6 * np.abs(ref).max()):
            bad.append(name)
        if f"gsum_{name}" in G.files:
            asum = float(G[f"gasum_{name}"])
            e_sum, e_asum = abs(g.sum() - float(G[f"gsum_{name}"])), abs(np.abs(g).sum() - asum)
            b_sum, b_asum = 4 * float(G[f"err32_sum_{name}"]) + 1e-6 * asum, 4 * float(G[f"err32_asum_{name}"]) + 1e-6 * asum
            print(f"{name}: sum err {e_sum:.3g} (bound {b_sum:.3g}), abs-sum err {e_asum:.3g} (bound {b_asum:.3g})")
            if e_sum > b_sum or e_asum > b_asum:
                bad.append(name + " (sums)")
    gp = p["pts_input"].grad
    assert gp is not None and gp.shape == p["pts_input"].shape
    gp = gp.cpu().numpy()[..., 3:].reshape(-1).astype(np.float64)[G["gi_pts_input"]]
    if not within("pts_input[..., 3:]", gp, G["g_pts_input"], float(G["err32_max_pts_input"]), float(G["err32_mean_pts_input"]),
                  1e-6 * np.abs(G["g_pts_input"]).max()):
        bad.append("pts_input")
    assert not bad, bad


def eval_inputs():
    inp = CO.make_inputs("b2", int(GE["input_bump"]))
    rc = CFG.RCNN
    pin = CO.pts_input_of(CO.pool_canonical(inp, rc.POOL_EXTRA_WIDTH, rc.NUM_POINTS, rc.USE_DEPTH, f32))
    sel = np.array(TO.TRAIN_ROIS)
    return {"pts_input": t(pin[sel]), "roi_boxes3d": t(inp["roi_boxes3d"].reshape(-1, 7)[sel][None]),
            "roi_scores_raw": t(inp["roi_scores_raw"].reshape(-1)[sel][None])}, pin[sel]


def test_eval_uses_the_updated_weights_after_an_optimizer_step():
    net = new_net()
    prop, pin = eval_inputs()
    net.eval()
    with torch.no_grad():
        before = net.network(prop)                           # fills the folded cache
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    _, losses = net(proposals(train_inputs()))
    losses["loss_box3d"].backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        after = net.network(prop)
    assert not torch.equal(before["rcnn_reg"], after["rcnn_reg"])
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    _, cls64, reg64 = CO.network(sd, CFG, pin, np.float64)
    for name, got, ref in (("rcnn_cls", after["rcnn_cls"], cls64), ("rcnn_reg", after["rcnn_reg"], reg64)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        emax, emean = float(GE[f"err32_max_{name}"]), float(GE[f"err32_mean_{name}"])
        print(f"{name} after the step: max err {err.max():.3g} (bound {4 * emax:.3g}), mean err {err.mean():.3g} (bound {2 * emean:.3g})")
        assert err.max() <= 4 * emax and err.mean() <= 2 * emean


def test_eval_outputs_are_bit_identical_to_an_eval_only_model():
    prop, _ = eval_inputs()
    a = new_net().eval()
    with torch.no_grad():
        ref = a.network(prop)
        lists_ref, _ = a(prop)
    b = new_net()
    b.train()
    b.eval()                                                 # a model that has been through train mode, before any training call
    with torch.no_grad():
        got = b.network(prop)
    assert torch.equal(ref["rcnn_cls"], got["rcnn_cls"]) and torch.equal(ref["rcnn_reg"], got["rcnn_reg"])
    c = new_net().train()
    _, losses = c(proposals(train_inputs()))                 # and one whose training forward ran, without an update
    losses["loss_box3d"].backward()
    c.eval()
    with torch.no_grad():
        got = c.network(prop)
        lists, _ = c(prop)
    assert torch.equal(ref["rcnn_cls"], got["rcnn_cls"]) and torch.equal(ref["rcnn_reg"], got["rcnn_reg"])
    assert len(lists) == len(lists_ref) == 1
    assert torch.equal(lists[0].get_field("box3d").bbox_3d, lists_ref[0].get_field("box3d").bbox_3d)


def test_training_still_raises_where_it_is_not_built():
    import copy
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    jit = copy.deepcopy(CFG)
    jit["RCNN"]["ROI_SAMPLE_JIT"] = True
    with pytest.raises(NotImplementedError, match="ProposalTargetLayer"):
        RCNNNet(jit, None).to(DEV).train()(proposals(train_inputs()))
    with pytest.raises(NotImplementedError):
        new_net().train().refine(proposals(train_inputs()))
    bn = copy.deepcopy(CFG)
    bn["RCNN"]["USE_BN"] = True
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        RCNNNet(bn, None).to(DEV).train()(proposals(train_inputs()))

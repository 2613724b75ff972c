"""PointRCNN training labels and losses on the GPU (disprcnn_amd/pts/train_targets.hip through layers/pointrcnn_loss.py and the
reference-named evaluators) against the reference's recordings (tests/golden/pointrcnn_loss_golden.npz) and tests/pointrcnn_loss_oracle.py,
which tests/test_pointrcnn_loss_host.py pins to those recordings to 1e-12.

Tolerance, the bound tests/test_hip_rpn.py uses for kernels: for a loss term |got - ref64| <= 2 e32 + 1e-6 |ref64|, for a gradient tensor
max|got - ref64| <= 2 e32 + 1e-6 max|ref64|, e32 being the reference's own fp32-vs-fp64 error recorded with the case.  Bin labels are
compared bit for bit with the fp32 reference's, on every row.
"""
import os

import numpy as np
import pytest
import torch

from . import pointrcnn_loss_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "pointrcnn_loss_golden.npz"))
RPN_VALS, RCNN_VALS = [str(v) for v in G["rpn_vals"]], [str(v) for v in G["rcnn_vals"]]


def L():
    from disprcnn_amd.layers import pointrcnn_loss
    return pointrcnn_loss


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def check_term(got, ref, e32, what):
    got = float(got.detach()) if isinstance(got, torch.Tensor) else float(got)
    ref, e32 = float(ref), float(e32)
    print(f"{what}: got {got!r} ref {ref!r} err {abs(got - ref):.3g} bound {2 * e32 + 1e-6 * abs(ref):.3g}")
    assert np.isfinite(got) and abs(got - ref) <= 2 * e32 + 1e-6 * abs(ref), what


def check_grad(got, ref, e32, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max(initial=0.0)
    bound = 2 * float(e32) + 1e-6 * np.abs(ref).max(initial=0.0)
    print(f"{what}: err {err:.3g} bound {bound:.3g} (|ref| <= {np.abs(ref).max(initial=0.0):.3g})")
    assert np.isfinite(got).all() and err <= bound, what


# ------------------------------------------------------------------------------------------------------------ regression loss
def run_reg(inp, lay):
    pred = dev(inp["pred"]).requires_grad_()
    loc, angle, size, terms = L().bin_reg_loss(pred, dev(inp["reg_label"]), dev(inp["row_mask"]), anchor_size=dev(inp["anchor"]),
                                               loss_mask=None if inp["loss_mask"] is None else dev(inp["loss_mask"]), **lay)
    g = O.GRAD_WEIGHTS
    (g[0] * loc + g[1] * angle + g[2] * size).backward()
    assert loc.dim() == 0 and loc.dtype == torch.float32 and loc.is_cuda
    return terms.detach().clone(), pred.grad.clone()


@pytest.mark.parametrize("name", list(O.REG_CASES))
def test_bin_reg_loss(name):
    case = O.REG_CASES[name]
    lay = O.LAYOUTS[case["layout"]]
    inp = O.make_reg_case(case, int(G[f"{name}_seed"]))
    terms, grad = run_reg(inp, lay)
    terms2, grad2 = run_reg(inp, lay)
    assert torch.equal(terms, terms2) and torch.equal(grad, grad2), "two runs differ"
    t, g = host(terms), host(grad)
    ref, e32 = G[f"{name}_terms"], G[f"{name}_terms_e32"]
    for i, tn in enumerate(O.TERMS):
        check_term(t[i], ref[i], e32[i], f"{name} {tn}")
    sel = inp["row_mask"]
    assert t[12] == sel.sum() and t[13] == (sel.sum() if inp["loss_mask"] is None else (sel & inp["loss_mask"]).sum())
    assert not g[~sel].any(), "gradient on an unselected row"
    check_grad(g[O.stored_rows(case)], G[f"{name}_grad"], G[f"{name}_grad_e32"], f"{name} grad (recorded rows)")
    check_grad(g, O.reg_loss(inp["pred"], inp["reg_label"], sel, lay, inp["anchor"], inp["loss_mask"])[1], G[f"{name}_grad_e32"],
               f"{name} grad (all rows, oracle)")


@pytest.mark.parametrize("lname", list(O.LAYOUTS))
def test_bin_reg_loss_without_rows(lname):
    lay = O.LAYOUTS[lname]
    C = O.channels(lay)
    pred = torch.zeros((0, C), device="cuda", requires_grad=True)
    loc, angle, size, terms = L().bin_reg_loss(pred, torch.zeros((0, 7), device="cuda"), None, anchor_size=dev(np.array(O.MEAN_SIZE, np.float32)),
                                               loss_mask=torch.zeros(0, dtype=torch.bool, device="cuda"), **lay)
    (loc + angle + size).backward()
    assert not host(terms).any() and pred.grad.shape == (0, C)


def bins_cases():
    out = [("reg", n) for n in O.REG_CASES] + [("rcnn", n) for n in O.RCNN_CASES] + [("edge", n) for n in O.LAYOUTS]
    return out


@pytest.mark.parametrize("kind,name", bins_cases())
def test_reg_bin_targets_are_the_fp32_references(kind, name):
    if kind == "reg":
        lay = O.LAYOUTS[O.REG_CASES[name]["layout"]]
        inp = O.make_reg_case(O.REG_CASES[name], int(G[f"{name}_seed"]))
        lab, anchor, ref = inp["reg_label"], inp["anchor"], G[f"{name}_bins"]
    elif kind == "rcnn":
        cfg = O.cfg_for(O.RCNN_CASES[name])
        lay = O.rcnn_layout(cfg)
        inp = O.make_rcnn_case(O.RCNN_CASES[name], int(G[f"{name}_seed"]))
        lab, ref = inp["gt_of_rois"], G[f"{name}_bins"]
        anchor = inp["roi_boxes3d"][:, 3:6] if cfg.RCNN.SIZE_RES_ON_ROI else np.array(O.MEAN_SIZE, np.float32)
    else:
        lay = O.LAYOUTS[name]
        lab, anchor, ref = O.make_edge_rows(lay), np.array(O.MEAN_SIZE, np.float32), G[f"edge_{name}_bins"]
    bins, res = L().reg_bin_targets(dev(lab), anchor_size=dev(anchor), **lay)
    assert bins.dtype == torch.int32 and bins.shape == (len(lab), 4) and res.shape == (len(lab), 7)
    got = bins.cpu().numpy().astype(np.int64)
    bad = np.nonzero((got != ref.astype(np.int64)).any(1))[0]
    assert len(bad) == 0, f"rows {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, fp32 reference {ref[bad[:8]].tolist()}"
    # the residual labels are the same fp32 expressions: a few ulps at the labels' scale (|label| <= 1 for bins, about 0.3 for sizes)
    want = O.bin_targets(lab, anchor, lay, np.float32)[1].astype(np.float64)
    assert np.abs(host(res) - want).max() <= 4 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------ classification losses
CLS_CASES = [n for n in O.RPN_CASES if n.startswith("c")]


def run_cls(kind, x, lab, mask, **kw):
    logits = dev(x).requires_grad_()
    loss, terms = L().point_cls_loss(kind, logits, dev(lab), None if mask is None else dev(mask), **kw)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    return terms.detach().clone(), logits.grad.clone()


@pytest.mark.parametrize("name", CLS_CASES)
def test_point_cls_loss(name):
    case = O.RPN_CASES[name]
    cfg = O.cfg_for(case)
    kind = cfg.RPN.LOSS_CLS
    inp = O.make_rpn_case(case, int(G[f"{name}_seed"]))
    x, lab = inp["rpn_cls"].reshape(-1), inp["cls_label"].reshape(-1)
    mask = None if kind == "DiceLoss" else np.repeat(inp["matched"] >= 0, case["N"])
    kw = dict(fg_weight=cfg.RPN.FG_WEIGHT, alpha=cfg.RPN.FOCAL_ALPHA[0], gamma=cfg.RPN.FOCAL_GAMMA)
    terms, grad = run_cls(kind, x, lab, mask, **kw)
    terms2, grad2 = run_cls(kind, x, lab, mask, **kw)
    assert torch.equal(terms, terms2) and torch.equal(grad, grad2), "two runs differ"
    t, g = host(terms), host(grad)
    vals, e32 = dict(zip(RPN_VALS, G[f"{name}_vals"])), dict(zip(RPN_VALS, G[f"{name}_vals_e32"]))
    check_term(t[0], vals["rpn_loss_cls"], e32["rpn_loss_cls"], f"{name} loss")
    if kind == "SigmoidFocalLoss":
        check_term(t[1], vals["rpn_loss_cls_pos"], e32["rpn_loss_cls_pos"], f"{name} positive part")
        check_term(t[2], vals["rpn_loss_cls_neg"], e32["rpn_loss_cls_neg"], f"{name} negative part")
    e = case.get("every", 1)
    check_grad(g[e - 1::e], G[f"{name}_gcls"], G[f"{name}_gcls_e32"], f"{name} grad (recorded)")
    check_grad(g, O.cls_loss(kind, x, lab, mask, **kw)["grad"], G[f"{name}_gcls_e32"], f"{name} grad (all, oracle)")


@pytest.mark.parametrize("kind", ["BinaryCrossEntropy", "SigmoidFocalLoss"])
def test_saturated_logits_stay_finite_with_a_live_gradient(kind):
    """Logits +-20, +-50, +-100: the fp32 reference's log(1 - sigmoid(x)) has clamped there (loss 100, gradient 0).  Against the closed
    form in fp64; e32 is taken as 0, so the bound is 1e-6 relative."""
    x, lab = O.make_saturation_case()
    terms, grad = run_cls(kind, x, lab, None, fg_weight=15.0)
    ref = O.cls_loss(kind, x, lab, None, fg_weight=15.0)
    check_term(host(terms)[0], ref["loss"], 0.0, f"saturated {kind}")
    check_grad(host(grad), ref["grad"], 0.0, f"saturated {kind} grad")
    wrong = (x > 0) != (lab > 0)
    assert (host(grad)[wrong] != 0).all(), "a wrong, saturated prediction has lost its gradient"


def test_reference_named_losses():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.utils import loss_utils as LU
    case = O.RPN_CASES["c65_focal"]
    inp = O.make_rpn_case(case, int(G["c65_focal_seed"]))
    x, lab = inp["rpn_cls"].reshape(-1), inp["cls_label"].reshape(-1)
    ref = O.cls_loss("SigmoidFocalLoss", x, lab)
    pos, neg = (lab > 0).astype(np.float32), (lab == 0).astype(np.float32)
    logits = dev(x).requires_grad_()
    out = LU.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0)(logits, dev(pos), dev((pos + neg) / max(pos.sum(), 1.0)))
    assert out.shape == logits.shape
    out.sum().backward()
    # every element is rounded to fp32 once (2^-24 relative) and so is each step of the sum: 1e-6 of the sum covers 65 of them
    check_term(out.sum(), ref["loss"], 0.0, "elementwise focal, summed")
    check_grad(host(logits.grad), ref["grad"], 1e-9, "elementwise focal grad")
    d = LU.DiceLoss(ignore_target=-1)(dev(x), dev(lab))
    check_term(d, O.cls_loss("DiceLoss", x, lab)["loss"], 0.0, "DiceLoss")
    # get_reg_loss on rows the caller selected
    rc = O.REG_CASES["r65_46m"]
    lay = O.LAYOUTS[rc["layout"]]
    ri = O.make_reg_case(rc, int(G["r65_46m_seed"]))
    s = ri["row_mask"]
    loc, angle, size, dct = LU.get_reg_loss(dev(ri["pred"][s]), dev(ri["reg_label"][s]), anchor_size=dev(ri["anchor"]),
                                            loss_mask=dev(ri["loss_mask"][s]), **lay)
    ref, e32 = G["r65_46m_terms"], G["r65_46m_terms_e32"]
    check_term(loc, ref[9], e32[9], "get_reg_loss loc")
    check_term(angle, ref[10], e32[10], "get_reg_loss angle")
    check_term(size, ref[8], e32[8], "get_reg_loss size")
    check_term(dct["loss_ry_res"], ref[7], e32[7], "get_reg_loss loss_ry_res")
    assert sorted(dct) == sorted(["loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res", "loss_y_offset", "loss_ry_bin", "loss_ry_res",
                                  "loss_loc", "loss_angle", "loss_size"])


# ------------------------------------------------------------------------------------------------------------ point labels
@pytest.mark.parametrize("name", list(O.LABEL_CASES))
def test_rpn_point_labels(name):
    pts, boxes7 = O.make_label_case(name, int(G[f"{name}_seed"]))
    corners, large, near = G[f"{name}_corners"], G[f"{name}_corners_large"], G[f"{name}_near_face"]
    cls, reg = L().rpn_point_labels(dev(pts), dev(boxes7), dev(corners), dev(large))
    cls2, reg2 = L().rpn_point_labels(dev(pts), dev(boxes7), dev(corners), dev(large))
    assert torch.equal(cls, cls2) and torch.equal(reg, reg2)
    c, r = host(cls), host(reg)
    ref = G[f"{name}_cls"].astype(np.float64)
    assert set(np.unique(c)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(c[~near], ref[~near]), f"{int((c != ref)[~near].sum())} labels differ away from the faces"
    want = O.point_labels(pts, boxes7, corners, large)[1]
    fg = (c == 1) & (ref == 1)
    check_grad(r[fg], want[fg], G[f"{name}_reg_e32"], f"{name} reg_label on foreground points")
    assert not r[c != 1].any(), "reg_label is not zero off the foreground"
    sub_ok = (fg & ~near)[:, ::8]
    assert np.array_equal(r[:, ::8][sub_ok], G[f"{name}_reg32_sub"].astype(np.float64)[sub_ok]), "one fp32 subtraction: the reference's bits"
    if name == "lb_16_768":
        inside = (c == 1).sum(1)
        assert inside[1] == 0 and inside[2] == pts.shape[1], "the empty cloud and the cloud inside the box"


def test_generate_rpn_training_labels():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import generate_rpn_training_labels
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    name = "lb_3_65"
    pts, boxes7 = O.make_label_case(name, int(G[f"{name}_seed"]))
    targets = []
    for b in range(len(boxes7)):
        t = BoxList(torch.tensor([[0.0, 0.0, 10.0, 10.0]]), (1242, 375), mode="xyxy")
        t.add_field("box3d", Box3DList(torch.from_numpy(boxes7[b:b + 1]), (1242, 375), mode="xyzhwl_ry"))
        targets.append(t)
    cls, reg = generate_rpn_training_labels(dev(pts), targets)
    near = G[f"{name}_near_face"]
    assert np.array_equal(host(cls)[~near], G[f"{name}_cls"].astype(np.float64)[~near])
    cls_k, reg_k = L().rpn_point_labels(dev(pts), dev(boxes7), dev(G[f"{name}_corners"]), dev(G[f"{name}_corners_large"]))
    assert torch.equal(cls, cls_k) and torch.equal(reg, reg_k)


# ------------------------------------------------------------------------------------------------------------ the evaluators
def run_rpn_evaluator(case, inp, tb):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn_loss import PointRCNNLossComputation
    ev = PointRCNNLossComputation(O.cfg_for(case))
    cls, reg = dev(inp["rpn_cls"]).requires_grad_(), dev(inp["rpn_reg"]).requires_grad_()
    out = ev(cls, reg, dev(inp["cls_label"]), dev(inp["reg_label"]), dev(inp["matched"]), tb_dict=tb)
    assert sorted(out) == ["rpn_loss_cls", "rpn_loss_reg"]
    (out["rpn_loss_cls"] + out["rpn_loss_reg"]).backward()
    return ev, out, cls.grad.clone(), reg.grad.clone()


@pytest.mark.parametrize("name", [n for n in O.RPN_CASES if n.startswith("ev_")])
def test_rpn_loss_computation(name):
    case = O.RPN_CASES[name]
    inp = O.make_rpn_case(case, int(G[f"{name}_seed"]))
    tb = {}
    ev, out, gcls, greg = run_rpn_evaluator(case, inp, tb)
    ev2, out2, gcls2, greg2 = run_rpn_evaluator(case, inp, {})
    assert torch.equal(ev.last_terms, ev2.last_terms) and torch.equal(gcls, gcls2) and torch.equal(greg, greg2), "two runs differ"
    vals, e32 = dict(zip(RPN_VALS, G[f"{name}_vals"])), dict(zip(RPN_VALS, G[f"{name}_vals_e32"]))
    assert sorted(tb) == sorted(str(k) for k in G[f"{name}_keys"])
    for k, v in tb.items():
        if k == "rpn_fg_sum":
            assert isinstance(v, int) and v == int(vals[k])
        else:
            check_term(v, vals[k], e32[k], f"{name} tb_dict[{k}]")
    assert ev.TERM_NAMES[:7] == tuple(RPN_VALS[:7]) and float(ev.last_terms[0]) == tb["rpn_loss_cls"]
    check_term(out["rpn_loss_cls"], vals["rpn_loss_cls"], e32["rpn_loss_cls"], f"{name} rpn_loss_cls")
    check_term(out["rpn_loss_reg"], vals["rpn_loss_reg"], e32["rpn_loss_reg"], f"{name} rpn_loss_reg")
    check_grad(host(gcls).reshape(-1), G[f"{name}_gcls"], G[f"{name}_gcls_e32"], f"{name} d/d rpn_cls")
    check_grad(host(greg).reshape(-1, greg.shape[-1]), G[f"{name}_greg"], G[f"{name}_greg_e32"], f"{name} d/d rpn_reg")
    if name == "ev_nofg":
        assert float(out["rpn_loss_reg"]) == 0.0 and out["rpn_loss_reg"].requires_grad and not host(greg).any()
    # without a tb_dict nothing reads the device
    cls, reg = dev(inp["rpn_cls"]).requires_grad_(), dev(inp["rpn_reg"]).requires_grad_()
    args = (dev(inp["cls_label"]), dev(inp["reg_label"]), dev(inp["matched"]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o = ev(cls, reg, *args)
        (o["rpn_loss_cls"] + o["rpn_loss_reg"]).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(cls.grad, gcls) and torch.equal(reg.grad, greg)


def run_rcnn_evaluator(ev, inp, tb):
    cls, reg = dev(inp["rcnn_cls"]).requires_grad_(), dev(inp["rcnn_reg"]).requires_grad_()
    labels = {"cls_label": dev(inp["cls_label"]), "reg_valid_mask": dev(inp["reg_valid_mask"]), "roi_boxes3d": dev(inp["roi_boxes3d"]),
              "gt_of_rois": dev(inp["gt_of_rois"]), "pts_input": torch.zeros((len(inp["cls_label"]), 1), device="cuda")}
    loss = ev({"rcnn_cls": cls, "rcnn_reg": reg}, None, labels, None, None, tb_dict=tb)
    loss.backward()
    return loss, cls.grad.clone(), reg.grad.clone(), labels


@pytest.mark.parametrize("name", list(O.RCNN_CASES))
def test_rcnn_loss_computation(name):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_loss import PointRCNNBox3dLossComputation
    case = O.RCNN_CASES[name]
    inp = O.make_rcnn_case(case, int(G[f"{name}_seed"]))
    ev = PointRCNNBox3dLossComputation(O.cfg_for(case))
    tb = {}
    loss, gcls, greg, labels = run_rcnn_evaluator(ev, inp, tb)
    terms = ev.last_terms.clone()
    loss2, gcls2, greg2, _ = run_rcnn_evaluator(ev, inp, {})
    assert torch.equal(terms, ev.last_terms) and torch.equal(gcls, gcls2) and torch.equal(greg, greg2), "two runs differ"
    vals, e32 = dict(zip(RCNN_VALS, G[f"{name}_vals"])), dict(zip(RCNN_VALS, G[f"{name}_vals_e32"]))
    assert sorted(tb) == sorted(str(k) for k in G[f"{name}_keys"])
    for k, v in tb.items():
        if k in ("rcnn_cls_fg", "rcnn_cls_bg", "rcnn_reg_fg"):
            assert isinstance(v, int) and v == int(vals[k])
        else:
            check_term(v, vals[k], e32[k], f"{name} tb_dict[{k}]")
    check_term(loss, vals["rcnn_loss"], e32["rcnn_loss"], f"{name} rcnn_loss")
    check_grad(host(gcls).reshape(-1), G[f"{name}_gcls"], G[f"{name}_gcls_e32"], f"{name} d/d rcnn_cls")
    check_grad(host(greg), G[f"{name}_greg"], G[f"{name}_greg_e32"], f"{name} d/d rcnn_reg")
    cls, reg = dev(inp["rcnn_cls"]).requires_grad_(), dev(inp["rcnn_reg"]).requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev({"rcnn_cls": cls, "rcnn_reg": reg}, None, labels, None).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(cls.grad, gcls) and torch.equal(reg.grad, greg)

"""PointRCNN training labels and losses, host side: tests/pointrcnn_loss_oracle.py pinned to the reference's recordings
(tests/golden/pointrcnn_loss_golden.npz, made by make_golden_pointrcnn_loss.py), the C ABI's declarations, and the no-fallback rule."""
import os
import re

import numpy as np
import pytest
import torch

from . import pointrcnn_loss_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "pointrcnn_loss_golden.npz"))
RPN_VALS, RCNN_VALS = [str(v) for v in G["rpn_vals"]], [str(v) for v in G["rcnn_vals"]]
SYMBOLS = ("drc_rpn_point_labels", "drc_bin_reg_targets", "drc_bin_reg_loss_fwd", "drc_bin_reg_loss_bwd", "drc_point_cls_loss_fwd",
           "drc_point_cls_loss_bwd", "drc_focal_elementwise", "drc_train_scratch_doubles")


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = 1e-12 * max(np.abs(ref).max(initial=0.0), 1e-300)
    err = np.abs(got - ref).max(initial=0.0)
    assert err <= bound, f"{what}: {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("name", list(O.REG_CASES))
def test_reg_loss_oracle_matches_reference(name):
    case = O.REG_CASES[name]
    lay = O.LAYOUTS[case["layout"]]
    inp = O.make_reg_case(case, int(G[f"{name}_seed"]))
    bins, _ = O.bin_targets(inp["reg_label"], inp["anchor"], lay, np.float32)
    assert np.array_equal(bins, G[f"{name}_bins"].astype(np.int64))
    terms, grad = O.reg_loss(inp["pred"], inp["reg_label"], inp["row_mask"], lay, inp["anchor"], inp["loss_mask"])
    close(terms, G[f"{name}_terms"], f"{name} terms")
    close(grad[O.stored_rows(case)], G[f"{name}_grad"], f"{name} grad")


@pytest.mark.parametrize("lname", list(O.LAYOUTS))
def test_edge_bins_oracle_matches_fp32_reference(lname):
    lay = O.LAYOUTS[lname]
    bins, _ = O.bin_targets(O.make_edge_rows(lay), np.array(O.MEAN_SIZE, np.float32), lay, np.float32)
    assert np.array_equal(bins, G[f"edge_{lname}_bins"].astype(np.int64))


def rpn_vals(out):
    return np.array([float(out.get(k, 0.0)) for k in RPN_VALS])


@pytest.mark.parametrize("name", list(O.RPN_CASES))
def test_rpn_loss_oracle_matches_reference(name):
    case = O.RPN_CASES[name]
    inp = O.make_rpn_case(case, int(G[f"{name}_seed"]))
    out, gcls, greg = O.rpn_loss(O.cfg_for(case), inp)
    close(rpn_vals(out), G[f"{name}_vals"], f"{name} values")
    assert sorted(out) == sorted(str(k) for k in G[f"{name}_keys"])
    e = case.get("every", 1)
    close(gcls[e - 1::e], G[f"{name}_gcls"], f"{name} d/d rpn_cls")
    if name.startswith("ev_"):
        close(greg, G[f"{name}_greg"], f"{name} d/d rpn_reg")


@pytest.mark.parametrize("name", list(O.RCNN_CASES))
def test_rcnn_loss_oracle_matches_reference(name):
    case = O.RCNN_CASES[name]
    cfg = O.cfg_for(case)
    inp = O.make_rcnn_case(case, int(G[f"{name}_seed"]))
    out, gcls, greg = O.rcnn_loss(cfg, inp)
    ref = dict(zip(RCNN_VALS, G[f"{name}_vals"]))
    for k, v in out.items():
        close(v, ref[k], f"{name} {k}")
    close(gcls, G[f"{name}_gcls"], f"{name} d/d rcnn_cls")
    close(greg, G[f"{name}_greg"], f"{name} d/d rcnn_reg")
    anchor = inp["roi_boxes3d"][:, 3:6] if cfg.RCNN.SIZE_RES_ON_ROI else np.array(O.MEAN_SIZE, np.float32)
    assert np.array_equal(O.bin_targets(inp["gt_of_rois"], anchor, O.rcnn_layout(cfg), np.float32)[0], G[f"{name}_bins"].astype(np.int64))


def test_saturated_bce_closed_form_is_finite_with_a_live_gradient():
    x, lab = O.make_saturation_case()
    for kind in ("BinaryCrossEntropy", "SigmoidFocalLoss"):
        r = O.cls_loss(kind, x, lab)
        assert np.isfinite(r["loss"]) and np.isfinite(r["grad"]).all()
        wrong = (x > 0) != (lab > 0)
        assert (r["grad"][wrong] != 0).all()
    assert abs(O.cls_loss("BinaryCrossEntropy", x, lab, fg_weight=1.0)["loss"] - (20 + 50 + 100) * 2 / 12) < 1e-8


@pytest.mark.parametrize("name", list(O.LABEL_CASES))
def test_point_labels_oracle_and_enlarge_box3d(name):
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    pts, boxes7 = O.make_label_case(name, int(G[f"{name}_seed"]))
    corners, large = G[f"{name}_corners"], G[f"{name}_corners_large"]
    near = G[f"{name}_near_face"]
    assert near.mean() <= 0.005
    cls, reg = O.point_labels(pts, boxes7, corners, large)
    assert np.array_equal(cls[~near], G[f"{name}_cls"].astype(np.float64)[~near])
    sub = G[f"{name}_reg32_sub"].astype(np.float64)
    ok = ~near[:, ::8]
    assert np.abs(reg[:, ::8][ok] - sub[ok]).max(initial=0.0) <= float(G[f"{name}_reg_e32"]) + 1e-7
    assert np.array_equal(reg[cls != 1], np.zeros_like(reg[cls != 1]))
    # Box3DList.enlarge_box3d and the corner conversion, against the reference's corners (same torch-CPU expressions: same bits)
    boxes = Box3DList(torch.from_numpy(boxes7), (1242, 375), mode="xyzhwl_ry")
    assert np.array_equal(boxes.convert("corners").bbox_3d.numpy().reshape(-1, 8, 3), corners)
    big = boxes.enlarge_box3d(0.2)
    assert big.mode == "xyzhwl_ry"
    assert np.array_equal(big.convert("corners").bbox_3d.numpy().reshape(-1, 8, 3), large)
    grown = big.bbox_3d.numpy() - boxes7
    assert np.allclose(grown[:, 3:6], 0.4, atol=1e-6) and np.allclose(grown[:, 1], 0.2, atol=1e-6) and not grown[:, [0, 2, 6]].any()
    assert boxes.convert("corners").enlarge_box3d(0.2).mode == "corners"


def test_symbols_declared_bound_and_built_from_source():
    from disprcnn_amd.pts import _lib, build
    assert "train_targets.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "disprcnn_amd", "pts", "train_targets.hip"))
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.EXPORTED_SYMBOLS


def test_cpu_tensors_raise():
    from disprcnn_amd.layers import pointrcnn_loss as L
    lay = O.LAYOUTS["rpn52"]
    pred, lab = torch.zeros(4, 52), torch.zeros(4, 7)
    with pytest.raises(RuntimeError):
        L.rpn_point_labels(torch.zeros(1, 4, 3), torch.zeros(1, 7), torch.zeros(1, 8, 3), torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError):
        L.reg_bin_targets(lab, anchor_size=torch.ones(3), **lay)
    with pytest.raises(RuntimeError):
        L.bin_reg_loss(pred, lab, None, anchor_size=torch.ones(3), **lay)
    for kind in L.CLS_KINDS:
        with pytest.raises(RuntimeError):
            L.point_cls_loss(kind, torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError):
        L.focal_loss_elementwise(torch.zeros(4), torch.zeros(4), torch.ones(4))
    with pytest.raises(NotImplementedError):
        L.point_cls_loss("CrossEntropy", torch.zeros(4), torch.zeros(4))


def test_reference_names_resolve_and_unsupported_settings_raise():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net import point_rcnn
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_loss import PointRCNNBox3dLossComputation
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn_loss import PointRCNNLossComputation
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.utils import loss_utils
    assert callable(point_rcnn.generate_rpn_training_labels)
    for n in ("DiceLoss", "SigmoidFocalClassificationLoss", "get_reg_loss"):
        assert hasattr(loss_utils, n)
    PointRCNNLossComputation(O.cfg_for({}))
    PointRCNNBox3dLossComputation(O.cfg_for({}))
    with pytest.raises(NotImplementedError):
        PointRCNNBox3dLossComputation(O.cfg_for({"rcnn": {"LOSS_CLS": "CrossEntropy"}}))
    with pytest.raises(NotImplementedError):
        PointRCNNLossComputation(O.cfg_for({"rpn": {"LOSS_CLS": "CrossEntropy"}}))
    with pytest.raises(ImportError):                      # the alias of the incomplete subtree stays pinned
        __import__("disprcnn.modeling.pointnet_module.point_rcnn.lib.net.rpn_loss")

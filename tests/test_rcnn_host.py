"""Host tests of the RCNN stage's fixtures and oracle: tests/rcnn_oracle.py (the NumPy restatement the GPU tests lean on) is pinned to the
recordings of the imported reference in tests/golden/rcnn_ref_golden.npz, the decode is checked on hand-computed cases, Box3DList
against the golden, and the new module tree and C ABI are checked for shape.  No GPU."""
import copy
import json
import os
import re

import numpy as np
import pytest

from . import rcnn_oracle as CO
from . import rpn_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


@pytest.fixture(scope="module")
def G():
    path = os.path.join(HERE, "golden", "rcnn_ref_golden.npz")
    assert os.path.getsize(path) < (1 << 20)
    return np.load(path)


@pytest.fixture(scope="module")
def cfg():
    with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as f:
        return RO.make_cfg(json.load(f))


def new_net(cfg):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    return RCNNNet(cfg, None).eval()


def test_state_dict_keys_and_shapes_equal_the_reference(G, cfg):
    sd = new_net(cfg).state_dict()
    assert list(sd.keys()) == [str(k) for k in G["state_dict_keys"]]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in G["state_dict_shapes"]]
    c = copy.deepcopy(cfg)
    c["RCNN"]["USE_BN"], c["RCNN"]["DP_RATIO"] = True, -1.0
    keys = list(new_net(c).state_dict().keys())
    assert "cls_layer.1.conv.weight" in keys and "xyz_up_layer.layer0.bn.bn.running_mean" in keys and "cls_layer.0.conv.bias" not in keys


def test_point_rcnn_holds_both_networks_under_the_reference_names(G, cfg):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    total = RO.make_cfg({"MODEL": {"POINTRCNN": json.loads(json.dumps(cfg))}})
    keys = list(PointRCNN(total).state_dict().keys())
    want = [str(k) for k in G["state_dict_keys"]]
    assert [k[len("rcnn_net."):] for k in keys if k.startswith("rcnn_net.")] == want
    assert all(k.startswith(("rpn.", "rcnn_net.")) for k in keys) and any(k.startswith("rpn.backbone_net.") for k in keys)
    total["MODEL"]["POINTRCNN"]["RCNN"]["ENABLED"] = False
    assert not hasattr(PointRCNN(total), "rcnn_net")


def test_unsupported_settings_raise(cfg):
    import torch
    for key, val in (("USE_INTENSITY", True), ("SIZE_RES_ON_ROI", True), ("USE_MASK", False)):
        c = copy.deepcopy(cfg)
        c["RCNN"][key] = val
        with pytest.raises(NotImplementedError):
            new_net(c)
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    with pytest.raises(NotImplementedError):
        RCNNNet(cfg, None, num_classes=3)
    m = new_net(cfg).train()
    with pytest.raises(NotImplementedError):
        m({})
    with pytest.raises(NotImplementedError):
        m.refine({})
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    with pytest.raises(NotImplementedError):
        Box3DList(torch.zeros(1, 7), (1, 1), "xyzhwl_ry", frame="velodyne")
    with pytest.raises(ValueError):
        Box3DList(torch.zeros(1, 7), (1, 1), "alpha_lhwxyz")


def test_fixtures_hold_the_cases_the_checks_need(G, cfg):
    S = cfg.RCNN.NUM_POINTS
    for tag in CO.BATCHES:
        inp = CO.make_inputs(tag, int(G["input_bump"]))
        M = inp["roi_boxes3d"].shape[1]
        assert M >= 16 and (inp["roi_boxes3d"][:, M - 1] == 0).all()
        cnt = G[f"{tag}_count"].reshape(-1, M)
        assert (cnt[:, 1] == 0).all() and ((cnt > 0) & (cnt < S)).any() and (cnt > S).any()
    assert G["b5_list_random"].tolist() == [0, 0, 0, 1, 0] and G["b5_list_random_len"][3] == 7          # the reference sizes it by the box's 7 values
    n_sel = (CO.sigmoid(G["b2_post_cls"].reshape(2, -1)) > F(cfg.RCNN.SCORE_THRESH)).sum(1)
    assert (G["b2_list_n"] < n_sel).any()                                                              # NMS dropped a box


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_oracle_pooling_reproduces_the_recorded_selection(G, cfg, tag):
    inp = CO.make_inputs(tag, int(G["input_bump"]))
    rc = cfg.RCNN
    p = CO.pool_canonical(inp, rc.POOL_EXTRA_WIDTH, rc.NUM_POINTS, rc.USE_DEPTH, F)
    assert np.array_equal(p["idx"], G[f"{tag}_sel_idx"]) and np.array_equal(p["empty"], G[f"{tag}_empty"])
    assert np.array_equal(p["count"], G[f"{tag}_count"]) and p["margin"] >= 1e-4
    assert float(G[f"{tag}_canon_err_eps"]) <= 6.0
    e = p["empty"] == 1
    assert (p["feat"][e] == 0).all() and (p["pts"][e][:, 3:] == 0).all() and (np.abs(p["xyz"][e]).max(axis=(1, 2)) > 1).any()


def test_oracle_network_reproduces_the_fp64_recordings(G, cfg):
    tag = "b2"
    inp = CO.make_inputs(tag, int(G["input_bump"]))
    rc = cfg.RCNN
    pin = CO.pts_input_of(CO.pool_canonical(inp, rc.POOL_EXTRA_WIDTH, rc.NUM_POINTS, rc.USE_DEPTH, F))
    model = new_net(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = CO.random_state(shapes, int(G["weight_seed"]))
    levels, cls, reg = CO.network(sd, cfg, pin, np.float64)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(cls, G[f"{tag}_rcnn_cls64"]) <= 1e-9 and rel(reg, G[f"{tag}_rcnn_reg64"]) <= 1e-9
    rois = G["b2_lev_rois"]
    for name in ("xyz_up", "merge_down", "sa0", "sa1", "sa2"):
        assert rel(levels[name][rois][:, :, G[f"b2_pts_{name}"]], G[f"b2_{name}64"]) <= 1e-9, name


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_oracle_decode_and_postprocess_reproduce_the_reference(G, cfg, tag):
    inp = CO.make_inputs(tag, int(G["input_bump"]))
    rc, rois = cfg.RCNN, inp["roi_boxes3d"]
    reg, pcls = G[f"{tag}_rcnn_reg"], G[f"{tag}_post_cls"]
    assert np.array_equal(pcls, CO.post_cls(tag, G[f"{tag}_rcnn_cls"]))
    assert np.array_equal(CO.decode_bins(reg, rc), G[f"{tag}_dec_bins"]) and CO.argmax_margin(reg, rc) >= 1e-4
    d64 = CO.decode(rois.reshape(-1, 7), reg, rc, cfg.MEAN_SIZE[0], np.float64, G[f"{tag}_dec_bins"].astype(np.int64))
    assert np.abs(d64 - G[f"{tag}_dec_boxes64"]).max() <= 1e-9 * np.abs(d64).max()
    d32 = CO.decode(rois.reshape(-1, 7), reg, rc, cfg.MEAN_SIZE[0], F)
    assert np.abs(d32.astype(np.float64) - G[f"{tag}_dec_boxes"]).max() <= 2 * float(G["err32_max_dec_boxes"])
    lists, m_score, m_nms = CO.postprocess(rc, cfg.MEAN_SIZE[0], rois, inp["roi_scores_raw"], pcls, reg)
    assert m_score >= 1e-4 and m_nms >= 1e-4
    assert [len(d["keep"]) for d in lists] == G[f"{tag}_list_n"].tolist()
    assert [int(d["fallback"]) for d in lists] == G[f"{tag}_list_random"].tolist()
    assert np.array_equal(np.concatenate([d["keep"] for d in lists]), G[f"{tag}_keep"])
    assert np.array_equal(np.concatenate([d["scores"] for d in lists]), G[f"{tag}_list_scores"])
    boxes = np.concatenate([CO.to_ry_lhwxyz(d["boxes"]) for d in lists])
    assert np.abs(boxes - G[f"{tag}_list_boxes"]).max() <= 2e-5
    best = CO.best_of(lists)
    assert all(int(np.argmax(d["scores"])) == 0 for d in lists) and len(best) == rois.shape[0]


def test_decode_hand_cases(cfg):
    rc = cfg.RCNN
    L = CO.reg_layout(rc)
    assert (L["nb"], L["hb"], L["R"]) == (6, 9, 46)
    reg = np.zeros((2, L["R"]), F)
    # row 0: x bin 4 (+0.75), z bin 1 (-0.75), residuals 0.2 / -0.4 bins, y offset 0.3, angle bin 4 (the middle: 0) + 0.5 half bins, sizes +10 %
    reg[0, 4], reg[0, 6 + 1] = 1, 1
    reg[0, 12 + 4], reg[0, 18 + 1] = 0.2, -0.4
    reg[0, 24] = 0.3
    reg[0, 25 + 4], reg[0, 34 + 4] = 1, 0.5
    reg[0, 43:46] = 0.1
    reg[1] = reg[0]
    roi = np.array([[10, 1, 20, 1.5, 1.6, 3.9, 0.0], [10, 1, 20, 1.5, 1.6, 3.9, np.pi / 2]], F)
    out = CO.decode(roi, reg, rc, cfg.MEAN_SIZE[0], np.float64)
    apc = (np.pi / 2) / 9
    px, pz = 0.75 + 0.2 * 0.5, -0.75 - 0.4 * 0.5
    h, w, l = (np.asarray(cfg.MEAN_SIZE[0], np.float64).astype(F).astype(np.float64) * F(1.1).astype(np.float64))
    assert np.allclose(out[0], [10 + px, 1.3, 20 + pz, h, w, l, 0.5 * apc / 2], atol=1e-6)
    # a ROI turned by 90 degrees: its own x axis points along -z of the camera frame
    assert np.allclose(out[1], [10 + pz, 1.3, 20 - px, h, w, l, float(F(np.pi / 2)) + 0.5 * apc / 2], atol=1e-6)
    tie = np.zeros((1, L["R"]), F)                         # all bins equal: the first maximum, bin 0
    assert CO.decode_bins(tie, rc).tolist() == [[0, 0, 0, 0]]
    c = copy.deepcopy(rc)
    c["LOC_Y_BY_BIN"] = True
    Ly = CO.reg_layout(c)
    assert Ly["R"] == 24 + 8 + 18 + 3
    r = np.zeros((1, Ly["R"]), F)
    r[0, 24 + 3], r[0, 28 + 3] = 1, 0.5                    # y bin 3 of 4 (+0.375), residual half a bin
    assert np.isclose(CO.decode(roi[:1], r, c, cfg.MEAN_SIZE[0], np.float64)[0, 1], 1 + 0.375 + 0.125)


def test_box3dlist_conversions_match_the_golden(G):
    import torch
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    b7 = torch.from_numpy(G["box_b7"])
    bl = Box3DList(b7, (1280, 720), "xyzhwl_ry")
    corners = bl.convert("corners")
    assert len(bl) == 12 and len(bl[2:5]) == 3 and bl.to("cpu").mode == "xyzhwl_ry" and bl.convert("xyzhwl_ry") is bl
    tol = 1e-5
    # *32: the reference's own Box3DList (it keeps fp32 whatever it is given); *64: the oracle's fp64 evaluation, stored for scale only
    assert np.abs(corners.bbox_3d.numpy() - G["box_corners32"]).max() <= tol and np.abs(G["box_corners64"] - G["box_corners32"]).max() <= tol
    assert np.abs(corners.convert("xyzhwl_ry").bbox_3d.numpy() - G["box_back32"]).max() <= tol
    ry = bl.convert("ry_lhwxyz").bbox_3d.numpy()
    assert np.abs(ry - G["box_rylhw32"]).max() <= tol and np.abs(CO.to_ry_lhwxyz(G["box_b7"]) - G["box_rylhw32"]).max() <= tol
    assert np.abs(CO.box_corners(G["box_b7"]) - G["box_corners32"]).max() <= tol                # the oracle against the reference
    assert (ry[-1] == 0).all()                             # a zero box stays a zero box with angle 0
    cam = CO.rois_to_camera(G["box_b7"].reshape(3, 4, 7), G["box_mean"], G["box_rot"])
    assert np.abs(cam - G["box_cam32"]).max() <= 2e-5
    assert Box3DList(torch.zeros(0, 3), (1, 1), "ry_lhwxyz").bbox_3d.shape == (0, 7)


def test_header_symbols_and_sources_agree_for_the_new_entries():
    from disprcnn_amd.pts import _lib, build
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "rcnn_ops.hip")).read()
    assert "rcnn_ops.hip" in build.SOURCES
    for name in ("drc_rcnn_pool_canonical_fwd", "drc_rcnn_decode_boxes"):
        assert name in _lib.EXPORTED_SYMBOLS
        decl = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r'extern "C" int\s+%s\s*\(([^{]*?)\)\s*\{' % name, src, re.S)
        assert decl and defn
        n_args = len(decl.group(1).split(","))
        assert n_args == len(defn.group(1).split(",")) == len(_lib._SIGS[name][1])
    assert "box3d_pt.h" in src and "box3d_pt.h" in open(os.path.join(ROOT, "disprcnn_amd", "pts", "boxes3d.hip")).read()

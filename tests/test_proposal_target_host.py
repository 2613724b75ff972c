"""ProposalTargetLayer without a GPU: tests/proposal_target_oracle.py against the imported reference's recording
(tests/golden/proposal_target_golden.npz), the C surface of the two new kernels, and the argument checks of the Python layers.

Tolerance of the oracle's fp32 mode against the fp64 recording, per case and tensor, the rule of tests/test_hip_rcnn_train.py: max error
<= 4 x and mean error <= 2 x the reference's own fp32-vs-fp64 error (err32_max_* / err32_mean_*), plus the floor 1e-6 * max|ref|.  Integers,
flags, indices and iteration counts are exact; the noise boxes, which the reference makes with additions and multiplications alone
('multiple'; the position of 'single'), are bit for bit the fp32 recording; the oracle's fp64 mode equals the fp64 recording to 1e-9.

The alias package keeps `disprcnn.modeling.pointnet_module` unresolved on purpose (tests/test_alias_package.py pins that), so the layer is
imported under the implementation's name here.
"""
import copy
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import proposal_target_oracle as PO
from tests import rcnn_train_oracle as TO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("drc_rcnn_sample_max_candidates", "drc_rcnn_sample_max_slots", "drc_rcnn_sample_rois", "drc_rcnn_pool_target_fwd")
f32 = np.float32


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "proposal_target_golden.npz"))


@pytest.fixture(scope="module")
def cfg_json():
    with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as f:
        return json.load(f)


_RUNS = {}


def oracle_run(G, cfg_json, case, dtype):
    """the oracle on one case's seeded inputs, computed once per (case, dtype)"""
    key = (case, dtype)
    if key not in _RUNS:
        st = PO.settings(PO.case_cfg(cfg_json, case))
        bump = int(G["input_bump"])
        _RUNS[key] = (st,) + PO.layer(st, PO.make_inputs(case, bump), PO.make_draws(case, bump), dtype)
    return _RUNS[key]


def within(name, got, ref, emax, emean, floor):
    err = np.abs(np.asarray(got, np.float64) - ref)
    r_max, r_mean = err.max() / (4 * emax + floor), err.mean() / (2 * emean + floor)
    print(f"{name}: max err {err.max():.3g} (reference fp32 {emax:.3g}), mean err {err.mean():.3g} (reference fp32 {emean:.3g}), floor {floor:.3g}; "
          f"ratio to the bound: max {r_max:.3f} mean {r_mean:.3f}")
    return r_max <= 1.0 and r_mean <= 1.0


def recorded_view(G, case, sampled, pool):
    """the oracle's results on the recorded clouds, under the recording's names"""
    nb, P = len(G["clouds"]), PO.CASES[case]["P"]
    assert list(G["clouds"]) == list(range(nb))
    R = nb * P
    return {"noise_rois": sampled["rois"][:nb], "gt_raw": sampled["gt_of_rois"][:nb], "gt_iou": sampled["roi_iou"][:nb].reshape(-1),
            "src_index": sampled["src_index"][:nb], "n_iter": sampled["n_iter"][:nb], "counts": sampled["counts"][:nb, :4],
            "cls_label": pool["cls_label"][:R], "reg_valid_mask": pool["reg_valid_mask"][:R], "roi_boxes3d": pool["roi_boxes3d"][:R],
            "gt_of_rois": pool["gt_of_rois"][:R], "sampled_pts": pool["xyz"][:R], "sel_idx": pool["idx"][:R], "empty": pool["empty_flag"][:R],
            "count": pool["count"][:R]}


@pytest.mark.parametrize("case", sorted(PO.CASES))
def test_oracle_equals_the_reference_recording(G, cfg_json, case):
    st, s32, p32 = oracle_run(G, cfg_json, case, f32)
    mine = recorded_view(G, case, s32, p32)
    for name in ("src_index", "n_iter", "counts", "cls_label", "reg_valid_mask", "sel_idx", "empty", "count"):
        assert np.array_equal(mine[name], G[f"{case}_{name}"]), name
    assert np.array_equal(mine["gt_raw"], G[f"{case}_gt_raw"])
    cols = slice(0, 7) if st["method"] == "multiple" else slice(0, 3)
    assert mine["noise_rois"].dtype == G[f"{case}_noise_rois"].dtype == f32
    assert np.array_equal(mine["noise_rois"][..., cols], G[f"{case}_noise_rois"][..., cols]), "the noise boxes are not the recording's bits"
    bad = []
    for name in ("noise_rois", "gt_iou", "roi_boxes3d", "gt_of_rois", "sampled_pts"):
        ref = G[f"{case}_{name}64"]
        if not within(f"{case} {name}", mine[name], ref, float(G[f"err32_max_{case}_{name}"]), float(G[f"err32_mean_{case}_{name}"]),
                      1e-6 * np.abs(ref).max()):
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize("case", sorted(PO.CASES))
def test_fp64_oracle_equals_the_fp64_recording(G, cfg_json, case):
    _, s64, p64 = oracle_run(G, cfg_json, case, np.float64)
    mine = recorded_view(G, case, s64, p64)
    for name in ("src_index", "n_iter", "counts", "cls_label", "reg_valid_mask"):
        assert np.array_equal(mine[name], G[f"{case}_{name}"]), name
    for name in ("noise_rois", "gt_iou", "roi_boxes3d", "gt_of_rois", "sampled_pts"):
        ref = G[f"{case}_{name}64"]
        assert np.abs(mine[name] - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1.0), name


def test_the_cloud_without_a_candidate_takes_its_candidates_in_turn(G, cfg_json):
    for case, k in PO.CASES.items():
        _, s, p = oracle_run(G, cfg_json, case, f32)
        b, P, M = PO.NONE_CLOUD, k["P"], k["M"]
        assert s["counts"][b].tolist() == [0, 0, 0, 0, 1] and not s["counts"][:b, 4].any()
        assert np.array_equal(s["src_index"][b], np.arange(P) % M) and not s["n_iter"][b].any()
        inp = PO.make_inputs(case, int(G["input_bump"]))
        assert np.array_equal(s["rois"][b], inp["roi_boxes3d"][b][np.arange(P) % M])
        assert (p["cls_label"][b * P:] == -1).all() and not p["reg_valid_mask"][b * P:].any()


def test_draw_layout(cfg_json):
    from disprcnn_amd.layers import proposal_target as PT
    for M, P, T in ((1, 5, 0), (70, 16, 10), (512, 64, 10)):
        o = PO.blocks(M, P, T)
        assert PT.draw_blocks(M, P, T) == o and PT.draws_per_cloud(M, P, T) == o["len"] == M + P + 9 * P * T + 3 * P
    g = torch.Generator().manual_seed(5)
    a = PT.proposal_draws(3, 7, 4, 2, "cpu", generator=g)
    b = PT.proposal_draws(3, 7, 4, 2, "cpu", generator=torch.Generator().manual_seed(5))
    assert a.shape == (3, PO.blocks(7, 4, 2)["len"]) and a.dtype == torch.float32 and torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0


def test_new_symbols_are_declared_defined_and_exported():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib, build
    assert "proposal_target.hip" in build.SOURCES
    assert any(p.endswith("box3d_iou.h") for p in build.SHARED)
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "proposal_target.hip")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name)
        decl = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^{;]*?)\)\s*\{" % name, src, re.S)
        assert decl and defn, name
        n_args = 0 if decl.group(1).strip() == "void" else len(decl.group(1).split(","))
        assert n_args == (0 if defn.group(1).strip() == "void" else len(defn.group(1).split(","))) == len(_lib._SIGS[name][1]), name
    assert handle.drc_rcnn_sample_max_candidates() >= 512 and handle.drc_rcnn_sample_max_slots() >= 64      # TRAIN.RPN_POST_NMS_TOP_N, the default
    for banned in ("hipMalloc", "hipMemcpy", "Synchronize", "atomic"):
        assert banned not in src
    boxes = open(os.path.join(ROOT, "disprcnn_amd", "pts", "boxes3d.hip")).read()
    assert '#include "box3d_iou.h"' in boxes and "struct BoxG" not in boxes           # one copy of the rotated-overlap code


def test_c_entries_refuse_bad_arguments_before_a_launch():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib
    L = _lib.lib()
    F, Dd, P = ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    mc, ms = L.drc_rcnn_sample_max_candidates(), L.drc_rcnn_sample_max_slots()

    def sample(B=1, M=8, N=1, Pn=4, T=2, fgpi=2, method=0, stride=None):
        stride = M + Pn + 9 * Pn * T + 3 * Pn if stride is None else stride
        return L.drc_rcnn_sample_rois(B, M, N, Pn, T, fgpi, method, F(0.55), F(0.45), F(0.05), Dd(0.8), P(0), P(0), P(0), stride, P(0), P(0), P(0), P(0),
                                      P(0), P(0), P(0))
    assert sample() == -1                                  # well-formed, null pointers
    assert sample(B=0) == 0
    for kw in (dict(M=0), dict(M=mc + 1), dict(Pn=0), dict(Pn=ms + 1), dict(N=0), dict(T=-1), dict(fgpi=5), dict(method=2), dict(stride=10)):
        assert sample(**kw) == -2, kw
    assert sample(M=mc, Pn=ms) == -1                       # the limits themselves are admitted

    def pool(B=1, N=10, Pn=4, C=2, S=8, aug=1, stride=12):
        return L.drc_rcnn_pool_target_fwd(B, N, Pn, C, S, P(0), P(0), P(0), P(0), 1, P(0), P(0), P(0), P(0), P(0), stride, aug, F(0.17), F(1), F(2), F(0.55),
                                          F(0.6), F(0.45), P(0), P(0), P(0), P(0), P(0), P(0), P(0), P(0), P(0))
    assert pool() == -1 and pool(B=0) == 0
    for kw in (dict(S=0), dict(S=L.drc_box3d_max_pool_samples() + 1), dict(stride=11), dict(C=-1)):
        assert pool(**kw) == -2, kw


def test_layers_validate_their_arguments(cfg_json):
    from disprcnn_amd.layers import proposal_target as PT
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.rpn.proposal_target_layer import ProposalTargetLayer
    assert list(inspect.signature(ProposalTargetLayer.__init__).parameters) == ["self", "cfg", "total_cfg"]
    rois, gt = torch.zeros(2, 8, 7), torch.zeros(2, 1, 7)
    draws = PT.proposal_draws(2, 8, 4, 2, "cpu")
    args = (4, 0.5, 0.55, 0.6, 0.45, 0.05, 0.8, 2)
    with pytest.raises(RuntimeError):                      # no CPU fallback
        PT.rcnn_sample_rois(rois, gt, draws, *args)
    with pytest.raises(NotImplementedError, match="normal"):
        PT.rcnn_sample_rois(rois, gt, draws, *args, aug_method="normal")
    with pytest.raises(NotImplementedError):
        PT.rcnn_sample_rois(rois, gt, draws, *args, aug_method="other")
    sampled = {"rois": torch.zeros(2, 4, 7), "gt_of_rois": torch.zeros(2, 4, 7), "roi_iou": torch.zeros(2, 4), "counts": torch.zeros(2, 5, dtype=torch.int32)}
    with pytest.raises(RuntimeError):
        PT.rcnn_pool_target(torch.zeros(2, 10, 3), torch.zeros(2, 3, 10), torch.zeros(2, 10), None, sampled, draws, 1.0, 0.55, 0.6, 0.45,
                            sampled_pt_num=8, num_candidates=8, fg_aug_times=2)
    cfg = PO.case_cfg(cfg_json, "a")
    normal = copy.deepcopy(cfg)
    normal["RCNN"]["REG_AUG_METHOD"] = "normal"
    layer = ProposalTargetLayer(normal, None)
    assert not list(layer.parameters())
    with pytest.raises(NotImplementedError, match="normal"):
        layer({}, gt)
    with pytest.raises(RuntimeError):
        ProposalTargetLayer(cfg, None)({"roi_boxes3d": rois, "rpn_xyz": torch.zeros(2, 10, 3), "backbone_features": torch.zeros(2, 3, 10),
                                        "seg_mask": torch.zeros(2, 10), "pts_depth": torch.zeros(2, 10)}, gt)
    # the training forward without the ground truth keeps raising, and names the layer
    jit = TO.train_cfg(cfg_json)
    jit["RCNN"]["ROI_SAMPLE_JIT"] = True
    net = RCNNNet(jit, None)
    assert isinstance(net.proposal_target_layer, ProposalTargetLayer)
    assert not any(k.startswith("proposal_target_layer") for k in net.state_dict())
    with pytest.raises(NotImplementedError, match="ProposalTargetLayer.*ground-truth"):
        net.train()({"roi_boxes3d": rois})
    with pytest.raises(NotImplementedError, match="ProposalTargetLayer"):
        net.train()({"roi_boxes3d": rois}, targets=None)

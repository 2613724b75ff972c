"""PointRCNN's training input on the CPU: the training draw against a direct NumPy restatement of the reference's calls, the two proposal
filters, Matcher and boxlist_iou against hand values, the gates of PointRCNN.forward and DispRCNN3D.forward in training mode, the C ABI of
the new entry points, and the reference's import names."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from disprcnn_amd.structures.bounding_box import BoxList
from disprcnn_amd.structures.bounding_box_3d import Box3DList
from tests import rpn_oracle as RO

from .conftest import GOLDEN, ROOT

NEW_SYMBOLS = {"drc_instance_points_train_fwd": "points.hip", "drc_instance_points_gather_train_fwd": "points.hip",
               "drc_match_targets_fwd": "match2d.hip", "drc_camera_to_rpn_fwd": "frame_ops_train.hip"}


# ---- 1. the draw
def _reference_stream(rs, counts, npoints, fixed):
    """point_rcnn.py:59-73 per ROI, then :145-154, on the generator rs"""
    out = []
    for n in counts:
        if n > npoints:
            choice = rs.choice(n, npoints, replace=False)
        else:
            choice = rs.choice(n, npoints - n, replace=True)
            choice = np.concatenate((np.arange(n), choice))
        rs.shuffle(choice)
        out.append(choice)
    scale, flip = 1.0, False
    if not fixed:
        scale = rs.uniform(0.95, 1.05)
        flip = rs.random() < 0.5
    return out, scale, flip


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_training_draw_is_the_reference_stream(seed):
    from disprcnn_amd.modeling.pointcloud import draw_augmentation, draw_choice_train
    npoints, counts = 96, [40, 96, 500, 1, 97, 95]
    want, scale, flip = _reference_stream(np.random.RandomState(seed), counts, npoints, False)
    rs = np.random.RandomState(seed)
    got = [draw_choice_train(n, npoints, rs) for n in counts]
    got_scale, got_flip = draw_augmentation(rs)
    for n, a, b in zip(counts, got, want):
        assert a.shape == (npoints,) and np.array_equal(a, b), n
        assert a.min() >= 0 and a.max() < n
        assert (len(set(a.tolist())) == npoints) if n >= npoints else (set(a.tolist()) == set(range(n)))
    assert got_scale == scale and got_flip == flip and 0.95 <= got_scale < 1.05 and isinstance(got_flip, bool)
    # the default generator is the numpy.random module itself, as in the reference: np.random.seed(k) gives the same stream
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        again = [draw_choice_train(n, npoints) for n in counts]
        assert all(np.array_equal(a, b) for a, b in zip(again, want)) and draw_augmentation() == (scale, flip)
        # RPN.FIXED: nothing is drawn after the clouds, so the next value of the stream is the one a fresh replay gives
        np.random.seed(seed)
        for n in counts:
            draw_choice_train(n, npoints)
        nxt = np.random.random()
    finally:
        np.random.set_state(state)
    rs = np.random.RandomState(seed)
    _reference_stream(rs, counts, npoints, True)
    assert nxt == rs.random()
    with pytest.raises(ValueError):
        draw_choice_train(0, npoints, rs)


# ---- 2. the filters
def _pair(left, right, size=(1242, 375)):
    lb = BoxList(torch.tensor(left, dtype=torch.float32).reshape(-1, 4), size)
    lb.add_field("tag", torch.arange(len(lb)))
    return lb, BoxList(torch.tensor(right, dtype=torch.float32).reshape(-1, 4), size)


def test_remove_too_right_proposals():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import remove_too_right_proposals
    l0, r0 = _pair([[100, 10, 150, 60], [100, 10, 150, 60], [100, 10, 150, 60], [0, 10, 50, 60], [0, 10, 50, 60]],
                   [[70, 10, 120, 60], [100, 10, 150, 60], [105, 10, 155, 60], [0, 10, 50, 60], [5, 10, 55, 60]])
    l1, r1 = _pair([], [])
    left, right = remove_too_right_proposals([l0, l1], [r0, r1])
    assert left[0].get_field("tag").tolist() == [0, 3, 4]                 # x1 > x1p, or x1 == 0 whatever the right box
    assert torch.equal(right[0].bbox, r0.bbox[[0, 3, 4]]) and len(left[1]) == len(right[1]) == 0
    assert len(l0) == 5                                                   # the inputs are left alone


def test_filter_unmatched_idxs():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import filter_unmatched_idxs
    matched = [torch.tensor([0, -1, 1]), torch.zeros(0, dtype=torch.int64), torch.tensor([-2, 0])]
    targets, r = [], 0
    for m in matched:
        t = BoxList(torch.arange(4.0 * len(m)).reshape(-1, 4) + r, (1242, 375))
        t.add_field("box3d", Box3DList(torch.arange(24.0 * len(m)).reshape(-1, 24) + r, (1242, 375), "corners"))
        t.add_field("calib", "calibration of the image")
        t.add_field("matched_idxs", m)
        targets.append(t)
        r += 100
    proposals = {"roi_boxes3d": torch.arange(5 * 2 * 7.0).reshape(5, 2, 7), "rpn_xyz": torch.arange(5 * 3 * 3.0).reshape(5, 3, 3)}
    out, kept = filter_unmatched_idxs(proposals, targets)
    assert sorted(out) == sorted(proposals)
    for k in proposals:
        assert torch.equal(out[k], proposals[k][[0, 2, 4]]), k
    assert [len(t) for t in kept] == [2, 0, 1]
    assert torch.equal(kept[0].get_field("box3d").bbox_3d, targets[0].get_field("box3d").bbox_3d[[0, 2]])
    assert torch.equal(kept[2].bbox, targets[2].bbox[[1]]) and kept[2].get_field("matched_idxs").tolist() == [0]
    assert kept[0].get_field("calib") == "calibration of the image" and kept[0].get_field("box3d").mode == "corners"
    # nothing unmatched: the same tensors come back
    for t in targets:
        t.add_field("matched_idxs", t.get_field("matched_idxs").clamp(min=0))
    out, kept = filter_unmatched_idxs(proposals, targets)
    assert all(out[k] is proposals[k] for k in proposals) and [len(t) for t in kept] == [3, 0, 2]


# ---- 3. Matcher and boxlist_iou
def test_boxlist_iou_and_matcher_hand_values():
    from disprcnn_amd.modeling.matcher import Matcher
    from disprcnn_amd.structures.boxlist_ops import boxlist_iou
    size = (100, 100)
    gt = BoxList(torch.tensor([[0.0, 0.0, 9.0, 9.0], [20.0, 20.0, 39.0, 29.0]]), size)                   # areas 100 and 200
    pr = BoxList(torch.tensor([[0.0, 0.0, 9.0, 9.0], [5.0, 0.0, 14.0, 9.0], [20.0, 20.0, 29.0, 29.0], [50.0, 50.0, 59.0, 59.0],
                               [0.0, 0.0, 9.0, 3.0]]), size)
    iou = boxlist_iou(gt, pr)
    want = torch.tensor([[1.0, 50.0 / 150.0, 0.0, 0.0, 0.4], [0.0, 0.0, 0.5, 0.0, 0.0]])
    assert iou.shape == (2, 5) and torch.allclose(iou, want, rtol=0, atol=1e-7) and iou[0, 0] == 1 and iou[1, 2] == 0.5      # TO_REMOVE = 1
    with pytest.raises(RuntimeError):
        boxlist_iou(gt, BoxList(pr.bbox, (99, 100)))
    m = Matcher(0.5, 0.35, allow_low_quality_matches=False)(iou.clone())
    assert m.dtype == torch.int64 and m.tolist() == [0, -1, 1, -1, -2]     # 1/3 < 0.35: below; 0.4: between; 0.5 >= high: matched
    assert (Matcher.BELOW_LOW_THRESHOLD, Matcher.BETWEEN_THRESHOLDS) == (-1, -2)
    # low-quality matches: every prediction that is some ground truth's best (ties included) gets its arg-max back
    q = torch.tensor([[0.2, 0.2, 0.1, 0.0], [0.0, 0.1, 0.3, 0.0]])
    assert Matcher(0.5, 0.35, allow_low_quality_matches=False)(q.clone()).tolist() == [-1, -1, -1, -1]
    assert Matcher(0.5, 0.35, allow_low_quality_matches=True)(q.clone()).tolist() == [0, 0, 1, -1]
    tie = torch.tensor([[0.7, 0.1], [0.7, 0.1]])
    assert Matcher(0.5, 0.5)(tie).tolist() == [0, -1]                      # ties go to the lowest ground-truth index
    with pytest.raises(ValueError):
        Matcher(0.5, 0.5)(torch.zeros(0, 3))
    with pytest.raises(ValueError):
        Matcher(0.5, 0.5)(torch.zeros(3, 0))
    with pytest.raises(ValueError):
        Matcher(0.3, 0.5)


# ---- 4. the gates
def _pointrcnn_cfg(fixed=True, rcnn=True, rcnn_train=True):
    with open(os.path.join(GOLDEN, "rcnn_cfg_car.json")) as f:
        c = json.load(f)
    c["RPN"]["FIXED"], c["RCNN"]["ENABLED"], c["RCNN"]["TRAIN"] = fixed, rcnn, rcnn_train
    c["TRAINED_MODEL"] = ""
    return RO.make_cfg(c)


def _detector_cfg(dispnet, det3d, train_pc, **kw):
    from disprcnn_amd.modeling.detector.disprcnn3d import default_cfg
    cfg = copy.deepcopy(default_cfg())
    cfg.MODEL.DISPNET_ON, cfg.MODEL.DET3D_ON, cfg.SOLVER.TRAIN_PC = dispnet, det3d, train_pc
    cfg.MODEL.POINTRCNN = _pointrcnn_cfg(**kw)
    return cfg


def test_training_gates_of_point_rcnn_and_the_detector():
    from disprcnn_amd.modeling.detector.disprcnn3d import DispRCNN3D
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    nothing = ({"left": None, "right": None}, {"left": [], "right": []}, {"left": []})
    # SOLVER.TRAIN_PC false: the 3D losses would be dropped; said before any input is read
    m = DispRCNN3D(_detector_cfg(False, True, False)).train()
    with pytest.raises(NotImplementedError, match="PointRCNN") as e:
        m(*nothing)
    assert "TRAIN_PC" in str(e.value) and ".eval()" in str(e.value) and "dropped" in str(e.value)
    # the RPN and the RCNN in one step
    joint = PointRCNN(RO.make_cfg({"MODEL": {"POINTRCNN": _pointrcnn_cfg(fixed=False)}})).train()
    with pytest.raises(NotImplementedError, match="KeyError"):
        joint([], [], [])
    # no targets
    with pytest.raises(ValueError, match="targets"):
        joint([], [])
    fixed = PointRCNN(RO.make_cfg({"MODEL": {"POINTRCNN": _pointrcnn_cfg()}})).train()
    with pytest.raises(ValueError, match="targets"):
        fixed([], [], None)
    assert fixed.masker_threshold == 0.5 and (fixed.fg_iou_threshold, fixed.bg_iou_threshold) == (0.5, 0.5)        # the cfg's, the defaults
    # neither stage
    bare = DispRCNN3D(_detector_cfg(False, False, True)).train()
    with pytest.raises(NotImplementedError, match="DISPNET_ON"):
        bare(*nothing)
    # SOLVER.TRAIN_PC true passes the gate: the next complaint is about the missing targets
    m = DispRCNN3D(_detector_cfg(False, True, True)).train()
    with pytest.raises(ValueError, match="lr_targets"):
        m({"left": None, "right": None}, {"left": [], "right": []}, None)


# ---- 5. the C ABI
def test_new_symbols_are_declared_defined_and_exported():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib, build
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, source in NEW_SYMBOLS.items():
        assert source in build.SOURCES
        src = open(os.path.join(ROOT, "disprcnn_amd", "pts", source)).read()
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r'extern "C" int\s+%s\s*\(([^{;]*?)\)\s*\{' % name, src, re.S)
        assert decl and defn, name
        norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]
        assert norm(decl.group(1)) == norm(defn.group(1)) and len(norm(decl.group(1))) == len(_lib._SIGS[name][1]), name
    # the eval entry points keep their signatures
    assert len(_lib._SIGS["drc_instance_points_fwd"][1]) == 13 and len(_lib._SIGS["drc_instance_points_gather_fwd"][1]) == 16
    assert len(_lib._SIGS["drc_rpn_to_camera_fwd"][1]) == 11
    # bad arguments are refused before any launch
    L = _lib.lib()
    assert L.drc_match_targets_fwd(-1, 0, None, None, None, None, 7, 0.5, 0.5, None, None, None) == -2
    assert L.drc_match_targets_fwd(0, 0, None, None, None, None, 7, 0.5, 0.5, None, None, None) == 0
    assert L.drc_match_targets_fwd(3, 1, None, None, None, None, 7, 0.5, 0.5, None, None, None) == -1
    assert L.drc_camera_to_rpn_fwd(2, 8, None, 1.0, 0, None, None, None, None) == -1
    assert L.drc_camera_to_rpn_fwd(0, 8, None, 1.0, 0, None, None, None, None) == 0
    assert L.drc_instance_points_train_fwd(None, 16, None, None, None, 14, 1, 0.7, 2, None, None, 0, None) == -1
    assert L.drc_instance_points_gather_train_fwd(None, 16, None, None, None, 2, None, None, None, 0, 160.0, 1.0, 0, None, None, None, None,
                                                  None) == -2


# ---- 6. the reference's names
def test_alias_names_import():
    from disprcnn.modeling.matcher import Matcher
    from disprcnn.structures.boxlist_ops import boxlist_iou
    import disprcnn_amd.modeling.matcher as real
    import disprcnn_amd.structures.boxlist_ops as real_ops
    assert Matcher is real.Matcher and boxlist_iou is real_ops.boxlist_iou


# ---- 7. the fixture's matching, on the CPU: the torch comparator gives the recorded indices
def test_torch_matcher_gives_the_recorded_indices():
    from disprcnn_amd.modeling.matcher import Matcher
    from disprcnn_amd.structures.boxlist_ops import boxlist_iou
    from tests import pointrcnn_train_oracle as TO
    g = np.load(TO.GOLDEN)
    size = (int(g["W"]), int(g["H"]))
    first_roi = np.concatenate([[0], np.cumsum(g["rois_per_image"])])
    first_gt = np.concatenate([[0], np.cumsum(g["gts_per_image"])])
    matcher = Matcher(float(g["fg_iou"]), float(g["bg_iou"]), allow_low_quality_matches=False)
    got = []
    for roi, img in zip(g["kept_rois"], g["cloud_image"]):
        assert first_roi[img] <= roi < first_roi[img + 1]
        gt = BoxList(torch.from_numpy(g["gt_boxes"][first_gt[img]:first_gt[img + 1]]), size)
        got.append(int(matcher(boxlist_iou(gt, BoxList(torch.from_numpy(g["left_boxes"][roi:roi + 1]), size)))[0]))
    assert got == g["matched_idxs"].tolist() and -1 in got and -2 in got and 1 in got


# ---- 8. the random matching cases of the GPU test: the chosen seed leaves out at most 1 % of them
def test_matching_cases_stay_clear_of_thresholds_and_ties():
    from tests import pointrcnn_train_oracle as TO
    matched, rows, unsafe = TO.matching_reference(TO.matching_case())
    assert len(matched) == sum(TO.MATCH_PROPOSALS) and rows.shape == (len(matched), 7)
    assert unsafe.mean() <= 0.01, unsafe.mean()
    assert {-1, -2, 0, 1} <= set(matched.tolist())                        # every outcome occurs

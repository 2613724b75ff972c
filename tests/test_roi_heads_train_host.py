"""Host-side checks behind tests/test_hip_roi_heads_train.py: the torch restatement of the ROI heads' training step
(tests/roi_heads_train_oracle.py) against the reference's recorded step and against torch's own layers, the ReLU margin of every GPU case,
and the wiring (config keys, state-dict keys, exported symbols).  No GPU.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import roi_heads_train_cases as CS
from tests import roi_heads_train_oracle as TO
from tests.helpers import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_case():
    """the recorded step's inputs rebuilt (tests/golden/make_golden_roi_heads_train.py) -> (fixture, oracle arguments)"""
    from disprcnn_amd.utils import synth
    z = golden_npz("roi_heads_train_golden.npz")
    fl, fr = synth.synth_pyramid(2, CS.BOX_IMG[1], CS.BOX_IMG[0], c=CS.BOX_C, tag=f"rht:golden:{int(z['variant'])}")
    shapes = {k: v for k, v in CS.box_params("shape-only").items()}
    state = synth.synth_det_state({k: torch.zeros(v.shape) for k, v in shapes.items()},
                                  gain={"predictor.cls_score.weight": 3.0, "predictor.bbox_pred.weight": 2.0})
    ends = np.cumsum([0] + list(z["counts"]))
    lb = [z["left_boxes"][a:b] for a, b in zip(ends[:-1], ends[1:])]
    rb = [z["right_boxes"][a:b] for a, b in zip(ends[:-1], ends[1:])]
    args = dict(feats_left=[f.numpy() for f in fl[:4]], feats_right=[f.numpy() for f in fr[:4]], left_boxes=lb, right_boxes=rb, img_h=CS.BOX_IMG[1],
                params={k: v.numpy() for k, v in state.items()}, labels=z["labels"], reg=z["regression_targets"], keep=z["keep"].astype(bool), p=0.2)
    return z, args


def test_oracle_reproduces_the_reference_step():
    """(i) |oracle64 - golden| <= 2 max|oracle32 - oracle64| + 1e-6 max|golden| per tensor: both losses and the parameter gradients"""
    z, args = golden_case()
    r64, r32 = TO.box_step(**args, dtype=torch.float64), TO.box_step(**args, dtype=torch.float32)
    assert r64["pre_lo"] >= 1e-4 * r64["pre_hi"]
    assert (z["labels"] > 0).sum() >= 2 and (z["labels"] == 0).sum() >= 2 and 0.1 < 1 - z["keep"].mean() < 0.3
    for k in ("loss_classifier", "loss_box_reg"):
        e32, err = abs(r32[k] - r64[k]), abs(r64[k] - float(z[k]))
        print(k, "err", err, "e32", e32)
        assert err <= 2 * e32 + 1e-6 * abs(float(z[k])), k
    for k in TO.BOX_PARAMS:
        g = z["grad:" + k].astype(np.float64)
        e32, err = np.abs(r32["grads"][k] - r64["grads"][k]).max(), np.abs(r64["grads"][k] - g).max()
        print(k, "err", err, "e32", e32, "max", np.abs(g).max())
        assert g.shape == r64["grads"][k].shape and np.abs(g).max() > 0 and err <= 2 * e32 + 1e-6 * np.abs(g).max(), k


@pytest.mark.parametrize("which", [5, 1])
def test_mask_oracle_is_torchs_layers(which):
    """(ii) the mask-head oracle equals nn.Conv2d / nn.ConvTranspose2d autograd on the same pooled features, to the same bound"""
    c = CS.cached("mask_case", which)
    r64, r32 = CS.mask_oracle(c, 64, feat_grad=False), CS.mask_oracle(c, 32, feat_grad=False)
    rois = TO.rois_of(c.boxes)
    x = TO.pool([torch.as_tensor(f).double() for f in c.feats], rois, TO.levels_of(rois[:, 1:]), c.img[1], 14, 14, 2)
    ch = CS.MASK_C
    convs = [torch.nn.Conv2d(ch, ch, 3, 1, 1).double() for _ in range(4)]
    deconv, logits = torch.nn.ConvTranspose2d(ch, ch, 2, 2, 0).double(), torch.nn.Conv2d(ch, CS.MASK_NCLS, 1).double()
    layers = convs + [deconv, logits]
    with torch.no_grad():
        for i, layer in enumerate(layers):
            layer.weight.copy_(torch.as_tensor(c.params[TO.MASK_PARAMS[2 * i]]))
            layer.bias.copy_(torch.as_tensor(c.params[TO.MASK_PARAMS[2 * i + 1]]))
    t = x
    for layer in convs + [deconv]:
        t = F.relu(layer(t))
    lg = logits(t)
    cls = torch.as_tensor(c.cls)
    loss = F.binary_cross_entropy_with_logits(lg[torch.arange(len(cls)), cls], torch.as_tensor(c.targets).double())
    loss.backward()
    assert abs(loss.item() - r64["loss_mask"]) <= 2 * abs(r32["loss_mask"] - r64["loss_mask"]) + 1e-6 * abs(loss.item())
    for i, layer in enumerate(layers):
        for k, prm in ((TO.MASK_PARAMS[2 * i], layer.weight), (TO.MASK_PARAMS[2 * i + 1], layer.bias)):
            g = prm.grad.numpy()
            e32, err = np.abs(r32["grads"][k] - r64["grads"][k]).max(), np.abs(r64["grads"][k] - g).max()
            assert np.abs(g).max() > 0 and err <= 2 * e32 + 1e-6 * np.abs(g).max(), k


def test_every_gpu_case_keeps_its_relu_inputs_away_from_zero():
    """(iii) smallest |pre-activation| >= 1e-4 largest in the fp64 oracle, for every case whose gradients the GPU tests compare; the
    combined case counts both heads' ReLU inputs as one set"""
    m = CS.margins()
    lo = min(m["combined_case box"][0], m["combined_case mask"][0])
    hi = max(m["combined_case box"][1], m["combined_case mask"][1])
    m["combined_case"] = (lo, hi)
    for name, (lo, hi) in m.items():
        print(name, lo, hi)
        assert np.isfinite(lo) and lo >= 1e-4 * hi, name
    z, args = golden_case()
    r = TO.box_step(**args)
    assert r["pre_lo"] >= 1e-4 * r["pre_hi"]
    for c in (CS.cached("box_full_case"), CS.cached("box_one_case"), CS.cached("combined_case")):
        for s in c.sampled:                                     # and no ROI sits on a level boundary (the level is decided in fp32 on both sides)
            assert TO.level_margin(s[3][:, :4]) > 1e-3 and TO.level_margin(s[3][:, [4, 1, 5, 3]]) > 1e-3
    for which in (5, 1):
        assert TO.level_margin(np.concatenate(CS.cached("mask_case", which).boxes)) > 1e-3
    assert TO.level_margin(z["left_boxes"]) > 1e-3 and TO.level_margin(z["right_boxes"]) > 1e-3


def test_cases_cover_what_they_claim():
    c = CS.cached("box_full_case")
    lv = np.concatenate([TO.levels_of(s[3][:, :4]) for s in c.sampled])
    assert set(lv) == {0, 1, 2, 3} and all(len(s[0]) > 0 for s in c.sampled) and c.R > 8
    assert sum((s[1] > 0).sum() for s in c.sampled) >= 2 and sum((s[1] == 0).sum() for s in c.sampled) >= 2
    assert CS.cached("box_one_case").R == 1
    m = CS.cached("mask_case", 5)
    assert set(TO.levels_of(np.concatenate(m.boxes))) == {0, 1, 2, 3} and 0 < m.targets.mean() < 1
    cc = CS.cached("combined_case")
    assert [len(p) for p in cc.pos_boxes] == [2, 2]


def test_default_cfg_carries_the_sampler_keys():
    """(iv)"""
    from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d
    h = default_cfg_2d().MODEL.ROI_HEADS
    assert (h.FG_IOU_THRESHOLD, h.BG_IOU_THRESHOLD, h.BATCH_SIZE_PER_IMAGE, h.POSITIVE_FRACTION) == (0.5, 0.5, 512, 0.25)


def test_state_dict_keys_are_unchanged_and_old_configs_still_construct():
    """(v) the evaluators add no state-dict keys; a config without the four keys constructs and evaluators read the defaults"""
    from disprcnn_amd.modeling.detector.disprcnn import DispRCNN, default_cfg_2d
    from disprcnn_amd.modeling.roi_heads.roi_heads import build_roi_heads
    from tests.test_oracle_det import det_templates
    t_rpn, t_heads = det_templates()
    m = DispRCNN(default_cfg_2d("R-50-FPN"))
    _ = m.roi_heads.box.loss_evaluator, m.roi_heads.mask.loss_evaluator
    got = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("backbone.")}
    want = {"rpn." + k: tuple(v.shape) for k, v in t_rpn.items()}
    want.update({"roi_heads." + k: tuple(v.shape) for k, v in t_heads.items()})
    assert got == want
    cfg = default_cfg_2d("R-50-FPN")
    for k in ("FG_IOU_THRESHOLD", "BG_IOU_THRESHOLD", "BATCH_SIZE_PER_IMAGE", "POSITIVE_FRACTION"):
        delattr(cfg.MODEL.ROI_HEADS, k)
    heads = build_roi_heads(cfg, 256)
    ev = heads.box.loss_evaluator
    assert (ev.proposal_matcher.high_threshold, ev.proposal_matcher.low_threshold) == (0.5, 0.5)
    assert (ev.fg_bg_sampler.batch_size_per_image, ev.fg_bg_sampler.positive_fraction) == (512, 0.25)
    assert heads.mask.loss_evaluator.discretization_size == 28
    assert set(heads.state_dict()) == set(t_heads)


def test_alias_names_resolve():
    import disprcnn.modeling.head_ops as a
    import disprcnn.modeling.roi_heads.mask_head as b
    import disprcnn_amd.modeling.head_ops as a2
    import disprcnn_amd.modeling.roi_heads.mask_head as b2
    assert a.gemm_bias_act_train is a2.gemm_bias_act_train and b.keep_only_positive_boxes is b2.keep_only_positive_boxes


def test_training_on_cpu_tensors_raises():
    from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d
    from disprcnn_amd.modeling.roi_heads.roi_heads import build_roi_heads
    from disprcnn_amd.structures.bounding_box import BoxList
    cfg = default_cfg_2d()
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 16
    heads = build_roi_heads(cfg, 4).train()
    feats = [torch.zeros(1, 4, 24 >> i, 40 >> i) for i in range(4)]
    box = BoxList(torch.tensor([[4.0, 4.0, 40.0, 40.0]]), (160, 96))
    box.add_field("labels", torch.ones(1, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        heads(feats, feats, [box], [box], [box], [box])
    with pytest.raises(RuntimeError):
        heads.mask(feats, [box], [box])


def test_build_lists_the_source_and_binds_the_entries():
    """(vi) the new C symbols: declared, bound, and exported by the built library"""
    import ctypes
    from disprcnn_amd import _lib
    from disprcnn_amd.csrc import build
    names = ("drc_linear_pack_cols", "drc_relu_dropout_fwd", "drc_act_bwd_rows", "drc_act_bwd_rows_scratch_doubles", "drc_act_bwd_blocked",
             "drc_act_bwd_blocked_scratch_doubles", "drc_roi_align_fpn_bwd")
    assert "head_train.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "disprcnn_hip.h")).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and name + "(" in header
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for name in names:
            assert hasattr(handle, name), name
    else:
        pytest.fail("the HIP library is not built")

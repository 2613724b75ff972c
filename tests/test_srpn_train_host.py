"""Host-side checks behind tests/test_hip_srpn_train.py: the torch restatement of the Stereo RPN's training step
(tests/srpn_train_oracle.py) against the step recorded from the reference (tests/golden/srpn_train_golden.npz, the sampler's captured masks
fed in), the ReLU margin of every GPU case, and the wiring (config keys, state-dict keys, exported symbols, what raises).  No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import srpn_train_cases as CS
from tests import srpn_train_oracle as TO
from tests.helpers import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("drc_srpn_active_pixels", "drc_srpn_gather_rows", "drc_srpn_col2im")


def golden_step(dtype):
    z = golden_npz("srpn_train_golden.npz")
    return z, CS.oracle(CS.cached("full"), dtype, feat_grad=False, pos=z["pos"], neg=z["neg"])


def test_golden_is_small_and_its_sample_is_a_sample():
    path = os.path.join(ROOT, "tests", "golden", "srpn_train_golden.npz")
    assert os.path.getsize(path) < (1 << 18)
    z = golden_npz("srpn_train_golden.npz")
    c = CS.cached("full")
    pos, neg = z["pos"].astype(bool), z["neg"].astype(bool)
    assert pos.shape == neg.shape == (c.n * c.total,) and not (pos & neg).any()
    assert (c.labels[pos] == 1).all() and (c.labels[neg] == 0).all()          # the reference sampled what the host targets call pos / neg
    for i in range(c.n):
        sl = slice(i * c.total, (i + 1) * c.total)
        assert 0 < pos[sl].sum() <= CS.BATCH * CS.FRACTION and pos[sl].sum() + neg[sl].sum() == CS.BATCH
    assert int(z["pre_nms"]) < c.total and all(len(z[f"prop_score{i}"]) == int(z["post_nms"]) for i in range(c.n))   # both cuts act
    for i in range(c.n):
        assert (np.diff(z[f"prop_score{i}"]) <= 0).all()


def test_oracle_reproduces_the_reference_step():
    """|oracle64 - golden| <= 2 max|oracle32 - oracle64| + 1e-6 max|golden| per tensor (the bound tests/test_roi_heads_train_host.py uses
    for its recorded step): the head maps, both losses and the six parameter gradients"""
    z, r64 = golden_step(64)
    _, r32 = golden_step(32)
    assert r64["pre_lo"] >= 1e-4 * r64["pre_hi"]

    def prob(zs):                                            # the reference's head hands over the pair softmax of the raw logits
        return [torch.as_tensor(v).view(v.shape[0], 2, -1, v.shape[3]).softmax(1).view(v.shape).numpy() for v in zs]
    for key, m64, m32 in (("obj", prob(r64["logits"]), prob(r32["logits"])), ("reg", r64["regs"], r32["regs"])):
        for lvl in range(len(CS.SHAPES)):
            idx, val = z[f"{key}{lvl}_idx"], z[f"{key}{lvl}_val"].astype(np.float64)
            a64, a32 = m64[lvl].reshape(-1)[idx], m32[lvl].reshape(-1)[idx]
            e32, err = np.abs(a32 - a64).max(), np.abs(a64 - val).max()
            print(key, lvl, "err", err, "e32", e32)
            assert err <= 2 * e32 + 1e-6 * np.abs(val).max(), (key, lvl)
            asum = float(z[f"{key}{lvl}_abssum"])
            assert abs(np.abs(m64[lvl]).sum() - asum) <= 1e-5 * asum
    for k in ("loss_objectness", "loss_rpn_box_reg"):
        e32, err = abs(r32[k] - r64[k]), abs(r64[k] - float(z[k]))
        print(k, "err", err, "e32", e32)
        assert float(z[k]) > 0 and err <= 2 * e32 + 1e-6 * abs(float(z[k])), k
    for k in TO.PARAMS:
        g = z["grad:" + k].astype(np.float64)
        e32, err = np.abs(r32["grads"][k] - r64["grads"][k]).max(), np.abs(r64["grads"][k] - g).max()
        print(k, "err", err, "e32", e32, "max", np.abs(g).max())
        assert g.shape == r64["grads"][k].shape and np.abs(g).max() > 0 and err <= 2 * e32 + 1e-6 * np.abs(g).max(), k


def test_every_gpu_case_keeps_its_relu_inputs_away_from_zero():
    """smallest |hidden pre-activation| at an active pixel >= 1e-4 of the largest in the fp64 oracle: no gradient element is ever excluded
    from a comparison"""
    for name, (lo, hi) in CS.margins().items():
        print(name, lo, hi)
        assert np.isfinite(lo) and hi > 0 and lo >= 1e-4 * hi, name
    _, r = golden_step(64)
    assert r["pre_lo"] >= 1e-4 * r["pre_hi"]


def test_cases_cover_what_they_claim():
    full, wide, none = CS.cached("full"), CS.cached("wide"), CS.cached("none")
    assert (full.n, full.c, wide.n, wide.c, none.n, none.c) == (2, 8, 1, 24, 2, 8)
    assert full.total == sum(h * w for h, w in CS.SHAPES) * CS.A == 3843
    for i in range(full.n):
        sl = slice(i * full.total, (i + 1) * full.total)
        assert full.pos[sl].sum() >= 2 and full.neg[sl].sum() >= 2 and full.pos[sl].sum() + full.neg[sl].sum() == CS.BATCH
    assert (full.gt_left[1][0] < 0).any() and (full.gt_left[1][0][2:] > np.array(CS.IMG)).any()       # a ground truth hangs over the image
    assert all((l != r).any() for l, r in zip(full.gt_left, full.gt_right))
    assert wide.pos.sum() >= 2 and wide.neg.sum() >= 2
    assert none.pos.sum() == 0 and none.neg.sum() == 0 and (none.labels == -1).all()
    r = CS.cached_oracle("none", 64)
    assert r["loss_objectness"] == 0 and r["loss_rpn_box_reg"] == 0 and all(np.abs(g).max() == 0 for g in r["grads"].values())
    r = CS.cached_oracle("full", 64)
    assert all(np.abs(g).max() > 0 for g in r["grads"].values())
    levels = [bool(m.any()) for m in TO.active_pixel_masks(full.pos, full.neg, full.n, CS.A, CS.SHAPES)]
    assert levels == [True, True, False, False, False]        # only the 32 and 64 pixel anchors fit into 96 x 160: three levels stay empty
    for on, gl, gr in zip(levels, r["gleft"], r["gright"]):                      # a level's feature gradient is zero iff it has no active pixel
        assert (np.abs(gl).max() > 0) == (np.abs(gr).max() > 0) == on


def test_default_cfg_carries_the_rpn_training_keys():
    from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d
    r = default_cfg_2d().MODEL.RPN
    assert (r.FG_IOU_THRESHOLD, r.BG_IOU_THRESHOLD, r.BATCH_SIZE_PER_IMAGE, r.POSITIVE_FRACTION) == (0.7, 0.3, 256, 0.5)
    assert (r.PRE_NMS_TOP_N_TRAIN, r.POST_NMS_TOP_N_TRAIN, r.FPN_POST_NMS_TOP_N_TRAIN) == (2000, 2000, 2000)
    assert (r.PRE_NMS_TOP_N_TEST, r.POST_NMS_TOP_N_TEST, r.NMS_THRESH, r.MIN_SIZE) == (6000, 300, 0.7, 0)


def test_state_dict_keys_are_unchanged_and_old_configs_still_construct():
    from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d
    from disprcnn_amd.modeling.rpn.stereo_rpn import StereoRPN
    from tests.test_oracle_det import det_templates
    t_rpn, _ = det_templates()
    m = StereoRPN(default_cfg_2d(), 256)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in t_rpn.items()}
    ev = m.loss_evaluator
    assert (ev.proposal_matcher.high_threshold, ev.proposal_matcher.low_threshold, ev.proposal_matcher.allow_low_quality_matches) == (0.7, 0.3, True)
    assert (ev.fg_bg_sampler.batch_size_per_image, ev.fg_bg_sampler.positive_fraction) == (256, 0.5)
    assert (m.pre_nms_top_n_train, m.post_nms_top_n_train, m.pre_nms_top_n, m.post_nms_top_n) == (2000, 2000, 6000, 300)
    cfg = default_cfg_2d()
    for k in ("FG_IOU_THRESHOLD", "BG_IOU_THRESHOLD", "BATCH_SIZE_PER_IMAGE", "POSITIVE_FRACTION", "PRE_NMS_TOP_N_TRAIN", "POST_NMS_TOP_N_TRAIN"):
        delattr(cfg.MODEL.RPN, k)
    old = StereoRPN(cfg, 256)                                # an eval-only config constructs; training it says which keys are missing
    assert set(old.state_dict()) == set(t_rpn)


def small_inputs(c=8):
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.image_list import ImageList
    images = ImageList(torch.zeros(1, 3, 96, 160), [(96, 160)])
    feats = [torch.zeros(1, c, h, w) for h, w in CS.SHAPES]
    box = BoxList(torch.tensor([[4.0, 4.0, 40.0, 40.0]]), (160, 96))
    return images, feats, box


def test_what_raises_on_the_host():
    from disprcnn_amd.modeling.detector.disprcnn import DispRCNN, default_cfg_2d
    from disprcnn_amd.modeling.rpn.stereo_rpn import StereoRPN
    images, feats, box = small_inputs()
    rpn = StereoRPN(default_cfg_2d(), 8).train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # CPU tensors raise as elsewhere
        rpn(images, images, feats, feats, [box], [box])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rpn.eval()(images, images, feats, feats)
    cfg = default_cfg_2d()
    cfg.MODEL.RPN_ONLY = True
    with pytest.raises(NotImplementedError, match="RPN_ONLY"):
        StereoRPN(cfg, 8).train()._forward_train(images, images, feats, feats, [box], [box], None, None)
    cfg = default_cfg_2d()
    delattr(cfg.MODEL.RPN, "PRE_NMS_TOP_N_TRAIN")
    with pytest.raises(ValueError, match="training keys"):
        StereoRPN(cfg, 8).train()._forward_train(images, images, feats, feats, [box], [box], None, None)
    with pytest.raises(ValueError, match="targets"):
        StereoRPN(default_cfg_2d(), 8).train()._forward_train(images, images, feats, feats, None, None, None, None)
    with pytest.raises(NotImplementedError, match="multiple of 16"):        # 2C = 8: a view's hidden channels do not fill a channel block
        StereoRPN(default_cfg_2d(), 4).train().head_train([f[:, :4] for f in feats], [f[:, :4] for f in feats])
    # the detector: a trainable backbone is refused first (naming the trunk's backward), then missing targets
    m = DispRCNN(default_cfg_2d("R-50-FPN")).train()
    lr = {"left": torch.zeros(1, 3, 64, 64), "right": torch.zeros(1, 3, 64, 64)}
    with pytest.raises(NotImplementedError, match="trunk's backward"):
        m(lr)
    with pytest.raises(NotImplementedError, match="trunk's backward"):
        m(lr, {"left": [box], "right": [box]})
    for p in m.backbone.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="targets"):
        m(lr)


def test_new_symbols_are_declared_defined_and_exported():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd import _lib
    from disprcnn_amd.csrc import build
    assert "srpn_train.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "disprcnn_hip.h")).read()
    src = open(os.path.join(ROOT, "disprcnn_amd", "csrc", "srpn_train.hip")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name)
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r"\bint\s+%s\s*\(([^{;]*?)\)\s*\{" % name, src, re.S)
        assert decl and defn, name
        assert len(decl.group(1).split(",")) == len(defn.group(1).split(",")) == len(_lib._SIGS[name][1]), name
    assert ctypes.sizeof(_lib.DrcSrpnLevels) == 6 * 4 + 2 * 8 * 4 + 9 * 8 + 6 * 8 * 8       # the layout of drc_srpn_levels
    assert "atomic" not in src.lower().replace("no atomics", "")
    for banned in ("hipMalloc", "hipMemcpy", "Synchronize"):
        assert banned not in src

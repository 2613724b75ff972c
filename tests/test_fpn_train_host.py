"""Host-side checks behind tests/test_hip_fpn_train.py: the oracle's resize pinned to F.interpolate and its autograd, the refusals of the
detector and of the backbone (they fire before any launch), freeze_body()'s bookkeeping, and the wiring (symbols, state-dict keys).
No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fpn_train_oracle as O
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((1, 1), (1, 1)), ((1, 1), (2, 2)), ((3, 5), (6, 10)), ((4, 3), (7, 5)), ((2, 7), (3, 13)), ((5, 4), (12, 9)), ((6, 6), (6, 6))]


@pytest.mark.parametrize("ihw,ohw", SHAPES)
def test_oracle_resize_is_f_interpolate(ihw, ohw):
    """The oracle's weights are the kernel's fp32 ones, torch's here fp64: they differ by the rounding of s * (o + 0.5) - 0.5 and of
    1 - t at coordinates below 16 (2^-20 at most); a value is four such terms of |x| <= ~4.5, a gradient at most 25: 1e-4 absolute is two
    orders above that and four below a wrong index or a swapped weight."""
    g_ = torch.Generator().manual_seed(ihw[0] * 1000 + ohw[1])
    x = torch.randn(2, 3, *ihw, dtype=torch.float64, generator=g_).requires_grad_(True)
    y = F.interpolate(x, size=ohw, mode="bilinear", align_corners=False)
    g = torch.randn(y.shape, dtype=torch.float64, generator=g_)
    y.backward(g)
    assert np.abs(O.resize_fwd(x.detach().numpy(), *ohw) - y.detach().numpy()).max() <= 1e-4
    bwd, mag = O.resize_bwd(g.numpy(), *ihw)
    assert np.abs(bwd - x.grad.numpy()).max() <= 1e-4
    assert (mag >= np.abs(bwd) - 1e-12).all()
    # the rows of the matrix: partitions of one, up to the rounding of the fp32 products
    assert np.abs(O.resize_matrix(*ihw, *ohw).sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -24


def test_oracle_subsample_adjoint_is_max_pool_1_2_0():
    for ih, iw in ((3, 5), (4, 4), (1, 1), (2, 7)):
        x = torch.randn(2, 3, ih, iw, dtype=torch.float64).requires_grad_(True)
        y = F.max_pool2d(x, 1, 2, 0)
        assert tuple(y.shape[2:]) == ((ih - 1) // 2 + 1, (iw - 1) // 2 + 1)
        g = torch.randn_like(y)
        y.backward(g)
        out, mag = O.resize_bwd(None, ih, iw, gsub=g.numpy())
        assert np.array_equal(out, x.grad.numpy()) and np.array_equal(mag, np.abs(out))


def test_oracle_fpn_is_the_forks_graph():
    """fpn_layer4 is outside the graph, the top-down path reads the layer block's output, P6 subsamples P5."""
    torch.manual_seed(3)
    ch, hw = (8, 24, 40, 72), ((13, 18), (7, 9), (4, 5), (2, 3))
    feats = [torch.randn(2, c, h, w) for c, (h, w) in zip(ch, hw)]
    params = {}
    for i, c in enumerate(ch, 1):
        params[f"fpn_inner{i}.weight"], params[f"fpn_inner{i}.bias"] = torch.randn(16, c, 1, 1) * 0.1, torch.randn(16)
        params[f"fpn_layer{i}.weight"], params[f"fpn_layer{i}.bias"] = torch.randn(16, 16, 3, 3) * 0.1, torch.randn(16)
    outs = O.fpn_forward([f.double() for f in feats], {k: v.double() for k, v in params.items()})
    assert [tuple(o.shape[2:]) for o in outs] == list(hw) + [(1, 2)]
    assert torch.equal(outs[4], outs[3][:, :, ::2, ::2])
    assert torch.equal(outs[3], F.conv2d(feats[3].double(), params["fpn_inner4.weight"].double(), params["fpn_inner4.bias"].double()))
    gouts = [torch.randn(o.shape) for o in outs]
    _, pg, cg = O.fpn_step(feats, params, gouts, torch.float64)
    assert pg["fpn_layer4.weight"] is None and pg["fpn_layer4.bias"] is None
    assert all(pg[k] is not None and pg[k].abs().max() > 0 for k in O.PARAM_NAMES if "layer4" not in k) and all(g is not None for g in cg)
    # the top-down path reads out3 = fpn_layer3(...): P4's own incoming gradient reaches fpn_layer3 only through that path's adjoint
    only = [torch.zeros_like(g) for g in gouts]
    only[0] = gouts[0]
    _, pg0, _ = O.fpn_step(feats, params, only, torch.float64)
    assert pg0["fpn_layer2.weight"].abs().max() > 0 and pg0["fpn_layer3.weight"].abs().max() > 0 and pg0["fpn_inner4.weight"].abs().max() > 0


def _detector():
    from disprcnn_amd.modeling.detector import DispRCNN, default_cfg_2d
    cfg = default_cfg_2d("R-50-FPN")
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 16
    return DispRCNN(cfg)


def _images():
    return {"left": torch.zeros(1, 3, 32, 64), "right": torch.zeros(1, 3, 32, 64)}


def test_detector_accepts_a_trainable_fpn_behind_a_frozen_body():
    """The test that fails without the feature: after freeze_body() the detector gets past the trunk check to the targets check."""
    m = _detector()
    m.backbone.freeze_body()
    m.train()
    assert any(p.requires_grad for p in m.backbone.fpn.parameters()) and not any(p.requires_grad for p in m.backbone.body.parameters())
    with pytest.raises(ValueError, match="targets"):
        m(_images())


def test_detector_still_refuses_a_trainable_body():
    m = _detector().train()
    with pytest.raises(NotImplementedError, match="trunk's backward") as ex:                    # nothing frozen
        m(_images())
    assert "freeze_body()" in str(ex.value) and "BatchNorm" in str(ex.value)
    m.backbone.freeze_body()
    m.train()
    next(m.backbone.body.parameters()).requires_grad_(True)                                     # one body parameter trainable
    with pytest.raises(NotImplementedError, match="trunk's backward"):
        m(_images())
    m.backbone.body.requires_grad_(False)
    with pytest.raises(ValueError, match="targets"):
        m(_images())
    m.backbone.body.train()                                                                     # the body in training mode
    with pytest.raises(NotImplementedError, match="trunk's backward"):
        m(_images())
    # fully frozen: today's path, whatever the body's mode
    m.backbone.requires_grad_(False)
    with pytest.raises(ValueError, match="targets"):
        m(_images())


def test_backbone_forward_refusals_in_training_mode():
    m = _detector().backbone
    x = torch.zeros(1, 3, 32, 64)
    m.train()
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm / backward are not built on the HIP engine yet"):
        m(x)
    m.freeze_body()
    m.train()
    next(m.body.parameters()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="body's backward"):
        m(x)
    m.body.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                   # past the refusals: the engine wants a GPU tensor
        m(x)


def test_freeze_body_survives_train_and_eval_round_trips():
    m = _detector()
    assert m.backbone.freeze_body() is m.backbone
    assert not m.backbone.body.training and not any(p.requires_grad for p in m.backbone.body.parameters())
    assert all(p.requires_grad for p in m.backbone.fpn.parameters())
    for _ in range(2):
        m.train()
        assert m.training and m.backbone.training and m.backbone.fpn.training and m.rpn.training
        assert not m.backbone.body.training and not any(mod.training for mod in m.backbone.body.modules())
        m.eval()
        assert not m.backbone.training and not m.backbone.body.training
    m.backbone.train()
    assert m.backbone.training and not m.backbone.body.training


def test_a_backbone_that_never_froze_its_body_behaves_as_before():
    m = _detector()
    m.train()
    assert m.backbone.body.training and all(mod.training for mod in m.backbone.body.modules())
    m.eval()
    assert not m.backbone.body.training
    m.backbone.train()
    assert m.backbone.body.training
    assert all(p.requires_grad for p in m.backbone.parameters())


def test_state_dict_keys_are_unchanged():
    m = _detector()
    z = np.load(os.path.join(GOLDEN, "backbone_golden.npz"))
    want = [str(k) for k in z["keys"]]
    assert list(m.backbone.state_dict().keys()) == want
    m.backbone.freeze_body()
    m.train()
    assert list(m.backbone.state_dict().keys()) == want
    assert [k for k in m.state_dict() if k.startswith("backbone.")] == ["backbone." + k for k in want]
    assert {"fpn." + k for k in O.PARAM_NAMES} == {k for k in want if k.startswith("fpn.")}


def test_build_lists_the_source_and_binds_the_entries():
    import ctypes
    from disprcnn_amd import _lib
    from disprcnn_amd.csrc import build
    names = ("drc_bilinear_resize_blocked_bwd", "drc_channel_sums_blocked", "drc_channel_sums_blocked_scratch_doubles")
    assert "fpn_train.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "disprcnn_hip.h")).read()
    source = open(os.path.join(ROOT, "disprcnn_amd", "csrc", "fpn_train.hip")).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and name + "(" in header and name + "(" in source
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for name in names:
            assert hasattr(handle, name)
        fn = handle.drc_channel_sums_blocked_scratch_doubles
        fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int] * 3
        assert fn(0, 5, 7) == 0 and fn(1, 5, 1) == 16 and fn(3, 40, 33) == ((99 + 7) // 8) * 48      # ceil(rows / 8) chunks x padded channels

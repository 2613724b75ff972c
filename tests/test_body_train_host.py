"""Host-side checks behind tests/test_hip_body_train.py: the opt-in's bookkeeping (enable_body_training / freeze_body / train()), the
refusals that stay for a backbone that was not opted in, the opted-in path getting past them, the oracle agreeing with itself in fp32 and
fp64 at the committed seeds, and the wiring of the new kernel.  No GPU."""
import os
import re

import pytest
import torch

from tests import body_train_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _detector():
    from disprcnn_amd.modeling.detector import DispRCNN, default_cfg_2d
    cfg = default_cfg_2d("R-50-FPN")
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 16
    return DispRCNN(cfg)


def _images():
    return {"left": torch.zeros(1, 3, 32, 64), "right": torch.zeros(1, 3, 32, 64)}


@pytest.mark.parametrize("freeze_at", [1, 2, 3, 4, 5])
def test_enable_body_training_sets_requires_grad_as_freeze_backbone_does(freeze_at):
    bb = _detector().backbone
    assert bb.enable_body_training(freeze_at) is bb
    frozen = ("stem.",) + tuple(f"layer{li}." for li in range(1, freeze_at))
    for name, p in bb.body.named_parameters():
        assert p.requires_grad == (not name.startswith(frozen)), name
    assert all(p.requires_grad for p in bb.fpn.parameters())
    assert bb._body_training and not bb._body_frozen


def test_default_freeze_at_is_two_and_zero_is_refused():
    bb = _detector().backbone.enable_body_training()
    assert not any(p.requires_grad for p in bb.body.stem.parameters()) and not any(p.requires_grad for p in bb.body.layer1.parameters())
    assert all(p.requires_grad for li in (2, 3, 4) for p in getattr(bb.body, f"layer{li}").parameters())
    fresh = _detector().backbone
    with pytest.raises(NotImplementedError, match="stem's weight gradient") as ex:
        fresh.enable_body_training(0)
    assert "max-pool adjoint" in str(ex.value) and not fresh._body_training
    for bad in (-1, 6, 2.5):
        with pytest.raises(ValueError, match="freeze_at"):
            fresh.enable_body_training(bad)


def test_train_keeps_modes_and_freeze_body_undoes_the_opt_in():
    m = _detector()
    bb = m.backbone.enable_body_training(3)
    for _ in range(2):
        m.train()
        assert bb.training and bb.body.training and all(mod.training for mod in bb.body.modules())      # every BatchNorm: batch statistics
        m.eval()
        assert not bb.training and not any(mod.training for mod in bb.body.modules())
    bb.freeze_body()
    m.train()
    assert not bb._body_training and bb._body_frozen and not bb.body.training
    assert not any(p.requires_grad for p in bb.body.parameters()) and all(p.requires_grad for p in bb.fpn.parameters())
    with pytest.raises(ValueError, match="targets"):            # today's FPN-training path
        m(_images())
    bb.enable_body_training(2)                                  # ... and back: the body leaves eval with the module's mode
    assert bb._body_training and not bb._body_frozen and bb.body.training
    m.eval()
    assert not bb.body.training


def test_a_backbone_that_was_not_opted_in_still_refuses_with_the_same_words():
    m = _detector().train()
    with pytest.raises(NotImplementedError, match="trunk's backward") as ex:
        m(_images())
    assert "freeze_body()" in str(ex.value) and "BatchNorm" in str(ex.value)
    x = torch.zeros(1, 3, 32, 64)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm / backward are not built on the HIP engine yet"):
        m.backbone(x)
    m.backbone.freeze_body()
    m.train()
    next(m.backbone.body.parameters()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="body's backward"):
        m.backbone(x)
    with pytest.raises(NotImplementedError, match="trunk's backward"):
        m(_images())
    # requires_grad set by hand as enable_body_training would, WITHOUT the call: still refused
    m2 = _detector().train()
    m2.backbone.body.stem.requires_grad_(False), m2.backbone.body.layer1.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="trunk's backward"):
        m2(_images())


def test_an_opted_in_backbone_gets_past_the_refusals():
    """The test that fails without the feature: the opted-in backbone in training mode reaches the engine, which wants a GPU tensor; the
    detector reaches its targets check, then the same place."""
    m = _detector()
    m.backbone.enable_body_training(2)
    m.train()
    assert m.backbone.body.training and any(p.requires_grad for p in m.backbone.body.parameters())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.backbone(torch.zeros(1, 3, 32, 64))
    with pytest.raises(ValueError, match="targets"):
        m(_images())
    from disprcnn_amd.structures.bounding_box import BoxList
    box = BoxList(torch.tensor([[4.0, 4.0, 40.0, 28.0]]), (64, 32), mode="xyxy")
    box.add_field("labels", torch.ones(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(_images(), {"left": [box], "right": [box]})
    m.eval()                                                     # eval: the usual path, the usual complaint
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.backbone(torch.zeros(1, 3, 32, 64))


def test_state_dict_keys_do_not_change_with_the_opt_in():
    m = _detector()
    want = list(m.backbone.state_dict().keys())
    m.backbone.enable_body_training(2)
    m.train()
    assert list(m.backbone.state_dict().keys()) == want


@pytest.mark.parametrize("name", sorted(O.UNIT_CASES))
def test_unit_oracle_agrees_with_itself(name):
    r64, r32 = O.unit_reference(name)
    es = O.unit_errors(r32, r64)
    worst = max(es, key=es.get)
    print(f"unit {name}: worst e_fp32 {es[worst]:.3e} at {worst}")
    assert es[worst] <= O.E32_MAX
    u, x, g = O.make_unit(name)
    assert tuple(r64[0].shape) == tuple(g.shape) and tuple(r64[1].shape) == tuple(x.shape)
    assert set(r64[2]) == {k for k, _ in u.named_parameters()} and all(v.abs().max() > 0 for v in r64[2].values())
    assert 0.2 < float((r64[0] == 0).double().mean()) < 0.8                                      # the ReLU mask is a real one
    for k, v in r64[3].items():                                                                 # the step moved every buffer
        assert not torch.equal(v.double(), dict(u.named_buffers())[k].double()), k


def test_body_oracle_agrees_with_itself_at_the_committed_seed():
    """The recorded yardstick meets the condition on the inputs (e_fp32 <= 1e-5 on every compared tensor).  The live fp32 step is held
    flip-free: its rounding differs between CPUs (1.29e-5 was measured where the record has 5.0e-6), one flipped mask shows at 3e-2, so 1e-4
    lies an order above the first and two below the second; and no tensor may be compared without a recorded yardstick."""
    r64, r32 = O.body_reference()
    es, rec = O.step_errors(r32, r64), O.recorded_e32()
    worst = max(es, key=es.get)
    print(f"body: worst live e_fp32 {es[worst]:.3e} at {worst}; worst recorded {max(rec.values()):.3e}; {len(es)} tensors")
    assert set(rec) == set(es) and max(rec.values()) <= O.E32_MAX
    assert es[worst] <= 1e-4
    body, x, gouts = O.make_body()
    assert [tuple(o.shape) for o in r64[0]] == [tuple(g.shape) for g in gouts] and tuple(r64[0][3].shape[2:]) == (2, 3)
    for k, p in body.named_parameters():
        frozen = k.startswith(("stem.", "layer1."))
        assert (r64[1][k] is None) == frozen, k
        assert frozen or r64[1][k].abs().max() > 0, k
    n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in body.modules())
    assert n_bn == 53 and sum(int(v.item()) for k, v in r64[2].items() if k.endswith("num_batches_tracked")) == n_bn


def test_oracle_wgrad_is_conv2ds_weight_gradient():
    for stride, hw in ((1, (5, 7)), (2, (5, 7)), (2, (6, 6))):
        a = torch.from_numpy(O.seeded((3, 5) + hw, "wg:a", stride, hw)).double()
        w = torch.zeros(7, 5, 1, 1, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(a, w, None, stride)
        b = torch.from_numpy(O.seeded(tuple(y.shape), "wg:b", stride, hw)).double()
        y.backward(b)
        gw, mag = O.wgrad_1x1(a.numpy(), b.numpy(), stride)
        assert abs(gw - w.grad[:, :, 0, 0].numpy()).max() <= 1e-12 and (mag >= abs(gw) - 1e-12).all()


def test_build_lists_the_source_and_binds_the_entries():
    import ctypes
    from disprcnn_amd.pts import _lib, build
    names = ("drc_conv1x1_wgrad_blocked", "drc_conv1x1_wgrad_scratch_floats", "drc_conv1x1_wgrad_default_chunk")
    assert "body_train.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    source = open(os.path.join(ROOT, "disprcnn_amd", "pts", "body_train.hip")).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and name + "(" in header and name + "(" in source
    assert "atomic" not in source.lower().replace("no atomics", "") and "asm" not in source
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in source
    decl = re.search(r"int drc_conv1x1_wgrad_blocked\(([^;]*)\);", header, re.S).group(1)
    assert len([p for p in decl.split(",") if p.strip()]) == len(_lib._SIGS["drc_conv1x1_wgrad_blocked"][1])
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        fn = handle.drc_conv1x1_wgrad_scratch_floats
        fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int] * 6
        assert fn(3, 5, 7, 24, 40, 36) == 3 * 24 * 40 and fn(0, 5, 7, 24, 40, 36) == 0 and fn(1, 6, 6, 16, 16, 36) == 256
        assert fn(1, 6, 6, 16, 16, 35) == 512 and fn(1, 5, 7, 0, 16, 4) == -1
        assert handle.drc_conv1x1_wgrad_default_chunk() == 512


def test_switch_values():
    from disprcnn_amd.modeling.backbone import body_train
    assert body_train.WGRAD_1X1["kernel"] in ("gemm", "tap", "auto")

"""Host tests of RCNNNet's training fixtures: tests/rcnn_train_oracle.py (the torch-CPU autograd restatement the GPU tests lean on) is
pinned to tests/rcnn_oracle.py in the forward and to the imported reference's recording (tests/golden/rcnn_train_golden.npz) in the loss
and every gradient; the new C symbols and the argument validation of the training forms are checked.  No GPU."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from . import rcnn_oracle as CO
from . import rcnn_train_oracle as TO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("drc_pn2_pointwise_mlp_dgrad", "drc_pn2_wgrad_chunk", "drc_pn2_wgrad_workspace_floats", "drc_pn2_pointwise_mlp_wgrad",
               "drc_pn2_group_max_fwd", "drc_pn2_group_max_bwd")


@pytest.fixture(scope="module")
def G():
    path = os.path.join(HERE, "golden", "rcnn_train_golden.npz")
    assert os.path.getsize(path) < (1 << 20)
    return np.load(path)


@pytest.fixture(scope="module")
def cfg_json():
    with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def step(G, cfg_json):
    """the oracle's fp64 training step on the recorded seeds, computed once"""
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    cfg = TO.train_cfg(cfg_json)
    shapes = {k: tuple(v.shape) for k, v in RCNNNet(cfg, None).state_dict().items()}
    sd = CO.random_state(shapes, int(G["weight_seed"]))
    prop = TO.make_train_inputs(cfg, int(G["input_bump"]), int(G["gt_seed"]))
    loss, grads, gpin, outs = TO.train_step(sd, cfg, prop, torch.float64)
    return dict(cfg=cfg, sd=sd, prop=prop, loss=loss, grads=grads, gpin=gpin, outs=outs)


def test_fixture_holds_the_cases_the_checks_need(G, step):
    prop = step["prop"]
    assert sorted(set(prop["cls_label"].tolist())) == [-1.0, 0.0, 1.0]
    assert sorted(set(prop["reg_valid_mask"].tolist())) == [0, 1]
    assert prop["pts_input"].shape == (4, 512, 3 + 2 + CO.N_FEAT) and G["rois"].tolist() == list(TO.TRAIN_ROIS)
    assert [str(k) for k in G["param_names"]] == sorted(step["grads"])


def test_oracle_forward_equals_the_eval_oracle(step):
    _, cls, reg = CO.network(step["sd"], step["cfg"], step["prop"]["pts_input"], np.float64)
    got_cls, got_reg = step["outs"]
    assert np.abs(got_cls - cls).max() <= 1e-12 and np.abs(got_reg - reg).max() <= 1e-12


def test_oracle_loss_and_gradients_equal_the_recording(G, step):
    assert abs(step["loss"] - float(G["loss64"])) <= 1e-9 * abs(float(G["loss64"]))
    for name in sorted(step["grads"]):
        g = step["grads"][name].reshape(-1)
        ref = G[f"g_{name}"]
        sel = G[f"gi_{name}"] if f"gi_{name}" in G.files else np.arange(g.size)
        scale = np.abs(ref).max()
        assert scale > 0, name
        assert np.abs(g[sel] - ref).max() <= 1e-9 * scale, name
        if f"gsum_{name}" in G.files:
            asum = float(G[f"gasum_{name}"])
            assert abs(g.sum() - float(G[f"gsum_{name}"])) <= 1e-9 * asum and abs(np.abs(g).sum() - asum) <= 1e-9 * asum, name
    gp = step["gpin"][..., 3:].reshape(-1)[G["gi_pts_input"]]
    assert np.abs(gp - G["g_pts_input"]).max() <= 1e-9 * np.abs(G["g_pts_input"]).max()
    assert np.count_nonzero(G["g_pts_input"]) > 0


def test_new_symbols_are_declared_defined_and_exported():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib, build
    assert "pn2_mlp_bwd.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "pn2_mlp_bwd.hip")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name)
        decl = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^{;]*?)\)\s*\{" % name, src, re.S)
        assert decl and defn, name
        n_args = 0 if decl.group(1).strip() == "void" else len(decl.group(1).split(","))
        assert n_args == (0 if defn.group(1).strip() == "void" else len(defn.group(1).split(","))) == len(_lib._SIGS[name][1]), name
    from disprcnn_amd.layers import pn2_mlp
    assert handle.drc_pn2_wgrad_chunk() == pn2_mlp.WGRAD_CHUNK
    assert "atomic" not in src.lower().replace("no atomics", "")
    for banned in ("hipMalloc", "hipMemcpy", "Synchronize"):
        assert banned not in src


def test_training_forms_validate_their_arguments(cfg_json):
    from disprcnn_amd.layers import pn2_mlp
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2 import pytorch_utils as U
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2.pointnet2_modules import PointnetSAModule
    with pytest.raises(RuntimeError):
        pn2_mlp.pointwise_mlp_train(torch.zeros(1, 4, 8), None, torch.zeros(6, 4), torch.zeros(6), True)
    with pytest.raises(RuntimeError):
        pn2_mlp.group_max(torch.zeros(1, 2, 3, 4))
    with pytest.raises(RuntimeError):
        pn2_mlp.sa_mlp_max_train(torch.zeros(1, 8, 3), torch.zeros(1, 2, 3), None, torch.zeros(1, 2, 4, dtype=torch.int32),
                                 [(torch.zeros(6, 3), torch.zeros(6))])
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        U.Conv1d(4, 6, bn=True).train()(torch.zeros(1, 4, 8))
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        PointnetSAModule(mlp=[4, 8], npoint=2, radius=0.5, nsample=4, bn=True).train()(torch.zeros(1, 8, 3), torch.zeros(1, 4, 8))
    with pytest.raises(RuntimeError):
        U.Conv1d(4, 6).train()(torch.zeros(1, 4, 8))        # no BatchNorm: reaches the kernel layer, which refuses a CPU tensor
    cfg = TO.train_cfg(cfg_json)
    jit = copy.deepcopy(cfg)
    jit["RCNN"]["ROI_SAMPLE_JIT"] = True
    with pytest.raises(NotImplementedError, match="ProposalTargetLayer"):
        RCNNNet(jit, None).train()({})
    with pytest.raises(NotImplementedError):
        RCNNNet(cfg, None).train().refine({})
    ce = copy.deepcopy(cfg)
    ce["RCNN"]["LOSS_CLS"] = "CrossEntropy"                 # the eval network accepts it; the loss is refused when training starts
    m = RCNNNet(ce, None)
    assert m.loss is None and list(m.state_dict()) == list(RCNNNet(cfg, None).state_dict())
    with pytest.raises(NotImplementedError, match="CrossEntropy"):
        m.train()({"pts_input": None})

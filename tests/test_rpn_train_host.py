"""Host tests of the RPN's training path: batch-stat BatchNorm is opt-in (pytorch_utils.enable_bn_training; the RPN opts in, nothing else
does), the new C symbols are declared, defined and exported, pts/pn2_bn.hip keeps the rules of the train step's kernels, its entry points
refuse bad arguments before anything is launched, and the BatchNorm step of tests/rpn_train_oracle.py equals torch.nn.BatchNorm2d in
fp64.  No GPU."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from . import rcnn_train_oracle as CTO
from . import rpn_train_oracle as TO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("drc_pn2_bn_chunk", "drc_pn2_bn_workspace_doubles", "drc_pn2_bn_stats", "drc_pn2_bn_apply_fwd", "drc_pn2_bn_bwd")


def test_without_the_flag_batchnorm_layers_still_refuse_training():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2 import pytorch_utils as U
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2.pointnet2_modules import (PointnetFPModule,
                                                                                                                 PointnetSAModule)
    x = torch.zeros(1, 4, 8)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        U.Conv1d(4, 6, bn=True).train()(x)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        U.SharedMLP([4, 6], bn=True).train().train_layers()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        PointnetSAModule(mlp=[4, 8], npoint=2, radius=0.5, nsample=4, bn=True).train()(torch.zeros(1, 8, 3), x)
    with pytest.raises(NotImplementedError):
        PointnetFPModule(mlp=[8, 6]).train()(torch.zeros(1, 8, 3), torch.zeros(1, 2, 3), x, torch.zeros(1, 4, 2))
    with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as f:
        cfg = CTO.train_cfg(json.load(f))
    bn = copy.deepcopy(cfg)
    bn["RCNN"]["USE_BN"] = True
    net = RCNNNet(bn, None)
    assert not any(getattr(m, "_bn_train", False) for m in net.modules())
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.train()({"pts_input": torch.zeros(1, 512, 133), "roi_boxes3d": torch.zeros(1, 7), "cls_label": torch.zeros(1),
                     "reg_valid_mask": torch.zeros(1, dtype=torch.int64), "gt_boxes3d_ct": torch.zeros(1, 7)})


def test_with_the_flag_the_kernel_layer_is_reached():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2 import pytorch_utils as U
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2.pointnet2_modules import (PointnetFPModule,
                                                                                                                 PointnetSAModule)
    x = torch.zeros(1, 4, 8)
    conv = U.enable_bn_training(U.Conv1d(4, 6, bn=True))
    assert conv._bn_train
    conv._fold = ("stale", None)
    with pytest.raises(RuntimeError, match="no CPU"):
        conv.train()(x)                                       # a CPU tensor: refused by the kernel layer, not by the module
    assert conv._fold is None, "a training forward drops the fold"
    layers = U.enable_bn_training(U.SharedMLP([4, 6, 5], bn=True)).train().train_layers()
    assert [len(l) for l in layers] == [3, 3] and all(l[1] is None and isinstance(l[2], torch.nn.BatchNorm2d) for l in layers)
    with pytest.raises(RuntimeError, match="no CPU"):
        U.enable_bn_training(PointnetSAModule(mlp=[4, 8], npoint=2, radius=0.5, nsample=4, bn=True)).train()(torch.zeros(1, 8, 3), x)
    fp = U.enable_bn_training(PointnetFPModule(mlp=[8, 6]))
    assert fp._bn_train and all(l._bn_train for l in fp.mlp)
    with pytest.raises(RuntimeError, match="no CPU"):
        fp.train()(torch.zeros(1, 8, 3), torch.zeros(1, 2, 3), x, torch.zeros(1, 4, 2))
    plain = U.Conv1d(4, 6)                                    # no BatchNorm: (weight, bias) with or without the flag
    assert len(U.enable_bn_training(plain).train_layer()) == 2


def test_the_rpn_opts_in_and_keeps_its_state_dict():
    from disprcnn_amd.layers import pn2_mlp
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn_loss import PointRCNNLossComputation
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2 import pytorch_utils as U
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2.pointnet2_modules import PointnetFPModule
    cfg = TO.small_cfg()
    m = RPN(cfg)
    flagged = [x for x in m.modules() if isinstance(x, (U._ConvBase, PointnetFPModule))]
    assert len(flagged) == 18 + 6 + 3 + 4 and all(x._bn_train for x in flagged)
    assert isinstance(m.loss_evaluator, PointRCNNLossComputation)
    assert all("loss" not in k and "_bn_train" not in k for k in m.state_dict())
    assert sum(k.endswith("num_batches_tracked") for k in m.state_dict()) == 26
    with pytest.raises(NotImplementedError):
        m.train()(torch.zeros(3, 96, 3))                      # no labels
    with pytest.raises(NotImplementedError, match="FIXED"):
        RPN(TO.small_cfg(fixed=True)).train()(torch.zeros(3, 96, 3), torch.zeros(3, 96), torch.zeros(3, 96, 7), [])
    bn = torch.nn.BatchNorm1d(6, momentum=None)
    with pytest.raises(NotImplementedError, match="momentum"):
        pn2_mlp.pointwise_bn_train(torch.zeros(1, 4, 8), None, torch.zeros(6, 4), bn, True)


def test_new_symbols_are_declared_defined_and_exported():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.layers import pn2_mlp
    from disprcnn_amd.pts import _lib, build
    assert "pn2_bn.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "pn2_bn.hip")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name)
        decl = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^{;]*?)\)\s*\{" % name, src, re.S)
        assert decl and defn, name
        n_args = 0 if decl.group(1).strip() == "void" else len(decl.group(1).split(","))
        assert n_args == (0 if defn.group(1).strip() == "void" else len(defn.group(1).split(","))) == len(_lib._SIGS[name][1]), name
    assert handle.drc_pn2_bn_chunk() == pn2_mlp.BN_CHUNK
    assert "atomic" not in src.lower().replace("no atomics", "")
    for banned in ("hipMalloc", "hipMemcpy", "Synchronize"):
        assert banned not in src


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.layers.pn2_mlp import BN_CHUNK
    from disprcnn_amd.pts import _lib
    L = _lib.lib()
    assert L.drc_pn2_bn_workspace_doubles(16, 16, 768 * 32) == 2 * 16 * (16 * 768 * 32 // BN_CHUNK + 1)
    assert L.drc_pn2_bn_workspace_doubles(1, 3, BN_CHUNK + 1) == 2 * 3 * 3
    for B, C, N in ((1, 4, 1), (0, 4, 8), (2, 0, 8), (2, 4, 0)):          # n < 2, no row, no channel, no column
        assert L.drc_pn2_bn_workspace_doubles(B, C, N) == -1
        assert L.drc_pn2_bn_stats(B, C, N, None, None, 1e-5, 0.1, None, None, None, None) == -1
        assert L.drc_pn2_bn_apply_fwd(B, C, N, 1, None, None, None, None, None, None) == -1
        assert L.drc_pn2_bn_bwd(B, C, N, 1, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.drc_pn2_bn_stats(2, 4, 8, None, None, 1e-5, 0.1, None, None, None, None) == -1                  # null pointers
    assert L.drc_pn2_bn_apply_fwd(2, 4, 8, 0, None, None, None, None, None, None) == -1
    assert L.drc_pn2_bn_bwd(2, 4, 8, 0, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.drc_pn2_bn_stats(2, 70000, 8, None, None, 1e-5, 0.1, None, None, None, None) == -2              # C past the grid's limit


@pytest.mark.parametrize("relu", [True, False])
def test_oracle_batchnorm_step_equals_torch_in_fp64(relu):
    rs = np.random.RandomState(3)
    y = rs.normal(0.3, 1.7, (3, 5, 7, 4))
    gz = rs.normal(0.0, 1.0, y.shape)
    gamma, beta = rs.uniform(0.5, 1.5, 5), rs.normal(0.0, 0.3, 5)
    gamma[1], gamma[2] = 0.0, -0.7
    rm, rv = rs.normal(0.0, 0.1, 5), rs.uniform(0.75, 1.25, 5)
    got = TO.bn_step(y, gamma, beta, rm, rv, gz, relu)
    bn = torch.nn.BatchNorm2d(5).double()
    with torch.no_grad():
        for dst, src in ((bn.weight, gamma), (bn.bias, beta), (bn.running_mean, rm), (bn.running_var, rv)):
            dst.copy_(torch.from_numpy(src))
    yt = torch.from_numpy(y).requires_grad_()
    z = bn.train()(yt)
    if relu:
        z = torch.relu(z)
    z.backward(torch.from_numpy(gz))
    assert int(bn.num_batches_tracked) == 1
    for name, ref in (("z", z.detach()), ("gy", yt.grad), ("ggamma", bn.weight.grad), ("gbeta", bn.bias.grad), ("running_mean", bn.running_mean),
                      ("running_var", bn.running_var)):
        ref = ref.numpy()
        assert np.abs(got[name] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name
    assert np.abs(got["mean"] - y.mean((0, 2, 3))).max() <= 1e-14 and np.abs(got["var"] - y.var((0, 2, 3))).max() <= 1e-14


def test_the_fixture_is_clear_of_relu_edges_and_winner_ties():
    cfg, inp = TO.small_cfg(), TO.make_inputs()
    with torch.no_grad():
        out = TO.train_step(TO.state(cfg), cfg, inp, torch.float64, backward=False)
    assert out["near_zero"] == 0 and out["near_tie"] == 0
    assert TO.find_seed(TO.WEIGHT_SEED, 1) == TO.WEIGHT_SEED
    assert len(out["bn_layers"]) == 26 and out["rpn_cls"].shape == (3, 96, 1)

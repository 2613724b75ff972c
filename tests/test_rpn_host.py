"""Host tests of the RPN's fixtures and oracle: tests/rpn_oracle.py (the NumPy restatement the GPU tests lean on) is pinned to the
recordings of the imported reference in tests/golden/rpn_ref_golden.npz, the decode is checked on hand-computed cases, and the new
module tree and C ABI are checked for shape.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

from . import rpn_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "rpn_ref_golden.npz"))


@pytest.fixture(scope="module")
def cfg():
    with open(os.path.join(HERE, "golden", "rpn_cfg_car.json")) as f:
        return RO.make_cfg(json.load(f))


def new_rpn(cfg):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN
    return RPN(cfg, None).eval()


def test_state_dict_keys_equal_the_reference(G, cfg):
    sd = new_rpn(cfg).state_dict()
    assert list(sd.keys()) == [str(k) for k in G["state_dict_keys"]]
    assert len(sd) == 208
    assert sum(v.numel() for k, v in sd.items() if not k.endswith("num_batches_tracked")) > 3_000_000


def test_unsupported_settings_raise(cfg):
    import copy
    import torch
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2 import pointnet2_modules as M, pytorch_utils as U
    with pytest.raises(NotImplementedError):
        M.PointnetSAModuleMSG(npoint=4, radii=[1.0], nsamples=[4], mlps=[[0, 8]], pool_method="avg_pool")
    with pytest.raises(NotImplementedError):
        M.PointnetSAModuleMSG(npoint=4, radii=[1.0], nsamples=[4], mlps=[[0, 8]], instance_norm=True)
    with pytest.raises(NotImplementedError):
        U.SharedMLP([3, 8], instance_norm=True)
    m = new_rpn(cfg)
    with pytest.raises(NotImplementedError):
        m.train()(torch.zeros(1, 16, 3))
    c = copy.deepcopy(cfg)
    c["TEST"]["RPN_DISTANCE_BASED_PROPOSE"] = True
    with pytest.raises(NotImplementedError):
        new_rpn(c).proposal_layer(torch.zeros(1, 4), torch.zeros(1, 4, 52), torch.zeros(1, 4, 3))


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_oracle_network_matches_the_reference_in_fp64(G, cfg, tag):
    """The NumPy forward in fp64 against the reference's fp64 recordings: within 4 x the reference's own fp32 error (it lands orders of
    magnitude below: both are fp64 sums of the same terms)."""
    kinds, seed = RO.BATCHES[tag]
    pts = RO.make_batch(kinds, seed)
    assert bool(G[f"{tag}_backbone_xyz_equals_input"])
    shapes = {k: tuple(v.shape) for k, v in new_rpn(cfg).state_dict().items()}
    sd = RO.random_state(shapes, int(G["weight_seed"]))
    xyz, feats, levels = RO.backbone(sd, cfg, pts)
    cls, reg = RO.heads(sd, feats)
    po = G[f"{tag}_pts_out"]
    for name, got, want in [("backbone_features", feats[:, :, po], G[f"{tag}_backbone_features64"]), ("rpn_cls", cls, G[f"{tag}_rpn_cls64"]),
                            ("rpn_reg", reg[:, po], G[f"{tag}_rpn_reg64"])]:
        err = np.abs(got - want).max()
        print(name, err, float(G[f"err32_max_{name}"]))
        assert err <= 4 * float(G[f"err32_max_{name}"]), name
    if tag == "b2":
        for kind in ("sa", "fp"):
            for k, lv in enumerate(levels[kind]):
                name = f"{kind}{k}"
                err = np.abs(lv[:, :, G[f"b2_pts_{name}"]] - G[f"b2_{name}64"]).max()
                assert err <= 4 * float(G[f"err32_max_{name}"]), name
    np.testing.assert_allclose(np.linalg.norm(pts.astype(np.float64), axis=2), G[f"{tag}_pts_depth"], rtol=3e-7)


def full_reg(G, tag, n=768):
    """rpn_reg with the recorded rows of the pre-NMS top-N points and zeros elsewhere: the only rows a proposal depends on"""
    top, reg_top = G[f"{tag}_top_idx"], G[f"{tag}_top_reg"]
    reg = np.zeros((top.shape[0], n, reg_top.shape[2]), F)
    for b in range(top.shape[0]):
        reg[b, top[b]] = reg_top[b]
    return reg


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_oracle_decode_and_proposals_bit_for_bit(G, cfg, tag):
    kinds, seed = RO.BATCHES[tag]
    pts = RO.make_batch(kinds, seed)
    rpn = cfg.RPN
    top = G[f"{tag}_top_idx"]
    for b in range(pts.shape[0]):
        boxes = RO.decode(pts[b][top[b]], G[f"{tag}_top_reg"][b], cfg.MEAN_SIZE[0], rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE, rpn.NUM_HEAD_BIN)
        np.testing.assert_array_equal(boxes, G[f"{tag}_top_boxes"][b])
    rois, scores, margins = RO.proposal_layer(cfg, G[f"{tag}_rpn_cls"][:, :, 0], full_reg(G, tag), pts)
    assert margins.min() >= 1e-4
    np.testing.assert_array_equal(rois, G[f"{tag}_roi_boxes3d"])
    np.testing.assert_array_equal(scores, G[f"{tag}_roi_scores_raw"])
    B = pts.shape[0]
    assert rois.shape == (B, 128 // B, 7) and top.shape == (B, 512 // B)          # mode 'TRAIN', both divided by the batch size
    seg = (1.0 / (1.0 + np.exp(-G[f"{tag}_rpn_cls"][:, :, 0].astype(np.float64))) > rpn.SCORE_THRESH).astype(np.uint8)
    np.testing.assert_array_equal(seg, G[f"{tag}_seg_mask"])


def _reg(nb=12, hb=12, **kw):
    """one regression row: all bins at 0 except the named winners; layout x bins, z bins, y, ry bins, ry residuals, h w l"""
    r = np.zeros(2 * nb + 1 + 2 * hb + 3, F)
    r[kw.get("xb", 0)] = 1
    r[nb + kw.get("zb", 0)] = 1
    r[2 * nb] = kw.get("y", 0)
    r[2 * nb + 1 + kw.get("rb", 0)] = 1
    r[2 * nb + 1 + hb + kw.get("rb", 0)] = kw.get("rres", 0)
    r[-3:] = kw.get("size", (0, 0, 0))
    return r


def test_decode_hand_computed_cases():
    mean = [1.5, 1.6, 3.9]
    d = lambda xyz, r: RO.decode(np.asarray([xyz], F), r[None], mean, 3.0, 0.5, 12)[0]          # noqa: E731
    # bin edges: bin 0 is centred at -2.75, bin 11 at +2.75; y = point y + offset + h / 2; size = mean * (1 + res)
    b = d([1.0, 2.0, 3.0], _reg(xb=0, zb=11, y=0.25, size=(1.0, 0.0, -0.5)))
    np.testing.assert_array_equal(b, np.asarray([1.0 - 2.75, 2.0 + 0.25 + 1.5, 3.0 + 2.75, 3.0, F(1.6), F(3.9) * F(0.5), 0.0], F))
    # first-maximum ties: equal bins resolve to the lowest index
    r = _reg()
    r[:12] = 1
    r[12:24] = 1
    r[25:37] = 1
    b = d([0, 0, 0], r)
    assert b[0] == F(-2.75) and b[2] == F(-2.75) and b[6] == 0
    # the ry wrap on both sides of pi: bin 6 is 180 degrees
    apc = F(2 * np.pi / 12)
    half = F(2 * np.pi / 12 / 2)
    lo = d([0, 0, 0], _reg(rb=6, rres=-0.5))[6]
    hi = d([0, 0, 0], _reg(rb=6, rres=0.5))[6]
    ang_lo, ang_hi = F(6) * apc + F(-0.5) * half, F(6) * apc + F(0.5) * half
    assert lo == ang_lo and 0 < lo <= F(np.pi)
    assert hi == F(ang_hi - F(2 * np.pi)) and -F(np.pi) < hi < 0
    # a negative angle (bin 0, negative residual) goes through remainder's sign rule and back
    neg = d([0, 0, 0], _reg(rb=0, rres=-1.0))[6]
    assert neg == F(F(F(-1.0) * half + F(2 * np.pi)) - F(2 * np.pi)) and neg < 0
    # the remainder itself, against C fmod semantics
    np.testing.assert_array_equal(RO.torch_remainder(np.asarray([-0.5, 7.0, 0.0, -7.0], F), F(2 * np.pi)),
                                  np.asarray([F(-0.5) + F(2 * np.pi), np.fmod(F(7.0), F(2 * np.pi)), 0.0, np.fmod(F(-7.0), F(2 * np.pi)) + F(2 * np.pi)], F))
    # LOC_XZ_FINE: the chosen bin's residual, scaled by the bin size
    r = np.zeros(4 * 12 + 1 + 24 + 3, F)
    r[3], r[12 + 4], r[24 + 3], r[36 + 4] = 1, 1, 0.5, -0.25
    r[49] = 1
    b = RO.decode(np.zeros((1, 3), F), r[None], mean, 3.0, 0.5, 12, xz_fine=True)[0]
    assert b[0] == F(3 * 0.5 + 0.25 - 3.0 + 0.25) and b[2] == F(4 * 0.5 + 0.25 - 3.0 - 0.125)


def test_decode_matches_torch_ops():
    """The oracle's decode against the same steps written with torch tensor ops on CPU (remainder, argmax, scalar promotion)."""
    import torch
    rs = np.random.RandomState(3)
    n, nb, hb = 4096, 12, 12
    reg = rs.normal(0, 1.5, (n, 52)).astype(F)
    xyz = rs.normal(0, 2, (n, 3)).astype(F)
    mean = [1.52563191462, 1.62856739989, 3.88311640418]
    got = RO.decode(xyz, reg, mean, 3.0, 0.5, 12)
    r, p = torch.from_numpy(reg), torch.from_numpy(xyz)
    anchor = torch.from_numpy(np.array(mean)).float()
    xb, zb = torch.argmax(r[:, :nb], 1), torch.argmax(r[:, nb:2 * nb], 1)
    px = xb.float() * 0.5 + 0.5 / 2 - 3.0
    pz = zb.float() * 0.5 + 0.5 / 2 - 3.0
    py = p[:, 1] + r[:, 24]
    rb = torch.argmax(r[:, 25:37], 1)
    apc = (2 * np.pi) / hb
    res = torch.gather(r[:, 37:49], 1, rb.unsqueeze(1)).squeeze(1) * (apc / 2)
    ry = (rb.float() * apc + res) % (2 * np.pi)
    ry[ry > np.pi] = ry[ry > np.pi] - 2 * np.pi
    hwl = r[:, 49:52] * anchor + anchor
    want = torch.stack([px + p[:, 0], py + hwl[:, 0] / 2, pz + p[:, 2], hwl[:, 0], hwl[:, 1], hwl[:, 2], ry], 1).numpy()
    np.testing.assert_array_equal(got, want)
    assert (got[:, 6] < 0).any() and (got[:, 6] > 0).any()


def test_bn_fold_matches_an_eval_batchnorm():
    import torch
    from disprcnn_amd.layers.pn2_mlp import fold_bn
    torch.manual_seed(0)
    conv, bn = torch.nn.Conv2d(7, 5, 1, bias=False).double(), torch.nn.BatchNorm2d(5).double()
    bn.running_mean.normal_(0, 0.3)
    bn.running_var.uniform_(0.5, 2.0)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_(0, 0.3)
    bn.eval()
    x = torch.randn(2, 7, 3, 4, dtype=torch.float64)
    w, b = fold_bn(conv.weight, None, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    assert w.dtype == torch.float32 and b.dtype == torch.float32
    want = bn(conv(x))
    got = torch.einsum("oc,bchw->bohw", w.double(), x) + b.double().view(1, -1, 1, 1)
    assert (got - want).abs().max() < 1e-6
    wo, bo = RO.fold_bn(conv.weight.detach().numpy(), None, bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.running_mean.numpy(),
                        bn.running_var.numpy(), bn.eps)
    np.testing.assert_array_equal(wo.astype(F), w.numpy())
    np.testing.assert_array_equal(bo.astype(F), b.numpy())


def test_header_declares_exactly_the_bound_symbols():
    from disprcnn_amd.pts import _lib
    with open(os.path.join(ROOT, "include", "disprcnn_pts.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(drc_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert set(decls) == set(_lib.EXPORTED_SYMBOLS)
    for name in ("drc_pn2_sa_mlp_max_fwd", "drc_pn2_pointwise_mlp_fwd", "drc_rpn_decode_proposals"):
        params = [p for p in decls[name].split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_lib._SIGS[name][1]), name


def test_fixture_sizes_and_build_sources():
    from disprcnn_amd.pts import build
    assert "pn2_mlp.hip" in build.SOURCES
    assert os.path.getsize(os.path.join(HERE, "golden", "rpn_ref_golden.npz")) < 1 << 20
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "pn2_mlp.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in src

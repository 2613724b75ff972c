"""PointRCNN's RPN inference on the MI355X: the fp32-MFMA shared-MLP kernels against fp64 on the same inputs, the whole network against
the imported reference's recordings (tests/golden/rpn_ref_golden.npz), and the proposal layer bit for bit.

Tolerances.  Kernels: err <= 2 * e32 + 1e-6 * max|out|, e32 being the error of torch's own fp32 conv chain on the CPU against the same
fp64 result (the bound tests/test_hip_s16.py applies to the regressor's layers).  Network: max error <= 4 x and mean error <= 2 x the
reference's own fp32-vs-fp64 error recorded per tensor by the golden maker.  Indices, decode and proposals: bit for bit.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rpn_oracle as RO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "rpn_ref_golden.npz"))
with open(os.path.join(HERE, "golden", "rpn_cfg_car.json")) as _f:
    CFG = RO.make_cfg(json.load(_f))
DEV = "cuda"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()


def P():
    from disprcnn_amd.layers import pn2_mlp
    return pn2_mlp


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def rand_layers(rs, cin, widths, bias_mean=0.0):
    out = []
    for w in widths:
        out.append((rs.normal(0, np.sqrt(2.0 / cin), (w, cin)).astype(f32), rs.normal(bias_mean, 0.1, w).astype(f32)))
        cin = w
    return out


def sa_case(rs, B, N, M, C, ns, radius):
    """xyz, new_xyz (a random subset of it), feats, and the ball-query indices (padded by repetition, as the op pads them)"""
    from disprcnn_amd.layers import pointnet2 as L
    xyz = np.stack([RO.make_cloud("surface", int(rs.randint(1 << 30)), N) for _ in range(B)])
    new_xyz = np.stack([xyz[b][rs.permutation(N)[:M]] for b in range(B)])
    feats = rs.normal(0, 1, (B, C, N)).astype(f32) if C else None
    idx = L.ball_query(radius, ns, t(xyz), t(new_xyz)).cpu().numpy()
    return xyz, new_xyz, feats, idx


def sa_chain(xyz, new_xyz, feats, idx, layers, dtype):
    """QueryAndGroup -> conv2d + ReLU per layer -> max with torch on the CPU in `dtype`"""
    B, M, ns = idx.shape
    ii = torch.from_numpy(idx.astype(np.int64)).reshape(B, 1, M * ns)
    x = torch.from_numpy(xyz).to(dtype).transpose(1, 2)
    g = torch.gather(x, 2, ii.expand(B, 3, -1)).reshape(B, 3, M, ns) - torch.from_numpy(new_xyz).to(dtype).transpose(1, 2).unsqueeze(-1)
    if feats is not None:
        f = torch.from_numpy(feats).to(dtype)
        g = torch.cat([g, torch.gather(f, 2, ii.expand(B, f.shape[1], -1)).reshape(B, f.shape[1], M, ns)], 1)
    for w, b in layers:
        g = F.relu(F.conv2d(g, torch.from_numpy(w).to(dtype)[:, :, None, None], torch.from_numpy(b).to(dtype)))
    return g.max(3)[0]


def check_bound(name, got, ref, e32):
    err = (got.double().cpu() - ref).abs().max().item()
    m = ref.abs().max().item()
    print(f"{name}: max|err| {err:.3e} (fp32 chain {e32:.3e}), max|ref| {m:.3f}")
    assert err <= 2.0 * e32 + 1e-6 * m, (name, err, e32)


def run_sa(name, rs, B, N, M, C, ns, radius, widths, bias_mean=0.0, idx_override=None):
    xyz, new_xyz, feats, idx = sa_case(rs, B, N, M, C, ns, radius)
    if idx_override is not None:
        idx = idx_override(idx)
    layers = rand_layers(rs, C + 3, widths, bias_mean)
    ref = sa_chain(xyz, new_xyz, feats, idx, layers, torch.float64)
    e32 = (sa_chain(xyz, new_xyz, feats, idx, layers, torch.float32).double() - ref).abs().max().item()
    got = P().sa_mlp_max(t(xyz), t(new_xyz), t(feats) if feats is not None else None, t(idx, torch.int32), [(t(w), t(b)) for w, b in layers])
    assert got.shape == (B, widths[-1], M)
    check_bound(name, got, ref, e32)
    return got, ref


CAR_SA = [(768, 768, 0, 16, 0.1, (16, 16, 32)), (768, 768, 0, 32, 0.5, (32, 32, 64)), (768, 512, 96, 16, 0.5, (64, 64, 128)),
          (768, 512, 96, 32, 1.0, (64, 96, 128)), (512, 256, 256, 16, 1.0, (128, 196, 256)), (512, 256, 256, 32, 2.0, (128, 196, 256)),
          (256, 64, 512, 16, 2.0, (256, 256, 512)), (256, 64, 512, 32, 4.0, (256, 384, 512))]


@pytest.mark.parametrize("N,M,C,ns,radius,widths", CAR_SA)
def test_sa_mlp_max_car_config_vs_fp64(N, M, C, ns, radius, widths):
    run_sa(f"sa C={C} ns={ns} {widths}", np.random.RandomState(C + ns), 2, N, M, C, ns, radius, widths)


@pytest.mark.parametrize("N,M,C,ns,widths", [
    (64, 37, 0, 1, (8,)), (64, 37, 0, 64, (8, 5)), (300, 37, 5, 5, (16, 7, 9)), (300, 129, 193, 48, (1,)), (100, 33, 512, 33, (3, 196)),
    (100, 19, 7, 17, (196, 515)), (50, 3, 0, 2, (515,)), (100, 70, 30, 16, (40, 600)), (40, 1, 2, 3, (300, 300, 2)), (90, 21, 64, 64, (130, 70, 33))])
def test_sa_mlp_max_edge_shapes_vs_fp64(N, M, C, ns, widths):
    run_sa(f"sa edge N={N} M={M} C={C} ns={ns} {widths}", np.random.RandomState(N + M + ns), 3, N, M, C, ns, 0.6, widths)


def test_sa_mlp_max_all_negative_and_repeated_indices():
    rs = np.random.RandomState(5)
    got, _ = run_sa("sa all-negative", rs, 2, 200, 50, 6, 16, 0.5, (32, 24), bias_mean=-100.0)
    assert (got == 0).all()                                                    # the max of zeros
    run_sa("sa one index repeated", rs, 2, 200, 50, 6, 16, 0.5, (32, 24), idx_override=lambda i: np.repeat(i[:, :, :1], 16, 2))


def test_sa_mlp_max_channel_offset_leaves_neighbours_untouched():
    rs = np.random.RandomState(6)
    xyz, new_xyz, feats, idx = sa_case(rs, 2, 200, 45, 9, 16, 0.5)
    layers = rand_layers(rs, 12, (20, 10))
    args = (t(xyz), t(new_xyz), t(feats), t(idx, torch.int32), [(t(w), t(b)) for w, b in layers])
    alone = P().sa_mlp_max(*args)
    out = torch.full((2, 25, 45), -7.0, device=DEV)
    P().sa_mlp_max(*args, out=out, c_off=8)
    assert torch.equal(out[:, 8:18], alone) and (out[:, :8] == -7).all() and (out[:, 18:] == -7).all()
    with pytest.raises(RuntimeError):
        P().sa_mlp_max(*args, out=out, c_off=16)


def pw_chain(in0, in1, w, b, relu, dtype):
    x = torch.from_numpy(in0 if in1 is None else np.concatenate([in0, in1], 1)).to(dtype)
    y = F.conv1d(x, torch.from_numpy(w).to(dtype)[:, :, None], torch.from_numpy(b).to(dtype))
    return F.relu(y) if relu else y


@pytest.mark.parametrize("N,C0,C1,cout,relu", [
    (256, 1024, 512, 512, True), (256, 512, 0, 512, True), (512, 512, 256, 512, True), (768, 512, 96, 256, True), (768, 256, 0, 128, True),
    (768, 128, 0, 128, True), (768, 128, 0, 1, False), (768, 128, 0, 52, False),                 # the car config's FP layers and heads
    (1, 1, 0, 1, False), (100, 1, 2, 3, True), (333, 196, 0, 515, False), (65, 515, 1, 196, True), (700, 3, 0, 1000, True)])
def test_pointwise_mlp_vs_fp64(N, C0, C1, cout, relu):
    rs = np.random.RandomState(N + C0 + cout)
    B = 3
    in0 = rs.normal(0, 1, (B, C0, N)).astype(f32)
    in1 = rs.normal(0, 1, (B, C1, N)).astype(f32) if C1 else None
    (w, b), = rand_layers(rs, C0 + C1, (cout,))
    ref = pw_chain(in0, in1, w, b, relu, torch.float64)
    e32 = (pw_chain(in0, in1, w, b, relu, torch.float32).double() - ref).abs().max().item()
    got = P().pointwise_mlp(t(in0), t(in1) if C1 else None, t(w), t(b), relu)
    check_bound(f"pointwise N={N} {C0}+{C1}->{cout}", got, ref, e32)
    out = torch.full((B, cout + 5, N), 3.0, device=DEV)
    P().pointwise_mlp(t(in0), t(in1) if C1 else None, t(w), t(b), relu, out=out, c_off=2)
    assert torch.equal(out[:, 2:2 + cout], got) and (out[:, :2] == 3).all() and (out[:, 2 + cout:] == 3).all()
    if not relu:
        assert (got < 0).any()


def test_unfused_torch_path_agrees_with_the_fused_kernel():
    """What tools/bench_rpn.py compares is equal work: the car config's 256-centroid level both ways, each within the kernel bound."""
    rs = np.random.RandomState(9)
    xyz, new_xyz, feats, idx = sa_case(rs, 2, 512, 256, 256, 32, 2.0)
    layers = rand_layers(rs, 259, (128, 196, 256))
    ref = sa_chain(xyz, new_xyz, feats, idx, layers, torch.float64)
    e32 = (sa_chain(xyz, new_xyz, feats, idx, layers, torch.float32).double() - ref).abs().max().item()
    args = (t(xyz), t(new_xyz), t(feats), t(idx, torch.int32), [(t(w), t(b)) for w, b in layers])
    check_bound("fused", P().sa_mlp_max(*args), ref, e32)
    check_bound("unfused", P().sa_mlp_max_unfused(*args), ref, e32)


# ---- the whole network
_MODEL = {}


def model():
    if "m" not in _MODEL:
        from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN
        m = RPN(CFG, None)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert list(shapes) == [str(k) for k in G["state_dict_keys"]]
        sd = RO.random_state(shapes, int(G["weight_seed"]))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _MODEL["m"] = m.to(DEV).eval()
    return _MODEL["m"]


def batch(tag):
    kinds, seed = RO.BATCHES[tag]
    return RO.make_batch(kinds, seed)


def forward(tag):
    if tag not in _MODEL:
        pts = batch(tag)
        ret, extra = model()(t(pts))
        assert extra == {}
        _MODEL[tag] = (pts, ret)
    return _MODEL[tag]


def check_net(name, got, want, errs):
    d = np.abs(got.astype(np.float64) - want)
    emax, emean = float(G[f"err32_max_{name}"]), float(G[f"err32_mean_{name}"])
    print(f"{name}: max err {d.max():.3e} (reference's own {emax:.3e}), mean err {d.mean():.3e} (reference's own {emean:.3e})")
    errs.append((name, d.max() <= 4 * emax and d.mean() <= 2 * emean, d.max(), d.mean()))


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_network_vs_reference_fp64(tag):
    pts, ret = forward(tag)
    assert set(ret) == {"rpn_cls", "rpn_reg", "backbone_xyz", "backbone_features", "rpn_xyz", "rpn_features", "seg_mask", "roi_boxes3d",
                        "roi_scores_raw", "pts_depth"}
    B = pts.shape[0]
    assert ret["rpn_reg"].shape == (B, 768, 52) and ret["rpn_cls"].shape == (B, 768, 1) and ret["backbone_features"].shape == (B, 128, 768)
    assert ret["rpn_features"].shape == (B, 768, 128) and torch.equal(ret["rpn_features"], ret["backbone_features"].permute(0, 2, 1))
    np.testing.assert_array_equal(ret["backbone_xyz"].cpu().numpy(), pts)
    np.testing.assert_array_equal(ret["rpn_xyz"].cpu().numpy(), pts)
    np.testing.assert_array_equal(ret["pts_depth"].cpu().numpy(), G[f"{tag}_pts_depth"])
    po = G[f"{tag}_pts_out"]
    errs = []
    check_net("backbone_features", ret["backbone_features"].cpu().numpy()[:, :, po], G[f"{tag}_backbone_features64"], errs)
    check_net("rpn_cls", ret["rpn_cls"].cpu().numpy(), G[f"{tag}_rpn_cls64"], errs)
    check_net("rpn_reg", ret["rpn_reg"].cpu().numpy()[:, po], G[f"{tag}_rpn_reg64"], errs)
    if tag == "b2":
        _, _, lv = model().backbone_net(t(pts), return_levels=True)
        for kind in ("sa", "fp"):
            for k, x in enumerate(lv[kind]):
                name = f"{kind}{k}"
                check_net(name, x.cpu().numpy()[:, :, G[f"b2_pts_{name}"]], G[f"b2_{name}64"], errs)
    assert all(e[1] for e in errs), [e for e in errs if not e[1]]


def full_reg(tag):
    top, reg_top = G[f"{tag}_top_idx"], G[f"{tag}_top_reg"]
    reg = np.zeros((top.shape[0], 768, reg_top.shape[2]), f32)
    for b in range(top.shape[0]):
        reg[b, top[b]] = reg_top[b]
    return reg


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_decode_and_propose_on_the_reference_values_bit_for_bit(tag):
    from disprcnn_amd.layers.rpn_proposals import decode_rpn_boxes, propose
    from tests import box3d_oracle as BO
    pts, rpn, B = batch(tag), CFG.RPN, len(RO.BATCHES[tag][0])
    boxes, bev = decode_rpn_boxes(t(pts), t(full_reg(tag)), CFG.MEAN_SIZE[0], rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE, rpn.NUM_HEAD_BIN, rpn.LOC_XZ_FINE)
    top = G[f"{tag}_top_idx"]
    for b in range(B):
        np.testing.assert_array_equal(boxes[b].cpu().numpy()[top[b]], G[f"{tag}_top_boxes"][b])
        np.testing.assert_array_equal(bev[b].cpu().numpy(), BO.boxes3d_to_bev(boxes[b].cpu().numpy()))
    rois, scores = propose(t(G[f"{tag}_rpn_cls"][:, :, 0]), boxes, bev, 512 // B, 128 // B, CFG.TRAIN.RPN_NMS_THRESH)
    np.testing.assert_array_equal(rois.cpu().numpy(), G[f"{tag}_roi_boxes3d"])
    np.testing.assert_array_equal(scores.cpu().numpy(), G[f"{tag}_roi_scores_raw"])
    # the module's ProposalLayer reads the same settings (mode 'TRAIN', both top-N divided by the batch size)
    r2, s2 = model().proposal_layer(t(G[f"{tag}_rpn_cls"][:, :, 0]), t(full_reg(tag)), t(pts))
    assert torch.equal(r2, rois) and torch.equal(s2, scores)


def test_decode_random_rows_and_xz_fine_bit_for_bit():
    from disprcnn_amd.layers.rpn_proposals import decode_rpn_boxes
    rs = np.random.RandomState(11)
    for fine, R in ((False, 52), (True, 76)):
        reg = rs.normal(0, 1.5, (3, 1000, R)).astype(f32)
        xyz = rs.normal(0, 2, (3, 1000, 3)).astype(f32)
        boxes, _ = decode_rpn_boxes(t(xyz), t(reg), CFG.MEAN_SIZE[0], 3.0, 0.5, 12, fine)
        want = RO.decode(xyz.reshape(-1, 3), reg.reshape(-1, R), CFG.MEAN_SIZE[0], 3.0, 0.5, 12, fine).reshape(3, 1000, 7)
        np.testing.assert_array_equal(boxes.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        decode_rpn_boxes(t(xyz), t(reg[:, :, :50]), CFG.MEAN_SIZE[0], 3.0, 0.5, 12, False)


def test_proposals_end_to_end_equal_the_oracle_on_the_modules_own_values():
    """Identical floats in, so score ties order identically.  A cloud is skipped only when the oracle walks an IoU within 1e-5 of the
    threshold on those values; at most 1 cloud in 8."""
    skipped = total = 0
    for tag in ("b2", "b5"):
        pts, ret = forward(tag)
        cls, reg = ret["rpn_cls"].cpu().numpy(), ret["rpn_reg"].cpu().numpy()
        rois, scores, margins = RO.proposal_layer(CFG, cls[:, :, 0], reg, pts)
        for b in range(pts.shape[0]):
            total += 1
            if margins[b] < 1e-5:
                skipped += 1
                continue
            np.testing.assert_array_equal(ret["roi_boxes3d"][b].cpu().numpy(), rois[b])
            np.testing.assert_array_equal(ret["roi_scores_raw"][b].cpu().numpy(), scores[b])
        want_mask = (torch.sigmoid(ret["rpn_cls"][:, :, 0]) > CFG.RPN.SCORE_THRESH).float()
        assert torch.equal(ret["seg_mask"], want_mask)
    assert skipped * 8 <= total, (skipped, total)


def test_batch_1_and_16_tiled_copies_reproduce_the_b2_features():
    pts, ret = forward("b2")
    big, _ = model()(t(np.tile(pts, (8, 1, 1))))
    for i in range(16):
        assert torch.equal(big["backbone_features"][i], ret["backbone_features"][i % 2])
        assert torch.equal(big["rpn_reg"][i], ret["rpn_reg"][i % 2]) and torch.equal(big["rpn_cls"][i], ret["rpn_cls"][i % 2])
    assert big["roi_boxes3d"].shape == (16, 8, 7) and big["roi_scores_raw"].shape == (16, 8)
    rois, scores, margins = RO.proposal_layer(CFG, big["rpn_cls"].cpu().numpy()[:, :, 0], big["rpn_reg"].cpu().numpy(), np.tile(pts, (8, 1, 1)))
    ok = margins >= 1e-5
    assert (~ok).sum() * 8 <= 16
    np.testing.assert_array_equal(big["roi_boxes3d"].cpu().numpy()[ok], rois[ok])
    one, _ = model()(t(pts[:1]))
    assert torch.equal(one["backbone_features"][0], ret["backbone_features"][0])
    assert one["roi_boxes3d"].shape == (1, 128, 7)


def test_two_forwards_are_bit_identical_reproducible():
    pts, ret = forward("b5")
    again, _ = model()(t(pts))
    for k in ret:
        assert torch.equal(again[k], ret[k]), k


def test_fold_cache_invalidation_and_training_mode_refusal():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN
    m = RPN(CFG, None)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in RO.random_state(shapes, int(G["weight_seed"])).items()}, strict=True)
    m = m.to(DEV).eval()
    pts = t(batch("b2"))
    a, _ = m(pts)
    assert torch.equal(a["rpn_reg"], forward("b2")[1]["rpn_reg"])              # a second module with the same state: the same bits
    with torch.no_grad():
        m.backbone_net.SA_modules[0].mlps[0].layer0.bn.bn.running_var.mul_(4.0)
    b, _ = m(pts)
    assert not torch.equal(a["backbone_features"], b["backbone_features"])
    with torch.no_grad():
        m.backbone_net.SA_modules[0].mlps[0].layer0.bn.bn.running_var.mul_(0.25)
    c, _ = m(pts)
    assert torch.equal(a["backbone_features"], c["backbone_features"])
    with pytest.raises(NotImplementedError):
        m.train()(pts)

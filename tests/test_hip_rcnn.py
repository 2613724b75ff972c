"""PointRCNN's RCNN stage on the MI355X: the fused ROI pooling, the GroupAll SA form, the network, the box decode and the post-process
against tests/rcnn_oracle.py and the imported reference's recordings (tests/golden/rcnn_ref_golden.npz).

Tolerances.  Pooling: indices, features, mask, depth, canonical y and the empty flags bit for bit (gathers, one correctly rounded
division, one subtraction); canonical x and z within 6 eps32 (|x - cx| + |z - cz|) of the fp64 oracle (one subtraction, cos / sin to
<= 2 ulp, two products, one sum).  GroupAll kernel: 2 * e32 + 1e-6 * max|out| of fp64, as tests/test_hip_rpn.py.  Network and decode:
max error <= 4 x and mean error <= 2 x the reference's own fp32-vs-fp64 error recorded per tensor by the golden maker (for the level outputs, which are stored on a subset of
ROIs and points: its error on that subset).  Bins, keep
lists, flags: exact.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import rcnn_oracle as CO
from tests import rpn_oracle as RO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "rcnn_ref_golden.npz"))
with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as _f:
    CFG = RO.make_cfg(json.load(_f))
RC = CFG.RCNN
DEV = "cuda"
f32 = np.float32
EPS = float(np.finfo(f32).eps)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def inputs(tag):
    return CO.make_inputs(tag, int(G["input_bump"]))


def proposals(inp):
    return {k: t(v) for k, v in inp.items()}


def pool_both(inp, S, use_depth=True, width=1.0):
    from disprcnn_amd.layers import roipool3d as L
    p = proposals(inp)
    args = (p["rpn_xyz"], p["backbone_features"], p["seg_mask"], p["pts_depth"] if use_depth else None, p["roi_boxes3d"], width, S)
    return [[o.cpu().numpy() for o in fn(*args)] for fn in (L.roipool3d_canonical, L.roipool3d_canonical_unfused)]


def check_pool(inp, S, use_depth=True):
    fused, unfused = pool_both(inp, S, use_depth)
    o32 = CO.pool_canonical(inp, 1.0, S, use_depth, f32)
    o64 = CO.pool_canonical(inp, 1.0, S, use_depth, np.float64)
    R = o32["idx"].shape[0]
    xyz, pts, feat, empty = fused
    assert xyz.shape == (R, S, 3) and pts.shape == (R, 4 + int(use_depth), S) and feat.shape == o32["feat"].shape and empty.shape == (R,)
    for name, a, b in zip(("xyz", "pts", "feat", "empty"), fused, unfused):
        assert a.shape == b.shape, name
    assert np.array_equal(empty, o32["empty"]) and np.array_equal(empty, unfused[3])
    assert np.array_equal(feat, o32["feat"]) and np.array_equal(feat, unfused[2])                   # pure gathers: the selected indices
    assert np.array_equal(pts[:, 3:], o32["pts"][:, 3:]) and np.array_equal(pts[:, 3:], unfused[1][:, 3:])      # mask, depth
    assert np.array_equal(xyz[..., 1], unfused[0][..., 1]) and np.array_equal(xyz[..., 1], o32["xyz"][..., 1])   # y: one subtraction
    assert np.array_equal(np.transpose(pts[:, :3], (0, 2, 1)), xyz)
    if R * S:
        B, M = inp["roi_boxes3d"].shape[:2]
        ctr = inp["roi_boxes3d"].reshape(R, 7)[:, None, :3].astype(np.float64)
        src = np.where(o32["empty"][:, None, None] == 1, 0.0, inp["rpn_xyz"].astype(np.float64)[np.repeat(np.arange(B), M)[:, None], o32["idx"]])
        bound = 6 * EPS * (np.abs(src[..., 0] - ctr[..., 0]) + np.abs(src[..., 2] - ctr[..., 2]))
        for k in (0, 2):
            err = np.abs(xyz[..., k].astype(np.float64) - o64["xyz"][..., k])
            print(f"pool S={S}: canonical {'xyz'[k]} max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert (err <= bound).all()
    return fused, o32


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_pooling_matches_the_unfused_path_the_oracle_and_the_golden(tag):
    inp = inputs(tag)
    fused, o32 = check_pool(inp, RC.NUM_POINTS)
    assert np.array_equal(o32["idx"], G[f"{tag}_sel_idx"].astype(np.int64)) and np.array_equal(fused[3], G[f"{tag}_empty"])
    cnt = G[f"{tag}_count"]
    assert (cnt == 0).any() and ((cnt > 0) & (cnt < RC.NUM_POINTS)).any() and (cnt > RC.NUM_POINTS).any()


@pytest.mark.parametrize("S,M,C,N,B,depth", [(1, 16, 128, 768, 2, True), (64, 1, 128, 768, 2, True), (512, 3, 1, 768, 3, True),
                                             (512, 5, 0, 768, 1, False), (512, 4, 128, 100, 2, True), (64, 0, 128, 768, 2, True),
                                             (64, 4, 128, 768, 0, True), (6, 7, 5, 33, 3, False)])
def test_pooling_at_edge_shapes(S, M, C, N, B, depth):
    inp = CO.make_inputs("b5", 3)
    inp = {k: v[:B] for k, v in inp.items()}
    inp["rpn_xyz"], inp["seg_mask"], inp["pts_depth"] = inp["rpn_xyz"][:, :N], inp["seg_mask"][:, :N], inp["pts_depth"][:, :N]
    inp["backbone_features"] = np.ascontiguousarray(inp["backbone_features"][:, :C, :N])
    inp["roi_boxes3d"], inp["roi_scores_raw"] = np.ascontiguousarray(inp["roi_boxes3d"][:, :M]), inp["roi_scores_raw"][:, :M]
    check_pool(inp, S, depth)


def test_group_all_sa_matches_the_unfused_form():
    from disprcnn_amd.layers import pn2_mlp, pointnet2 as L
    rs = np.random.RandomState(5)
    B, N, C = 7, 32, 256
    xyz = rs.normal(0, 1, (B, N, 3)).astype(f32)
    feats = rs.normal(0, 1, (B, C, N)).astype(f32)
    layers, cin = [], C + 3
    for w in (256, 256, 512):
        layers.append((rs.normal(0, np.sqrt(2.0 / cin), (w, cin)).astype(f32), rs.normal(0, 0.1, w).astype(f32)))
        cin = w
    idx = np.broadcast_to(np.arange(N, dtype=np.int32), (B, 1, N)).copy()
    zero = np.zeros((B, 1, 3), f32)
    ref64 = RO.sa_mlp_max(xyz, zero, feats, idx, layers, np.float64)
    lt = [(t(w), t(b)) for w, b in layers]
    got = pn2_mlp.sa_mlp_max(t(xyz), t(zero), t(feats), t(idx, torch.int32), lt).cpu().numpy()
    grouped = L.GroupAll()(t(xyz), None, t(feats))                                              # (B, 3+C, 1, N)
    assert np.array_equal(grouped.cpu().numpy()[:, :, 0], np.concatenate([np.transpose(xyz, (0, 2, 1)), feats], 1))
    unf = pn2_mlp.sa_mlp_max_unfused(t(xyz), t(zero), t(feats), t(idx, torch.int32), lt).cpu().numpy()
    e32 = np.abs(RO.sa_mlp_max(xyz, zero, feats, idx, layers, f32).astype(np.float64) - ref64).max()
    bound = 2 * e32 + 1e-6 * np.abs(ref64).max()
    print(f"GroupAll: fused err {np.abs(got - ref64).max():.3g}, unfused err {np.abs(unf - ref64).max():.3g}, bound {bound:.3g}")
    assert np.abs(got - ref64).max() <= bound and np.abs(got - unf).max() <= 2 * bound
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2.pointnet2_modules import PointnetSAModule
    m = PointnetSAModule(mlp=[C, 64], npoint=None, radius=100, nsample=64, bn=False).to(DEV).eval()
    new_xyz, out = m(t(xyz), t(feats))
    assert new_xyz is None and out.shape == (B, 64, 1)
    with pytest.raises(NotImplementedError):
        m(t(rs.normal(0, 1, (1, 65, 3)).astype(f32)), t(rs.normal(0, 1, (1, C, 65)).astype(f32)))


def new_net(jit=True):
    import copy
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    cfg = copy.deepcopy(CFG)
    cfg["RCNN"]["ROI_SAMPLE_JIT"] = jit
    m = RCNNNet(cfg, None).eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CO.random_state(shapes, int(G["weight_seed"])).items()}, strict=True)
    return m.to(DEV)


def within(name, got, ref64, scale_max=4.0, scale_mean=2.0):
    err = np.abs(got.astype(np.float64) - ref64)
    emax, emean = float(G[f"err32_max_{name}"]), float(G[f"err32_mean_{name}"])
    print(f"{name}: max err {err.max():.3g} (reference fp32 {emax:.3g}), mean err {err.mean():.3g} (reference fp32 {emean:.3g})")
    assert err.max() <= scale_max * emax and err.mean() <= scale_mean * emean


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_network_matches_the_reference_recordings(tag):
    inp = inputs(tag)
    pin = CO.pts_input_of(CO.pool_canonical(inp, RC.POOL_EXTRA_WIDTH, RC.NUM_POINTS, RC.USE_DEPTH, f32))
    net = new_net(jit=False)
    prop = {"pts_input": t(pin), "roi_boxes3d": t(inp["roi_boxes3d"]), "roi_scores_raw": t(inp["roi_scores_raw"])}
    with torch.no_grad():
        xyz, pts, feat = net.pool(prop)
        levels = net.backbone(xyz, pts, feat)
        out = net.network(prop)
    within("rcnn_cls", out["rcnn_cls"].cpu().numpy(), G[f"{tag}_rcnn_cls64"])
    within("rcnn_reg", out["rcnn_reg"].cpu().numpy(), G[f"{tag}_rcnn_reg64"])
    if tag == "b2":
        rois = G["b2_lev_rois"]
        for name, lv in zip(("xyz_up", "merge_down", "sa0", "sa1", "sa2"), levels):
            within("lev_" + name, lv.cpu().numpy()[rois][:, :, G[f"b2_pts_{name}"]], G[f"b2_{name}64"])
    lists, _ = net(prop)
    assert len(lists) == inp["roi_boxes3d"].shape[0]


def test_jit_form_equals_the_pts_input_form_on_its_own_pooling():
    inp = inputs("b2")
    p = proposals(inp)
    a = new_net(jit=True).network(p)
    from disprcnn_amd.layers.roipool3d import roipool3d_canonical
    xyz, pts, feat, _ = roipool3d_canonical(p["rpn_xyz"], p["backbone_features"], p["seg_mask"], p["pts_depth"], p["roi_boxes3d"], 1.0, 512)
    b = new_net(jit=False).network({"pts_input": torch.cat([pts, feat], 1).transpose(1, 2).contiguous(), "roi_boxes3d": p["roi_boxes3d"]})
    assert torch.equal(a["rcnn_cls"], b["rcnn_cls"]) and torch.equal(a["rcnn_reg"], b["rcnn_reg"])
    ref = p["backbone_features"].permute(0, 2, 1)          # the reference's dict form: rpn_features only
    q = {k: v for k, v in p.items() if k != "backbone_features"}
    q["rpn_features"] = ref
    c = new_net(jit=True).network(q)
    assert torch.equal(a["rcnn_reg"], c["rcnn_reg"])


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_decode_matches_the_golden(tag):
    from disprcnn_amd.layers.rcnn_boxes import decode_rcnn_boxes
    inp = inputs(tag)
    roi = inp["roi_boxes3d"].reshape(-1, 7)
    reg, cls = G[f"{tag}_rcnn_reg"], G[f"{tag}_post_cls"].reshape(-1)
    boxes, bev, score = (o.cpu().numpy() for o in decode_rcnn_boxes(t(roi), t(reg), t(cls), CFG.MEAN_SIZE[0], RC.LOC_SCOPE, RC.LOC_BIN_SIZE,
                                                                    RC.NUM_HEAD_BIN, RC.LOC_Y_BY_BIN, RC.LOC_Y_SCOPE, RC.LOC_Y_BIN_SIZE))
    bins = G[f"{tag}_dec_bins"].astype(np.int64)
    assert np.array_equal(CO.decode_bins(reg, RC), bins)
    # the fp64 decode uses the golden's bins: a kernel that took another bin would lie a bin width away
    within("dec_boxes", boxes, G[f"{tag}_dec_boxes64"])
    assert np.abs(boxes - G[f"{tag}_dec_boxes"]).max() <= 4 * float(G["err32_max_dec_boxes"])          # and of the reference's own fp32 decode
    from tests import box3d_oracle as BO
    assert np.array_equal(bev, BO.boxes3d_to_bev(boxes))
    assert np.abs(score.astype(np.float64) - 1.0 / (1.0 + np.exp(-cls.astype(np.float64)))).max() <= 4 * EPS


@pytest.mark.parametrize("by_bin", [False, True])
def test_decode_y_by_bin_both_ways(by_bin):
    import copy
    from disprcnn_amd.layers.rcnn_boxes import decode_rcnn_boxes, reg_channels
    rc = copy.deepcopy(RC)
    rc["LOC_Y_BY_BIN"] = by_bin
    rs = np.random.RandomState(3)
    n = 300
    R = reg_channels(rc.LOC_SCOPE, rc.LOC_BIN_SIZE, rc.NUM_HEAD_BIN, by_bin, rc.LOC_Y_SCOPE, rc.LOC_Y_BIN_SIZE)
    assert R == CO.reg_layout(rc)["R"]
    reg = rs.normal(0, 1, (n, R)).astype(f32)
    roi = np.concatenate([rs.normal(0, 5, (n, 3)), rs.uniform(1, 4, (n, 3)), rs.uniform(-np.pi, np.pi, (n, 1))], 1).astype(f32)
    boxes = decode_rcnn_boxes(t(roi), t(reg), t(np.zeros(n, f32)), CFG.MEAN_SIZE[0], rc.LOC_SCOPE, rc.LOC_BIN_SIZE, rc.NUM_HEAD_BIN, by_bin,
                              rc.LOC_Y_SCOPE, rc.LOC_Y_BIN_SIZE)[0].cpu().numpy()
    ref64 = CO.decode(roi, reg, rc, CFG.MEAN_SIZE[0], np.float64, CO.decode_bins(reg, rc))
    assert np.abs(boxes - ref64).max() <= 4 * float(G["err32_max_dec_boxes"])


def lists_to_numpy(lists):
    out = []
    for bl in lists:
        lab = bl.get_field("labels")
        out.append(dict(n=len(bl.get_field("box3d")), len2d=len(bl), boxes=bl.get_field("box3d").bbox_3d.cpu().numpy(),
                        scores=bl.get_field("box3d_score").cpu().numpy(), labels=np.atleast_1d(lab if isinstance(lab, int) else lab.cpu().numpy()),
                        random=bl.get_field("random").cpu().numpy(), has_iou=bl.has_field("iou_score"), mode=bl.get_field("box3d").mode))
    return out


def post_case(tag):
    inp = inputs(tag)
    prop = {"roi_boxes3d": t(inp["roi_boxes3d"]), "roi_scores_raw": t(inp["roi_scores_raw"])}
    return inp, prop, {"rcnn_cls": t(G[f"{tag}_post_cls"]), "rcnn_reg": t(G[f"{tag}_rcnn_reg"])}


def check_refine_is_argmax(post, out, prop):
    lists = lists_to_numpy(post(out, prop))
    box, score, random = (o.cpu().numpy() for o in post.best(out, prop))
    for b, d in enumerate(lists):
        i = int(np.argmax(d["scores"]))
        assert np.array_equal(box[b], d["boxes"][i]) and score[b] == d["scores"][i] and random[b] == d["random"][i]
    return lists


@pytest.mark.parametrize("tag", ["b2", "b5"])
def test_postprocess_lists_equal_the_golden_and_refine_is_their_argmax(tag):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_inference import Box3DPointRCNNPostProcess
    inp, prop, out = post_case(tag)
    post = Box3DPointRCNNPostProcess(CFG)
    lists = check_refine_is_argmax(post, out, prop)
    lists_raw = post(out, prop)
    off = np.concatenate([[0], np.cumsum(G[f"{tag}_list_n"])])
    tol = 4 * float(G["err32_max_dec_boxes"])
    M = inp["roi_boxes3d"].shape[1]
    raw = G[f"{tag}_post_cls"].reshape(-1, M)
    for b, d in enumerate(lists):
        assert d["mode"] == "ry_lhwxyz" and d["n"] == G[f"{tag}_list_n"][b] and d["len2d"] == G[f"{tag}_list_len2d"][b]
        assert d["random"][0] == G[f"{tag}_list_random"][b] and len(d["random"]) == G[f"{tag}_list_random_len"][b]
        assert d["has_iou"] == bool(G[f"{tag}_list_has_iou"][b])
        keep = G[f"{tag}_keep"][off[b]:off[b + 1]]
        if d["random"][0]:
            assert np.array_equal(d["scores"], np.zeros(1, f32)) and keep[0] == M - 1                # the padding slot
        else:
            assert np.array_equal(d["scores"], raw[b, keep]) and np.array_equal(d["scores"], G[f"{tag}_list_scores"][off[b]:off[b + 1]])
        if d["random"][0]:
            assert lists_raw[b].get_field("labels") == 1 and isinstance(lists_raw[b].get_field("labels"), int)     # the reference's scalar
        else:
            assert len(d["labels"]) == d["n"] and np.array_equal(d["labels"], G[f"{tag}_list_labels"][off[b]:off[b + 1]])
        assert np.abs(d["boxes"] - G[f"{tag}_list_boxes"][off[b]:off[b + 1]]).max() <= tol + 2e-6
    if tag == "b5":
        assert any(d["random"][0] for d in lists)


def test_refine_resolves_a_built_tie_to_the_lower_index():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_inference import Box3DPointRCNNPostProcess
    inp, prop, out = post_case("b2")
    cls = G["b2_post_cls"].copy().reshape(2, -1)
    top = float(cls.max()) + 1.0
    cls[0, [9, 4]] = top                    # two best boxes with one score; 1 and 2 would do too
    cls[1, [12, 3, 7]] = top
    out["rcnn_cls"] = t(cls.reshape(-1, 1))
    post = Box3DPointRCNNPostProcess(CFG)
    check_refine_is_argmax(post, out, prop)
    box = post.best(out, prop)[0].cpu().numpy()
    dec = CO.decode(inp["roi_boxes3d"].reshape(-1, 7), G["b2_rcnn_reg"], RC, CFG.MEAN_SIZE[0], np.float64, G["b2_dec_bins"].astype(np.int64))
    M = cls.shape[1]
    for b, lo in ((0, 4), (1, 3)):
        assert np.abs(box[b] - CO.to_ry_lhwxyz(dec[b * M + lo][None])[0]).max() <= 4 * float(G["err32_max_dec_boxes"]) + 2e-6


def test_refine_does_not_sync_the_host():
    inp = inputs("b2")
    p = proposals(inp)
    net = new_net(jit=True)
    net.refine(p)                                          # folds and packs the weights (host work, once)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        box, score, random = net.refine(p)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert box.shape == (2, 7) and score.shape == (2,) and random.shape == (2,)


def test_new_kernels_report_no_scratch():
    import re
    import subprocess
    import tempfile
    from disprcnn_amd.csrc.build import FLAGS, HIPCC
    src = os.path.join(os.path.dirname(HERE), "disprcnn_amd", "pts", "rcnn_ops.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "rcnn_ops.o")],
                           capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    print(list(zip(names, scratch, lds)))
    assert len(names) == 2 and any("pool_canonical_kernel" in n for n in names) and any("rcnn_decode_kernel" in n for n in names)
    assert scratch == [0, 0] and max(lds) <= 64            # the index list is dynamic LDS sized to S, not a static 32 KB


def test_pooling_and_group_all_allocate_only_their_outputs():
    from disprcnn_amd.layers import roipool3d as L
    p = proposals(inputs("b2"))
    args = (p["rpn_xyz"], p["backbone_features"], p["seg_mask"], p["pts_depth"], p["roi_boxes3d"], 1.0, 512)
    L.roipool3d_canonical(*args)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    outs = L.roipool3d_canonical(*args)
    peak = torch.cuda.max_memory_allocated() - before
    need = sum(-(-o.numel() * o.element_size() // 512) * 512 for o in outs)          # the allocator's 512-byte granules
    assert peak <= need, (peak, need)
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2.pointnet2_modules import PointnetSAModule
    m = PointnetSAModule(mlp=[16, 32], npoint=None, radius=100, nsample=64, bn=False).to(DEV).eval()
    xyz, f = torch.randn(4, 32, 3, device=DEV), torch.randn(4, 16, 32, device=DEV)
    m(xyz, f)
    const = m._group_all
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _, out = m(xyz, f)
    assert m._group_all is const and torch.cuda.max_memory_allocated() - before <= -(-out.numel() * 4 // 512) * 512


def test_pooling_refuses_no_samples():
    from disprcnn_amd.layers import roipool3d as L
    p = proposals(inputs("b2"))
    with pytest.raises(RuntimeError):
        L.roipool3d_canonical(p["rpn_xyz"], p["backbone_features"], p["seg_mask"], p["pts_depth"], p["roi_boxes3d"], 1.0, 0)


def test_postprocess_without_roi_slots_raises():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_inference import Box3DPointRCNNPostProcess
    R = CO.reg_layout(RC)["R"]
    with pytest.raises(RuntimeError):
        Box3DPointRCNNPostProcess(CFG)({"rcnn_cls": torch.zeros(0, 1, device=DEV), "rcnn_reg": torch.zeros(0, R, device=DEV)},
                                       {"roi_boxes3d": torch.zeros(2, 0, 7, device=DEV), "roi_scores_raw": torch.zeros(2, 0, device=DEV)})


# ---- PointRCNN eval forward
def total_cfg(n_inst, rois_per_cloud=16, rcnn=True):
    import copy
    c = copy.deepcopy(CFG)
    c["TRAIN"]["RPN_POST_NMS_TOP_N"] = rois_per_cloud * n_inst        # ProposalLayer divides by the batch; keeps the fp64 oracle run short
    c["RCNN"]["ENABLED"] = rcnn
    return RO.make_cfg({"MODEL": {"POINTRCNN": c}})


def new_point_rcnn(n_inst, rcnn=True):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    m = PointRCNN(total_cfg(n_inst, rcnn=rcnn)).eval()
    sd = {}
    shapes = {k: tuple(v.shape) for k, v in m.rpn.state_dict().items()}
    sd.update({"rpn." + k: v for k, v in RO.random_state(shapes, 3).items()})
    if rcnn:
        shapes = {k: tuple(v.shape) for k, v in m.rcnn_net.state_dict().items()}
        sd.update({"rcnn_net." + k: v for k, v in CO.random_state(shapes, int(G["weight_seed"])).items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV), {k[len("rcnn_net."):]: v for k, v in sd.items() if k.startswith("rcnn_net.")}


def scene():
    from tests import test_hip_points as TP
    left, right, calibs = TP._golden_inputs(torch.device(DEV))
    return left, right, calibs


def test_proposals_to_camera_matches_the_reference_recording():
    m, _ = new_point_rcnn(3, rcnn=False)
    rs = np.random.RandomState(1)
    rois, mean, rot = G["box_b7"].reshape(3, 4, 7), G["box_mean"], G["box_rot"]
    cloud = rs.normal(0, 2, (3, 50, 3)).astype(f32)
    d = {"backbone_xyz": t(cloud), "rpn_xyz": t(cloud), "roi_boxes3d": t(rois), "seg_mask": t(cloud[..., 0])}
    out = m.proposals_to_camera(d, t(mean), t(rot, torch.float64))
    assert np.abs(out["roi_boxes3d"].cpu().numpy() - G["box_cam32"]).max() <= 2e-5            # the reference's own fp32 run
    back = CO.rotate_back(cloud, mean, rot)
    assert np.abs(out["rpn_xyz"].cpu().numpy() - back).max() <= 8 * EPS * np.abs(back).max()
    ref = out["backbone_xyz"].double().norm(dim=2).cpu().numpy()                              # |p| of the rotated-back cloud
    assert np.abs(out["pts_depth"].cpu().numpy() - ref).max() <= 2 * EPS * ref.max()
    assert out["seg_mask"] is d["seg_mask"] and d["roi_boxes3d"].cpu().numpy().tolist() == rois.tolist()      # the input dict is left alone


def test_point_rcnn_eval_equals_the_oracle_composition():
    """Discrete parts (which ROI wins, fallback or not) are compared where the oracle's margins hold: logit gaps and bin gaps of
    1e-3, ten times the network's error bound (4 x err32_max of rcnn_cls / rcnn_reg, about 1e-4), and 1e-4 around SCORE_THRESH on
    the sigmoid (its slope is at most 1/4).  An instance failing them is left out of the comparison, at most 1 in 8.
    Box tolerance: 4 x err32_max_rcnn_reg times the largest factor a regression value meets in the decode (the anchor length),
    plus the decode's own 4 x err32_max, plus 2e-5 for the two passes through corners at |coordinate| <= 50."""
    left, right, calibs = scene()
    n_inst = sum(len(a) for a in left)
    m, sd = new_point_rcnn(n_inst)
    with pytest.raises(ValueError):
        m(left, right)
    got_l, got_r, losses = m(left, right, calibs)
    assert losses == {} and [len(a) for a in got_l] == [len(a) for a in left]
    for lr in got_l:
        b3 = lr.get_field("box3d")
        assert b3.mode == "ry_lhwxyz" and len(b3) == len(lr) and b3.size == lr.size
        assert lr.get_field("scores_3d").shape == (len(lr),) and lr.get_field("random").shape == (len(lr),)
        assert not lr.get_field("scores_3d").is_cuda and lr.get_field("random").dtype == torch.int64
    box = torch.cat([lr.get_field("box3d").bbox_3d for lr in got_l]).numpy()
    score = torch.cat([lr.get_field("scores_3d") for lr in got_l]).numpy()
    random = torch.cat([lr.get_field("random") for lr in got_l]).numpy()
    # the oracle composition on the HIP RPN's outputs
    with torch.no_grad():
        pts, mean, rot = m.pointcloud(left, right, calibs)
        rpn_out, _ = m.rpn(pts)
        cam = m.proposals_to_camera(rpn_out, mean, rot)
        xyz, p5, feat = m.rcnn_net.pool(cam)
    assert cam["roi_boxes3d"].shape == (n_inst, 16, 7)
    pin = torch.cat([p5, feat], 1).transpose(1, 2).cpu().numpy()
    _, cls64, reg64 = CO.network(sd, CFG, pin, np.float64)
    rois = cam["roi_boxes3d"].cpu().numpy()
    prop_scores = rpn_out["roi_scores_raw"].cpu().numpy()
    M = rois.shape[1]
    cls64, reg64 = cls64.reshape(n_inst, M), reg64.reshape(n_inst, M, -1)
    tol = 4 * float(G["err32_max_rcnn_reg"]) * max(CFG.MEAN_SIZE[0]) + 4 * float(G["err32_max_dec_boxes"]) + 2e-5
    skipped = 0
    for b in range(n_inst):
        norm = 1.0 / (1.0 + np.exp(-cls64[b]))
        valid = norm > f32(RC.SCORE_THRESH)
        ok = np.abs(norm - float(f32(RC.SCORE_THRESH))).min() >= 1e-4
        if valid.any():
            order = np.argsort(-np.where(valid, cls64[b], -np.inf), kind="stable")
            i = int(order[0])
            ok &= valid.sum() == 1 or cls64[b, order[0]] - cls64[b, order[1]] >= 1e-3
            ok &= CO.argmax_margin(reg64[b, i][None], RC) >= 1e-3
            want = CO.to_ry_lhwxyz(CO.decode(rois[b, i][None], reg64[b, i][None], RC, CFG.MEAN_SIZE[0], np.float64, CO.decode_bins(reg64[b, i][None], RC)))[0]
            want_score, want_random = cls64[b, i], 0
        else:
            i = int(np.argmax(prop_scores[b]))
            want, want_score, want_random = CO.to_ry_lhwxyz(rois[b, i][None])[0], 0.0, 1
        print(f"instance {b}: margins ok {bool(ok)}, random {want_random}, roi {i}, valid {int(valid.sum())}, box err {np.abs(box[b] - want).max():.3g} (tol {tol:.3g})")
        if not ok:
            skipped += 1
            continue
        assert random[b] == want_random and abs(score[b] - want_score) <= 4 * float(G["err32_max_rcnn_cls"])
        d = np.abs(box[b] - want)
        d[0] = min(d[0], abs(d[0] - 2 * np.pi))
        assert d.max() <= tol
    assert skipped * 8 <= n_inst


def test_point_rcnn_empty_input_and_rpn_only_branch():
    from disprcnn_amd.structures.bounding_box import BoxList
    left, right, calibs = scene()
    n_inst = sum(len(a) for a in left)
    m, _ = new_point_rcnn(n_inst)
    e = BoxList(torch.zeros(0, 4, device=DEV), left[0].size)
    e.add_field("disparity", left[0].get_field("disparity")[:0])
    e.add_field("mask", left[0].get_field("mask")[:0])
    out_l, _, _ = m([e], [BoxList(torch.zeros(0, 4, device=DEV), e.size)], calibs[:1])
    assert len(out_l[0].get_field("box3d")) == 0 and out_l[0].get_field("box3d").mode == "ry_lhwxyz"
    assert out_l[0].get_field("scores_3d").numel() == 0 and out_l[0].get_field("random").numel() == 0
    # RPN only: the best proposal of each instance, moved back to the camera frame through its corners
    m2, _ = new_point_rcnn(n_inst, rcnn=False)
    assert not hasattr(m2, "rcnn_net")
    got_l, _, _ = m2(left, right, calibs)
    assert [len(a.get_field("box3d")) for a in got_l] == [len(a) for a in left]                # split over the images
    assert all(a.get_field("box3d").mode == "xyzhwl_ry" and not a.has_field("random") for a in got_l)
    with torch.no_grad():
        pts, mean, rot = m2.pointcloud(left, right, calibs)
        rpn_out, _ = m2.rpn(pts)
    rois, sc = rpn_out["roi_boxes3d"].cpu().numpy().astype(np.float64), rpn_out["roi_scores_raw"].cpu().numpy()
    idx = sc.argmax(1)
    best = rois[np.arange(n_inst), idx]
    best[:, :3] += mean.cpu().numpy()
    corners = CO.rotate_back(CO.box_corners(best).reshape(n_inst, 8, 3), np.zeros((n_inst, 3)), rot.cpu().numpy())
    want = CO.corners_to_box(corners.reshape(n_inst, 24))
    got = torch.cat([a.get_field("box3d").bbox_3d for a in got_l]).cpu().numpy()
    assert np.abs(got - want).max() <= 16 * EPS * np.abs(want).max()
    assert np.array_equal(torch.cat([a.get_field("scores_3d") for a in got_l]).numpy(), sc[np.arange(n_inst), idx])

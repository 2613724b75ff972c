"""ProposalTargetLayer on the MI355X: the two kernels of pts/proposal_target.hip, the module and RCNNNet's ROI_SAMPLE_JIT training step
against tests/proposal_target_oracle.py and the imported reference's recording (tests/golden/proposal_target_golden.npz; the host tests
pin the oracle to it).

The cases (tests/proposal_target_oracle.py: CASES) run the sampler at M in {1, 63, 70, 130} candidates (one lane, a wave edge, crossing
waves, more than two waves), P in {5, 16, 64} slots, N in {1, 3} boxes, T in {0, 1, 10} iterations, and the pooling at 300 and 257 points
(one over the workgroup), S in {1, 48, 64}, C in {0, 5, 8}, with and without depth; each on B = 6 clouds, one per candidate mix, the last
one without a foreground or background candidate.

Exact: source indices, iteration counts, class counts, flags, labels, empty flags and the selected point indices.  Bit-equal to the fp32
oracle: what the reference makes with additions and multiplications alone (the noise boxes of 'multiple', the position of 'single') and
every gathered value.  Everything through an IoU, sin / cos / atan2: max error <= 4 x and mean error <= 2 x the reference's own
fp32-vs-fp64 error on that case and tensor (err32_max_* / err32_mean_*), plus the floor 1e-6 * max|ref|: the rule of
tests/test_hip_rcnn_train.py.  The cloud without a candidate, where the reference raises, is checked against the oracle alone.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import proposal_target_oracle as PO
from tests import rcnn_oracle as CO
from tests import rcnn_train_oracle as TO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "proposal_target_golden.npz"))
GT = np.load(os.path.join(HERE, "golden", "rcnn_train_golden.npz"))
with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as _f:
    CFG_JSON = json.load(_f)
DEV = "cuda"
f32 = np.float32
BUMP = int(G["input_bump"])
NB = len(G["clouds"])
CASES = sorted(PO.CASES)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def n(x):
    return x.detach().cpu().numpy()


def within(name, got, ref, emax, emean, floor):
    err = np.abs(np.asarray(got, np.float64) - ref)
    r_max, r_mean = err.max() / (4 * emax + floor), err.mean() / (2 * emean + floor)
    print(f"{name}: max err {err.max():.3g} (reference fp32 {emax:.3g}), mean err {err.mean():.3g} (reference fp32 {emean:.3g}), floor {floor:.3g}; "
          f"ratio to the bound: max {r_max:.3f} mean {r_mean:.3f}")
    return r_max <= 1.0 and r_mean <= 1.0


def within_recording(case, name, got):
    ref = G[f"{case}_{name}64"]
    return within(f"{case} {name}", np.asarray(got).reshape(ref.shape), ref, float(G[f"err32_max_{case}_{name}"]),
                  float(G[f"err32_mean_{case}_{name}"]), 1e-6 * np.abs(ref).max())


_CACHE = {}


def case_data(case):
    """one case's seeded inputs, draws, cfg and fp32 oracle results: computed once and shared, never modified"""
    if case not in _CACHE:
        cfg = PO.case_cfg(CFG_JSON, case)
        st = PO.settings(cfg)
        inp, draws = PO.make_inputs(case, BUMP), PO.make_draws(case, BUMP)
        s, p = PO.layer(st, inp, draws, f32)
        last = {k: v[PO.NONE_CLOUD:] for k, v in inp.items()}              # the cloud the recording cannot hold: the oracle's fp64 mode
        s64, p64 = PO.layer(st, last, draws[PO.NONE_CLOUD:], np.float64)
        _CACHE[case] = dict(cfg=cfg, st=st, inp=inp, draws=draws, s=s, p=p, s64=s64, p64=p64)
    return _CACHE[case]


def input_dict(inp, reference_form=False):
    d = {"roi_boxes3d": t(inp["roi_boxes3d"]), "rpn_xyz": t(inp["rpn_xyz"]), "seg_mask": t(inp["seg_mask"]), "pts_depth": t(inp["pts_depth"])}
    if reference_form:
        d["rpn_features"] = t(inp["backbone_features"]).permute(0, 2, 1)
    else:
        d["backbone_features"] = t(inp["backbone_features"])
    return d


def run_sampler(c):
    from disprcnn_amd.layers import proposal_target as PT
    st, inp = c["st"], c["inp"]
    return PT.rcnn_sample_rois(t(inp["roi_boxes3d"]), t(inp["gt_boxes3d"]), t(c["draws"]), st["P"], st["fg_ratio"], st["reg_fg"], st["cls_fg"],
                               st["cls_bg"], st["cls_bg_lo"], st["hard_ratio"], st["T"], st["method"])


def run_pool(c, sampled, seg_mask=None):
    from disprcnn_amd.layers import proposal_target as PT
    st, inp = c["st"], c["inp"]
    return PT.rcnn_pool_target(t(inp["rpn_xyz"]), t(inp["backbone_features"]), t(inp["seg_mask"] if seg_mask is None else seg_mask),
                               t(inp["pts_depth"]) if st["depth"] else None, sampled, t(c["draws"]) if st["aug"] else None, st["extra"],
                               st["reg_fg"], st["cls_fg"], st["cls_bg"], sampled_pt_num=st["S"], aug_data=st["aug"], aug_rot_range=st["rot_range"],
                               num_candidates=inp["roi_boxes3d"].shape[1], fg_aug_times=st["T"])


@pytest.mark.parametrize("case", CASES)
def test_sampler_against_the_oracle_and_the_recording(case):
    c = case_data(case)
    o, P = c["s"], c["st"]["P"]
    got = {k: n(v) for k, v in run_sampler(c).items()}
    for name in ("src_index", "n_iter", "counts"):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], o[name]), name
    assert np.array_equal(got["counts"][:NB, :4], G[f"{case}_counts"]) and np.array_equal(got["src_index"][:NB], G[f"{case}_src_index"])
    assert np.array_equal(got["n_iter"][:NB], G[f"{case}_n_iter"])
    assert np.array_equal(got["gt_of_rois"], o["gt_of_rois"]) and np.array_equal(got["gt_of_rois"][:NB], G[f"{case}_gt_raw"])
    cols = slice(0, 7) if c["st"]["method"] == "multiple" else slice(0, 3)
    assert np.array_equal(got["rois"][..., cols], o["rois"][..., cols]), "the noise boxes are not the fp32 oracle's bits"
    assert np.array_equal(got["rois"][:NB][..., cols], G[f"{case}_noise_rois"][..., cols])
    assert np.array_equal(got["rois"][PO.NONE_CLOUD], c["inp"]["roi_boxes3d"][PO.NONE_CLOUD][np.arange(P) % c["inp"]["roi_boxes3d"].shape[1]])
    assert within_recording(case, "noise_rois", got["rois"][:NB])
    assert within_recording(case, "gt_iou", got["roi_iou"][:NB])
    # the cloud the recording cannot hold: its IoUs are the candidates' own; the same yardstick against the oracle's fp64 mode
    emax, emean = float(G[f"err32_max_{case}_gt_iou"]), float(G[f"err32_mean_{case}_gt_iou"])
    ref = c["s64"]["roi_iou"]
    assert within(f"{case} gt_iou, no-candidate cloud", got["roi_iou"][NB:], ref, emax, emean, 1e-6 * np.abs(ref).max())


@pytest.mark.parametrize("case", CASES)
def test_pooling_against_the_oracle_and_the_recording(case):
    c = case_data(case)
    st, o, inp = c["st"], c["p"], c["inp"]
    P, S, R = st["P"], st["S"], NB * st["P"]
    sampled = run_sampler(c)
    got = {k: n(v) for k, v in run_pool(c, sampled).items()}
    assert got["cls_label"].dtype == got["reg_valid_mask"].dtype == np.int64 and got["empty_flag"].dtype == np.int32
    for name in ("cls_label", "reg_valid_mask", "empty_flag"):
        assert np.array_equal(got[name], o[name]), name
    assert np.array_equal(got["cls_label"][:R], G[f"{case}_cls_label"]) and np.array_equal(got["reg_valid_mask"][:R], G[f"{case}_reg_valid_mask"])
    assert np.array_equal(got["empty_flag"][:R], G[f"{case}_empty"])
    assert (got["cls_label"][PO.NONE_CLOUD * P:] == -1).all() and not got["reg_valid_mask"][PO.NONE_CLOUD * P:].any()
    # the selected points: pooled again with the point's own index in the mask channel
    index = np.broadcast_to(np.arange(inp["rpn_xyz"].shape[1], dtype=f32), inp["seg_mask"].shape)
    sel = n(run_pool(c, sampled, seg_mask=index)["pts"])[:, 3, :]
    full = ~o["empty_flag"].astype(bool)
    assert np.array_equal(sel[full], o["idx"][full].astype(f32)) and not sel[~full].any()
    assert np.array_equal(sel[:R][full[:R]], G[f"{case}_sel_idx"][full[:R]].astype(f32))
    # gathers: mask, depth and feature channels, from the un-augmented cloud
    assert np.array_equal(got["pts"][:, 3:], o["pts"][:, 3:]) and np.array_equal(got["feat"], o["feat"])
    assert got["pts"].shape == (PO.B * P, 4 + int(st["depth"]), S) and got["feat"].shape == (PO.B * P, inp["backbone_features"].shape[1], S)
    assert np.array_equal(got["pts"][:, 0:3], np.transpose(got["xyz"], (0, 2, 1)))
    if not st["aug"]:                                      # without the augmentation the ROI is the noise box itself
        assert np.array_equal(got["roi_boxes3d"], n(sampled["rois"]).reshape(-1, 7))
    bad = [name for name, key in (("sampled_pts", "xyz"), ("roi_boxes3d", "roi_boxes3d"), ("gt_of_rois", "gt_of_rois"))
           if not within_recording(case, name, got[key][:R])]
    # the no-candidate cloud against the oracle's fp64 mode, with the yardstick of the same tensors
    for name, key in (("sampled_pts", "xyz"), ("roi_boxes3d", "roi_boxes3d"), ("gt_of_rois", "gt_of_rois")):
        ref = c["p64"][key]
        if not within(f"{case} {name}, no-candidate cloud", got[key][R:], ref, float(G[f"err32_max_{case}_{name}"]),
                      float(G[f"err32_mean_{case}_{name}"]), 1e-6 * np.abs(ref).max()):
            bad.append(name + " (no-candidate cloud)")
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_forward_returns_the_reference_dict(case):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.rpn.proposal_target_layer import ProposalTargetLayer
    c = case_data(case)
    st, inp = c["st"], c["inp"]
    P, S, R = st["P"], st["S"], NB * st["P"]
    layer = ProposalTargetLayer(c["cfg"], None).to(DEV)
    out = layer(input_dict(inp, reference_form=True), t(inp["gt_boxes3d"]), draws=t(c["draws"]))
    assert sorted(out) == sorted(["sampled_pts", "pts_feature", "cls_label", "reg_valid_mask", "gt_of_rois", "gt_iou", "roi_boxes3d"])
    E, C = 1 + int(st["depth"]), inp["backbone_features"].shape[1]
    shapes = {"sampled_pts": (PO.B * P, S, 3), "pts_feature": (PO.B * P, S, E + C), "cls_label": (PO.B * P,), "reg_valid_mask": (PO.B * P,),
              "gt_of_rois": (PO.B * P, 7), "gt_iou": (PO.B * P,), "roi_boxes3d": (PO.B * P, 7)}
    for k, v in out.items():
        assert tuple(v.shape) == shapes[k] and v.dtype == (torch.int64 if k in ("cls_label", "reg_valid_mask") else torch.float32), k
    got = {k: n(v) for k, v in out.items()}
    mine = PO.reference_dict(c["p"], c["s"])
    assert np.array_equal(got["pts_feature"], mine["pts_feature"])             # the maker pinned these gathers to the reference's, bit for bit
    assert np.array_equal(got["cls_label"][:R], G[f"{case}_cls_label"]) and np.array_equal(got["reg_valid_mask"][:R], G[f"{case}_reg_valid_mask"])
    bad = [k for k in ("sampled_pts", "gt_of_rois", "gt_iou", "roi_boxes3d") if not within_recording(case, k, got[k][:R])]
    assert not bad, bad
    # the network form holds the same values, and both feature layouts give the same result
    s = layer.sample(input_dict(inp), t(inp["gt_boxes3d"]), draws=t(c["draws"]))
    assert torch.equal(s["xyz"], out["sampled_pts"]) and torch.equal(s["gt_of_rois"], out["gt_of_rois"])
    assert torch.equal(torch.cat([s["pts"][:, 3:], s["feat"]], 1).transpose(1, 2), out["pts_feature"])


# ---- the whole step
STEP_CLOUDS, STEP_P, STEP_C, STEP_S = 2, 4, 128, 256        # S: enough for the first SA level's 128 centres


def step_cfg(jit):
    c = TO.train_cfg(CFG_JSON)                             # the focal classification loss: the labels hold -1
    c["RCNN"]["ROI_SAMPLE_JIT"] = jit
    c["RCNN"]["ROI_PER_IMAGE"] = STEP_P
    c["RCNN"]["NUM_POINTS"] = STEP_S
    c["AUG_DATA"], c["AUG_ROT_RANGE"] = True, 18
    return c


def step_inputs():
    """the first two clouds of case "a" (fg + both bg; fg only) with the network's 128 feature channels"""
    inp = case_data("a")["inp"]
    rs = np.random.RandomState(5)
    d = {k: inp[k][:STEP_CLOUDS] for k in ("roi_boxes3d", "rpn_xyz", "seg_mask", "pts_depth", "gt_boxes3d")}
    d["backbone_features"] = np.maximum(rs.normal(0.0, 0.6, (STEP_CLOUDS, STEP_C, d["rpn_xyz"].shape[1])), 0).astype(f32)
    return d


def step_targets(gt):
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    out = []
    for b in range(gt.shape[0]):
        bl = BoxList(torch.tensor([[0.0, 0.0, 10.0, 10.0]], device=DEV), (1280, 384), "xyxy")
        bl.add_field("box3d", Box3DList(t(gt[b]), (1280, 384), "xyzhwl_ry"))
        out.append(bl)
    return out


def new_net(jit):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
    cfg = step_cfg(jit)
    m = RCNNNet(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CO.random_state(shapes, int(GT["weight_seed"])).items()}, strict=True)
    return m.to(DEV).train(), cfg


def step_proposals(inp, cfg, seed=11):
    from disprcnn_amd.layers import proposal_target as PT
    rc = cfg.RCNN
    p = input_dict(inp)
    p["roi_scores_raw"] = torch.zeros(inp["roi_boxes3d"].shape[:2], device=DEV)
    p["draws"] = PT.proposal_draws(inp["roi_boxes3d"].shape[0], inp["roi_boxes3d"].shape[1], rc.ROI_PER_IMAGE, rc.ROI_FG_AUG_TIMES, DEV,
                                   generator=torch.Generator(device=DEV).manual_seed(seed))
    return p


def test_jit_training_step_equals_the_presampled_path():
    inp = step_inputs()
    net, cfg = new_net(True)
    prop = step_proposals(inp, cfg)
    targets = step_targets(inp["gt_boxes3d"])
    ret, losses = net(prop, targets)
    assert ret is prop and sorted(losses) == ["loss_box3d"]
    loss = losses["loss_box3d"]
    assert loss.dim() == 0 and loss.requires_grad and bool(torch.isfinite(loss))
    loss.backward()
    # the layer's own outputs, repacked as the sampled ROIs of the ROI_SAMPLE_JIT = False path (which is pinned to the reference's recording)
    s = net.proposal_target_layer.sample(prop, t(inp["gt_boxes3d"]), draws=prop["draws"])
    assert s["xyz"].shape == (STEP_CLOUDS * STEP_P, cfg.RCNN.NUM_POINTS, 3)
    assert int((s["cls_label"] == 1).sum()) > 0 and int((s["reg_valid_mask"] == 1).sum()) > 0
    other, _ = new_net(False)
    pre = {"pts_input": torch.cat([s["pts"], s["feat"]], 1).transpose(1, 2).contiguous(), "roi_boxes3d": s["roi_boxes3d"],
           "cls_label": s["cls_label"].float(), "reg_valid_mask": s["reg_valid_mask"], "gt_boxes3d_ct": s["gt_of_rois"]}
    _, losses2 = other(pre)
    losses2["loss_box3d"].backward()
    print(f"loss {loss.item():.9g} (JIT), {losses2['loss_box3d'].item():.9g} (sampled beforehand)")
    assert torch.equal(loss.detach(), losses2["loss_box3d"].detach())
    pa, pb = dict(net.named_parameters()), dict(other.named_parameters())
    assert sorted(pa) == sorted(pb)
    for name in sorted(pa):
        ga, gb = pa[name].grad, pb[name].grad
        assert ga is not None and ga.shape == pa[name].shape and bool(torch.isfinite(ga).all()), name
        assert torch.equal(ga, gb), name
    assert any(float(p.grad.abs().max()) > 0 for p in pa.values())


def test_layer_and_jit_forward_do_not_read_the_host():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.rpn.proposal_target_layer import ProposalTargetLayer
    c = case_data("a")
    layer = ProposalTargetLayer(c["cfg"], None).to(DEV)
    d, gt, draws = input_dict(c["inp"]), t(c["inp"]["gt_boxes3d"]), t(c["draws"])
    inp = step_inputs()
    net, cfg = new_net(True)
    prop, targets = step_proposals(inp, cfg), step_targets(inp["gt_boxes3d"])
    layer(d, gt, draws=draws)                              # loads the library
    net(prop, targets)                                     # host work that happens once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = layer(d, gt, draws=draws)
        drawn = layer(d, gt)                               # draws from torch's generator: still no host read
        _, losses = net(prop, targets)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out["sampled_pts"].shape == drawn["sampled_pts"].shape and losses["loss_box3d"].requires_grad
    assert net.loss.last_terms is not None                 # tb_dict is None: the terms stay on the device


def test_limits_are_refused_with_the_shape_and_the_workload_sizes_admitted():
    from disprcnn_amd.layers import proposal_target as PT
    args = (0.5, 0.55, 0.6, 0.45, 0.05, 0.8)
    gt = torch.zeros(1, 1, 7, device=DEV)
    for M, P, T in ((0, 4, 1), (PT.MAX_CANDIDATES() + 1, 4, 1), (8, PT.MAX_SLOTS() + 1, 0), (8, 0, 0)):
        with pytest.raises(RuntimeError, match=r"\(1, %d, 7\)|ROI_PER_IMAGE" % M):
            PT.rcnn_sample_rois(torch.zeros(1, M, 7, device=DEV), gt, torch.zeros(1, PT.draws_per_cloud(M, max(P, 0), T), device=DEV), P, *args, T)
    with pytest.raises(RuntimeError, match="draws"):
        PT.rcnn_sample_rois(torch.zeros(1, 8, 7, device=DEV), gt, torch.zeros(1, 5, device=DEV), 4, *args, 1)
    with pytest.raises(RuntimeError, match="gt_boxes3d"):
        PT.rcnn_sample_rois(torch.zeros(1, 8, 7, device=DEV), torch.zeros(1, 0, 7, device=DEV), torch.zeros(1, PT.draws_per_cloud(8, 4, 1), device=DEV),
                            4, *args, 1)
    # TRAIN.RPN_POST_NMS_TOP_N candidates and the default ROI_PER_IMAGE
    M, P, T = 512, 64, 10
    rs = np.random.RandomState(3)
    g = np.array([[[0.0, 1.0, 20.0, 1.5, 1.6, 3.9, 0.3]]], f32)
    cand = (g + rs.normal(0, 1, (1, M, 7)) * np.array([1.0, 0.1, 1.5, 0.05, 0.05, 0.1, 0.2])).astype(f32)
    draws = PT.proposal_draws(1, M, P, T, DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    out = PT.rcnn_sample_rois(t(cand), t(g), draws, P, *args, T)
    st = dict(P=P, T=T, fg_ratio=0.5, reg_fg=0.55, cls_fg=0.6, cls_bg=0.45, cls_bg_lo=0.05, hard_ratio=0.8, method="multiple")
    o = PO.sample_rois(st, cand, g, n(draws), f32)
    if o["margin"] >= 1e-5:                                # random candidates: compare only when no decision hangs on an IoU's last bits
        assert np.array_equal(n(out["src_index"]), o["src_index"]) and np.array_equal(n(out["n_iter"]), o["n_iter"])
    assert np.array_equal(n(out["counts"])[:, :3].sum(1) <= M, [True]) and int(n(out["src_index"]).max()) < M


def test_reproducibility_the_same_draws_give_the_same_bits():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.rpn.proposal_target_layer import ProposalTargetLayer
    c = case_data("a")
    layer = ProposalTargetLayer(c["cfg"], None).to(DEV)
    d, gt, draws = input_dict(c["inp"]), t(c["inp"]["gt_boxes3d"]), t(c["draws"])
    a, b = layer.sample(d, gt, draws=draws), layer.sample(d, gt, draws=draws)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ga = layer.sample(d, gt, generator=torch.Generator(device=DEV).manual_seed(9))
    gb = layer.sample(d, gt, generator=torch.Generator(device=DEV).manual_seed(9))
    assert all(torch.equal(ga[k], gb[k]) for k in ga)


def test_property_draws_are_uniforms_that_repeat_with_the_seed():
    from disprcnn_amd.layers import proposal_target as PT
    a = PT.proposal_draws(6, 70, 16, 10, DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    b = PT.proposal_draws(6, 70, 16, 10, DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    assert a.shape == (6, 70 + 16 + 9 * 16 * 10 + 3 * 16) and a.dtype == torch.float32 and torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0 and 0.4 < float(a.mean()) < 0.6
    assert not torch.equal(a, PT.proposal_draws(6, 70, 16, 10, DEV, generator=torch.Generator(device=DEV).manual_seed(5)))


def test_property_aug_data_off_equals_the_identity_draws():
    """Scale draw 0.5 gives 1 + 0 * 0.05 = 1 and flip draw 0.5 counts as no flip; the rotation (u - 1) * range is zero only at u = 1, the
    closed end of the interval, which the kernel evaluates like any other value.  With these the centres, sizes, y, features and labels
    equal AUG_DATA off exactly.  ry is recomputed as sign(b) pi / 2 + (-sign(b) pi / 2 + b + ry) - b: four roundings of values below
    2 pi, so |d ry| <= 4 eps 2 pi, and the canonical x, z, which turn by ry, move by at most |d ry| |p| plus their own roundings
    (4 eps |p|)."""
    c = case_data("a")
    assert c["st"]["aug"]
    sampled = run_sampler(c)
    draws = c["draws"].copy()
    k = PO.CASES["a"]
    o = PO.blocks(k["M"], k["P"], k["T"])
    draws[:, o["aug"]:] = np.tile(np.array([1.0, 0.5, 0.5], f32), k["P"])
    on = run_pool(dict(c, draws=draws), sampled)
    off = run_pool(dict(c, st=dict(c["st"], aug=False)), sampled)
    for name in ("feat", "empty_flag", "cls_label", "reg_valid_mask"):
        assert torch.equal(on[name], off[name]), name
    assert torch.equal(on["pts"][:, 3:], off["pts"][:, 3:]) and torch.equal(on["xyz"][..., 1], off["xyz"][..., 1])
    assert torch.equal(on["roi_boxes3d"][:, :6], off["roi_boxes3d"][:, :6])
    assert torch.equal(on["gt_of_rois"][:, [1, 3, 4, 5]], off["gt_of_rois"][:, [1, 3, 4, 5]])
    eps = float(np.finfo(f32).eps)
    d_ry = 4 * eps * 2 * np.pi
    for name in ("roi_boxes3d", "gt_of_rois"):
        d = (on[name][:, 6] - off[name][:, 6]).abs()
        d = torch.minimum(d, (d - 2 * np.pi).abs())        # the canonical angle may land on the other side of the modulo
        assert float(d.max()) <= 2 * d_ry, name            # gt: its own ry and the ROI's
    for a, b in ((on["xyz"], off["xyz"]), (on["gt_of_rois"][:, [0, 2]], off["gt_of_rois"][:, [0, 2]])):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= (d_ry + 4 * eps) * 2 * scale

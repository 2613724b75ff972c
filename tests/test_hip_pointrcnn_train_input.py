"""PointRCNN's training forward on the MI355X: process_input against the reference's recording
(tests/golden/pointrcnn_train_input_golden.npz, made by tests/golden/make_golden_pointrcnn_train_input.py), the 2D matching kernel against
the torch Matcher(boxlist_iou), PointRCNN(train) with the rpn and the rcnn config against the networks called on process_input's
outputs, DispRCNN3D(train) with DET3D_ON, and the batch without a cloud.

Tolerances.  counts, chosen pixels, matched indices, flip, scale and the class labels: exact (the fixture keeps every mask value, IoU,
disparity and drawn point clear of its decision, see the generator).  rot_angle: 1e-12.  Points and means: the bound of
tests/test_hip_points.py, 2e-4 |p| + 1e-4 uncentred and twice that centred, which was taken over the reference's depth error.  Target
corners, regression labels and the corners taken back: against the fp64 restatement tests/pointrcnn_train_oracle.py fed with this
run's own means, angles and points, within 2 x the reference's own fp32 error against that restatement fed with the reference's, plus
1e-6 x the largest value (the rule of tests/test_hip_rcnn.py)."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import pointrcnn_train_oracle as TO
from tests import rcnn_oracle as CO
from tests import rcnn_train_oracle as RTO
from tests import rpn_oracle as RO
from tests import rpn_train_oracle as RPO

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(TO.GOLDEN)
CASES = [str(c) for c in G["cases"]]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def rpn_total_cfg(fixed=False):
    """tests/rpn_train_oracle.small_cfg as PointRCNN's cfg: no RCNN, the fixture's mask and matcher thresholds"""
    c = RPO.small_cfg(fixed=fixed)
    c["RCNN"] = RO.make_cfg({"ENABLED": False})
    c["MASK_THRESH"] = float(G["mask_thresh"])
    return RO.make_cfg({"MODEL": {"POINTRCNN": c, "ROI_HEADS": {"FG_IOU_THRESHOLD": float(G["fg_iou"]), "BG_IOU_THRESHOLD": float(G["bg_iou"])}}})


@functools.lru_cache(maxsize=None)
def rpn_state():
    return RPO.state(rpn_total_cfg().MODEL.POINTRCNN)


def new_rpn_model(fixed=False):
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    m = PointRCNN(rpn_total_cfg(fixed))
    m.rpn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rpn_state().items()}, strict=True)
    return m.to(DEV).train()


def bound(name, got, ref64_own, recorded, ref64_recorded):
    e32 = np.abs(np.asarray(recorded, np.float64) - ref64_recorded).max()
    limit = 2 * e32 + 1e-6 * np.abs(ref64_recorded).max()
    err = np.abs(np.asarray(got, np.float64) - ref64_own).max()
    print(f"{name}: err {err:.3g} against fp64, the reference's own {e32:.3g}, bound {limit:.3g}")
    return err <= limit


# ---- 1. process_input against the recording
@pytest.mark.parametrize("case", CASES)
def test_process_input_matches_the_reference(case):
    g = lambda k: G[f"{case}_{k}"]
    fixed, seed = bool(g("fixed")), int(g("seed"))
    m = new_rpn_model(fixed)
    left, right, targets = TO.scene(G, DEV)                               # with the image that has ROIs and no ground truth
    assert len(targets[2]) == 0 and len(left[2]) > 0
    pts, cls_label, reg_label, matched = m.process_input(left, right, targets, rng=np.random.RandomState(seed))
    ipc = m.train_pointcloud
    assert ipc.last_counts == g("counts").tolist()
    assert np.array_equal(ipc.last_src_pix.cpu().numpy(), g("src_pix"))
    assert m.aug_flip == bool(g("flip")) and m.aug_scale == float(g("scale"))
    assert len(matched) == 2 and [len(t) for t in matched] == [int((G["cloud_image"] == i).sum()) for i in range(2)]
    mi = torch.cat([t.get_field("matched_idxs") for t in matched])
    assert not mi.is_cuda and mi.dtype == torch.int64 and mi.tolist() == g("matched_idxs").tolist()
    assert all(t.has_field("calib") and t.get_field("box3d").mode == "corners" for t in matched)
    rot, mean = m.rot_angle.cpu().numpy(), m.pts_mean.cpu().numpy()
    np.testing.assert_allclose(rot, g("rot_angle"), rtol=0, atol=1e-12)
    assert (np.sign(rot) == np.sign(g("rot_angle"))).all()
    # points: the bound of tests/test_hip_points.py
    got, ref = (pts + m.pts_mean[:, None]).cpu().numpy(), g("pts") + g("pts_mean")[:, None]
    scale = np.linalg.norm(ref, axis=2, keepdims=True)
    print(f"{case}: points err {np.abs(got - ref).max():.3g}, mean err {np.abs(mean - g('pts_mean')).max():.3g}")
    assert (np.abs(got - ref) <= 2e-4 * scale + 1e-4).all()
    ms = np.linalg.norm(g("pts_mean"), axis=1, keepdims=True)
    assert (np.abs(mean - g("pts_mean")) <= 2e-4 * ms + 1e-4).all()
    assert (np.abs(pts.cpu().numpy() - g("pts")) <= 2 * (2e-4 * scale + 1e-4)).all()
    # labels
    assert np.array_equal(cls_label.cpu().numpy(), g("cls_label"))
    rows = TO.matched_rows(G)
    corners = torch.cat([t.get_field("box3d").bbox_3d for t in matched]).view(-1, 8, 3)
    own64 = TO.to_cloud_frame(rows, m.aug_scale, m.aug_flip, rot, mean)
    rec64 = TO.to_cloud_frame(rows, float(g("scale")), bool(g("flip")), g("rot_angle"), g("pts_mean"))
    ok = [bound("target corners", corners.cpu().numpy(), own64, g("corners"), rec64)]
    ok.append(bound("reg_label", reg_label.cpu().numpy(), TO.labels(own64, pts.cpu().numpy(), g("cls_label")), g("reg_label"),
                    TO.labels(rec64, g("pts"), g("cls_label"))))
    # the way back for the targets
    back = torch.cat([t.get_field("box3d").bbox_3d for t in m.targets_to_camera(matched, m.pts_mean, m.rot_angle)]).view(-1, 8, 3)
    ok.append(bound("corners back", back.cpu().numpy(), TO.to_camera_frame(corners.cpu().numpy(), rot, mean), g("corners_back"),
                    TO.to_camera_frame(g("corners"), g("rot_angle"), g("pts_mean"))))
    assert all(ok), ok
    # the image without ground truth changes nothing
    again = m.process_input(*[x[:2] for x in (left, right, targets)], rng=np.random.RandomState(seed))
    assert torch.equal(again[0], pts) and torch.equal(again[1], cls_label) and torch.equal(again[2], reg_label)


# ---- 2. the matching kernel
def test_matching_kernel_equals_the_torch_matcher():
    from disprcnn_amd.layers.match2d import match_targets
    case = TO.matching_case()
    want, want_rows, unsafe = TO.matching_reference(case)
    assert unsafe.mean() <= 0.01
    boxes = np.concatenate([c[0] for c in case])
    first = np.cumsum([0] + [len(c[1]) for c in case])
    span = np.concatenate([np.tile(np.array([[first[i], len(c[1])]], np.int32), (len(c[0]), 1)) for i, c in enumerate(case)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    matched, rows = match_targets(t(boxes), t(span), t(np.concatenate([c[1] for c in case])), t(np.concatenate([c[2] for c in case])),
                                  TO.MATCH_HIGH, TO.MATCH_LOW)
    assert matched.dtype == torch.int64 and matched.shape == (len(boxes),) and rows.shape == (len(boxes), 7)
    ok = ~unsafe
    assert np.array_equal(matched.cpu().numpy()[ok], want[ok]) and np.array_equal(rows.cpu().numpy()[ok], want_rows[ok])
    # the indices may be written into a caller's buffer: the tail of the one the point counts are read through
    buf = torch.full((len(boxes) + 3,), 77, dtype=torch.int64, device=DEV)
    match_targets(t(boxes), t(span), t(np.concatenate([c[1] for c in case])), t(np.concatenate([c[2] for c in case])), TO.MATCH_HIGH,
                  TO.MATCH_LOW, matched=buf[3:])
    assert buf[:3].tolist() == [77] * 3 and torch.equal(buf[3:], matched)


# ---- 3. the rpn config
def _rpn_step(via_forward, seed=1):
    m = new_rpn_model()
    left, right, targets = TO.scene(G, DEV)
    if via_forward:
        ret, losses = m(left, right, targets, rng=np.random.RandomState(seed))
    else:
        pts, cls_label, reg_label, matched = m.process_input(left, right, targets, rng=np.random.RandomState(seed))
        ret, losses = m.rpn.train()(pts, cls_label, reg_label, matched)
    assert sorted(losses) == ["rpn_loss_cls", "rpn_loss_reg"] and sorted(ret) == ["backbone_features", "backbone_xyz", "rpn_cls", "rpn_reg"]
    (losses["rpn_loss_cls"] + losses["rpn_loss_reg"]).backward()
    return m, losses


def test_point_rcnn_rpn_step_is_the_rpn_on_its_own_input():
    a, la = _rpn_step(True)
    b, lb = _rpn_step(False)
    c, lc = _rpn_step(True)
    for k in la:
        print(k, la[k].item())
        assert bool(torch.isfinite(la[k])) and torch.equal(la[k].detach(), lb[k].detach()) and torch.equal(la[k].detach(), lc[k].detach()), k
    pa, pb, pc = dict(a.named_parameters()), dict(b.named_parameters()), dict(c.named_parameters())
    assert pa and all(n.startswith("rpn.") for n in pa)
    for n in pa:
        assert pa[n].grad is not None and bool(torch.isfinite(pa[n].grad).all()), n
        assert torch.equal(pa[n].grad, pb[n].grad) and torch.equal(pa[n].grad, pc[n].grad), n
    assert any(float(p.grad.abs().max()) > 0 for p in pa.values())
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)                     # the BatchNorm statistics moved the same way


# ---- 4. the rcnn config
STEP_P, STEP_S = 4, 256                                                   # tests/test_hip_proposal_target.py's step_cfg


def rcnn_total_cfg(n_clouds):
    with open(os.path.join(HERE, "golden", "rcnn_cfg_car.json")) as f:
        c = RTO.train_cfg(json.load(f))                                   # the focal classification loss
    c["RCNN"]["ROI_SAMPLE_JIT"], c["RCNN"]["ROI_PER_IMAGE"], c["RCNN"]["NUM_POINTS"] = True, STEP_P, STEP_S
    c["TRAIN"]["RPN_POST_NMS_TOP_N"] = 16 * n_clouds
    assert c["RPN"]["FIXED"] and c["RCNN"]["ENABLED"] and c["RCNN"]["TRAIN"]
    return RO.make_cfg({"MODEL": {"POINTRCNN": c, "ROI_HEADS": {"FG_IOU_THRESHOLD": float(G["fg_iou"]), "BG_IOU_THRESHOLD": float(G["bg_iou"])}}})


@functools.lru_cache(maxsize=None)
def rcnn_state():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    m = PointRCNN(rcnn_total_cfg(len(G["cloud_image"])))
    sd = {"rpn." + k: v for k, v in RO.random_state({k: tuple(v.shape) for k, v in m.rpn.state_dict().items()}, 3).items()}
    sd.update({"rcnn_net." + k: v for k, v in CO.random_state({k: tuple(v.shape) for k, v in m.rcnn_net.state_dict().items()}, 11).items()})
    return sd


def new_rcnn_model():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    m = PointRCNN(rcnn_total_cfg(len(G["cloud_image"])))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rcnn_state().items()}, strict=True)
    return m.to(DEV).train()


def test_point_rcnn_rcnn_step_is_the_rcnn_on_the_fixed_rpns_proposals():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import filter_unmatched_idxs, proposals_to_camera_unfused
    left, right, targets = TO.scene(G, DEV)
    a = new_rcnn_model()
    before = {k: v.clone() for k, v in a.rpn.state_dict().items()}
    torch.manual_seed(0)
    ret, losses = a(left, right, targets, rng=np.random.RandomState(5))
    assert sorted(losses) == ["loss_box3d"]
    loss = losses["loss_box3d"]
    assert loss.dim() == 0 and loss.requires_grad and bool(torch.isfinite(loss))
    loss.backward()
    assert not a.rpn.training and a.rcnn_net.training
    after = a.rpn.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)          # no parameter, no running statistic moved
    assert all(p.grad is None for p in a.rpn.parameters())
    for n, p in a.rcnn_net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert any(float(p.grad.abs().max()) > 0 for p in a.rcnn_net.parameters())
    n_kept = int((G["matched_idxs"] >= 0).sum())
    assert ret["roi_boxes3d"].shape[0] == n_kept < len(G["matched_idxs"])

    def by_hand(frame_change):
        b = new_rcnn_model()
        pts, _, _, matched = b.process_input(left, right, targets, rng=np.random.RandomState(5))
        b.rpn.eval()
        with torch.no_grad():
            proposals, _ = b.rpn(pts)
        proposals = frame_change(b, proposals)
        proposals, matched = filter_unmatched_idxs(proposals, b.targets_to_camera(matched, b.pts_mean, b.rot_angle))
        torch.manual_seed(0)
        return proposals, b.rcnn_net(proposals, matched)[1]["loss_box3d"]

    fused, loss_fused = by_hand(lambda b, p: b.proposals_to_camera(p, b.pts_mean, b.rot_angle))
    assert torch.equal(loss.detach(), loss_fused.detach())
    unfused, loss_unfused = by_hand(lambda b, p: proposals_to_camera_unfused(p, b.pts_mean, b.rot_angle))
    # the frame change's bound (tests/test_hip_rcnn.py: 2e-5 for a pass through corners at |coordinate| <= 50, an fp32 rounding bound and
    # so proportional to the magnitude: a random RPN proposes boxes up to the 160 m depth clamp) on what the RCNN reads ...
    for k in ("roi_boxes3d", "rpn_xyz", "pts_depth"):
        d, size = float((fused[k] - unfused[k]).abs().max()), float(fused[k].abs().max())
        print(f"{k}: fused vs torch composition {d:.3g} at magnitude {size:.3g}")
        assert d <= 2e-5 * max(1.0, size / 50), k
    # ... and on the loss: its regression terms are residuals over bins of LOC_BIN_SIZE = 0.5 and sizes over anchors > 1.5, so 2e-5 on a
    # coordinate is at most 4e-5 on a term; eight terms and the same again for the canonical points through the network: 1e-3 of a loss
    # of order one
    print(f"loss {loss.item():.9g}, by hand {loss_fused.item():.9g}, with the torch composition {loss_unfused.item():.9g}")
    assert abs(loss.item() - loss_unfused.item()) <= 1e-3 * max(1.0, abs(loss.item()))


# ---- 5. DispRCNN3D
def detector_cfg(dispnet, train_psm=False):
    from disprcnn_amd.modeling.detector.disprcnn3d import default_cfg
    from tests.test_oracle_train_caller import RES
    cfg = copy.deepcopy(default_cfg(48, -48, RES))
    cfg.MODEL.DISPNET_ON, cfg.MODEL.DET3D_ON = dispnet, True
    cfg.SOLVER.TRAIN_PC, cfg.SOLVER.TRAIN_PSM = True, train_psm
    total = rpn_total_cfg()
    cfg.MODEL.POINTRCNN, cfg.MODEL.ROI_HEADS = total.MODEL.POINTRCNN, total.MODEL.ROI_HEADS
    return cfg


def new_detector(dispnet, train_psm=False):
    from disprcnn_amd.modeling.detector import build_detection_model
    m = build_detection_model(detector_cfg(dispnet, train_psm))
    m.pcnet.rpn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rpn_state().items()}, strict=True)
    if dispnet:
        from tests.helpers import state_for
        m.dispnet.load_state_dict(state_for("B"), strict=True)
    return m.to(DEV).train()


def _detector_steps(steps):
    from disprcnn_amd.solver import FusedSGD
    m = new_detector(False)
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9)
    state = np.random.get_state()
    out = []
    try:
        np.random.seed(4)                                                 # the detector draws from numpy.random, as the reference
        for _ in range(steps):
            left, right, targets = TO.scene(G, DEV)
            losses = m({"left": None, "right": None}, {"left": left, "right": right}, {"left": targets})
            sum(losses.values()).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            out.append({k: v.detach().clone() for k, v in losses.items()})
    finally:
        np.random.set_state(state)
    return m, out


def test_detector_without_dispnet_returns_pcnets_losses_and_trains():
    m, a = _detector_steps(3)
    _, b = _detector_steps(3)
    assert all(sorted(x) == ["rpn_loss_cls", "rpn_loss_reg"] for x in a)
    for x, y in zip(a, b):
        for k in x:
            print(k, x[k].item())
            assert bool(torch.isfinite(x[k])) and torch.equal(x[k], y[k]), k
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert not torch.equal(a[0]["rpn_loss_reg"], a[2]["rpn_loss_reg"])    # the parameters moved
    # the first step is pcnet's own: PointRCNN on the same inputs with the same stream
    pc = new_rpn_model()
    left, right, targets = TO.scene(G, DEV)
    _, want = pc(left, right, targets, rng=np.random.RandomState(4))
    assert all(torch.equal(a[0][k], want[k].detach()) for k in want)


def test_detector_with_both_stages_returns_the_disparity_and_the_3d_losses():
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    from disprcnn_amd.structures.calib import Calib
    from tests.test_hip_train_caller import _inputs
    from tests.test_oracle_train_caller import H, W, scene
    from types import SimpleNamespace
    images, results, targets = _inputs(scene(), torch.device(DEV))
    results = {k: [b.to(DEV) for b in v] for k, v in results.items()}      # the 3D stage reads its boxes on the device
    for t in targets["left"]:                                             # a 3D box and a calibration per ground truth
        n = len(t)
        t.add_field("box3d", Box3DList(torch.tensor([[0.0, 1.6, 12.0, 1.5, 1.6, 3.9, 0.1]]).repeat(n, 1), (W, H), "xyzhwl_ry"))
        t.add_field("calib", Calib(SimpleNamespace(P2=G["P2s"][0], P3=G["P3s"][0]), (W, H)))
    m = new_detector(True, train_psm=True)
    state = np.random.get_state()
    try:
        np.random.seed(2)
        losses = m(images, results, targets)
    finally:
        np.random.set_state(state)
    assert sorted(losses) == ["disp_loss", "rpn_loss_cls", "rpn_loss_reg"]
    assert m.pcnet.pts_mean.shape[0] > 0                                  # clouds were made from PSMNet's disparities
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert any(float(p.grad.abs().max()) > 0 for p in m.pcnet.parameters())


# ---- 6. the batch without a cloud
@pytest.mark.parametrize("config", ["rpn", "rcnn"])
def test_empty_batch_gives_zero_losses_that_reach_every_trainable_parameter(config):
    m = new_rpn_model() if config == "rpn" else new_rcnn_model()
    left, right, targets = TO.scene(G, DEV)
    # only the image that has ROIs and no ground truth, and an image whose ROIs are all removed by the filters
    left, right, targets = [left[2], left[0][[5]]], [right[2], right[0][[5]]], [targets[2], targets[0]]
    ret, losses = m(left, right, targets, rng=np.random.RandomState(0))
    stage = m.rpn if config == "rpn" else m.rcnn_net
    assert ret == {} and sorted(losses) == (["rpn_loss_cls", "rpn_loss_reg"] if config == "rpn" else ["loss_box3d"])
    assert all(v.item() == 0.0 for v in losses.values())
    sum(losses.values()).backward()
    for n, p in stage.named_parameters():
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0, n
    if config == "rcnn":
        assert all(p.grad is None for p in m.rpn.parameters())
    assert m.pts_mean.shape == (0, 3)

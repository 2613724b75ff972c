"""DispRCNN3D with MODEL.DET3D_ON on the MI355X: the frame-change kernel against the fp64 oracle (tests/rcnn_oracle.py) and against the
torch composition it replaces, the offline form (2D results that carry their disparities) and the online form (a stereo pair) against the
stand-alone 3D stage, and the 3D results through the predictions file and the KITTI lines.

Tolerance of the kernel: measured in the same test, 2 x the torch composition's own maximum error against fp64 per output, plus
1e-6 * max|coordinate| -- what the project allows its fused kernels over the torch chain (tests/test_hip_s16.py).  Both orders of
operations are the same, so what differs is torch's bmm / norm summation and its device cos / sin / atan2.  Everything that joins two
runs of the same kernels on the same inputs is compared bit for bit.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rcnn_oracle as CO
from tests import rpn_oracle as RO
from tests import test_hip_rcnn as TR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
f32 = np.float32
G = TR.G
t = TR.t


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()


# ---- 6. the kernel
def frame_case(B, N, M, seed):
    """Clouds and proposals in the centred, rotated frame of their instance: |coordinate| <= 50 in the camera frame, sizes in [0.5, 5],
    angles over the full circle, zero padding boxes in the last quarter of the slots (with one slot: in cloud 2), rot[0] = 0, and the
    point 0 of every cloud at the origin (it comes back as the rotated mean)."""
    rs = np.random.RandomState(seed)
    mean = np.stack([rs.uniform(-12, 12, B), rs.uniform(-2, 2, B), rs.uniform(8, 34, B)], 1).astype(f32)
    rot = rs.uniform(-0.8, 0.8, B)
    rot[0] = 0.0
    xyz = np.clip(rs.normal(0, 2.0, (B, N, 3)), -6, 6).astype(f32)
    xyz[:, 0] = 0
    boxes = np.concatenate([rs.uniform(-5, 5, (B, M, 3)), rs.uniform(0.5, 5, (B, M, 3)), rs.uniform(-np.pi, np.pi, (B, M, 1))], 2).astype(f32)
    zero = np.zeros((B, M), bool)
    zero[:, M - M // 4:] = True
    if M == 1 and B > 2:
        zero[2, 0] = True
    boxes[zero] = 0
    return xyz, boxes, mean, rot, zero


def frame_errors(out_xyz, out_depth, out_boxes, ref_xyz, ref_boxes):
    ang = np.abs(out_boxes[..., 6].astype(np.float64) - ref_boxes[..., 6])
    return {"points": np.abs(out_xyz - ref_xyz).max(), "depth": np.abs(out_depth - np.sqrt((ref_xyz ** 2).sum(-1))).max(),
            "centre": np.abs(out_boxes[..., :3] - ref_boxes[..., :3]).max(), "size": np.abs(out_boxes[..., 3:6] - ref_boxes[..., 3:6]).max(),
            "angle": np.minimum(ang, np.abs(ang - 2 * np.pi)).max()}


@pytest.mark.parametrize("M", [1, 16, 512])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_frame_change_kernel_against_fp64_and_the_torch_composition(B, M):
    from disprcnn_amd.layers.rpn_proposals import points_depth, rpn_to_camera
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import proposals_to_camera_unfused
    N = 768
    xyz, boxes, mean, rot, zero = frame_case(B, N, M, 100 * B + M)
    ref_xyz = CO.rotate_back(xyz, mean, rot)
    ref_boxes = CO.rois_to_camera(boxes, mean, rot)
    scale = max(np.abs(ref_xyz).max(), np.abs(ref_boxes[..., :3]).max())
    assert scale <= 50
    d = {"backbone_xyz": t(xyz), "rpn_xyz": t(xyz), "roi_boxes3d": t(boxes)}
    unf = proposals_to_camera_unfused(d, t(mean), t(rot, torch.float64))
    got_xyz, got_depth, got_boxes = rpn_to_camera(t(xyz), t(boxes), t(mean), t(rot, torch.float64))
    assert torch.equal(got_depth, points_depth(got_xyz))                                   # the fixed rounding: same bits
    e_unf = frame_errors(unf["backbone_xyz"].cpu().numpy(), unf["pts_depth"].cpu().numpy(), unf["roi_boxes3d"].cpu().numpy(), ref_xyz, ref_boxes)
    gx, gb = got_xyz.cpu().numpy(), got_boxes.cpu().numpy()
    e_got = frame_errors(gx, got_depth.cpu().numpy(), gb, ref_xyz, ref_boxes)
    for k in e_got:
        print(f"B={B} M={M} {k}: kernel err {e_got[k]:.3g}, torch composition err {e_unf[k]:.3g}, bound {2 * e_unf[k] + 1e-6 * scale:.3g}")
    for k in e_got:
        assert e_got[k] <= 2 * e_unf[k] + 1e-6 * scale, k
    # zero padding boxes: the rotated mean (what the cloud's point at the origin becomes), zero size, angle -0.0; the composition's
    # convention is the same
    assert zero.any() or M == 1
    ub = unf["roi_boxes3d"].cpu().numpy()
    assert np.array_equal(gb[zero][:, :3], np.broadcast_to(gx[:, None, 0], (B, M, 3))[zero])
    assert (gb[zero][:, 3:] == 0).all() and np.signbit(gb[zero][:, 6]).all()
    assert (ub[zero][:, 3:] == 0).all() and np.array_equal(np.signbit(ub[zero][:, 6]), np.signbit(gb[zero][:, 6]))
    # rot = 0: nothing but the mean is added
    assert np.array_equal(gx[0], (xyz[0] + mean[0]).astype(f32))


def test_frame_change_kernel_on_the_reference_recording_and_at_edge_shapes():
    from disprcnn_amd.layers.rpn_proposals import points_depth, rpn_to_camera
    rs = np.random.RandomState(1)
    rois, mean, rot = G["box_b7"].reshape(3, 4, 7), G["box_mean"], G["box_rot"]
    cloud = rs.normal(0, 2, (3, 50, 3)).astype(f32)                                       # 50 points: the path without 16-byte accesses
    xyz, depth, boxes = rpn_to_camera(t(cloud), t(rois), t(mean), t(rot, torch.float64))
    assert np.abs(boxes.cpu().numpy() - G["box_cam32"]).max() <= 2e-5                     # the reference's own fp32 run
    back = CO.rotate_back(cloud, mean, rot)
    assert np.abs(xyz.cpu().numpy() - back).max() <= 8 * TR.EPS * np.abs(back).max()
    assert torch.equal(depth, points_depth(xyz))
    # the two point paths give the same bits: 768 points four at a time against the same points one at a time (a view that starts
    # 12 bytes into the buffer is made contiguous, 767 is not a multiple of 4)
    big = t(rs.normal(0, 3, (3, 768, 3)).astype(f32))
    a = rpn_to_camera(big, t(rois), t(mean), t(rot, torch.float64))
    b = rpn_to_camera(big[:, 1:], t(rois), t(mean), t(rot, torch.float64))
    assert torch.equal(a[0][:, 1:], b[0]) and torch.equal(a[1][:, 1:], b[1]) and torch.equal(a[2], b[2])
    # nothing to do: no launch, empty outputs of the right shapes
    for B, N, M in ((0, 50, 4), (3, 0, 0), (3, 0, 4), (3, 50, 0)):
        o = rpn_to_camera(t(cloud[:B, :N]), t(rois[:B, :M]), t(mean[:B]), t(rot[:B], torch.float64))
        assert o[0].shape == (B, N, 3) and o[1].shape == (B, N) and o[2].shape == (B, M, 7)
        if B and N:
            assert torch.equal(o[0], xyz[:, :N])
        if B and M:
            assert torch.equal(o[2], boxes[:, :M])
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        rpn_to_camera(t(cloud), t(rois), t(mean), t(rot))                                  # rot must be fp64


# ---- 7. the offline form
def fields_of(lists):
    out = []
    for lr in lists:
        d = {"box3d": lr.get_field("box3d").bbox_3d.cpu(), "mode": lr.get_field("box3d").mode, "size": lr.get_field("box3d").size,
             "scores_3d": lr.get_field("scores_3d").cpu()}
        if lr.has_field("random"):
            d["random"] = lr.get_field("random").cpu()
        out.append(d)
    return out


def same_fields(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) and x["mode"] == y["mode"] and x["size"] == y["size"]
        for k in ("box3d", "scores_3d", "random"):
            if k in x:
                assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k


def offline_model(n_inst, rcnn):
    from disprcnn_amd.modeling.detector.disprcnn3d import DispRCNN3D
    alone, _ = TR.new_point_rcnn(n_inst, rcnn=rcnn)
    cfg = RO.make_cfg({"MODEL": {"DISPNET_ON": False, "DET3D_ON": True, "POINTRCNN": TR.total_cfg(n_inst, rcnn=rcnn).MODEL.POINTRCNN}})
    model = DispRCNN3D(cfg).eval()
    model.load_state_dict({"pcnet." + k: v.cpu() for k, v in alone.state_dict().items()}, strict=True)
    assert not hasattr(model, "dispnet")
    return model.to(DEV)


def with_an_empty_image(left, right, calibs):
    from disprcnn_amd.structures.bounding_box import BoxList
    e = BoxList(torch.zeros(0, 4, device=DEV), left[0].size)
    e.add_field("disparity", left[0].get_field("disparity")[:0])
    e.add_field("mask", left[0].get_field("mask")[:0])
    return [left[0], e] + left[1:], [right[0], BoxList(torch.zeros(0, 4, device=DEV), e.size)] + right[1:], [calibs[0], calibs[0]] + calibs[1:]


@pytest.mark.parametrize("rcnn", [True, False])
def test_offline_form_equals_the_standalone_3d_stage(rcnn, tmp_path):
    from disprcnn_amd.utils.kitti_io import kitti_label_lines
    from disprcnn_amd.utils.predictions_io import load_predictions, save_predictions
    left, right, calibs = with_an_empty_image(*TR.scene())
    n_inst = sum(len(a) for a in left)
    assert n_inst == 12 and [len(a) for a in left][1] == 0
    model = offline_model(n_inst, rcnn)
    with torch.no_grad():
        out = model("the images are not read", {"left": left, "right": right}, {"left": calibs})
        l2, r2, c2 = with_an_empty_image(*TR.scene())
        want_l, _, _ = model.pcnet(l2, r2, c2)
    assert sorted(out) == ["left", "right"] and [len(a) for a in out["left"]] == [len(a) for a in left]
    got, want = fields_of(out["left"]), fields_of(want_l)
    same_fields(got, want)
    assert [len(g["box3d"]) for g in got] == [len(a) for a in left] and ("random" in got[0]) == rcnn
    assert got[0]["mode"] == ("ry_lhwxyz" if rcnn else "xyzhwl_ry") and len(got[1]["box3d"]) == 0 and got[1]["scores_3d"].numel() == 0
    with pytest.raises(ValueError):
        model("images", {"left": left, "right": right})
    # a batch without any ROI
    el, er, ec = with_an_empty_image(*TR.scene())
    with torch.no_grad():
        none = model(None, {"left": el[1:2], "right": er[1:2]}, {"left": ec[1:2]})
    assert len(none["left"][0].get_field("box3d")) == 0 and none["left"][0].get_field("scores_3d").numel() == 0
    # 9. the results of a real run through the predictions file and the KITTI lines
    path = str(tmp_path / "predictions.pth")
    save_predictions(out, path)
    back = load_predictions(path)
    same_fields(fields_of(back["left"]), got)
    for b, src in zip(back["left"], out["left"]):
        assert torch.equal(b.bbox, src.bbox.cpu()) and not b.get_field("box3d").bbox_3d.is_cuda
        lines = kitti_label_lines(b)
        assert len(lines) == len(b) == len(src)
        conv = b.get_field("box3d").convert("xyzhwl_ry").bbox_3d.tolist()
        for ln, c, s in zip(lines, conv, b.get_field("scores_3d").tolist()):
            tok = ln.split(" ")
            assert len(tok) == 16 and tok[0] == "Car" and [float(v) for v in tok[8:15]] == [c[3], c[4], c[5], c[0], c[1], c[2], c[6]]
            assert float(tok[15]) == s


def test_gather_predictions_takes_the_real_output_to_one_device():
    """The 3D stage leaves `bbox` on the GPU and attaches `box3d`, `scores_3d`, `random` as CPU tensors.  A collective takes tensors of
    the group's device only, so gather_predictions must put every part on the boxes' device before it concatenates: checked here on
    the real output in one process (the two-rank exchange itself is tests/test_comm_gloo_box3d.py's)."""
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    from disprcnn_amd.utils import comm
    left, right, calibs = with_an_empty_image(*TR.scene())
    model = offline_model(sum(len(a) for a in left), True)
    with torch.no_grad():
        out = model(None, {"left": left, "right": right}, {"left": calibs})["left"]
    assert all(lr.bbox.is_cuda and not lr.get_field("scores_3d").is_cuda and not lr.get_field("box3d").bbox_3d.is_cuda for lr in out)
    got = comm.gather_predictions({i: lr for i, lr in enumerate(out)}, ("box3d", "scores_3d", "random", "disparity"))
    assert len(got) == len(out)
    for g, src in zip(got, out):
        dev = src.bbox.device
        b3 = g.get_field("box3d")
        assert type(b3) is Box3DList and b3.mode == "ry_lhwxyz" and b3.size == src.size and len(g) == len(src) and g.bbox.device == dev
        assert b3.bbox_3d.device == dev and torch.equal(b3.bbox_3d.cpu(), src.get_field("box3d").bbox_3d)
        for f in ("scores_3d", "random", "disparity"):
            assert g.get_field(f).device == dev and g.get_field(f).dtype == src.get_field(f).dtype
            assert torch.equal(g.get_field(f).cpu(), src.get_field(f).cpu()), f


# ---- 8. the online form
KITTI_P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
KITTI_P3 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]])


def test_online_form_stereo_pair_to_3d_boxes():
    from disprcnn_amd.modeling.detector import build_detection_model
    from disprcnn_amd.modeling.detector.disprcnn3d import default_cfg
    from disprcnn_amd.structures import BoxList, ImageList
    from disprcnn_amd.structures.calib import Calib
    from disprcnn_amd.utils import synth
    from tests.helpers import state_for
    W, H, res = 320, 256, 224
    n_inst = 3
    alone, _ = TR.new_point_rcnn(n_inst)
    cfg = default_cfg(48, -48, res)
    cfg.MODEL.DET3D_ON, cfg.MODEL.POINTRCNN = True, TR.total_cfg(n_inst).MODEL.POINTRCNN
    model = build_detection_model(cfg)
    model.dispnet.load_state_dict(state_for("B"), strict=True)
    model.pcnet.load_state_dict({k: v.cpu() for k, v in alone.state_dict().items()}, strict=True)
    assert set(model.state_dict()) == {"dispnet." + k for k in model.dispnet.state_dict()} | {"pcnet." + k for k in alone.state_dict()}
    model = model.to(DEV).eval()
    base = synth.hash_uniform("det3d:L", (2, 3, H // 8, W // 8), 0.0, 1.0)
    limg = torch.nn.functional.interpolate(base, (H, W), mode="bilinear", align_corners=True)
    rimg = torch.roll(limg, -5, 3)                                    # a 5-pixel shift: with fu * baseline = 384.4 every depth is positive
    lb = [torch.tensor([[20.4, 10.2, 200.7, 180.3], [0.5, 0.5, 1.2, 1.4], [150.2, 60.5, 300.9, 240.1]]), torch.tensor([[60.3, 30.8, 170.2, 200.6]])]
    rb = [torch.tensor([[14.9, 10.0, 195.2, 181.0], [0.5, 0.5, 1.2, 1.4], [144.0, 60.0, 295.5, 241.0]]), torch.tensor([[55.1, 31.0, 164.7, 200.0]])]

    def results():
        lres, rres = [], []
        for l, r in zip(lb, rb):
            a = BoxList(l.to(DEV), (W, H))
            a.add_field("mask", torch.ones(len(l), 1, 28, 28, device=DEV))
            lres.append(a)
            rres.append(BoxList(r.to(DEV), (W, H)))
        return {"left": lres, "right": rres}

    calibs = [Calib(SimpleNamespace(P2=KITTI_P2, P3=KITTI_P3), (W, H)) for _ in lb]
    images = {"left": ImageList(limg.to(DEV), [(H, W)] * 2), "right": ImageList(rimg.to(DEV), [(H, W)] * 2)}
    with torch.no_grad():
        out = model(images, results(), {"left": calibs})
    counts = model.pcnet.pointcloud.last_counts
    print("kept points per ROI:", counts)
    assert len(counts) == n_inst and min(counts) >= 1                 # every ROI keeps points: none is skipped below
    assert [len(a) for a in out["left"]] == [2, 1] == [len(a) for a in out["right"]]
    for lr in out["left"]:
        n = len(lr)
        assert tuple(lr.get_field("disparity").shape) == (n, res, res) and tuple(lr.get_field("roi_geom").shape) == (n, 4)
        b3 = lr.get_field("box3d")
        assert b3.mode == "ry_lhwxyz" and len(b3) == n and b3.size == (W, H) and torch.isfinite(b3.bbox_3d).all()
        assert lr.get_field("scores_3d").shape == (n,) and lr.get_field("random").shape == (n,) and lr.get_field("random").dtype == torch.int64
    # the 3D stage alone on what the disparity stage left behind
    l2 = [lr.copy_with_fields(["disparity", "mask"]) for lr in out["left"]]
    r2 = [BoxList(rr.bbox, rr.size) for rr in out["right"]]
    with torch.no_grad():
        want_l, _, _ = model.pcnet(l2, r2, calibs)
    same_fields(fields_of(out["left"]), fields_of(want_l))
    with pytest.raises(ValueError):
        model(images, results())


# ---- 10. resources
def test_frame_change_kernel_reports_no_scratch():
    import re
    import subprocess
    import tempfile
    from disprcnn_amd.csrc.build import FLAGS, HIPCC
    src = os.path.join(os.path.dirname(HERE), "disprcnn_amd", "pts", "frame_ops.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "frame_ops.o")],
                           capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    print(list(zip(names, scratch, lds)))
    assert len(names) == 2 and all("rpn_to_camera_kernel" in n for n in names)             # four points at a time, and one at a time
    assert scratch == [0, 0] and lds == [0, 0]

"""Host checks of the 3D box ops (no GPU): the NumPy oracle against the reference's recorded outputs and an independent fp64 clip,
hand-computed geometry, the C ABI declarations and the CPU-only names of roipool3d_cuda."""
import math
import os
import re

import numpy as np
import pytest

from tests import box3d_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "boxes3d_ref_golden.npz"))
THS = (0.0, 0.1, 0.8, 1.0)
PI = np.float32(np.pi)


def test_oracle_pairwise_vs_golden():
    a, b = G["bev_a"], G["bev_b"]
    np.testing.assert_allclose(O.box_overlap(a, b), G["bev_overlap"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(O.iou_bev(a, b), G["bev_iou"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(O.iou_normal(a, b), G["bev_iou_normal"])
    np.testing.assert_allclose(O.iou_bev(G["hand_a"], G["hand_b"]), G["hand_iou"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(O.box_overlap(G["hand_a"], G["hand_b"]), G["hand_overlap"], rtol=1e-5, atol=1e-6)


def test_oracle_iou3d_and_bev_vs_golden():
    # NumPy's float32 cos / sin are not glibc's: a last-place difference moves the IoU by a few ulp
    np.testing.assert_allclose(O.iou3d(G["b7_a"], G["b7_b"]), G["iou3d"], rtol=4e-6, atol=1e-6)
    np.testing.assert_array_equal(O.boxes3d_to_bev(G["b7_a"]), G["bev_of_a"])
    np.testing.assert_array_equal(O.enlarge_box3d(G["b7_a"], 1.0), G["enlarged_a"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 768])
@pytest.mark.parametrize("normal", [False, True])
def test_oracle_nms_vs_golden(n, normal):
    tag = f"nms{'n' if normal else 'r'}_{n}"
    for t in THS:
        np.testing.assert_array_equal(O.nms_sorted(G[tag + "_boxes"], t, normal), G[f"{tag}_keep_{t}"])


def test_oracle_roipool_vs_golden():
    pts, boxes = G["pool_pts"], G["pool_boxes"]
    for w in (0.0, 1.0):
        for b in range(pts.shape[0]):
            big = O.enlarge_box3d(boxes[b], w)
            flags = O.pts_in_boxes3d(pts[b], big)
            np.testing.assert_array_equal(np.packbits(flags.astype(np.uint8), axis=-1), G[f"pool_{w}_flags"][b])
            idx, empty = O.pooled_idx(flags, 512)
            np.testing.assert_array_equal(empty, G[f"pool_{w}_empty"][b])
            np.testing.assert_array_equal(idx[empty == 0], G[f"pool_{w}_idx"][b][empty == 0])
    counts = np.unpackbits(G["pool_0.0_flags"], axis=-1)[..., :pts.shape[1]].sum(-1)
    assert {0, 1, 511, 512, 600, 4} <= set(counts.ravel().tolist())


def test_fp32_restatement_vs_fp64_clip():
    r = np.random.RandomState(3)
    c = r.uniform(-3, 3, (60, 2))
    s = r.uniform(0.3, 4, (60, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2, r.uniform(-4, 4, (60, 1))], 1).astype(np.float32)
    a, b = boxes[:30], boxes[30:]
    got = O.box_overlap(a, b)
    want = np.array([[O.clip_overlap64(x, y) for y in b] for x in a])
    assert (want > 0).mean() > 0.2
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("a,b,area,iou", [
    ([0, 0, 2, 2, 0], [0, 0, 2, 2, 0], 4.0, 1.0),                     # identical
    ([0, 0, 2, 2, 0], [0.5, 0.5, 1.5, 1.5, 0], 1.0, 0.25),            # containment
    ([0, 0, 2, 2, 0], [5, 5, 6, 6, 0], 0.0, 0.0),                     # disjoint
    ([0, 0, 2, 2, 0], [2, 0, 4, 2, 0], 0.0, 0.0),                     # touching edges
    ([0, 0, 2, 2, 0], [0, 0, 2, 2, math.pi / 2], 4.0, 1.0),           # pi/2: coincident edges
    ([0, 0, 4, 2, math.pi], [0, 0, 4, 2, -math.pi], 8.0, 1.0),       # ry = +-pi
    ([0, 0, 4, 2, 0], [1, -1, 3, 3, math.pi / 2], 8.0, 1.0),          # a 2x4 box turned by pi/2 onto a 4x2 one
    ([1, 1, 1, 3, 0], [0, 0, 2, 2, 0], 0.0, 0.0),                     # zero-area box
])
def test_hand_cases(a, b, area, iou):
    a, b = np.array([a], np.float32), np.array([b], np.float32)
    assert abs(float(O.box_overlap(a, b)[0, 0]) - area) < 1e-5
    assert abs(float(O.iou_bev(a, b)[0, 0]) - iou) < 1e-6
    assert abs(O.clip_overlap64(a[0], b[0]) - area) < 1e-5      # fp32 pi is not pi


def test_hand_nms_and_stable_order():
    boxes = np.array([[0, 0, 2, 2, 0], [0.1, 0, 2.1, 2, 0], [5, 5, 6, 6, 0], [0, 0, 2, 2, 0.05]], np.float32)
    np.testing.assert_array_equal(O.nms(boxes, np.array([0.9, 0.8, 0.7, 0.6], np.float32), 0.5), [0, 2])
    np.testing.assert_array_equal(O.nms(boxes, np.array([0.5, 0.5, 0.5, 0.5], np.float32), 0.5), [0, 2])    # ties: index order
    np.testing.assert_array_equal(O.nms(boxes, np.array([0.1, 0.9, 0.2, 0.3], np.float32), 0.5), [1, 2])    # score order out


def test_pts_in_box_on_faces():
    box = np.array([[11.0, 1.0, 30.0, 1.0, 1.0, 2.0, 0.0]], np.float32)
    pts = np.array([[10, 1, 30], [12, 1, 30], [11, 1, 29.5], [11, 0, 30.5], [12.001, 0.5, 30], [11, 1.001, 30], [11, -0.001, 30]], np.float32)
    np.testing.assert_array_equal(O.pts_in_boxes3d(pts, box)[0], [1, 1, 1, 1, 0, 0, 0])
    far = np.array([[0, 0, 0, 1, 30, 30, 0]], np.float32)          # max_dis 10 cuts a box wider than 20 m
    np.testing.assert_array_equal(O.pts_in_boxes3d(np.array([[9.9, -0.5, 0], [10.1, -0.5, 0]], np.float32), far)[0], [1, 0])


def test_sigs_match_header():
    from disprcnn_amd.pts import _lib
    hdr = open(os.path.join(HERE, "..", "include", "disprcnn_pts.h")).read()
    for name in ("drc_box3d_bev", "drc_box3d_iou3d", "drc_box3d_nms", "drc_roipool3d_fwd", "drc_box3d_max_pool_samples", "drc_pts_in_boxes3d"):
        m = re.search(r"\bint\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_lib._SIGS[name][1]), name


def test_cpu_only_names_raise():
    from disprcnn_amd import roipool3d_cuda
    with pytest.raises(NotImplementedError, match="pts_in_boxes3d_cpu"):
        roipool3d_cuda.pts_in_boxes3d_cpu(None, None, None)
    with pytest.raises(NotImplementedError, match="roipool3d_cpu"):
        roipool3d_cuda.roipool3d_cpu(None, None, None, None, None, None)

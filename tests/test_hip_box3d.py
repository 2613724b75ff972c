"""PointRCNN's 3D box ops on the MI355X against the reference's recorded outputs (tests/golden/boxes3d_ref_golden.npz) and the NumPy
oracle (tests/box3d_oracle.py).  IoU within 1e-6 (the overlap area within 1e-5 relative): host libm and the device's atan2 / cos / sin
may differ in the last place.  NMS keep lists and roipool3d outputs bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import box3d_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "boxes3d_ref_golden.npz"))
THS = (0.0, 0.1, 0.8, 1.0)
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def L():
    from disprcnn_amd.layers import iou3d
    return iou3d


def R():
    from disprcnn_amd.layers import roipool3d
    return roipool3d


def rand_bev(r, n, span=40.0):
    c, s = r.uniform(-span, span, (n, 2)), r.uniform(0.5, 5.0, (n, 2))
    return np.concatenate([c - s / 2, c + s / 2, r.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


def rand_b7(r, n):
    return np.stack([r.uniform(-30, 30, n), r.uniform(1, 2, n), r.uniform(2, 80, n), r.uniform(1.2, 2.2, n), r.uniform(1.4, 2, n),
                     r.uniform(3, 5, n), r.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)


def overlap_close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


def iou_close(got, want):
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6)


def kitti_iou_close(got, want):
    """At 80 m the fp32 corner coordinates are 8e-6 apart, so a last-place difference between NumPy's float32 cos / sin (the oracle)
    and the device's moves an overlap area, and the IoU, by a few 1e-6 relative."""
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


def test_bev_vs_golden_and_oracle():
    for a, b, ov, iou in ((G["bev_a"], G["bev_b"], G["bev_overlap"], G["bev_iou"]), (G["hand_a"], G["hand_b"], G["hand_overlap"], G["hand_iou"])):
        got_ov = L().boxes_overlap_bev(t(a), t(b)).cpu().numpy()
        got_iou = L().boxes_iou_bev(t(a), t(b)).cpu().numpy()
        overlap_close(got_ov, ov)
        iou_close(got_iou, iou)
        overlap_close(got_ov, O.box_overlap(a, b))
        iou_close(got_iou, O.iou_bev(a, b))


def test_iou3d_vs_golden_and_oracle():
    got = L().boxes_iou3d_gpu(t(G["b7_a"]), t(G["b7_b"])).cpu().numpy()
    iou_close(got, G["iou3d"])
    iou_close(got, O.iou3d(G["b7_a"], G["b7_b"]))
    np.testing.assert_array_equal(L().boxes3d_to_bev_torch(t(G["b7_a"])).cpu().numpy(), G["bev_of_a"])
    np.testing.assert_array_equal(R().enlarge_box3d(t(G["b7_a"]), 1.0).cpu().numpy(), G["enlarged_a"])


@pytest.mark.parametrize("na", [0, 1, 15, 16, 17, 257])
@pytest.mark.parametrize("nb", [0, 1, 16, 17, 257])
def test_shapes(na, nb):
    r = np.random.RandomState(na * 1000 + nb)
    a, b = rand_bev(r, na, span=3.0), rand_bev(r, nb, span=3.0)
    got = L().boxes_iou_bev(t(a), t(b)).cpu().numpy()
    if na == 0 or nb == 0:
        assert got.shape == (1, 1)
    else:
        iou_close(got, O.iou_bev(a, b))
    a7, b7 = rand_b7(r, na), rand_b7(r, nb)
    if na and nb:
        b7[: min(na, nb)] = a7[: min(na, nb)] + r.normal(0, 0.3, (min(na, nb), 7)).astype(np.float32)
    got = L().boxes_iou3d_gpu(t(a7), t(b7)).cpu().numpy()
    if na == 0 or nb == 0:
        assert got.shape == (nb, na)
    else:
        kitti_iou_close(got, O.iou3d(a7, b7))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 768, 9000])
@pytest.mark.parametrize("normal", [False, True])
def test_nms_vs_golden(n, normal):
    tag = f"nms{'n' if normal else 'r'}_{n}"
    boxes = G[tag + "_boxes"]
    scores = t(np.linspace(1.0, 0.0, n, dtype=np.float32)) if n else torch.zeros(0, device=DEV)    # already in score order
    fn = L().nms_normal_gpu if normal else L().nms_gpu
    for th in THS:
        got = fn(t(boxes).reshape(-1, 5), scores, th).cpu().numpy()
        np.testing.assert_array_equal(got, G[f"{tag}_keep_{th}"])
        if n <= 65:
            np.testing.assert_array_equal(got, O.nms_sorted(boxes, th, normal))


def test_nms_score_order_and_ties():
    boxes = np.array([[0, 0, 2, 2, 0], [0.1, 0, 2.1, 2, 0], [5, 5, 6, 6, 0], [0, 0, 2, 2, 0.05]], np.float32)
    for sc in ([0.1, 0.9, 0.2, 0.3], [0.5, 0.5, 0.5, 0.5]):
        s = np.array(sc, np.float32)
        got = L().nms_gpu(t(boxes), t(s), 0.5).cpu().numpy()
        np.testing.assert_array_equal(got, O.nms(boxes, s, 0.5))


def _batched_case(r, B, N, counts):
    centers = rand_bev(r, 8, span=10.0).astype(np.float64)
    k = r.randint(0, 8, (B, N))
    boxes = (centers[k] + r.normal(0, 1, (B, N, 5)) * np.array([0.4, 0.4, 0.4, 0.4, 0.15])).astype(np.float32)
    boxes[..., 2] = np.maximum(boxes[..., 2], boxes[..., 0] + 0.3)
    boxes[..., 3] = np.maximum(boxes[..., 3], boxes[..., 1] + 0.3)
    scores = r.permutation(B * N).reshape(B, N).astype(np.float32) / (B * N)
    return boxes, scores, np.asarray(counts, np.int32)


@pytest.mark.parametrize("shape", [(16, 562, 0.8), (16, 100, 0.1)])        # ProposalLayer (9000 // 16), rcnn_inference
@pytest.mark.parametrize("max_keep", [-1, 6])
@pytest.mark.parametrize("normal", [False, True])
def test_nms_batched_equals_loop(shape, max_keep, normal):
    B, N, th = shape
    r = np.random.RandomState(N + max_keep)
    counts = r.randint(1, N + 1, B)
    counts[3], counts[7], counts[0] = 0, N, 1
    boxes, scores, counts = _batched_case(r, B, N, counts)
    keep, num = L().nms_gpu_batched(t(boxes), t(scores), t(counts, torch.int32), th, max_keep=max_keep, normal=normal)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    assert keep.shape == (B, min(max_keep, N) if max_keep > 0 else N)
    fn = L().nms_normal_gpu if normal else L().nms_gpu
    for b in range(B):
        c = int(counts[b])
        ref = fn(t(boxes[b, :c]).reshape(-1, 5), t(scores[b, :c]), th).cpu().numpy()
        if max_keep > 0:
            ref = ref[:max_keep]
        assert num[b] == ref.size
        np.testing.assert_array_equal(keep[b, :num[b]], ref)
        assert (keep[b, num[b]:] == -1).all()


def _pool_feat(B, N, C, seed=5):
    return np.random.RandomState(seed).standard_normal((B, N, C)).astype(np.float32)


@pytest.mark.parametrize("C", [0, 130])
@pytest.mark.parametrize("w", [0.0, 1.0])
def test_roipool3d_vs_golden_and_oracle(C, w):
    pts, boxes = G["pool_pts"], G["pool_boxes"]
    feat = _pool_feat(pts.shape[0], pts.shape[1], C)
    pooled, empty = R().roipool3d_gpu(t(pts), t(feat), t(boxes), w, 512)
    pooled, empty = pooled.cpu().numpy(), empty.cpu().numpy()
    assert pooled.dtype == np.float32 and empty.dtype == np.int32 and pooled.shape == (2, 6, 512, 3 + C)
    np.testing.assert_array_equal(empty, G[f"pool_{w}_empty"])
    want = np.zeros_like(pooled)
    for b in range(2):
        rows = np.concatenate([pts[b], feat[b]], 1)
        for m in range(6):
            if not G[f"pool_{w}_empty"][b, m]:
                want[b, m] = rows[G[f"pool_{w}_idx"][b, m].astype(np.int64)]
    np.testing.assert_array_equal(pooled, want)
    o_pooled, o_empty = O.roipool3d(pts, feat, boxes, w, 512)
    np.testing.assert_array_equal(pooled, o_pooled)
    np.testing.assert_array_equal(empty, o_empty)


def test_pts_in_boxes3d_vs_golden():
    pts, boxes = G["pool_pts"], G["pool_boxes"]
    for w in (0.0, 1.0):
        big = torch.stack([R().enlarge_box3d(t(boxes[b]), w) for b in range(2)])
        got = R().pts_in_boxes3d_gpu(t(pts), big).cpu().numpy()
        np.testing.assert_array_equal(np.packbits(got.astype(np.uint8), axis=-1), G[f"pool_{w}_flags"])
    single = R().pts_in_boxes3d_gpu(t(pts[0]), t(boxes[0])).cpu().numpy()
    np.testing.assert_array_equal(single, O.pts_in_boxes3d(pts[0], boxes[0]))


def test_roipool3d_small_S_and_lds_limit():
    from disprcnn_amd import roipool3d_cuda
    pts, boxes = G["pool_pts"], G["pool_boxes"]
    feat = _pool_feat(2, pts.shape[1], 4)
    for S in (1, 7, 513):
        got = R().roipool3d_gpu(t(pts), t(feat), t(boxes), 0.5, S)
        want = O.roipool3d(pts, feat, boxes, 0.5, S)
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1])
    with pytest.raises(RuntimeError, match="LDS"):
        R().roipool3d_gpu(t(pts), t(feat), t(boxes), 0.0, roipool3d_cuda.max_sampled_pt_num() + 1)


def test_argument_errors():
    from disprcnn_amd import iou3d_cuda, roipool3d_cuda
    a = torch.zeros(4, 5, device=DEV)
    out = torch.zeros(4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        iou3d_cuda.boxes_iou_bev_gpu(a.cpu(), a, out)
    with pytest.raises(RuntimeError, match="float32"):
        iou3d_cuda.boxes_iou_bev_gpu(a.double(), a, out)
    with pytest.raises(RuntimeError, match="contiguous"):
        iou3d_cuda.boxes_overlap_bev_gpu(torch.zeros(5, 4, device=DEV).t(), a, out)
    with pytest.raises(RuntimeError, match="elements"):
        iou3d_cuda.boxes_iou_bev_gpu(a, a, torch.zeros(3, 4, device=DEV))
    with pytest.raises(RuntimeError, match="int64"):
        iou3d_cuda.nms_gpu(a, torch.zeros(4, dtype=torch.int32), 0.5)
    with pytest.raises(RuntimeError):
        L().boxes_iou3d_gpu(torch.zeros(3, 7), torch.zeros(3, 7))
    pts, bx, ft = torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 2, 7, device=DEV), torch.zeros(1, 8, 2, device=DEV)
    pooled, flag = torch.zeros(1, 2, 4, 5, device=DEV), torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        roipool3d_cuda.forward(pts.cpu(), bx, ft, pooled, flag)
    with pytest.raises(RuntimeError, match="int32"):
        roipool3d_cuda.forward(pts, bx, ft, pooled, flag.long())
    with pytest.raises(RuntimeError, match="contiguous"):
        roipool3d_cuda.forward(pts, bx, torch.zeros(1, 2, 8, device=DEV).transpose(1, 2), pooled, flag)
    with pytest.raises(RuntimeError, match="shape"):
        roipool3d_cuda.forward(pts, bx, ft, torch.zeros(1, 2, 4, 6, device=DEV), flag)


def test_deterministic():
    r = np.random.RandomState(9)
    a, b = rand_bev(r, 300, span=5.0), rand_bev(r, 200, span=5.0)
    x = [L().boxes_iou_bev(t(a), t(b)) for _ in range(2)]
    assert torch.equal(x[0], x[1])
    a7 = rand_b7(r, 512)
    x = [L().boxes_iou3d_gpu(t(a7), t(a7[:64])) for _ in range(2)]
    assert torch.equal(x[0], x[1])
    boxes, scores, counts = _batched_case(r, 16, 562, r.randint(0, 563, 16))
    x = [L().nms_gpu_batched(t(boxes), t(scores), t(counts, torch.int32), 0.8) for _ in range(2)]
    assert torch.equal(x[0][0], x[1][0]) and torch.equal(x[0][1], x[1][1])
    pts, bx = G["pool_pts"], G["pool_boxes"]
    feat = _pool_feat(2, pts.shape[1], 130)
    x = [R().roipool3d_gpu(t(pts), t(feat), t(bx), 1.0) for _ in range(2)]
    assert torch.equal(x[0][0], x[1][0]) and torch.equal(x[0][1], x[1][1])


def test_drop_in_extension_calls():
    """iou3d_utils.py / roipool3d_utils.py's calls, argument for argument, against layers.iou3d / layers.roipool3d."""
    from disprcnn_amd import iou3d_cuda, roipool3d_cuda
    r = np.random.RandomState(11)
    a, b = t(rand_bev(r, 33, span=4.0)), t(rand_bev(r, 20, span=4.0))
    ans_iou = torch.zeros((33, 20), dtype=torch.float32, device=DEV)
    assert iou3d_cuda.boxes_iou_bev_gpu(a.contiguous(), b.contiguous(), ans_iou) == 1
    assert torch.equal(ans_iou, L().boxes_iou_bev(a, b))
    ov = torch.zeros((33, 20), dtype=torch.float32, device=DEV)
    iou3d_cuda.boxes_overlap_bev_gpu(a.contiguous(), b.contiguous(), ov)
    assert torch.equal(ov, L().boxes_overlap_bev(a, b))
    scores = t(r.permutation(33).astype(np.float32))
    for name in ("nms_gpu", "nms_normal_gpu"):
        order = scores.sort(0, descending=True)[1]
        boxes = a[order].contiguous()
        keep = torch.LongTensor(boxes.size(0))
        num_out = getattr(iou3d_cuda, name)(boxes, keep, 0.1)
        assert keep.device.type == "cpu"
        got = order[keep[:num_out].cuda()].contiguous()
        assert torch.equal(got, getattr(L(), name)(a, scores, 0.1))
    pts, bx = G["pool_pts"], G["pool_boxes"]
    feat = t(_pool_feat(2, pts.shape[1], 130))
    pooled_boxes3d = R().enlarge_box3d(t(bx).view(-1, 7), 1.0).view(2, -1, 7)
    pooled_features = torch.zeros((2, 6, 512, 3 + 130), dtype=torch.float32, device=DEV)
    pooled_empty_flag = torch.zeros((2, 6), dtype=torch.int32, device=DEV)
    roipool3d_cuda.forward(t(pts).contiguous(), pooled_boxes3d.contiguous(), feat.contiguous(), pooled_features, pooled_empty_flag)
    want = R().roipool3d_gpu(t(pts), feat, t(bx), 1.0, 512)
    assert torch.equal(pooled_features, want[0]) and torch.equal(pooled_empty_flag, want[1])

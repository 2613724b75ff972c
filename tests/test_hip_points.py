"""The 3D stage's point ops on the MI355X: InstancePointCloud vs the reference's golden, the PointNet++ kernels vs tests/pn2_oracle.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pn2_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "points_ref_golden.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs cuda:0")
    return torch.device("cuda:0")


EDGES = os.path.join(os.path.dirname(__file__), "golden", "points_ref_edges_golden.npz")


def _golden_inputs(dev, g=None, cams=None):
    """Per-image BoxLists and Calibs of a golden scene.  cams: one (P2, P3) per image; by default the two cameras of GOLDEN."""
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.calib import Calib
    g = g if g is not None else np.load(GOLDEN)
    W, H = int(g["W"]), int(g["H"])
    left, right, calibs, r = [], [], [], 0
    cams = cams if cams is not None else [(g["P2"], g["P3"]), (g["P2B"], g["P3B"])]
    for i, n in enumerate(g["rois_per_image"].tolist()):
        lb = BoxList(torch.from_numpy(g["left_boxes"][r:r + n]).to(dev), (W, H))
        lb.add_field("disparity", torch.from_numpy(g["disparity"][r:r + n]).to(dev))
        lb.add_field("mask", torch.from_numpy(g["mask"][r:r + n]).to(dev))
        left.append(lb)
        right.append(BoxList(torch.from_numpy(g["right_boxes"][r:r + n]).to(dev), (W, H)))
        calibs.append(Calib(SimpleNamespace(P2=cams[i][0], P3=cams[i][1]), (W, H)))
        r += n
    return left, right, calibs


def _edge_cams(g):
    return list(zip(g["P2s"], g["P3s"]))


def _check_against(g, ipc, pts, mean, rot):
    """InstancePointCloud's outputs vs a golden scene; returns the per-point scale of the bound."""
    assert pts.shape == g["pts"].shape and mean.shape == g["pts_mean"].shape and rot.dtype == torch.float64
    assert ipc.last_counts == g["counts"].tolist()
    src = ipc.last_src_pix.cpu().numpy()
    for r in range(src.shape[0]):
        assert np.array_equal(np.sort(src[r]), np.sort(g["src_pix"][r])), r
    assert np.array_equal(src, g["src_pix"])                       # same draw -> same order
    np.testing.assert_allclose(rot.cpu().numpy(), g["rot_angle"], rtol=0, atol=1e-12)
    # test_hip_post's roi_depth_maps bounds (rtol 2e-4, atol 1e-4) on depth, carried to the points in the uncentred frame
    got = (pts + mean[:, None]).cpu().numpy()
    ref = g["pts"] + g["pts_mean"][:, None]
    scale = np.linalg.norm(ref, axis=2, keepdims=True)
    assert (np.abs(got - ref) <= 2e-4 * scale + 1e-4).all(), np.abs(got - ref).max()
    ms = np.linalg.norm(g["pts_mean"], axis=1, keepdims=True)
    assert (np.abs(mean.cpu().numpy() - g["pts_mean"]) <= 2e-4 * ms + 1e-4).all()
    # centred points: the same error bound (it comes from the depth, not from the centred magnitude)
    assert (np.abs(pts.cpu().numpy() - g["pts"]) <= 2 * (2e-4 * scale + 1e-4)).all()
    return scale


def test_instance_points_match_the_reference(dev):
    from disprcnn_amd.modeling.pointcloud import InstancePointCloud
    g = np.load(GOLDEN)
    ipc = InstancePointCloud(npoints=int(g["npoints"]))
    pts, mean, rot = ipc(*_golden_inputs(dev, g))
    scale = _check_against(g, ipc, pts, mean, rot)
    back = InstancePointCloud.rotate_back(pts + mean[:, None], rot)
    assert back.shape == pts.shape and torch.isfinite(back).all()
    # ... and it inverts the rotation: the reference's points rotated back in fp64, at the same bound
    ref = g["pts"] + g["pts_mean"][:, None]
    a = -g["rot_angle"][:, None]
    ref_back = ref.astype(np.float64).copy()
    ref_back[..., 0] = ref[..., 0] * np.cos(a) - ref[..., 2] * np.sin(a)
    ref_back[..., 2] = ref[..., 0] * np.sin(a) + ref[..., 2] * np.cos(a)
    assert (np.abs(back.cpu().numpy() - ref_back) <= 2e-4 * scale + 1e-4).all()


def test_instance_points_match_the_reference_at_the_edges(dev):
    """points_ref_edges_golden.npz (make_golden_points.py --edges): depths past the 160 m clamp, negative disparity, right boxes wider
    and narrower than the left, boxes on all four image borders, 1-px-high and 2-px-wide boxes, a graded mask, a non-empty mask the
    reference does not apply, an image without ROIs, and > 1<<20 box pixels in all (the workspace grows)."""
    from disprcnn_amd.modeling.pointcloud import InstancePointCloud
    g = np.load(EDGES)
    assert not g["mask_applied"].all() and g["rois_per_image"][1] == 0
    ipc = InstancePointCloud(npoints=int(g["npoints"]))
    pts, mean, rot = ipc(*_golden_inputs(dev, g, _edge_cams(g)))
    assert ipc._ws[dev].numel() > 1 << 20                                # the regrow pass ran
    scale = _check_against(g, ipc, pts, mean, rot)
    # rotate_back undoes the rotation: back_project's points (before rotation) at the same bound
    back = InstancePointCloud.rotate_back(pts + mean[:, None], rot).cpu().numpy()
    assert (np.abs(back - g["pts_pre_rotation"]) <= 2e-4 * scale + 1e-4).all(), np.abs(back - g["pts_pre_rotation"]).max()
    assert (g["pts_pre_rotation"][..., 2] == 160).any()                 # the max_depth clamp acted
    # a second, smaller call on the grown workspace
    g0 = np.load(GOLDEN)
    _check_against(g0, ipc, *ipc(*_golden_inputs(dev, g0)))


def test_instance_points_are_bit_identical_across_calls(dev):
    from disprcnn_amd.modeling.pointcloud import InstancePointCloud
    inputs = _golden_inputs(dev)
    a = InstancePointCloud()(*inputs)
    b = InstancePointCloud()(*inputs)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_instance_points_without_rois_and_without_points(dev):
    from disprcnn_amd.modeling.pointcloud import InstancePointCloud
    from disprcnn_amd.structures.bounding_box import BoxList
    left, right, calibs = _golden_inputs(dev)
    e = BoxList(torch.zeros(0, 4, device=dev), left[0].size)
    e.add_field("disparity", torch.zeros(0, 224, 224, device=dev))
    e.add_field("mask", torch.zeros(0, 1, 28, 28, device=dev))
    pts, mean, rot = InstancePointCloud()([e], [BoxList(torch.zeros(0, 4, device=dev), e.size)], calibs[:1])
    assert tuple(pts.shape) == (0, 768, 3) and tuple(mean.shape) == (0, 3) and tuple(rot.shape) == (0,)
    z = left[0][[0]]
    z.bbox = torch.tensor([[100.0, 50.0, 100.0, 90.0]], device=dev)        # zero-width integer box: no pixel, no point
    z.add_field("disparity", left[0].get_field("disparity")[:1])
    z.add_field("mask", left[0].get_field("mask")[:1])
    with pytest.raises(EOFError, match="mask is nonvalid"):
        InstancePointCloud()([z], [right[0][[0]]], calibs[:1])


def _cloud(B, N, seed, dup=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, N, 3, generator=g) * torch.tensor([8.0, 3.0, 10.0]) + torch.tensor([-4.0, -1.0, 5.0])
    if dup:
        x[:, N // 2:] = x[:, :N - N // 2]
    return x.contiguous()


# RPN config (configs/kitti/car/vob/rpn.yaml; config/defaults.py:201-208): 16 ROIs x 768 points, SA npoints 768/512/256/64
SA = [(768, (0.1, 0.5), (16, 32)), (512, (0.5, 1.0), (16, 32)), (256, (1.0, 2.0), (16, 32)), (64, (2.0, 4.0), (16, 32))]


def test_fps_ball_query_group_on_the_rpn_shapes(dev):
    from disprcnn_amd.layers import pointnet2 as P
    xyz = _cloud(16, 768, 1)
    cur = xyz
    for npoint, radii, nsamples in SA:
        idx = P.furthest_point_sample(cur.to(dev), npoint).cpu().numpy()
        assert np.array_equal(idx, O.fps(cur.numpy(), npoint))
        new = torch.from_numpy(O.gather(cur.transpose(1, 2).numpy(), idx)).transpose(1, 2).contiguous()
        feats = torch.randn(16, 8, cur.shape[1])
        for r, ns in zip(radii, nsamples):
            bi = P.ball_query(r, ns, cur.to(dev), new.to(dev)).cpu().numpy()
            assert np.array_equal(bi, O.ball_query(r, ns, cur.numpy(), new.numpy()))
            gp = P.grouping_operation(feats.to(dev).contiguous(), torch.from_numpy(bi).to(dev)).cpu().numpy()
            assert np.array_equal(gp, O.group(feats.numpy(), bi))
        cur = new


def test_fps_large_and_with_duplicates(dev):
    from disprcnn_amd.layers import pointnet2 as P
    xyz = _cloud(2, 16384, 2)
    idx = P.furthest_point_sample(xyz.to(dev), 4096).cpu().numpy()
    assert np.array_equal(idx, O.fps(xyz.numpy(), 4096))
    # a cloud with duplicates (ties everywhere): the gathered coordinates must agree
    dup = _cloud(3, 1000, 3, dup=True)
    got = P.furthest_point_sample(dup.to(dev), 300).cpu().numpy()
    ref = O.fps(dup.numpy(), 300)
    assert np.array_equal(O.gather(dup.transpose(1, 2).numpy(), got), O.gather(dup.transpose(1, 2).numpy(), ref))


def test_three_nn_and_interpolate_on_the_fp_shapes(dev):
    from disprcnn_amd.layers import pointnet2 as P
    for B, n, m, c in [(16, 768, 512, 32), (16, 256, 64, 64), (2, 16384, 4096, 16)]:
        unknown, known = _cloud(B, n, 4 + n), _cloud(B, m, 5 + m)
        dist, idx = P.three_nn(unknown.to(dev), known.to(dev))
        d2, ridx = O.three_nn(unknown.numpy(), known.numpy())
        assert np.array_equal(idx.cpu().numpy(), ridx)
        np.testing.assert_allclose(dist.cpu().numpy(), np.sqrt(d2), rtol=1e-6, atol=0)
        w = torch.rand(B, n, 3)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        feats = torch.randn(B, c, m)
        out = P.three_interpolate(feats.to(dev), idx, w.to(dev)).cpu().numpy()
        ref = O.three_interpolate(feats.numpy(), ridx, w.numpy())
        np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-6)


def _grad(fn, src, *args):
    x = src.clone().requires_grad_(True)
    y = fn(x, *args)
    g = torch.Generator().manual_seed(7)
    go = torch.randn(y.shape, generator=g).to(y.device)
    y.backward(go)
    return x.grad.detach().cpu(), go.cpu()


def test_backward_is_deterministic_and_matches_a_float64_scatter(dev):
    from disprcnn_amd.layers import pointnet2 as P
    B, C, N = 4, 24, 768
    feats = torch.randn(B, C, N).to(dev)
    gidx = torch.randint(0, N, (B, 512), dtype=torch.int32)
    gidx[:, :64] = 5                                                     # a heavy source
    bidx = torch.randint(0, N, (B, 256, 32), dtype=torch.int32)
    iidx = torch.randint(0, N, (B, 2048, 3), dtype=torch.int32)
    w = torch.rand(B, 2048, 3).to(dev)
    cases = [(P.gather_operation, (gidx.to(dev),), gidx, None), (P.grouping_operation, (bidx.to(dev),), bidx, None),
             (P.three_interpolate, (iidx.to(dev), w), iidx, w)]
    for fn, args, idx, wt in cases:
        g1, go = _grad(fn, feats, *args)
        g2, _ = _grad(fn, feats, *args)
        assert torch.equal(g1, g2), fn
        ref = O.scatter_grad(go.reshape(B, C, -1).numpy(), idx.numpy(), N, None if wt is None else wt.cpu().numpy())
        np.testing.assert_allclose(g1.double().numpy(), ref, rtol=1e-5, atol=1e-5)


def test_query_and_group_and_group_all(dev):
    from disprcnn_amd.layers import pointnet2 as P
    xyz = _cloud(2, 768, 9).to(dev)
    new = xyz[:, :64].contiguous()
    feats = torch.randn(2, 5, 768, device=dev)
    out = P.QueryAndGroup(1.0, 16)(xyz, new, feats)
    bi = O.ball_query(1.0, 16, xyz.cpu().numpy(), new.cpu().numpy())
    gx = O.group(xyz.transpose(1, 2).contiguous().cpu().numpy(), bi) - new.transpose(1, 2).cpu().numpy()[..., None]
    ref = np.concatenate([gx, O.group(feats.cpu().numpy(), bi)], axis=1)
    assert out.shape == (2, 8, 64, 16) and np.array_equal(out.cpu().numpy(), ref)
    ga = P.GroupAll()(xyz, None, feats)
    assert ga.shape == (2, 8, 1, 768)


def test_pointnet2_cuda_signatures_write_in_place(dev):
    from disprcnn_amd import pointnet2_cuda as pn
    xyz = _cloud(2, 100, 11).to(dev)
    out = torch.empty(2, 10, dtype=torch.int32, device=dev)
    temp = torch.full((2, 100), 1e10, device=dev)
    assert pn.furthest_point_sampling_wrapper(2, 100, 10, xyz, temp, out) == 1
    assert np.array_equal(out.cpu().numpy(), O.fps(xyz.cpu().numpy(), 10))
    assert float(temp.max()) < 1e10
    with pytest.raises(RuntimeError):
        pn.gather_points_wrapper(2, 3, 100, 10, xyz.cpu(), out, torch.empty(2, 3, 10, device=dev))

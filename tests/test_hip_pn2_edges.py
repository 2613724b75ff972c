"""The PointNet++ kernels (disprcnn_amd/pts/pointnet2.hip) at the shapes and values where they can go wrong, against two pins:

  oracle     tests/pn2_oracle.py, our NumPy restatement (fp32 in the kernels' order; fp64 for the backward);
  reference  the reference's own kernels, compiled for gfx950 into oracle/_ref/libpn2_ref.so by oracle/build_pn2_ref.py.  Forward
             results must be bit-identical (both sides build without FP contraction).  Its backward adds with float atomics, so it
             is compared within the fp32 rounding bound of a sum, and both backwards are compared to the fp64 scatter.

The reference kernels do no bounds checks: they only ever see in-range indices.  Out-of-range indices go to our kernels and the
oracle alone.  Where the library was not built, the reference comparisons skip with the reason; the oracle ones still run.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import build_pn2_ref
from tests import pn2_oracle as O

pytestmark = pytest.mark.gpu
AGAINST = ["oracle", "reference"]
U32 = 2.0 ** -24                                  # fp32 unit roundoff


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs cuda:0")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref_lib(dev):
    return build_pn2_ref.load()                   # None if never built; a library that exists but does not load raises here


def _ref(ref_lib):
    if ref_lib is None:
        pytest.skip(f"{build_pn2_ref.LIB} not built: build() compiles it only where the reference's sources exist")
    torch.cuda.synchronize()
    return ref_lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _call(fn, *args):
    assert fn(*args) == 0


# ---- furthest point sampling
FPS_N = [1, 2, 3, 31, 63, 64, 65, 100, 1023, 1024, 1025, 4097, 16383, 16384]


def _fps_clouds(n):
    """Batch row 0: a uniform cloud.  Row 1: an integer grid of 4^3 sites, so most distances tie (and, past 64 points, repeat)."""
    g = torch.Generator().manual_seed(1000 + n)
    a = torch.rand(n, 3, generator=g) * torch.tensor([8.0, 3.0, 10.0])
    b = torch.randint(0, 4, (n, 3), generator=g).float()
    return torch.stack([a, b]).contiguous()


def _ours_fps(xyz, m, dev):
    from disprcnn_amd import pointnet2_cuda as pn
    B, n, _ = xyz.shape
    idx = torch.full((B, m), -5, dtype=torch.int32, device=dev)
    temp = torch.full((B, n), 1e10, device=dev)
    pn.furthest_point_sampling_wrapper(B, n, m, xyz.to(dev), temp, idx)
    return idx.cpu().numpy(), temp.cpu().numpy()


@pytest.mark.parametrize("against", AGAINST)
@pytest.mark.parametrize("n", FPS_N)
def test_fps_edges_and_the_temp_left_behind(dev, ref_lib, against, n):
    xyz = _fps_clouds(n)
    for m in sorted({1, 2, n, n + 7}):
        idx, temp = _ours_fps(xyz, m, dev)
        if against == "oracle":
            want, wtemp = O.fps(xyz.numpy(), m, return_temp=True)
        else:
            lib = _ref(ref_lib)
            xd = xyz.to(dev)
            wi = torch.zeros(2, m, dtype=torch.int32, device=dev)
            wt = torch.full((2, n), 1e10, device=dev)
            _call(lib.pn2_ref_furthest_point_sampling, 2, n, m, _p(xd), _p(wt), _p(wi))
            want, wtemp = wi.cpu().numpy(), wt.cpu().numpy()
        assert np.array_equal(idx, want), (m, np.flatnonzero(idx != want)[:8])
        assert np.array_equal(temp, wtemp), m
    if n > 1:
        assert (idx[:, n:] == 0).all()            # m > n: every distance is 0, the tie order's first point is point 0


def test_fps_refuses_more_than_16384_points(dev):
    from disprcnn_amd.layers import pointnet2 as P
    with pytest.raises(RuntimeError, match="status -2"):
        P.furthest_point_sample(torch.zeros(1, 16385, 3, device=dev), 4)


# ---- ball query
BQ_N = [1, 63, 65, 1000]
BQ_NSAMPLE = [1, 63, 64, 65, 128, 200]


def _bq_inputs(n):
    """0.5-grid points and centres: every squared distance is exact, and many points sit exactly on the spheres of radius 1 and 2.
    Off-grid centres, and far centres whose neighbourhood is empty."""
    g = torch.Generator().manual_seed(2000 + n)
    xyz = torch.randint(-4, 5, (2, n, 3), generator=g).float() * 0.5
    on = torch.randint(-4, 5, (2, 160, 3), generator=g).float() * 0.5
    off = torch.rand(2, 64, 3, generator=g) * 4 - 2
    far = torch.rand(2, 32, 3, generator=g) + 100
    return xyz.contiguous(), torch.cat([on, off, far], 1).contiguous()


@pytest.mark.parametrize("against", AGAINST)
@pytest.mark.parametrize("nsample", BQ_NSAMPLE)
@pytest.mark.parametrize("n", BQ_N)
def test_ball_query_edges(dev, ref_lib, against, n, nsample):
    from disprcnn_amd.layers import pointnet2 as P
    xyz, new = _bq_inputs(n)
    for radius in (0.0, 1.0, 2.0):
        got = P.ball_query(radius, nsample, xyz.to(dev), new.to(dev)).cpu().numpy()
        if against == "oracle":
            want = O.ball_query(radius, nsample, xyz.numpy(), new.numpy())
        else:
            lib = _ref(ref_lib)
            nd, xd = new.to(dev), xyz.to(dev)                  # held: a pointer must not outlive its tensor
            w = torch.zeros(2, new.shape[1], nsample, dtype=torch.int32, device=dev)
            _call(lib.pn2_ref_ball_query, 2, n, new.shape[1], radius, nsample, _p(nd), _p(xd), _p(w))
            want = w.cpu().numpy()
        assert np.array_equal(got, want), (radius, np.argwhere(got != want)[:4])
        assert (got[:, -32:] == 0).all()                     # the far centres: empty neighbourhood, the row stays zero
        if radius == 0.0:
            assert (got == 0).all()


# ---- three_nn
NN_M = [1, 2, 3, 4, 1023, 1024, 1025, 2049]
NN_N = [1, 255, 257]


def _nn_inputs(n, m):
    """Known points on a 0.5 grid with the second half a copy of the first: exact distance ties between duplicates and across
    grid sites.  Unknown points: half on the grid, half off it."""
    g = torch.Generator().manual_seed(3000 + 7 * n + m)
    known = torch.randint(-6, 7, (2, m, 3), generator=g).float() * 0.5
    known[:, m // 2:] = known[:, :m - m // 2].clone()
    unknown = torch.randint(-6, 7, (2, n, 3), generator=g).float() * 0.5
    unknown[:, n // 2:] = torch.rand(2, n - n // 2, 3, generator=g) * 6 - 3
    return unknown.contiguous(), known.contiguous()


@pytest.mark.parametrize("against", AGAINST)
@pytest.mark.parametrize("m", NN_M)
@pytest.mark.parametrize("n", NN_N)
def test_three_nn_edges(dev, ref_lib, against, n, m):
    from disprcnn_amd import pointnet2_cuda as pn
    unknown, known = _nn_inputs(n, m)
    d2 = torch.empty(2, n, 3, device=dev)
    idx = torch.empty(2, n, 3, dtype=torch.int32, device=dev)
    pn.three_nn_wrapper(2, n, m, unknown.to(dev), known.to(dev), d2, idx)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    if against == "oracle":
        wd, wi = O.three_nn(unknown.numpy(), known.numpy())
    else:
        lib = _ref(ref_lib)
        ud, kd = unknown.to(dev), known.to(dev)
        wd_t = torch.empty(2, n, 3, device=dev)
        wi_t = torch.empty(2, n, 3, dtype=torch.int32, device=dev)
        _call(lib.pn2_ref_three_nn, 2, n, m, _p(ud), _p(kd), _p(wd_t), _p(wi_t))
        wd, wi = wd_t.cpu().numpy(), wi_t.cpu().numpy()
    assert np.array_equal(idx, wi), np.argwhere(idx != wi)[:4]
    assert np.array_equal(d2.view(np.uint32), wd.view(np.uint32))                 # bit for bit, inf where m < 3
    if m < 3:
        assert np.isinf(d2[..., m:]).all() and (idx[..., m:] == 0).all()


# ---- gather / group / three_interpolate past the grid-stride limit (65536 blocks x 256 threads), forward and backward.
# Each launch sizes its grid by its own total: the forward kernels by the output (B*C*K), csr_scatter_add by the source (B*C*N) and
# csr_bounds by the index entries (B*E).  Every case puts the forward past the limit; `past` names the backward totals it also puts
# there, asserted below.
BIG = 65536 * 256


def _big_case(kind):
    """(features [B,C,N], idx, weight or None, backward totals past the limit)."""
    g = torch.Generator().manual_seed({"gather": 41, "group": 42, "group_long": 44, "interpolate": 43}[kind])
    if kind == "gather":                                                   # B*C*N = 17.0 M: csr_scatter_add's second pass
        B, C, N, M = 2, 1024, 8300, 8209
        idx = torch.randint(0, N, (B, M), generator=g, dtype=torch.int32)
        idx[:, :300] = 17                                                  # a heavy source
        return torch.randn(B, C, N, generator=g), idx, None, ("scatter",)
    if kind == "group":                                                    # the RPN's SA2 grouping: 16 ROIs x 96 ch x 512 x 32
        B, C, N, M, S = 16, 96, 512, 512, 32
        return torch.randn(B, C, N, generator=g), torch.randint(0, N, (B, M, S), generator=g, dtype=torch.int32), None, ()
    if kind == "group_long":                                               # B*E = 17.2 M index entries: csr_bounds' second pass
        B, C, N, M, S = 4, 1, 4096, 4200, 1024
        return torch.randn(B, C, N, generator=g), torch.randint(0, N, (B, M, S), generator=g, dtype=torch.int32), None, ("bounds",)
    B, C, M, N = 16, 128, 8200, 8300                                       # B*C*M = 16.8 M: the weighted scatter's second pass
    w = torch.rand(B, N, 3, generator=g)
    idx = torch.randint(0, M, (B, N, 3), generator=g, dtype=torch.int32)
    return torch.randn(B, C, M, generator=g), idx, w / w.sum(2, keepdim=True), ("scatter",)


def _ours_fwd_bwd(kind, feats, idx, w, go_seed, dev):
    from disprcnn_amd.layers import pointnet2 as P
    x = feats.to(dev).requires_grad_(True)
    if kind == "gather":
        y = P.gather_operation(x, idx.to(dev))
    elif kind.startswith("group"):
        y = P.grouping_operation(x, idx.to(dev))
    else:
        y = P.three_interpolate(x, idx.to(dev), w.to(dev))
    go = torch.randn(y.shape, generator=torch.Generator().manual_seed(go_seed))
    y.backward(go.to(dev))
    return y.detach(), x.grad.detach(), go


@pytest.mark.parametrize("against", AGAINST)
@pytest.mark.parametrize("kind", ["gather", "group", "group_long", "interpolate"])
def test_gather_group_interpolate_past_the_grid_stride_limit(dev, ref_lib, against, kind):
    feats, idx, w, past = _big_case(kind)
    B, C, N = feats.shape
    y, grad, go = _ours_fwd_bwd(kind, feats, idx, w, 7, dev)
    assert y.numel() > BIG
    assert ("scatter" not in past or B * C * N > BIG) and ("bounds" not in past or idx.numel() > BIG)
    grad = grad.cpu().numpy().astype(np.float64)
    ref64 = O.scatter_grad(go.reshape(B, C, -1).numpy(), idx.numpy(), N, None if w is None else w.numpy())
    # |fl(sum of k terms) - sum| <= k u sum|terms| (one more u for the weight product): the fp32 bound for every element
    absg = O.scatter_grad(np.abs(go.reshape(B, C, -1).numpy()), idx.numpy(), N, None if w is None else w.numpy())
    k = np.stack([np.bincount(idx[b].reshape(-1).numpy(), minlength=N) for b in range(B)])[:, None, :]
    bound = (k + 1) * U32 * absg
    assert (np.abs(grad - ref64) <= bound).all()
    if against == "oracle":
        if kind == "gather":
            want = O.gather(feats.numpy(), idx.numpy())
        elif kind.startswith("group"):
            want = O.group(feats.numpy(), idx.numpy())
        else:
            want = O.three_interpolate(feats.numpy(), idx.numpy(), w.numpy())
        assert np.array_equal(y.cpu().numpy(), want)
        return
    lib = _ref(ref_lib)
    fd, idd, god = feats.to(dev), idx.to(dev), go.to(dev).contiguous()
    out = torch.empty(y.shape, device=dev)
    rgrad = torch.zeros(B, C, N, device=dev)
    if kind == "gather":
        M = idx.shape[1]
        _call(lib.pn2_ref_gather_points, B, C, N, M, _p(fd), _p(idd), _p(out))
        _call(lib.pn2_ref_gather_points_grad, B, C, N, M, _p(god), _p(idd), _p(rgrad))
    elif kind.startswith("group"):
        M, S = idx.shape[1:]
        _call(lib.pn2_ref_group_points, B, C, N, M, S, _p(fd), _p(idd), _p(out))
        _call(lib.pn2_ref_group_points_grad, B, C, N, M, S, _p(god), _p(idd), _p(rgrad))
    else:
        n = idx.shape[1]
        wd = w.to(dev).contiguous()
        _call(lib.pn2_ref_three_interpolate, B, C, N, n, _p(fd), _p(idd), _p(wd), _p(out))
        _call(lib.pn2_ref_three_interpolate_grad, B, C, n, N, _p(god), _p(idd), _p(wd), _p(rgrad))
    assert torch.equal(out, y)
    rgrad = rgrad.cpu().numpy().astype(np.float64)
    assert (np.abs(rgrad - ref64) <= bound).all()
    assert (np.abs(rgrad - grad) <= 2 * bound).all()


# ---- the API's own rules, beyond the reference: out-of-range indices, and backward adding into a non-zero gradient
def test_out_of_range_indices_read_zero_and_are_skipped_in_backward(dev):
    from disprcnn_amd.layers import pointnet2 as P
    B, C, N = 2, 5, 40
    bad = torch.tensor([-1, N, 2 ** 31 - 1], dtype=torch.int32)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, C, N, generator=g)
    gi = torch.randint(0, N, (B, 30), generator=g, dtype=torch.int32)
    gi[:, ::4] = bad.repeat(3)[:8]
    bi = torch.randint(0, N, (B, 6, 7), generator=g, dtype=torch.int32)
    bi[:, :, 2] = bad[torch.arange(6) % 3]
    ii = torch.randint(0, N, (B, 50, 3), generator=g, dtype=torch.int32)
    ii[:, ::5, 1] = bad[torch.arange(10) % 3]
    w = torch.rand(B, 50, 3, generator=g)
    for op, idx, wt, fwd in [(P.gather_operation, gi, None, O.gather), (P.grouping_operation, bi, None, O.group),
                             (P.three_interpolate, ii, w, O.three_interpolate)]:
        x = feats.to(dev).requires_grad_(True)
        y = op(x, idx.to(dev)) if wt is None else op(x, idx.to(dev), wt.to(dev))
        want = fwd(feats.numpy(), idx.numpy()) if wt is None else fwd(feats.numpy(), idx.numpy(), wt.numpy())
        np.testing.assert_allclose(y.detach().cpu().numpy(), want, rtol=0, atol=0)
        go = torch.randn(y.shape, generator=g)
        y.backward(go.to(dev))
        ref = O.scatter_grad(go.reshape(B, C, -1).numpy(), idx.numpy(), N, None if wt is None else wt.numpy())
        np.testing.assert_allclose(x.grad.cpu().double().numpy(), ref, rtol=1e-6, atol=1e-6)


def test_backward_wrappers_add_into_a_nonzero_gradient(dev):
    from disprcnn_amd import pointnet2_cuda as pn
    B, C, N = 2, 6, 300
    g = torch.Generator().manual_seed(6)
    init = torch.randn(B, C, N, generator=g)
    gi = torch.randint(0, N, (B, 200), generator=g, dtype=torch.int32)
    bi = torch.randint(0, N, (B, 40, 9), generator=g, dtype=torch.int32)
    ii = torch.randint(0, N, (B, 700, 3), generator=g, dtype=torch.int32)
    w = torch.rand(B, 700, 3, generator=g)
    cases = [(gi, None, lambda go, gp: pn.gather_points_grad_wrapper(B, C, N, 200, go, gi.to(dev), gp)),
             (bi, None, lambda go, gp: pn.group_points_grad_wrapper(B, C, N, 40, 9, go, bi.to(dev), gp)),
             (ii, w, lambda go, gp: pn.three_interpolate_grad_wrapper(B, C, 700, N, go, ii.to(dev), w.to(dev), gp))]
    for idx, wt, call in cases:
        go = torch.randn(B, C, idx[0].numel() // (1 if wt is None else 3), generator=g)
        gp = init.to(dev)
        call(go.to(dev), gp)
        ref = init.double().numpy() + O.scatter_grad(go.numpy(), idx.numpy(), N, None if wt is None else wt.numpy())
        np.testing.assert_allclose(gp.cpu().double().numpy(), ref, rtol=1e-5, atol=1e-5)
        assert not np.allclose(gp.cpu().numpy(), init.numpy())

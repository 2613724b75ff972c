"""`pointnet2_cuda` -- the names of PointRCNN's compiled PointNet++ extension (pointnet2_lib/pointnet2/src/pointnet2_api.cpp),
served by libdisprcnn_pts.so.

The reference's pointnet2_utils.py binds its kernels with `import pointnet2_cuda as pointnet2` and calls the nine wrappers below with
the positional signatures of src/{sampling,ball_query,group_points,interpolate}.cpp: sizes first, then tensors, the outputs written in
place.  This module keeps exactly those signatures, so that file runs unchanged with ``sys.modules['pointnet2_cuda']`` pointed here
(the same story as disprcnn_amd/_C.py).  Differences by design:
  - every tensor is checked (device, dtype, contiguity, size) before a kernel sees it; an index outside its source reads as 0;
  - the three backward wrappers add into the gradient deterministically (a per-source CSR of the index tensor, no float atomics):
    the reference's atomicAdd order, and so its rounding, varies from run to run; here the gradient is bit-identical.
GPU tensors only: there is no CPU kernel and no fallback.
"""
import math

import torch

from . import engine as E
from .pts import _lib


def opt_n_threads(work_size):
    """cuda_utils.h: the block size of the reference's sampling kernel, which fixes how its argmax breaks ties."""
    pow_2 = int(math.log(float(work_size)) / math.log(2.0))
    return max(min(1 << pow_2, 1024), 1)


def _check(t, what, dtype, numel):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"pointnet2_cuda: {what} must be a CUDA/HIP tensor (no CPU kernel)")
    if t.dtype != dtype:
        raise RuntimeError(f"pointnet2_cuda: {what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"pointnet2_cuda: {what} must be contiguous")
    if t.numel() != numel:
        raise RuntimeError(f"pointnet2_cuda: {what} has {t.numel()} elements, expected {numel}")
    return E._ptr(t)


def _f(t, what, numel):
    return _check(t, what, torch.float32, numel)


def _i(t, what, numel):
    return _check(t, what, torch.int32, numel)


def _stream(t):
    return E._stream_ptr(t.device)


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    """sampling.cpp: points (B,N,3), temp (B,N) filled with 1e10, idx (B,M) <- indices."""
    if b > 0 and m > 0:
        st = _lib.lib().drc_pn2_furthest_point_sampling(b, n, m, _f(points_tensor, "points", b * n * 3), _f(temp_tensor, "temp", b * n),
                                                        _i(idx_tensor, "idx", b * m), opt_n_threads(max(n, 1)), _stream(points_tensor))
        _lib.check(st, "drc_pn2_furthest_point_sampling")
    return 1


def gather_points_wrapper(b, c, n, npoints, points_tensor, idx_tensor, out_tensor):
    """sampling.cpp: points (B,C,N), idx (B,npoints) -> out (B,C,npoints)."""
    st = _lib.lib().drc_pn2_gather_points(b, c, n, npoints, _f(points_tensor, "points", b * c * n), _i(idx_tensor, "idx", b * npoints),
                                          _f(out_tensor, "out", b * c * npoints), _stream(points_tensor))
    _lib.check(st, "drc_pn2_gather_points")
    return 1


def _csr(idx2d, n):
    """Per-source CSR of an index tensor [B,E]: the stable sort's permutation and the [start, end) run of every source."""
    keys, perm = torch.sort(idx2d, dim=1, stable=True)
    keys, perm = keys.contiguous(), perm.to(torch.int32).contiguous()
    B, Ent = idx2d.shape
    start = torch.zeros(B, n, dtype=torch.int32, device=idx2d.device)
    end = torch.zeros_like(start)
    st = _lib.lib().drc_pn2_csr_bounds(B, Ent, n, E._ptr(keys), E._ptr(start), E._ptr(end), _stream(idx2d))
    _lib.check(st, "drc_pn2_csr_bounds")
    return perm, start, end


def _scatter_add(b, c, n, k, ent, per_col, grad_out, idx, weight, grad_points):
    perm, start, end = _csr(idx.view(b, ent), n)
    st = _lib.lib().drc_pn2_csr_scatter_add(b, c, n, k, ent, per_col, E._ptr(grad_out), E._ptr(perm), E._ptr(start), E._ptr(end),
                                            E._ptr(weight), E._ptr(grad_points), _stream(grad_out))
    _lib.check(st, "drc_pn2_csr_scatter_add")


def gather_points_grad_wrapper(b, c, n, npoints, grad_out_tensor, idx_tensor, grad_points_tensor):
    """sampling.cpp: grad_out (B,C,npoints), idx (B,npoints) -> grad_points (B,C,N) += scatter."""
    _f(grad_out_tensor, "grad_out", b * c * npoints)
    _i(idx_tensor, "idx", b * npoints)
    _f(grad_points_tensor, "grad_points", b * c * n)
    if b * c * n:
        _scatter_add(b, c, n, npoints, npoints, 1, grad_out_tensor, idx_tensor, None, grad_points_tensor)
    return 1


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz_tensor, xyz_tensor, idx_tensor):
    """ball_query.cpp: new_xyz (B,M,3), xyz (B,N,3) -> idx (B,M,nsample), caller-zeroed."""
    st = _lib.lib().drc_pn2_ball_query(b, n, m, float(radius), nsample, _f(new_xyz_tensor, "new_xyz", b * m * 3),
                                       _f(xyz_tensor, "xyz", b * n * 3), _i(idx_tensor, "idx", b * m * nsample), _stream(xyz_tensor))
    _lib.check(st, "drc_pn2_ball_query")
    return 1


def group_points_wrapper(b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor):
    """group_points.cpp: points (B,C,N), idx (B,npoints,nsample) -> out (B,C,npoints,nsample)."""
    st = _lib.lib().drc_pn2_group_points(b, c, n, npoints, nsample, _f(points_tensor, "points", b * c * n),
                                         _i(idx_tensor, "idx", b * npoints * nsample), _f(out_tensor, "out", b * c * npoints * nsample),
                                         _stream(points_tensor))
    _lib.check(st, "drc_pn2_group_points")
    return 1


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out_tensor, idx_tensor, grad_points_tensor):
    """group_points.cpp: grad_out (B,C,npoints,nsample), idx (B,npoints,nsample) -> grad_points (B,C,N) += scatter."""
    k = npoints * nsample
    _f(grad_out_tensor, "grad_out", b * c * k)
    _i(idx_tensor, "idx", b * k)
    _f(grad_points_tensor, "grad_points", b * c * n)
    if b * c * n:
        _scatter_add(b, c, n, k, k, 1, grad_out_tensor, idx_tensor, None, grad_points_tensor)
    return 1


def three_nn_wrapper(b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor):
    """interpolate.cpp: unknown (B,N,3), known (B,M,3) -> dist2, idx (B,N,3)."""
    st = _lib.lib().drc_pn2_three_nn(b, n, m, _f(unknown_tensor, "unknown", b * n * 3), _f(known_tensor, "known", b * m * 3),
                                     _f(dist2_tensor, "dist2", b * n * 3), _i(idx_tensor, "idx", b * n * 3), _stream(unknown_tensor))
    _lib.check(st, "drc_pn2_three_nn")


def three_interpolate_wrapper(b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor):
    """interpolate.cpp: points (B,C,M), idx / weight (B,N,3) -> out (B,C,N)."""
    st = _lib.lib().drc_pn2_three_interpolate(b, c, m, n, _f(points_tensor, "points", b * c * m), _i(idx_tensor, "idx", b * n * 3),
                                              _f(weight_tensor, "weight", b * n * 3), _f(out_tensor, "out", b * c * n),
                                              _stream(points_tensor))
    _lib.check(st, "drc_pn2_three_interpolate")


def three_interpolate_grad_wrapper(b, c, n, m, grad_out_tensor, idx_tensor, weight_tensor, grad_points_tensor):
    """interpolate.cpp: grad_out (B,C,N), idx / weight (B,N,3) -> grad_points (B,C,M) += scatter."""
    _f(grad_out_tensor, "grad_out", b * c * n)
    _i(idx_tensor, "idx", b * n * 3)
    _f(weight_tensor, "weight", b * n * 3)
    _f(grad_points_tensor, "grad_points", b * c * m)
    if b * c * m:
        _scatter_add(b, c, m, n, n * 3, 3, grad_out_tensor, idx_tensor, weight_tensor, grad_points_tensor)

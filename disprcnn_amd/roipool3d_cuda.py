"""`roipool3d_cuda` -- the names of PointRCNN's compiled roipool3d extension (point_rcnn/lib/utils/roipool3d/src/roipool3d.cpp), served
by libdisprcnn_pts.so.

The reference's roipool3d_utils.py calls `roipool3d_cuda.forward(pts, boxes3d, pts_feature, pooled_features, pooled_empty_flag)` with
caller-zeroed outputs; the sizes come from the tensors as in roipool3d.cpp (B, N from pts; M from boxes3d; C from pts_feature; S from
pooled_features).  This module keeps that signature, so the file runs unchanged with ``sys.modules['roipool3d_cuda']`` pointed here.
Every tensor is checked before the kernel sees it.  `forward_slow` (the reference's one-thread-per-box kernel) computes the same result
and is served by the same kernel.  The CPU entry points have no counterpart here and raise NotImplementedError.
"""
import torch

from . import engine as E
from .pts import _lib


def _check(t, what, dtype, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"roipool3d_cuda: {what} must be a CUDA/HIP tensor (no CPU kernel)")
    if t.dtype != dtype:
        raise RuntimeError(f"roipool3d_cuda: {what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"roipool3d_cuda: {what} must be contiguous")
    if t.dim() != len(dims) or any(d is not None and s != d for s, d in zip(t.shape, dims)):
        want = "x".join("?" if d is None else str(d) for d in dims)
        raise RuntimeError(f"roipool3d_cuda: {what} has shape {tuple(t.shape)}, expected [{want}]")
    return E._ptr(t)


def max_sampled_pt_num():
    """The largest S the kernel holds in LDS: a larger sampled_pt_num is refused (RuntimeError)."""
    return _lib.lib().drc_box3d_max_pool_samples()


def forward(pts, boxes3d, pts_feature, pooled_features, pooled_empty_flag):
    """roipool3d.cpp: pts (B,N,3), boxes3d (B,M,7), pts_feature (B,N,C) -> pooled_features (B,M,S,3+C), pooled_empty_flag (B,M) int32."""
    if not isinstance(pts, torch.Tensor) or pts.dim() != 3 or not isinstance(boxes3d, torch.Tensor) or boxes3d.dim() != 3 or \
            not isinstance(pts_feature, torch.Tensor) or pts_feature.dim() != 3 or \
            not isinstance(pooled_features, torch.Tensor) or pooled_features.dim() != 4:
        raise RuntimeError("roipool3d_cuda.forward expects pts (B,N,3), boxes3d (B,M,7), pts_feature (B,N,C), pooled_features (B,M,S,3+C)")
    b, n, m, c, s = pts.shape[0], pts.shape[1], boxes3d.shape[1], pts_feature.shape[2], pooled_features.shape[2]
    args = (_check(pts, "pts", torch.float32, (b, n, 3)), _check(boxes3d, "boxes3d", torch.float32, (b, m, 7)),
            _check(pts_feature, "pts_feature", torch.float32, (b, n, c)),
            _check(pooled_features, "pooled_features", torch.float32, (b, m, s, 3 + c)),
            _check(pooled_empty_flag, "pooled_empty_flag", torch.int32, (b, m)))
    if any(t.device != pts.device for t in (boxes3d, pts_feature, pooled_features, pooled_empty_flag)):
        raise RuntimeError("roipool3d_cuda.forward: all tensors must be on one device")
    st = _lib.lib().drc_roipool3d_fwd(b, n, m, c, s, args[0], args[1], args[2], args[3], args[4], E._stream_ptr(pts.device))
    if st < 0 and s > max_sampled_pt_num():
        raise RuntimeError(f"roipool3d_cuda.forward: sampled_pt_num {s} exceeds the kernel's LDS limit of {max_sampled_pt_num()}")
    _lib.check(st, "drc_roipool3d_fwd")
    return 1


forward_slow = forward


def pts_in_boxes3d(pts, boxes3d, pts_flag):
    """The device counterpart of pts_in_boxes3d_cpu, batched: pts (B,N,3), boxes3d (B,M,7) -> pts_flag (B,M,N) bool / uint8."""
    b, n, m = pts.shape[0], pts.shape[1], boxes3d.shape[1]
    if pts_flag.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"roipool3d_cuda: pts_flag must be bool or uint8, got {pts_flag.dtype}")
    p = _check(pts, "pts", torch.float32, (b, n, 3))
    bx = _check(boxes3d, "boxes3d", torch.float32, (b, m, 7))
    f = _check(pts_flag, "pts_flag", pts_flag.dtype, (b, m, n))
    st = _lib.lib().drc_pts_in_boxes3d(b, n, m, p, bx, f, E._stream_ptr(pts.device))
    _lib.check(st, "drc_pts_in_boxes3d")
    return 1


def _cpu_only(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"roipool3d_cuda.{name}: the reference's CPU kernel has no counterpart on MI355X; "
                                  "use disprcnn_amd.layers.roipool3d (roipool3d_gpu / pts_in_boxes3d_gpu) on device tensors")
    fn.__name__ = name
    return fn


pts_in_boxes3d_cpu = _cpu_only("pts_in_boxes3d_cpu")
roipool3d_cpu = _cpu_only("roipool3d_cpu")

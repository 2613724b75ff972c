"""PointRCNN's RPN proposal layer (point_rcnn/lib/rpn/proposal_layer.py, utils/bbox_transform.py:decode_bbox_target) on HIP.

    decode_rpn_boxes(xyz, reg, mean_size, loc_scope, loc_bin_size, num_head_bin, xz_fine) -> (boxes7 [B,N,7], bev5 [B,N,5])
    propose(scores, boxes7, bev5, pre_nms_top_n, post_nms_top_n, nms_thresh)               -> (rois [B,post,7], roi_scores [B,post])
    points_depth(xyz)                                                                      -> |p| [B,N]
    rpn_to_camera(xyz, boxes, mean, rot)                                                   -> (xyz_cam [B,N,3], depth [B,N], boxes_cam [B,M,7])

decode is one kernel (bin argmax, residuals, the angle wrap, y moved to the box bottom, and the BEV form for the NMS), fp32 in the
reference's expression order, so equal inputs give the reference's bits.  The reference's constants are Python doubles that meet the
fp32 tensor one at a time; they are computed here in double the same way and rounded to fp32 at the call.

propose is score_based_proposal for all clouds at once: a stable descending sort (ties keep index order, the rule nms_gpu_batched
documents), the cut to `pre`, ONE batched rotated NMS stopped at `post` kept boxes, and zero padding.  No host sync.
"""
import ctypes as C
import math

import torch

from .. import engine as E
from ..pts import _lib
from .iou3d import nms_gpu_batched


def decode_rpn_boxes(xyz, reg, mean_size, loc_scope, loc_bin_size, num_head_bin, xz_fine=False):
    what = "decode_rpn_boxes"
    E.require_gpu(xyz, what)
    E.require_gpu(reg, what)
    if xyz.dim() != 3 or xyz.shape[2] != 3 or reg.dim() != 3 or reg.shape[:2] != xyz.shape[:2]:
        raise RuntimeError(f"{what}: xyz [B,N,3] and reg [B,N,R] expected, got {tuple(xyz.shape)} and {tuple(reg.shape)}")
    B, N, R = reg.shape
    per_loc_bin_num = int(loc_scope / loc_bin_size) * 2
    num_head_bin = int(num_head_bin)
    want = per_loc_bin_num * (4 if xz_fine else 2) + 1 + 2 * num_head_bin + 3
    if R != want:
        raise RuntimeError(f"{what}: reg has {R} channels, the bin layout needs {want}")
    h, w, l = (float(v) for v in mean_size)
    angle_per_class = (2 * math.pi) / num_head_bin
    boxes = torch.empty((B, N, 7), dtype=torch.float32, device=xyz.device)
    bev = torch.empty((B, N, 5), dtype=torch.float32, device=xyz.device)
    if B * N:
        f = C.c_float
        st = _lib.lib().drc_rpn_decode_proposals(B * N, R, E._ptr(xyz.contiguous()), E._ptr(reg.contiguous()), per_loc_bin_num, num_head_bin,
                                                 1 if xz_fine else 0, f(loc_bin_size), f(loc_bin_size / 2), f(loc_scope), f(angle_per_class),
                                                 f(angle_per_class / 2), f(2 * math.pi), f(math.pi), f(h), f(w), f(l), E._ptr(boxes),
                                                 E._ptr(bev), E._stream_ptr(xyz.device))
        _lib.check(st, "drc_rpn_decode_proposals")
    return boxes, bev


def points_depth(xyz):
    """xyz (B,N,3) -> (B,N) = |p|, the RPN's pts_depth.  One kernel with a fixed rounding (squares accumulated by fused multiply-adds in
    x, y, z order, as torch's CPU reduction does), so the result does not depend on how a torch build reduces on the device."""
    E.require_gpu(xyz, "points_depth")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise RuntimeError(f"points_depth: xyz [B,N,3] expected, got {tuple(xyz.shape)}")
    out = torch.empty(xyz.shape[:2], dtype=torch.float32, device=xyz.device)
    if out.numel():
        _lib.check(_lib.lib().drc_rpn_points_depth(out.numel(), E._ptr(xyz.contiguous()), E._ptr(out), E._stream_ptr(xyz.device)),
                   "drc_rpn_points_depth")
    return out


def rpn_to_camera(xyz, boxes, mean, rot):
    """The RPN's clouds xyz (B,N,3) and proposals boxes (B,M,7) 'xyzhwl_ry', both in the centred, rotated frame of their instance
    (mean (B,3) fp32, rot (B) fp64), -> (xyz_cam (B,N,3), depth (B,N), boxes_cam (B,M,7)) in the camera frame.  One kernel: the points are
    un-centred and rotated back, depth is points_depth of the result (same bits), the boxes go through their corners as Box3DList does."""
    what = "rpn_to_camera"
    if not (xyz.is_cuda and boxes.is_cuda and mean.is_cuda and rot.is_cuda):
        raise RuntimeError(f"{what}: expected CUDA/HIP tensors on an MI355X; the HIP path has no CPU fallback")
    B = mean.shape[0]
    if xyz.dim() != 3 or xyz.shape[2] != 3 or boxes.dim() != 3 or boxes.shape[2] != 7 or xyz.shape[0] != B or boxes.shape[0] != B or \
            mean.shape != (B, 3) or rot.shape != (B,):
        raise RuntimeError(f"{what}: xyz [B,N,3], boxes [B,M,7], mean [B,3], rot [B] expected, got {tuple(xyz.shape)}, {tuple(boxes.shape)}, "
                           f"{tuple(mean.shape)}, {tuple(rot.shape)}")
    if xyz.dtype != torch.float32 or boxes.dtype != torch.float32 or mean.dtype != torch.float32 or rot.dtype != torch.float64:
        raise RuntimeError(f"{what}: fp32 xyz, boxes and mean and an fp64 rot expected")
    N, M = xyz.shape[1], boxes.shape[1]
    dev = xyz.device
    xyz_cam = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((B, N), dtype=torch.float32, device=dev)
    boxes_cam = torch.empty((B, M, 7), dtype=torch.float32, device=dev)
    if B and (N or M):
        st = _lib.lib().drc_rpn_to_camera_fwd(B, N, M, E._ptr(xyz.contiguous()), E._ptr(boxes.contiguous()), E._ptr(mean.contiguous()),
                                              E._ptr(rot.contiguous()), E._ptr(xyz_cam), E._ptr(depth), E._ptr(boxes_cam), E._stream_ptr(dev))
        _lib.check(st, "drc_rpn_to_camera_fwd")
    return xyz_cam, depth, boxes_cam


def propose(scores, boxes7, bev5, pre_nms_top_n, post_nms_top_n, nms_thresh):
    what = "propose"
    E.require_gpu(scores, what)
    E.require_gpu(boxes7, what)
    E.require_gpu(bev5, what)
    B, N = scores.shape
    if boxes7.shape != (B, N, 7) or bev5.shape != (B, N, 5):
        raise RuntimeError(f"{what}: scores [B,N], boxes7 [B,N,7], bev5 [B,N,5] expected, got {tuple(scores.shape)}, "
                           f"{tuple(boxes7.shape)}, {tuple(bev5.shape)}")
    pre, post = min(int(pre_nms_top_n), N), int(post_nms_top_n)
    rois = torch.zeros((B, post, 7), dtype=torch.float32, device=scores.device)
    roi_scores = torch.zeros((B, post), dtype=torch.float32, device=scores.device)
    if B == 0 or pre <= 0 or post <= 0:
        return rois, roi_scores
    top_scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
    top_scores, order = top_scores[:, :pre].contiguous(), order[:, :pre]
    top_boxes = torch.gather(boxes7, 1, order.unsqueeze(2).expand(B, pre, 7))
    top_bev = torch.gather(bev5, 1, order.unsqueeze(2).expand(B, pre, 5)).contiguous()
    counts = torch.full((B,), pre, dtype=torch.int32, device=scores.device)
    keep, _ = nms_gpu_batched(top_bev, top_scores, counts, float(nms_thresh), max_keep=post)      # (B, min(post, pre)), -1 padded
    K = keep.shape[1]
    valid = keep >= 0
    pos = keep.clamp(min=0)
    rois[:, :K] = torch.where(valid.unsqueeze(2), torch.gather(top_boxes, 1, pos.unsqueeze(2).expand(B, K, 7)), rois[:, :K])
    roi_scores[:, :K] = torch.where(valid, torch.gather(top_scores, 1, pos), roi_scores[:, :K])
    return rois, roi_scores

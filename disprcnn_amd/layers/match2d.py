"""PointRCNN's 2D matching and the way into the cloud frame on HIP.

    match_targets(boxes, span, gt, gt_rows, high, low, matched=None) -> (matched [R] int64, rows [R,row])
    camera_to_rpn(xyz, mean, rot, scale=1.0, flip=False)             -> xyz in the clouds' frame [B,K,3]

match_targets is PointRCNN.match_targets_to_proposals (point_rcnn.py:87-95) for all images in one launch: boxlist_iou of each left
proposal with the ground truths of its own image, the max (ties to the lowest index), Matcher(high, low) without low-quality matches,
and the matched target's row taken at the index clamped at zero.  `matched` may be a caller's int64 buffer (PointRCNN passes the tail
of the buffer its point counts are read through, so the indices reach the host in that one copy).

camera_to_rpn is the twin of rpn_to_camera (layers/rpn_proposals.py): camera-frame points times `scale`, x negated when `flip`, rotated
about y by `rot` (the signed angle InstancePointCloud.train_clouds returned), minus `mean`.  fp32 in the reference's order.
"""
import torch

from .. import engine as E
from ..pts import _lib


def match_targets(boxes, span, gt, gt_rows, high, low, matched=None):
    what = "match_targets"
    for t in (boxes, span, gt, gt_rows):
        if not t.is_cuda:
            raise RuntimeError(f"{what}: expected CUDA/HIP tensors on an MI355X; the HIP path has no CPU fallback")
    R, G = boxes.shape[0], gt.shape[0]
    if boxes.shape != (R, 4) or span.shape != (R, 2) or gt.shape != (G, 4) or gt_rows.dim() != 2 or gt_rows.shape[0] != G:
        raise RuntimeError(f"{what}: boxes [R,4], span [R,2], gt [G,4], gt_rows [G,row] expected, got {tuple(boxes.shape)}, {tuple(span.shape)}, "
                           f"{tuple(gt.shape)}, {tuple(gt_rows.shape)}")
    if boxes.dtype != torch.float32 or gt.dtype != torch.float32 or gt_rows.dtype != torch.float32 or span.dtype != torch.int32:
        raise RuntimeError(f"{what}: fp32 boxes, gt and gt_rows and an int32 span expected")
    row = gt_rows.shape[1]
    dev = boxes.device
    if matched is None:
        matched = torch.empty(R, dtype=torch.int64, device=dev)
    elif matched.shape != (R,) or matched.dtype != torch.int64 or not matched.is_cuda or not matched.is_contiguous():
        raise RuntimeError(f"{what}: `matched` must be a contiguous int64 [R] device tensor")
    rows = torch.empty((R, row), dtype=torch.float32, device=dev)
    if R:
        st = _lib.lib().drc_match_targets_fwd(R, G, E._ptr(boxes.contiguous()), E._ptr(span.contiguous()), E._ptr(gt.contiguous()),
                                              E._ptr(gt_rows.contiguous()), row, float(high), float(low), E._ptr(matched), E._ptr(rows),
                                              E._stream_ptr(dev))
        _lib.check(st, "drc_match_targets_fwd")
    return matched, rows


def camera_to_rpn(xyz, mean, rot, scale=1.0, flip=False):
    what = "camera_to_rpn"
    if not (xyz.is_cuda and mean.is_cuda and rot.is_cuda):
        raise RuntimeError(f"{what}: expected CUDA/HIP tensors on an MI355X; the HIP path has no CPU fallback")
    B = mean.shape[0]
    if xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.shape[0] != B or mean.shape != (B, 3) or rot.shape != (B,):
        raise RuntimeError(f"{what}: xyz [B,K,3], mean [B,3], rot [B] expected, got {tuple(xyz.shape)}, {tuple(mean.shape)}, {tuple(rot.shape)}")
    if xyz.dtype != torch.float32 or mean.dtype != torch.float32 or rot.dtype != torch.float64:
        raise RuntimeError(f"{what}: fp32 xyz and mean and an fp64 rot expected")
    K = xyz.shape[1]
    out = torch.empty((B, K, 3), dtype=torch.float32, device=xyz.device)
    if B and K:
        st = _lib.lib().drc_camera_to_rpn_fwd(B, K, E._ptr(xyz.contiguous()), float(scale), int(bool(flip)), E._ptr(mean.contiguous()),
                                              E._ptr(rot.contiguous()), E._ptr(out), E._stream_ptr(xyz.device))
        _lib.check(st, "drc_camera_to_rpn_fwd")
    return out

"""`iou3d_cuda` -- the names of PointRCNN's compiled 3D IoU / NMS extension (point_rcnn/lib/utils/iou3d/src/iou3d.cpp), served by
libdisprcnn_pts.so.

The reference's iou3d_utils.py binds it with `import iou3d_cuda` and calls the four functions below with the positional signatures of
iou3d.cpp's PYBIND11_MODULE, the outputs written in place.  This module keeps exactly those signatures, so that file runs unchanged with
``sys.modules['iou3d_cuda']`` pointed here (the same story as disprcnn_amd/_C.py and pointnet2_cuda.py).  Differences by design:
  - every tensor is checked (device, dtype, contiguity, size) before a kernel sees it;
  - nms_gpu / nms_normal_gpu build the suppression mask and walk it on the device in a caller-owned workspace (the reference
    cudaMallocs the mask, copies it to the host and walks it there); the kept positions and their count come back in one read.
GPU tensors only (except `keep`, which the reference passes as a CPU LongTensor): there is no CPU kernel and no fallback.
"""
import torch

from . import engine as E
from .layers.nms import _mask_workspace
from .pts import _lib


def _check(t, what, dtype, numel=None, gpu=True):
    if not isinstance(t, torch.Tensor) or (gpu and not t.is_cuda):
        raise RuntimeError(f"iou3d_cuda: {what} must be a CUDA/HIP tensor (no CPU kernel)")
    if t.dtype != dtype:
        raise RuntimeError(f"iou3d_cuda: {what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"iou3d_cuda: {what} must be contiguous")
    if numel is not None and t.numel() != numel:
        raise RuntimeError(f"iou3d_cuda: {what} has {t.numel()} elements, expected {numel}")
    return E._ptr(t)


def _boxes(t, what, width):
    _check(t, what, torch.float32)
    if t.dim() != 2 or t.shape[1] != width:
        raise RuntimeError(f"iou3d_cuda: {what} must be [N,{width}], got {tuple(t.shape)}")
    return t.shape[0]


def _pairwise(boxes_a, boxes_b, out, mode, name):
    na, nb = _boxes(boxes_a, "boxes_a", 5), _boxes(boxes_b, "boxes_b", 5)
    _check(out, "ans", torch.float32, na * nb)
    if boxes_b.device != boxes_a.device or out.device != boxes_a.device:
        raise RuntimeError(f"iou3d_cuda.{name}: all tensors must be on one device")
    st = _lib.lib().drc_box3d_bev(na, nb, E._ptr(boxes_a), E._ptr(boxes_b), mode, E._ptr(out), E._stream_ptr(boxes_a.device))
    _lib.check(st, "drc_box3d_bev")
    return 1


def boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap):
    """iou3d.cpp: boxes_a (N,5), boxes_b (M,5) [x1,y1,x2,y2,ry] -> ans_overlap (N,M) rotated BEV overlap areas."""
    return _pairwise(boxes_a, boxes_b, ans_overlap, 0, "boxes_overlap_bev_gpu")


def boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou):
    """iou3d.cpp: boxes_a (N,5), boxes_b (M,5) -> ans_iou (N,M) rotated BEV IoU."""
    return _pairwise(boxes_a, boxes_b, ans_iou, 1, "boxes_iou_bev_gpu")


def nms_rows(boxes, counts, thresh, normal=False, max_keep=-1):
    """The batched kernel pair: boxes [B,N,5] (each row in score order), counts [B] int32 on the device ->
    (keep [B,K] int64 positions, -1 past the count; num [B] int32), K = min(max_keep, N) or N.  No host sync."""
    _check(boxes, "boxes", torch.float32)
    if boxes.dim() != 3 or boxes.shape[2] != 5:
        raise RuntimeError(f"iou3d_cuda: boxes must be [B,N,5], got {tuple(boxes.shape)}")
    b, n = boxes.shape[0], boxes.shape[1]
    _check(counts, "counts", torch.int32, b)
    if counts.device != boxes.device:
        raise RuntimeError("iou3d_cuda: boxes and counts must be on one device")
    k = min(max_keep, n) if max_keep > 0 else n
    dev = boxes.device
    keep = torch.full((b, k), -1, dtype=torch.int64, device=dev)
    num = torch.zeros(b, dtype=torch.int32, device=dev)
    mask = _mask_workspace(b, n, dev) if n > 0 else None
    st = _lib.lib().drc_box3d_nms(b, n, E._ptr(boxes), E._ptr(counts), float(thresh), int(bool(normal)), int(max_keep), E._ptr(mask),
                                  E._ptr(keep), k, E._ptr(num), E._stream_ptr(dev))
    _lib.check(st, "drc_box3d_nms")
    return keep, num


def _nms(boxes, keep, thresh, normal):
    n = _boxes(boxes, "boxes", 5)
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.int64 or not keep.is_contiguous() or keep.numel() < n:
        raise RuntimeError(f"iou3d_cuda: keep must be a contiguous int64 tensor of at least {n} elements")
    if n == 0:
        return 0
    counts = torch.full((1,), n, dtype=torch.int32, device=boxes.device)
    kd, num = nms_rows(boxes.view(1, n, 5), counts, thresh, normal)
    res = torch.cat((num.to(torch.int64), kd[0])).cpu()         # the one host sync, as the reference's mask copy
    cnt = int(res[0])
    keep.view(-1)[:cnt].copy_(res[1:1 + cnt])
    return cnt


def nms_gpu(boxes, keep, nms_overlap_thresh):
    """iou3d.cpp: boxes (N,5) [x1,y1,x2,y2,ry] in score order -> keep[:k] = kept positions (rotated IoU > thresh suppresses); returns k."""
    return _nms(boxes, keep, nms_overlap_thresh, False)


def nms_normal_gpu(boxes, keep, nms_overlap_thresh):
    """iou3d.cpp: as nms_gpu with the axis-aligned iou_normal (ry ignored)."""
    return _nms(boxes, keep, nms_overlap_thresh, True)

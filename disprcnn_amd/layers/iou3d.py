"""iou3d -- PointRCNN's 3D box IoU and NMS (point_rcnn/lib/utils/iou3d/iou3d_utils.py, kitti_utils.boxes3d_to_bev_torch) on the HIP kernels
of libdisprcnn_pts.so.  Same signatures and results as the reference, with these differences:

  - the score sort is STABLE (descending, ties in index order), as layers/nms.py's.  The reference's `scores.sort` is not stable, so on
    tied scores its keep order is undefined; with distinct scores the two agree exactly.  This is the one intended difference;
  - empty inputs give the reference's shapes -- boxes_iou_bev (1,1), boxes_iou3d_gpu (Nb,Na) -- filled with zeros and on the input's
    device (the reference returns uninitialised CPU tensors);
  - boxes_iou3d_gpu is one kernel (BEV conversion, rotated overlap, height overlap, volumes and the clamp(min=1e-7) division, in the
    torch steps' fp32 order) instead of six torch ops around the overlap kernel;
  - nms_gpu_batched: the rotated / axis-aligned NMS of many rows (ProposalLayer's per-ROI proposals) in one mask launch and one on-device
    walk, with no host sync at all.
"""
import torch

from .. import engine as E
from .. import iou3d_cuda


def boxes3d_to_bev_torch(boxes3d):
    """(N,7) [x, y, z, h, w, l, ry] -> (N,5) [x1, y1, x2, y2, ry] (kitti_utils.py)."""
    boxes_bev = boxes3d.new(torch.Size((boxes3d.shape[0], 5)))
    cu, cv = boxes3d[:, 0], boxes3d[:, 2]
    half_l, half_w = boxes3d[:, 5] / 2, boxes3d[:, 4] / 2
    boxes_bev[:, 0], boxes_bev[:, 1] = cu - half_l, cv - half_w
    boxes_bev[:, 2], boxes_bev[:, 3] = cu + half_l, cv + half_w
    boxes_bev[:, 4] = boxes3d[:, 6]
    return boxes_bev


def _boxes(t, width, what):
    E.require_gpu(t, what)
    if t.dim() != 2 or t.shape[1] != width:
        raise RuntimeError(f"{what}: expected [N,{width}] boxes, got {tuple(t.shape)}")
    return t.contiguous()


def boxes_iou_bev(boxes_a, boxes_b):
    """(Na,5), (Nb,5) [x1,y1,x2,y2,ry] -> (Na,Nb) rotated BEV IoU; (1,1) zeros when either is empty (the reference's shape)."""
    if boxes_a.numel() == 0 or boxes_b.numel() == 0:
        return torch.zeros((1, 1), dtype=torch.float32, device=boxes_a.device)
    a, b = _boxes(boxes_a, 5, "boxes_iou_bev"), _boxes(boxes_b, 5, "boxes_iou_bev")
    ans = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    iou3d_cuda.boxes_iou_bev_gpu(a, b, ans)
    return ans


def boxes_overlap_bev(boxes_a, boxes_b):
    """(Na,5), (Nb,5) -> (Na,Nb) rotated BEV overlap areas (iou3d_cuda.boxes_overlap_bev_gpu)."""
    a, b = _boxes(boxes_a, 5, "boxes_overlap_bev"), _boxes(boxes_b, 5, "boxes_overlap_bev")
    ans = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    if ans.numel():
        iou3d_cuda.boxes_overlap_bev_gpu(a, b, ans)
    return ans


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """(Na,7), (Nb,7) [x,y,z,h,w,l,ry] -> (Na,Nb) 3D IoU in one kernel; (Nb,Na) zeros when either is empty (the reference's shape)."""
    if boxes_a.numel() == 0 or boxes_b.numel() == 0:
        return torch.zeros((boxes_b.shape[0], boxes_a.shape[0]), dtype=torch.float32, device=boxes_a.device)
    a, b = _boxes(boxes_a, 7, "boxes_iou3d_gpu"), _boxes(boxes_b, 7, "boxes_iou3d_gpu")
    if b.device != a.device:
        raise RuntimeError("boxes_iou3d_gpu: both box sets must be on one device")
    ans = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    st = iou3d_cuda._lib.lib().drc_box3d_iou3d(a.shape[0], b.shape[0], E._ptr(a), E._ptr(b), E._ptr(ans), E._stream_ptr(a.device))
    iou3d_cuda._lib.check(st, "drc_box3d_iou3d")
    return ans


def _order(scores):
    return torch.sort(scores.float(), dim=-1, descending=True, stable=True)[1]


def _nms(boxes, scores, thresh, normal):
    b = _boxes(boxes, 5, "nms_gpu")
    n = b.shape[0]
    if scores.shape != (n,):
        raise RuntimeError(f"nms_gpu: scores must be [{n}], got {tuple(scores.shape)}")
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=b.device)
    order = _order(scores)
    counts = torch.full((1,), n, dtype=torch.int32, device=b.device)
    keep, num = iou3d_cuda.nms_rows(b.index_select(0, order).view(1, n, 5), counts, thresh, normal)
    return order[keep[0, :int(num.item())]].contiguous()     # the one host sync: the kept count


def nms_gpu(boxes, scores, thresh):
    """Rotated NMS: boxes (N,5) [x1,y1,x2,y2,ry], scores (N) -> int64 indices of the kept boxes in descending-score order
    (order[keep], as the reference; NOT ascending like layers.nms).  A box is dropped when its BEV IoU with a kept one is > thresh."""
    return _nms(boxes, scores, thresh, False)


def nms_normal_gpu(boxes, scores, thresh):
    """Axis-aligned NMS (ry ignored): as nms_gpu, kept indices in descending-score order."""
    return _nms(boxes, scores, thresh, True)


def nms_gpu_batched(boxes_bev, scores, counts, thresh, max_keep=-1, normal=False):
    """NMS of B rows at once: boxes_bev (B,N,5), scores (B,N), counts (B) (row b uses its first counts[b] boxes; clamped to [0,N]).
    -> (keep (B,K) int64, num (B) int64): row b's first num[b] entries are exactly what nms_gpu (normal=False) or nms_normal_gpu
    (normal=True) returns for that row alone, cut to max_keep; the rest are -1.  K = min(max_keep, N) when max_keep > 0, else N.
    One mask launch and one walk launch for all rows, no host sync."""
    b = boxes_bev
    E.require_gpu(b, "nms_gpu_batched")
    if b.dim() != 3 or b.shape[2] != 5 or scores.shape != b.shape[:2]:
        raise RuntimeError(f"nms_gpu_batched expects boxes_bev [B,N,5] and scores [B,N], got {tuple(b.shape)} and {tuple(scores.shape)}")
    B, N = b.shape[0], b.shape[1]
    counts = torch.as_tensor(counts, device=b.device).to(torch.int32).contiguous()
    if counts.shape != (B,):
        raise RuntimeError(f"nms_gpu_batched: counts must be [{B}], got {tuple(counts.shape)}")
    pos = torch.arange(N, device=b.device)
    valid = pos.view(1, N) < counts.view(B, 1)
    # padding sorts last: -inf, and the stable sort keeps it behind the row's own -inf scores (lower indices)
    order = _order(torch.where(valid, scores.float(), torch.full_like(scores, float("-inf"), dtype=torch.float32)))
    sorted_boxes = torch.gather(b, 1, order.unsqueeze(2).expand(B, N, 5)).contiguous()
    keep, num = iou3d_cuda.nms_rows(sorted_boxes, counts, thresh, normal, max_keep)
    idx = torch.gather(order, 1, keep.clamp(min=0))
    return torch.where(keep >= 0, idx, keep), num.to(torch.int64)

"""roipool3d -- PointRCNN's point pooling into 3D boxes (point_rcnn/lib/utils/roipool3d/roipool3d_utils.py, kitti_utils.enlarge_box3d)
on the HIP kernel of libdisprcnn_pts.so.  Same signature, outputs and dtypes as the reference's roipool3d_gpu: the first
`sampled_pt_num` points inside each (enlarged) box in index order, repeated cyclically when there are fewer, as `xyz ++ feature` rows;
a box without a point gets pooled_empty_flag 1 and zero rows.  One workgroup per box; no per-call B*N*M assignment buffer.
sampled_pt_num above roipool3d_cuda.max_sampled_pt_num() is refused with a RuntimeError.
"""
import numpy as np
import torch

from .. import roipool3d_cuda


def enlarge_box3d(boxes3d, extra_width):
    """(N,7) [x, y, z, h, w, l, ry]: h, w, l grow by 2 * extra_width and the bottom y moves down by extra_width (kitti_utils.py)."""
    if isinstance(boxes3d, np.ndarray):
        large_boxes3d = boxes3d.copy()
    else:
        large_boxes3d = boxes3d.clone()
    large_boxes3d[:, 3:6] = large_boxes3d[:, 3:6] + extra_width * 2
    large_boxes3d[:, 1] = large_boxes3d[:, 1] + extra_width
    return large_boxes3d


def roipool3d_gpu(pts, pts_feature, boxes3d, pool_extra_width, sampled_pt_num=512):
    """pts (B,N,3), pts_feature (B,N,C), boxes3d (B,M,7) -> pooled_features (B,M,S,3+C) fp32, pooled_empty_flag (B,M) int32."""
    batch_size, boxes_num, feature_len = pts.shape[0], boxes3d.shape[1], pts_feature.shape[2]
    pooled_boxes3d = enlarge_box3d(boxes3d.view(-1, 7), pool_extra_width).view(batch_size, -1, 7)
    pooled_features = torch.zeros((batch_size, boxes_num, sampled_pt_num, 3 + feature_len), dtype=torch.float32, device=pts.device)
    pooled_empty_flag = torch.zeros((batch_size, boxes_num), dtype=torch.int32, device=pts.device)
    roipool3d_cuda.forward(pts.contiguous(), pooled_boxes3d.contiguous(), pts_feature.contiguous(), pooled_features, pooled_empty_flag)
    return pooled_features, pooled_empty_flag


def pts_in_boxes3d_gpu(pts, boxes3d):
    """The device counterpart of pts_in_boxes3d_cpu: pts (N,3) or (B,N,3), boxes3d (M,7) or (B,M,7) [x,y,z,h,w,l,ry] ->
    bool (M,N) or (B,M,N), the reference's pt_in_box3d test of every point against every box."""
    single = pts.dim() == 2
    p, bx = (pts.unsqueeze(0), boxes3d.unsqueeze(0)) if single else (pts, boxes3d)
    if p.dim() != 3 or bx.dim() != 3 or bx.shape[0] != p.shape[0]:
        raise RuntimeError(f"pts_in_boxes3d_gpu expects pts (B,N,3) and boxes3d (B,M,7), got {tuple(pts.shape)} and {tuple(boxes3d.shape)}")
    flags = torch.zeros((p.shape[0], bx.shape[1], p.shape[1]), dtype=torch.bool, device=p.device)
    roipool3d_cuda.pts_in_boxes3d(p.contiguous(), bx.contiguous(), flags)
    return flags[0] if single else flags

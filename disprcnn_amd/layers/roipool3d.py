"""roipool3d -- PointRCNN's point pooling into 3D boxes (point_rcnn/lib/utils/roipool3d/roipool3d_utils.py, kitti_utils.enlarge_box3d)
on the HIP kernel of libdisprcnn_pts.so.  Same signature, outputs and dtypes as the reference's roipool3d_gpu: the first
`sampled_pt_num` points inside each (enlarged) box in index order, repeated cyclically when there are fewer, as `xyz ++ feature` rows;
a box without a point gets pooled_empty_flag 1 and zero rows.  One workgroup per box; no per-call B*N*M assignment buffer.
sampled_pt_num above roipool3d_cuda.max_sampled_pt_num() is refused with a RuntimeError.

`roipool3d_canonical` is the RCNN stage's form (rcnn_net.py, the ROI_SAMPLE_JIT eval branch): pooling fused with the canonical transform,
reading the RPN's outputs in the layouts it returns them and writing what the shared MLPs read, in one kernel (pts/rcnn_ops.hip).
`roipool3d_canonical_unfused` composes the same result from `roipool3d_gpu` and torch the reference's way, for the tests and
tools/bench_rcnn.py to compare against; the modules never call it.
"""
import ctypes as C

import numpy as np
import torch

from .. import engine as E
from .. import roipool3d_cuda
from ..pts import _lib


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


def roipool3d_canonical(rpn_xyz, backbone_features, seg_mask, pts_depth, roi_boxes3d, pool_extra_width, sampled_pt_num=512):
    """rpn_xyz (B,N,3), backbone_features (B,C,N) channel-major, seg_mask (B,N), pts_depth (B,N) or None (no depth channel),
    roi_boxes3d (B,M,7) -> xyz (R,S,3), pts (R,3+E,S), feat (R,C,S), empty_flag (R) int32 with R = B*M, E = 1 + (pts_depth given):
    the first S points inside each enlarged ROI (cyclically repeated), moved to the ROI's centre and rotated by its angle; pts holds the
    canonical x, y, z, the mask and pts_depth / 70 - 0.5.  An empty ROI has zero features and xyz = rotate(-centre)."""
    what = "roipool3d_canonical"
    for t in (rpn_xyz, backbone_features, seg_mask, roi_boxes3d):
        E.require_gpu(t, what)
    if rpn_xyz.dim() != 3 or rpn_xyz.shape[2] != 3:
        raise RuntimeError(f"{what}: rpn_xyz must be [B,N,3], got {tuple(rpn_xyz.shape)}")
    B, N, _ = rpn_xyz.shape
    if backbone_features.dim() != 3 or backbone_features.shape[0] != B or backbone_features.shape[2] != N:
        raise RuntimeError(f"{what}: backbone_features must be [{B},C,{N}], got {tuple(backbone_features.shape)}")
    if roi_boxes3d.dim() != 3 or roi_boxes3d.shape[0] != B or roi_boxes3d.shape[2] != 7:
        raise RuntimeError(f"{what}: roi_boxes3d must be [{B},M,7], got {tuple(roi_boxes3d.shape)}")
    if seg_mask.shape != (B, N) or (pts_depth is not None and pts_depth.shape != (B, N)):
        raise RuntimeError(f"{what}: seg_mask and pts_depth must be [{B},{N}]")
    Cf, M, S = backbone_features.shape[1], roi_boxes3d.shape[1], int(sampled_pt_num)
    if not 1 <= S <= roipool3d_cuda.max_sampled_pt_num():
        raise RuntimeError(f"{what}: sampled_pt_num must be in 1..{roipool3d_cuda.max_sampled_pt_num()}, got {S}")
    use_depth = pts_depth is not None
    if use_depth:
        E.require_gpu(pts_depth, what)
    dev, R = rpn_xyz.device, B * M
    xyz = torch.empty((R, S, 3), dtype=torch.float32, device=dev)
    pts = torch.empty((R, 4 + int(use_depth), S), dtype=torch.float32, device=dev)
    feat = torch.empty((R, Cf, S), dtype=torch.float32, device=dev)
    empty_flag = torch.empty((R,), dtype=torch.int32, device=dev)
    if R:
        w = float(pool_extra_width)
        st = _lib.lib().drc_rcnn_pool_canonical_fwd(B, N, M, Cf, S, E._ptr(rpn_xyz.contiguous()), E._ptr(backbone_features.contiguous()),
                                                    E._ptr(seg_mask.contiguous()), E._ptr(pts_depth.contiguous() if use_depth else None),
                                                    int(use_depth), E._ptr(roi_boxes3d.contiguous()), C.c_float(w), C.c_float(w * 2),
                                                    E._ptr(xyz), E._ptr(pts), E._ptr(feat), E._ptr(empty_flag), E._stream_ptr(dev))
        _lib.check(st, "drc_rcnn_pool_canonical_fwd")
    return xyz, pts, feat, empty_flag


def rotate_pc_along_y_torch(pc, rot_angle):
    """kitti_utils.rotate_pc_along_y_torch: pc (M,S,3+C) rotated in place about y by rot_angle (M)."""
    cosa = torch.cos(rot_angle).view(-1, 1)
    sina = torch.sin(rot_angle).view(-1, 1)
    raw_1 = torch.cat([cosa, -sina], dim=1)
    raw_2 = torch.cat([sina, cosa], dim=1)
    R = torch.cat((raw_1.unsqueeze(dim=1), raw_2.unsqueeze(dim=1)), dim=1)
    pc_temp = pc[:, :, [0, 2]]
    pc[:, :, [0, 2]] = torch.matmul(pc_temp, R.permute(0, 2, 1))
    return pc


def roipool3d_canonical_unfused(rpn_xyz, backbone_features, seg_mask, pts_depth, roi_boxes3d, pool_extra_width, sampled_pt_num=512):
    """The same outputs the reference's way, on the operators that existed before the fused kernel: the (B,N,C) permute, the
    (B,N,E+C) concat, roipool3d_gpu's zero-filled (B,M,S,3+E+C) tensor, the subtraction, the per-cloud rotation and the transposes.
    pts_depth is divided by a tensor of 70s: a scalar divisor would become a multiplication by its reciprocal on the device."""
    B, M, S = roi_boxes3d.shape[0], roi_boxes3d.shape[1], int(sampled_pt_num)
    if B * M == 0:                                          # roipool3d_gpu's views need at least one box
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=rpn_xyz.device)
        return (z(0, S, 3), z(0, 4 + int(pts_depth is not None), S), z(0, backbone_features.shape[1], S),
                torch.zeros((0,), dtype=torch.int32, device=rpn_xyz.device))
    rpn_features = backbone_features.permute(0, 2, 1)
    extra = [seg_mask.unsqueeze(2)]
    if pts_depth is not None:
        extra.append((pts_depth / torch.full_like(pts_depth, 70.0) - 0.5).unsqueeze(2))
    pts_feature = torch.cat(extra + [rpn_features], dim=2)
    pooled, empty_flag = roipool3d_gpu(rpn_xyz, pts_feature, roi_boxes3d, pool_extra_width, sampled_pt_num=sampled_pt_num)
    pooled[:, :, :, 0:3] = pooled[:, :, :, 0:3] - roi_boxes3d[:, :, 0:3].unsqueeze(2)
    for k in range(roi_boxes3d.shape[0]):
        pooled[k, :, :, 0:3] = rotate_pc_along_y_torch(pooled[k, :, :, 0:3], roi_boxes3d[k, :, 6])
    pts_input = pooled.view(pooled.shape[0] * pooled.shape[1], pooled.shape[2], pooled.shape[3])
    n_in = 3 + len(extra)
    xyz = pts_input[..., 0:3].contiguous()
    pts = pts_input[..., 0:n_in].transpose(1, 2).contiguous()
    feat = pts_input[..., n_in:].transpose(1, 2).contiguous()
    return xyz, pts, feat, empty_flag.view(-1)

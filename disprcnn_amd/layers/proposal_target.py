"""The two operators of PointRCNN's ProposalTargetLayer (point_rcnn/lib/rpn/proposal_target_layer.py) on the HIP kernels of
libdisprcnn_pts.so (pts/proposal_target.hip), and the random draws they consume.

    proposal_draws(B, M, P, T, device, generator=None) -> draws (B, M + P + 9 P T + 3 P) fp32 uniforms in [0,1)
    rcnn_sample_rois(roi_boxes3d, gt_boxes3d, draws, ...) -> the sampled, noise-augmented ROIs of every cloud (sample_rois_for_rcnn)
    rcnn_pool_target(rpn_xyz, backbone_features, seg_mask, pts_depth, sampled, draws, ...) -> the pooled, augmented, canonical network
        input with its labels (the rest of the reference's forward)

The randomness is an input: every random decision reads one uniform of `draws`.  Per cloud, with M candidates, P = ROI_PER_IMAGE slots
and T = ROI_FG_AUG_TIMES iterations, draws[b] = key[M] | pick[P] | noise[P][T][9] | aug[P][3] (include/disprcnn_pts.h).
Neither operator reads anything back from the device.

Limits: 1 <= M <= MAX_CANDIDATES() (1024, the sampler's LDS lists), 1 <= P <= MAX_SLOTS() (256, one workgroup per cloud), N >= 1
ground-truth boxes per cloud, sampled_pt_num as roipool3d_canonical.  Anything else is refused with a RuntimeError before a launch.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import engine as E
from .. import roipool3d_cuda
from ..pts import _lib

AUG_METHODS = {"multiple": 0, "single": 1}
NOISE_DRAWS = 9                                            # per iteration: keep, range row, 3 position, 3 size, angle
AUG_DRAWS = 3                                              # per slot: rotation, scale, flip
N_COUNTS = 5                                               # per cloud: fg, hard bg, easy bg candidates, fg slots, no-candidate flag


def MAX_CANDIDATES():
    return _lib.lib().drc_rcnn_sample_max_candidates()


def MAX_SLOTS():
    return _lib.lib().drc_rcnn_sample_max_slots()


def draws_per_cloud(M, P, T):
    return M + P + NOISE_DRAWS * P * T + AUG_DRAWS * P


def draw_blocks(M, P, T):
    """-> the offsets of key, pick, noise, aug in one cloud's draws, and its length"""
    return {"key": 0, "pick": M, "noise": M + P, "aug": M + P + NOISE_DRAWS * P * T, "len": draws_per_cloud(M, P, T)}


def proposal_draws(B, M, P, T, device, generator=None):
    """One torch.rand call for every random decision of the layer: (B, M + P + 9 P T + 3 P) fp32 in [0,1)."""
    return torch.rand((int(B), draws_per_cloud(int(M), int(P), int(T))), dtype=torch.float32, device=device, generator=generator)


def _check_draws(draws, B, M, P, T, what):
    E.require_gpu(draws, what)
    if draws.dim() != 2 or draws.shape[0] != B or draws.shape[1] != draws_per_cloud(M, P, T):
        raise RuntimeError(f"{what}: draws must be [{B},{draws_per_cloud(M, P, T)}] (M={M}, P={P}, T={T}), got {tuple(draws.shape)}")


def rcnn_sample_rois(roi_boxes3d, gt_boxes3d, draws, roi_per_image, fg_ratio, reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo,
                     hard_bg_ratio, fg_aug_times, aug_method="multiple"):
    """roi_boxes3d (B,M,7) candidates, gt_boxes3d (B,N,7 or 8) [x,y,z,h,w,l,ry(,cls)], draws (B, draws_per_cloud(M,P,T)) ->
    dict: rois (B,P,7) after the noise loop, gt_of_rois (B,P,7), roi_iou (B,P), src_index (B,P) int32, n_iter (B,P) int32,
    counts (B,5) int32 [fg, hard bg, easy bg candidates, fg slots, no-candidate flag]."""
    what = "rcnn_sample_rois"
    if aug_method == "normal":
        raise NotImplementedError("RCNN.REG_AUG_METHOD = 'normal': the reference's branch calls torch.rand() without a size and cannot run")
    if aug_method not in AUG_METHODS:
        raise NotImplementedError(f"RCNN.REG_AUG_METHOD = {aug_method!r}")
    for t in (roi_boxes3d, gt_boxes3d):
        E.require_gpu(t, what)
    if roi_boxes3d.dim() != 3 or roi_boxes3d.shape[2] != 7:
        raise RuntimeError(f"{what}: roi_boxes3d must be [B,M,7], got {tuple(roi_boxes3d.shape)}")
    B, M, _ = roi_boxes3d.shape
    if gt_boxes3d.dim() != 3 or gt_boxes3d.shape[0] != B or gt_boxes3d.shape[2] not in (7, 8):
        raise RuntimeError(f"{what}: gt_boxes3d must be [{B},N,7] (or 8 with the class), got {tuple(gt_boxes3d.shape)}")
    N, P, T = gt_boxes3d.shape[1], int(roi_per_image), int(fg_aug_times)
    if N < 1:
        raise RuntimeError(f"{what}: every cloud needs at least one ground-truth box, got gt_boxes3d {tuple(gt_boxes3d.shape)}")
    if not 1 <= M <= MAX_CANDIDATES():
        raise RuntimeError(f"{what}: 1..{MAX_CANDIDATES()} candidates per cloud are supported, got roi_boxes3d {tuple(roi_boxes3d.shape)}")
    if not 1 <= P <= MAX_SLOTS():
        raise RuntimeError(f"{what}: ROI_PER_IMAGE must be in 1..{MAX_SLOTS()}, got {P}")
    if T < 0:
        raise RuntimeError(f"{what}: ROI_FG_AUG_TIMES must be >= 0, got {T}")
    fg_per_image = int(np.round(fg_ratio * P))
    if not 0 <= fg_per_image <= P or not 0.0 <= float(hard_bg_ratio) <= 1.0:
        raise RuntimeError(f"{what}: FG_RATIO {fg_ratio} and HARD_BG_RATIO {hard_bg_ratio} must lie in [0, 1]")
    _check_draws(draws, B, M, P, T, what)
    dev = roi_boxes3d.device
    gt7 = gt_boxes3d[..., 0:7].contiguous()
    out = {"rois": torch.empty((B, P, 7), dtype=torch.float32, device=dev), "gt_of_rois": torch.empty((B, P, 7), dtype=torch.float32, device=dev),
           "roi_iou": torch.empty((B, P), dtype=torch.float32, device=dev), "src_index": torch.empty((B, P), dtype=torch.int32, device=dev),
           "n_iter": torch.empty((B, P), dtype=torch.int32, device=dev), "counts": torch.empty((B, N_COUNTS), dtype=torch.int32, device=dev)}
    if B:
        draws = draws.contiguous()
        st = _lib.lib().drc_rcnn_sample_rois(B, M, N, P, T, fg_per_image, AUG_METHODS[aug_method], C.c_float(min(reg_fg_thresh, cls_fg_thresh)),
                                             C.c_float(cls_bg_thresh), C.c_float(cls_bg_thresh_lo), C.c_double(hard_bg_ratio),
                                             E._ptr(roi_boxes3d.contiguous()), E._ptr(gt7), E._ptr(draws), draws.shape[1], E._ptr(out["rois"]),
                                             E._ptr(out["gt_of_rois"]), E._ptr(out["roi_iou"]), E._ptr(out["src_index"]), E._ptr(out["n_iter"]),
                                             E._ptr(out["counts"]), E._stream_ptr(dev))
        _lib.check(st, "drc_rcnn_sample_rois")
    return out


def rcnn_pool_target(rpn_xyz, backbone_features, seg_mask, pts_depth, sampled, draws, pool_extra_width, reg_fg_thresh, cls_fg_thresh,
                     cls_bg_thresh, sampled_pt_num=512, aug_data=True, aug_rot_range=18, num_candidates=None, fg_aug_times=None):
    """rpn_xyz (B,N,3), backbone_features (B,C,N) channel-major, seg_mask (B,N), pts_depth (B,N) or None, `sampled` = rcnn_sample_rois's
    dict; draws (B, draws_per_cloud(num_candidates, P, fg_aug_times)) or None when aug_data is off (no draw is read then) ->
    dict: xyz (R,S,3), pts (R,3+E,S), feat (R,C,S), empty_flag (R) int32, roi_boxes3d (R,7) augmented, gt_of_rois (R,7) canonical,
    cls_label (R) int64, reg_valid_mask (R) int64, with R = B * P and E = 1 + (pts_depth given)."""
    what = "rcnn_pool_target"
    rois, gts, iou, counts = sampled["rois"], sampled["gt_of_rois"], sampled["roi_iou"], sampled["counts"]
    for t in (rpn_xyz, backbone_features, seg_mask, rois, gts, iou):
        E.require_gpu(t, what)
    if rpn_xyz.dim() != 3 or rpn_xyz.shape[2] != 3:
        raise RuntimeError(f"{what}: rpn_xyz must be [B,N,3], got {tuple(rpn_xyz.shape)}")
    B, N, _ = rpn_xyz.shape
    if backbone_features.dim() != 3 or backbone_features.shape[0] != B or backbone_features.shape[2] != N:
        raise RuntimeError(f"{what}: backbone_features must be [{B},C,{N}], got {tuple(backbone_features.shape)}")
    if rois.dim() != 3 or rois.shape[0] != B or rois.shape[2] != 7:
        raise RuntimeError(f"{what}: rois must be [{B},P,7], got {tuple(rois.shape)}")
    P = rois.shape[1]
    if gts.shape != rois.shape or iou.shape != (B, P) or counts.shape != (B, N_COUNTS) or counts.dtype != torch.int32 or not counts.is_cuda:
        raise RuntimeError(f"{what}: gt_of_rois must be [{B},{P},7], roi_iou [{B},{P}] and counts int32 [{B},{N_COUNTS}], got "
                           f"{tuple(gts.shape)}, {tuple(iou.shape)}, {tuple(counts.shape)} {counts.dtype}")
    if seg_mask.shape != (B, N) or (pts_depth is not None and pts_depth.shape != (B, N)):
        raise RuntimeError(f"{what}: seg_mask and pts_depth must be [{B},{N}]")
    Cf, S = backbone_features.shape[1], int(sampled_pt_num)
    if not 1 <= S <= roipool3d_cuda.max_sampled_pt_num():
        raise RuntimeError(f"{what}: sampled_pt_num must be in 1..{roipool3d_cuda.max_sampled_pt_num()}, got {S}")
    use_depth = pts_depth is not None
    if use_depth:
        E.require_gpu(pts_depth, what)
    aug_ptr, stride = None, 0
    if aug_data:
        if draws is None or num_candidates is None or fg_aug_times is None:
            raise RuntimeError(f"{what}: aug_data needs draws, num_candidates and fg_aug_times")
        M, T = int(num_candidates), int(fg_aug_times)
        _check_draws(draws, B, M, P, T, what)
        draws = draws.contiguous()
        stride = draws.shape[1]
        aug_ptr = C.c_void_p(draws.data_ptr() + 4 * draw_blocks(M, P, T)["aug"]) if B else None
    dev, R = rpn_xyz.device, B * P
    out = {"xyz": torch.empty((R, S, 3), dtype=torch.float32, device=dev), "pts": torch.empty((R, 4 + int(use_depth), S), dtype=torch.float32, device=dev),
           "feat": torch.empty((R, Cf, S), dtype=torch.float32, device=dev), "empty_flag": torch.empty((R,), dtype=torch.int32, device=dev),
           "roi_boxes3d": torch.empty((R, 7), dtype=torch.float32, device=dev), "gt_of_rois": torch.empty((R, 7), dtype=torch.float32, device=dev),
           "cls_label": torch.empty((R,), dtype=torch.int64, device=dev), "reg_valid_mask": torch.empty((R,), dtype=torch.int64, device=dev)}
    if R:
        w = float(pool_extra_width)
        st = _lib.lib().drc_rcnn_pool_target_fwd(
            B, N, P, Cf, S, E._ptr(rpn_xyz.contiguous()), E._ptr(backbone_features.contiguous()), E._ptr(seg_mask.contiguous()),
            E._ptr(pts_depth.contiguous() if use_depth else None), int(use_depth), E._ptr(rois.contiguous()), E._ptr(gts.contiguous()),
            E._ptr(iou.contiguous()), E._ptr(counts.contiguous()), aug_ptr if aug_data else C.c_void_p(0), stride, int(bool(aug_data)),
            C.c_float(math.pi / aug_rot_range), C.c_float(w), C.c_float(w * 2), C.c_float(reg_fg_thresh), C.c_float(cls_fg_thresh),
            C.c_float(cls_bg_thresh), E._ptr(out["xyz"]), E._ptr(out["pts"]), E._ptr(out["feat"]), E._ptr(out["empty_flag"]),
            E._ptr(out["roi_boxes3d"]), E._ptr(out["gt_of_rois"]), E._ptr(out["cls_label"]), E._ptr(out["reg_valid_mask"]), E._stream_ptr(dev))
        _lib.check(st, "drc_rcnn_pool_target_fwd")
    return out

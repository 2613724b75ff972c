"""ctypes binding of libdisprcnn_pts.so (the C ABI declared in include/disprcnn_pts.h).

As disprcnn_amd/_lib.py: NO fallback -- if the library is missing or a symbol is absent, ``lib()`` raises, and a non-zero
status becomes ``RuntimeError``.
"""
import ctypes as C
import os

import torch  # noqa: F401  -- must be imported BEFORE the .so: both must share torch's libamdhip64 runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdisprcnn_pts.so")

_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_F = C.c_float
_D = C.c_double
_SIGS = {
    "drc_pts_version": (C.c_char_p, []),
    "drc_instance_points_fwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _F, _I, _P, _P, _L, _P]),
    "drc_instance_points_gather_fwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P]),
    "drc_instance_points_train_fwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _F, _I, _P, _P, _L, _P]),
    "drc_instance_points_gather_train_fwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _F, _F, _I, _P, _P, _P, _P, _P]),
    "drc_match_targets_fwd": (_I, [_I, _I, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P]),
    "drc_pn2_furthest_point_sampling": (_I, [_I, _I, _I, _P, _P, _P, _I, _P]),
    "drc_pn2_gather_points": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "drc_pn2_ball_query": (_I, [_I, _I, _I, _F, _I, _P, _P, _P, _P]),
    "drc_pn2_group_points": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "drc_pn2_three_nn": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "drc_pn2_three_interpolate": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "drc_pn2_csr_bounds": (_I, [_I, _I, _I, _P, _P, _P, _P]),
    "drc_pn2_csr_scatter_add": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "drc_box3d_bev": (_I, [_I, _I, _P, _P, _I, _P, _P]),
    "drc_box3d_iou3d": (_I, [_I, _I, _P, _P, _P, _P]),
    "drc_box3d_nms": (_I, [_I, _I, _P, _P, _F, _I, _I, _P, _P, _I, _P, _P]),
    "drc_roipool3d_fwd": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "drc_box3d_max_pool_samples": (_I, []),
    "drc_pts_in_boxes3d": (_I, [_I, _I, _I, _P, _P, _P, _P]),
    "drc_pn2_sa_mlp_max_fwd": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _I, _I, _P]),
    "drc_pn2_pointwise_mlp_fwd": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _I, _I, _P]),
    "drc_pn2_pointwise_mlp_dgrad": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "drc_pn2_wgrad_chunk": (_I, []),
    "drc_pn2_wgrad_workspace_floats": (_L, [_I, _I, _I, _I, _I]),
    "drc_pn2_pointwise_mlp_wgrad": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_pn2_group_max_fwd": (_I, [_L, _I, _P, _P, _P, _P]),
    "drc_pn2_group_max_bwd": (_I, [_L, _I, _P, _P, _P, _P]),
    "drc_pn2_bn_chunk": (_I, []),
    "drc_pn2_bn_workspace_doubles": (_L, [_I, _I, _I]),
    "drc_pn2_bn_stats": (_I, [_I, _I, _I, _P, _P, _F, _F, _P, _P, _P, _P]),
    "drc_pn2_bn_apply_fwd": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "drc_pn2_bn_bwd": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_rpn_points_depth": (_I, [_L, _P, _P, _P]),
    "drc_rpn_decode_proposals": (_I, [_L, _I, _P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _P, _P, _P]),
    "drc_rcnn_pool_canonical_fwd": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _F, _F, _P, _P, _P, _P, _P]),
    "drc_rcnn_decode_boxes": (_I, [_L, _I, _P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _P, _P, _P, _P]),
    "drc_rcnn_sample_max_candidates": (_I, []),
    "drc_rcnn_sample_max_slots": (_I, []),
    "drc_rcnn_sample_rois": (_I, [_I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _D, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P, _P]),
    "drc_rcnn_pool_target_fwd": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F, _F, _F, _F, _F, _F, _P, _P, _P, _P,
                                      _P, _P, _P, _P, _P]),
    "drc_rpn_to_camera_fwd": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_camera_to_rpn_fwd": (_I, [_I, _I, _P, _F, _I, _P, _P, _P, _P]),
    "drc_train_scratch_doubles": (_I, []),
    "drc_rpn_point_labels": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "drc_bin_reg_targets": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P]),
    "drc_bin_reg_loss_fwd": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_bin_reg_loss_bwd": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_point_cls_loss_fwd": (_I, [_L, _I, _P, _P, _P, _F, _F, _F, _F, _P, _P, _P, _P]),
    "drc_point_cls_loss_bwd": (_I, [_L, _I, _P, _P, _P, _F, _F, _F, _F, _P, _P, _P, _P]),
    "drc_focal_elementwise": (_I, [_L, _P, _P, _P, _F, _F, _P, _P, _P]),
    "drc_kitti_eval_max_det": (_I, []),
    "drc_kitti_eval_max_gt": (_I, []),
    "drc_kitti_eval_clean": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "drc_kitti_eval_overlaps": (_I, [_I, _L, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "drc_kitti_eval_pass1": (_I, [_I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _D, _D, _P, _P, _P]),
    "drc_kitti_eval_pass2": (_I, [_I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _D, _D, _I, _P, _P, _P, _P, _P]),
    "drc_kitti_eval_reduce": (_I, [_I, _P, _P, _P, _P, _P]),
    "drc_solver_chunk": (_I, []),
    "drc_solver_grad_norm": (_I, [_L, _L, _P, _P, _P, _P]),
    "drc_solver_prepare": (_I, [_L, _P, _I, _F, _I, _I, _P, _P, _P, _P, _P]),
    "drc_solver_sgd_step": (_I, [_L, _L, _I, _P, _P, _P, _P, _P, _I, _P]),
    "drc_solver_adam_step": (_I, [_L, _L, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "drc_det2d_max_gt": (_I, []),
    "drc_det2d_max_images": (_I, []),
    "drc_det2d_match_fwd": (_I, [_I, _P, _P, _I, _P, _P, _P, _P, _P, _F, _F, _I, _P, _P, _P, _P, _P, _P, _P]),
    "drc_det2d_sample_fwd": (_I, [_I, _P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "drc_det2d_srpn_loss_partials": (_L, [_I, _I, _I, _P]),
    "drc_det2d_srpn_loss_fwd": (_I, [_I, _I, _I, _P, _L, _P, _P, _P, _P, _D, _P, _P, _P]),
    "drc_det2d_fastrcnn_loss_fwd": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_det2d_mask_loss_fwd": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "drc_conv1x1_wgrad_default_chunk": (_I, []),
    "drc_conv1x1_wgrad_scratch_floats": (_L, [_I, _I, _I, _I, _I, _I]),
    "drc_conv1x1_wgrad_blocked": (_I, [_P, _L, _L, _L, _L, _P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P]),
    "drc_input_default_max_blocks": (_I, []),
    "drc_input_batch_fwd": (_I, [_P, _L, _P, _L, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "drc_mask_job_cols": (_I, []),
    "drc_mask_resize_flip_fwd": (_I, [_P, _I, _L, _I, _P]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None


def lib():
    """Load (once) and return the point-ops library; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the point-ops HIP library is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or python -m disprcnn_amd.pts.build). "
                "There is no CPU/torch fallback for this path.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        kind = "bad argument / unsupported shape" if status < 0 else "hipError_t"
        raise RuntimeError(f"{what} failed: status {status} ({kind})")

from .roi_align import ROIAlign, roi_align  # noqa: F401
from .nms import nms, nms_pair, nms_pair_sorted_joint  # noqa: F401
from .iou3d import boxes_iou3d_gpu, boxes_iou_bev, nms_gpu, nms_gpu_batched, nms_normal_gpu  # noqa: F401
from .roipool3d import pts_in_boxes3d_gpu, roipool3d_gpu  # noqa: F401
from .pn2_mlp import pointwise_mlp, sa_mlp_max  # noqa: F401
from .rpn_proposals import decode_rpn_boxes, propose  # noqa: F401


def smooth_l1_loss(input, target, beta=1. / 9, size_average=True):
    """The reference's layers/smooth_l1_loss.py in plain torch: torch's smooth L1 with the extra beta (mean, or the sum when not
    size_average).  The 2D stage's HIP losses (layers/det2d_loss.py) evaluate the same expression in their kernels; this is the function the
    reference exports and the one their oracle compares with."""
    import torch
    n = torch.abs(input - target)
    loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return loss.mean() if size_average else loss.sum()

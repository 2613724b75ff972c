from .roi_align import ROIAlign, roi_align  # noqa: F401
from .nms import nms, nms_pair, nms_pair_sorted_joint  # noqa: F401
from .iou3d import boxes_iou3d_gpu, boxes_iou_bev, nms_gpu, nms_gpu_batched, nms_normal_gpu  # noqa: F401
from .roipool3d import pts_in_boxes3d_gpu, roipool3d_gpu  # noqa: F401
from .pn2_mlp import pointwise_mlp, sa_mlp_max  # noqa: F401
from .rpn_proposals import decode_rpn_boxes, propose  # noqa: F401

"""PointRCNN's RCNN box decode and scoring (point_rcnn/lib/net/rcnn_inference.py, utils/bbox_transform.py:decode_bbox_target) on HIP.

    decode_rcnn_boxes(roi, reg, cls, mean_size, loc_scope, loc_bin_size, num_head_bin, loc_y_by_bin, loc_y_scope, loc_y_bin_size)
        -> (boxes7 [n,7], bev5 [n,5], norm_score [n])

One kernel: the bins' first-maximum argmax, the residuals, the fine angle, the rotation by -roi_ry, `+ roi_ry`, the ROI's centre on x and
z (y is `roi_y + offset`), the BEV form for the NMS and the sigmoid of the class logit; fp32 in the reference's expression order.  The
reference's constants are Python doubles that meet the fp32 tensor one at a time; they are computed here in double the same way and
rounded to fp32 at the call, as layers/rpn_proposals.py does.
"""
import ctypes as C
import math

import torch

from .. import engine as E
from ..pts import _lib


def reg_channels(loc_scope, loc_bin_size, num_head_bin, loc_y_by_bin, loc_y_scope, loc_y_bin_size):
    """The width of rcnn_reg (rcnn_net.py): 4 xz groups, the y offset or its 2 bin groups, 2 angle groups, 3 sizes."""
    per_loc_bin_num = int(loc_scope / loc_bin_size) * 2
    loc_y_bin_num = int(loc_y_scope / loc_y_bin_size) * 2
    return per_loc_bin_num * 4 + int(num_head_bin) * 2 + 3 + (loc_y_bin_num * 2 if loc_y_by_bin else 1)


def decode_rcnn_boxes(roi, reg, cls, mean_size, loc_scope, loc_bin_size, num_head_bin, loc_y_by_bin=False, loc_y_scope=0.5,
                      loc_y_bin_size=0.25):
    """roi (n,7) [x,y,z,h,w,l,ry], reg (n,R), cls (n) raw class logits -> boxes (n,7), bev (n,5) [x1,y1,x2,y2,ry], sigmoid(cls) (n)."""
    what = "decode_rcnn_boxes"
    for t in (roi, reg, cls):
        E.require_gpu(t, what)
    if roi.dim() != 2 or roi.shape[1] != 7 or reg.dim() != 2 or reg.shape[0] != roi.shape[0] or cls.shape != (roi.shape[0],):
        raise RuntimeError(f"{what}: roi [n,7], reg [n,R], cls [n] expected, got {tuple(roi.shape)}, {tuple(reg.shape)}, {tuple(cls.shape)}")
    n, R = reg.shape
    want = reg_channels(loc_scope, loc_bin_size, num_head_bin, loc_y_by_bin, loc_y_scope, loc_y_bin_size)
    if R != want:
        raise RuntimeError(f"{what}: reg has {R} channels, the bin layout needs {want}")
    per_loc_bin_num = int(loc_scope / loc_bin_size) * 2
    loc_y_bin_num = int(loc_y_scope / loc_y_bin_size) * 2
    num_head_bin = int(num_head_bin)
    h, w, l = (float(v) for v in mean_size)
    angle_per_class = (math.pi / 2) / num_head_bin
    boxes = torch.empty((n, 7), dtype=torch.float32, device=roi.device)
    bev = torch.empty((n, 5), dtype=torch.float32, device=roi.device)
    score = torch.empty((n,), dtype=torch.float32, device=roi.device)
    if n:
        f = C.c_float
        st = _lib.lib().drc_rcnn_decode_boxes(n, R, E._ptr(roi.contiguous()), E._ptr(reg.contiguous()), E._ptr(cls.contiguous()),
                                              per_loc_bin_num, loc_y_bin_num, num_head_bin, 1 if loc_y_by_bin else 0, f(loc_bin_size),
                                              f(loc_bin_size / 2), f(loc_scope), f(loc_y_bin_size), f(loc_y_bin_size / 2), f(loc_y_scope),
                                              f(angle_per_class), f(angle_per_class / 2), f(math.pi / 4), f(h), f(w), f(l), E._ptr(boxes),
                                              E._ptr(bev), E._ptr(score), E._stream_ptr(roi.device))
        _lib.check(st, "drc_rcnn_decode_boxes")
    return boxes, bev, score

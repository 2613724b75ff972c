"""fp64 CPU oracle (test infrastructure) for the last two steps of the disparity path: the soft-argmin head and the post-processing
(per-ROI disparities -> full-image disparity / depth maps, DisparityMap.resize).

Restated from the reference's arithmetic, not from the kernels':
  upsample_softargmin  stackhourglass.py:169-173, submodule.py:51-57 -- oracle/psmnet_oracle.upsample_softargmin, which keeps the dtype
  roi_patch            utils/stereo_utils.py:219-229 (expand_box_to_integer), structures/disparity.py:38-77 (resize, crop),
                       modeling/psmnet/inference.py:18-47: F.interpolate(bilinear, align_corners=True) to (y2-y1) x max(x2-x1, x2p-x1p),
                       times dst_w / S, cropped to the left width, plus x1 - x1p
  disparity_map        the same file, with the clamp at 0 and the masks of modeling/detector/disprcnn3d.py:161-190; max over the stack
  roi_depth_maps       pointnet_module/point_rcnn/lib/net/point_rcnn.py:121-133: fuxb / (disparity + 1e-6) inside the box
  disparity_resize     structures/disparity.py:39-62, both modes
oracle/post_oracle.py is the same chain with the reference's `.float()`; every function here takes a `dtype` so that the fp32 chain
(the e32 of the tolerance rule) and the fp64 result come from one piece of code.

The tolerance rule of tests/test_hip_rpn.py and tests/test_hip_s16.py: err <= 2 * e32 + 1e-6 * max|ref|, e32 being the error of the fp32
reference chain on the CPU against fp64 on the same inputs (`e32_bound`).
"""
import math

import torch
import torch.nn.functional as F

from oracle import psmnet_oracle

F64 = torch.float64


def e32_bound(ref64, ref32):
    """-> (bound, e32): 2 * max|ref32 - ref64| + 1e-6 * max|ref64|."""
    ref64 = ref64.double()
    e32 = (ref32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    m = ref64.abs().max().item() if ref64.numel() else 0.0
    return 2.0 * e32 + 1e-6 * m, e32


def upsample_softargmin(cost, maxdisp, mindisp, H, W, dtype=F64):
    """cost [N,D',H',W'] (or [N,1,D',H',W']) -> [N,H,W]: trilinear(align_corners=True), softmax over D, sum d * p."""
    if cost.dim() == 4:
        cost = cost[:, None]
    return psmnet_oracle.upsample_softargmin(cost.to(dtype), maxdisp, mindisp, H, W)


def expand_box_to_integer(box):
    x1, y1, x2, y2 = box
    return math.floor(x1), math.floor(y1), math.ceil(x2), math.ceil(y2)


def bilinear_align_corners(d, oh, ow):
    """[IH,IW] -> [oh,ow] with F.interpolate's align_corners=True rule written out: source coordinate = dst * (in-1)/(out-1), blend of the
    four neighbours.  In the dtype of `d`; the self-test holds F.interpolate in fp64 to it."""
    ih, iw = d.shape
    def axis(n_in, n_out):
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        f = torch.arange(n_out, dtype=d.dtype) * scale
        i0 = f.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        return i0, i1, f - i0.to(d.dtype)
    y0, y1, ty = axis(ih, oh)
    x0, x1, tx = axis(iw, ow)
    top = d[y0][:, x0] * (1 - tx) + d[y0][:, x1] * tx
    bot = d[y1][:, x0] * (1 - tx) + d[y1][:, x1] * tx
    return top * (1 - ty)[:, None] + bot * ty[:, None]


def roi_patch(left_box, right_box, disp_roi, dtype=F64):
    """-> (x1, y1, x2, y2), patch [y2-y1, x2-x1] (None for an empty box)."""
    x1, y1, x2, y2 = expand_box_to_integer(left_box)
    x1p, _, x2p, _ = expand_box_to_integer((right_box[0], left_box[1], right_box[2], left_box[3]))
    if x2 <= x1 or y2 <= y1:
        return (x1, y1, x2, y2), None
    dst_w, dst_h = max(x2 - x1, x2p - x1p), y2 - y1
    d = disp_roi.to(dtype)
    t = F.interpolate(d[None, None], (dst_h, dst_w), mode="bilinear", align_corners=True)[0, 0]
    t = t / d.shape[1] * dst_w
    return (x1, y1, x2, y2), t[:, :x2 - x1] + x1 - x1p


def disparity_map(left_bbox, right_bbox, disparity_preds, height, width, clamp0=False, masks=None, dtype=F64):
    """left/right_bbox [R,4] xyxy, disparity_preds [R,S,S] -> [height,width]: max over the per-ROI maps (zero outside a box)."""
    if len(left_bbox) == 0:
        return torch.zeros((height, width), dtype=dtype)
    maps = []
    for i, (lb, rb) in enumerate(zip(left_bbox.tolist(), right_bbox.tolist())):
        (x1, y1, x2, y2), patch = roi_patch(lb, rb, disparity_preds[i], dtype)
        m = torch.zeros((height, width), dtype=dtype)
        if patch is not None:
            m[y1:y2, x1:x2] = patch[:max(0, min(y2, height) - y1), :max(0, min(x2, width) - x1)]
        if clamp0:
            m = m.clamp(min=0)
        if masks is not None:
            m = m * masks[i].to(dtype)
        maps.append(m)
    return torch.stack(maps).max(dim=0)[0]


def roi_depth_maps(left_bbox, right_bbox, disparity_preds, height, width, fuxb, dtype=F64, return_disparity=False):
    """One depth map per ROI, fuxb / (disparity + 1e-6) inside the box and zero elsewhere -> [R,height,width] (and, on request, the
    disparities themselves with NaN outside the boxes)."""
    out = torch.zeros((len(left_bbox), height, width), dtype=dtype)
    disp = torch.full((len(left_bbox), height, width), float("nan"), dtype=dtype)
    for i, (lb, rb) in enumerate(zip(left_bbox.tolist(), right_bbox.tolist())):
        (x1, y1, x2, y2), patch = roi_patch(lb, rb, disparity_preds[i], dtype)
        if patch is None:
            continue
        patch = patch[:max(0, min(y2, height) - y1), :max(0, min(x2, width) - x1)]
        out[i, y1:y2, x1:x2] = fuxb / (patch + 1e-6)
        disp[i, y1:y2, x1:x2] = patch
    return (out, disp) if return_disparity else out


def disparity_resize(d, dst_w, dst_h, use_max_pooling=False, dtype=F64):
    """[IH,IW] -> [dst_h,dst_w], values times dst_w / IW.  Bilinear(align_corners=True), or the signed max pooling: adaptive max pooling
    of the positive part minus adaptive max pooling of the negated negative part -- a selection, then ONE / IW * dst_w."""
    x = d.to(dtype)[None, None]
    if use_max_pooling:
        pos, neg = (x > 0).to(dtype), (x < 0).to(dtype)
        t = F.adaptive_max_pool2d(x * pos, (dst_h, dst_w))[0, 0] - F.adaptive_max_pool2d(-x * neg, (dst_h, dst_w))[0, 0]
    else:
        t = F.interpolate(x, (dst_h, dst_w), mode="bilinear", align_corners=True)[0, 0]
    return t / d.shape[1] * dst_w

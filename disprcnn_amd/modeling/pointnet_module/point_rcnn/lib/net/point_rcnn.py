"""PointRCNN: the 3D stage of Disp R-CNN (reference: point_rcnn/lib/net/point_rcnn.py), evaluation forward (`_forward_val`) on HIP.

2D results with per-ROI disparities and masks -> remove_empty_proposals -> InstancePointCloud (modeling/pointcloud.py) -> RPN ->
the RPN's clouds and proposals moved back to the camera frame (un-centred, rotated back; the proposals through their corners, as the
reference does) -> RCNNNet.refine -> the fields `box3d` ('ry_lhwxyz'), `scores_3d` and `random` on the left results, one box per
instance.  Without an instance the fields are empty (`random` too, which the reference omits there); with RCNN.ENABLED = False the best RPN proposal of each instance is returned
(`box3d` in 'xyzhwl_ry', `scores_3d`).  The reference writes that branch's fields to the first image only; here they are split over
the images as the RCNN branch's are, which is the same for its one-image batches.

The frame change between the networks is one kernel (`proposals_to_camera`; its torch composition is kept as
`proposals_to_camera_unfused`, the comparator).  From the RPN's output to the end of `refine` nothing reads the device; the fields are
then packed on the device and brought to the host in one copy (the reference's fields are CPU tensors too).

The state-dict keys are the reference's (`rpn.*`, `rcnn_net.*`).  No training forward.
"""
import torch
import torch.nn as nn

from disprcnn_amd.layers.pointrcnn_loss import rpn_point_labels
from disprcnn_amd.layers.rpn_proposals import points_depth, rpn_to_camera
from disprcnn_amd.modeling.pointcloud import InstancePointCloud
from disprcnn_amd.structures.bounding_box_3d import Box3DList

from .rcnn_net import RCNNNet
from .rpn import RPN


def remove_empty_proposals(left_results, right_results):
    """Drop the pairs whose left or right box is not more than a pixel wide and high."""
    ret_left, ret_right = [], []
    for lr, rr in zip(left_results, right_results):
        keep = (lr.bbox[:, 2] > lr.bbox[:, 0] + 1) & (lr.bbox[:, 3] > lr.bbox[:, 1] + 1) & \
               (rr.bbox[:, 2] > rr.bbox[:, 0] + 1) & (rr.bbox[:, 3] > rr.bbox[:, 1] + 1)
        ret_left.append(lr[keep])
        ret_right.append(rr[keep])
    return ret_left, ret_right


def _attach(left_results, fields):
    """fields: {name: (R, ...) tensor over all instances} -> split over the images in order"""
    counts = [len(a) for a in left_results]
    for name, (value, wrap) in fields.items():
        for lr, v in zip(left_results, torch.split(value, counts)):
            lr.add_field(name, wrap(v, lr) if wrap else v)
    return left_results


def _to_host_once(*tensors):
    """Device tensors -> CPU tensors of the same dtypes, shapes and values through ONE device-to-host copy: their bytes are packed on the
    device, widest element first so that every part starts at a multiple of its element size."""
    if not any(t.is_cuda for t in tensors):
        return tuple(t.cpu() for t in tensors)
    order = sorted(range(len(tensors)), key=lambda i: -tensors[i].element_size())
    host = torch.cat([tensors[i].contiguous().view(-1).view(torch.uint8) for i in order]).cpu()
    out, off = [None] * len(tensors), 0
    for i in order:
        n = tensors[i].numel() * tensors[i].element_size()
        # a host copy of its own per tensor: torch.save refuses tensors of different dtypes that share one storage
        out[i] = host[off:off + n].view(tensors[i].dtype).view(tensors[i].shape).clone()
        off += n
    return tuple(out)


def combine_2d_3d(left_results, box, score, random):
    """box (R,7) 'ry_lhwxyz', score (R), random (R) of every instance in order -> fields on the left results (CPU tensors)."""
    box, score, random = _to_host_once(box, score, random)
    return _attach(left_results, {"box3d": (box, lambda v, lr: Box3DList(v, size=lr.size, mode="ry_lhwxyz")),
                                  "scores_3d": (score, None), "random": (random, None)})


def proposals_to_camera_unfused(rpn_proposals, pts_mean, rot_angle):
    """PointRCNN.proposals_to_camera as a composition of torch ops (a few dozen small launches): the comparator of the kernel in the tests
    and in tools/bench_det3d.py.  Nothing in the product calls it."""
    back = lambda p: InstancePointCloud.rotate_back(p + pts_mean[:, None, :], rot_angle)
    out = dict(rpn_proposals)
    out["backbone_xyz"] = back(rpn_proposals["backbone_xyz"])
    out["pts_depth"] = points_depth(out["backbone_xyz"])
    out["rpn_xyz"] = back(rpn_proposals["rpn_xyz"])
    B = pts_mean.shape[0]
    corners = Box3DList(rpn_proposals["roi_boxes3d"].reshape(-1, 7), (1, 1), "xyzhwl_ry").convert("corners").bbox_3d
    out["roi_boxes3d"] = Box3DList(back(corners.view(B, -1, 3)).contiguous(), (1, 1), "corners").convert("xyzhwl_ry").bbox_3d.view(B, -1, 7)
    return out


def generate_rpn_training_labels(pts, targets):
    """The RPN's per-point training labels: pts (B,N,3) and, per cloud, a BoxList whose `box3d` field holds its one ground-truth box
    -> cls_label (B,N): 1 inside the box, -1 inside only the box enlarged by 0.2 (ignored), else 0; reg_label (B,N,7): centre - p (the
    centre at half height), h, w, l, ry on the inside points, zero elsewhere.  The boxes go through Box3DList as the reference's do; the
    inside tests and the labels of all clouds are one kernel (layers/pointrcnn_loss.py:rpn_point_labels)."""
    box3d = [target.get_field('box3d') for target in targets]
    gt_boxes3d = torch.cat([b.convert('xyzhwl_ry').bbox_3d for b in box3d])
    gt_corners = torch.cat([b.convert('corners').bbox_3d.view(-1, 8, 3) for b in box3d])
    extend_box_corners = torch.cat([b.enlarge_box3d(0.2).convert('corners').bbox_3d.view(-1, 8, 3) for b in box3d])
    dev = pts.device
    return rpn_point_labels(pts, gt_boxes3d.to(dev), gt_corners.to(dev), extend_box_corners.to(dev))


class PointRCNN(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.total_cfg = cfg
        self.cfg = cfg.MODEL.POINTRCNN
        if not self.cfg.RPN.ENABLED:
            raise NotImplementedError("PointRCNN without its RPN: the RCNN stage reads the RPN's outputs")
        self.rpn = RPN(self.cfg, self.total_cfg)
        if self.cfg.RCNN.ENABLED:
            self.rcnn_net = RCNNNet(self.cfg, self.total_cfg)
        self.pointcloud = InstancePointCloud(npoints=self.cfg.RPN.NPOINTS, mask_threshold=0.5, mask_padding=1)    # _forward_val's Masker

    def proposals_to_camera(self, rpn_proposals, pts_mean, rot_angle):
        """The RPN's dict in the centred, rotated frame of its clouds -> the same dict in the camera frame (point_rcnn.py:296-312), one
        kernel (layers/rpn_proposals.py:rpn_to_camera).  The input dict is left alone; what is not moved is passed through."""
        out = dict(rpn_proposals)
        backbone, rpn, rois = rpn_proposals["backbone_xyz"], rpn_proposals["rpn_xyz"], rpn_proposals["roi_boxes3d"]
        out["backbone_xyz"], out["pts_depth"], out["roi_boxes3d"] = rpn_to_camera(backbone, rois, pts_mean, rot_angle)
        if rpn is backbone:                             # the RPN returns one tensor under both names
            out["rpn_xyz"] = out["backbone_xyz"]
        else:
            out["rpn_xyz"] = rpn_to_camera(rpn, rois[:, :0], pts_mean, rot_angle)[0]
        return out

    def _forward_val(self, left_results, right_results, targets):
        if targets is None:
            raise ValueError("PointRCNN: the evaluation forward needs `targets`: one BoxList with a 'calib' field (or one calibration) per image")
        left_results, right_results = remove_empty_proposals(left_results, right_results)
        calibs = [t.get_field("calib") if hasattr(t, "get_field") else t for t in targets]
        pts_input, pts_mean, rot_angle = self.pointcloud(left_results, right_results, calibs)
        if pts_input.numel() == 0:
            for lr in left_results:
                lr.add_field("box3d", Box3DList(torch.empty((0, 7)), size=lr.size, mode="ry_lhwxyz"))
                lr.add_field("scores_3d", torch.empty((0,)))
                if hasattr(self, "rcnn_net"):                      # the reference leaves this one out; consumers of the RCNN branch read it
                    lr.add_field("random", torch.empty((0,), dtype=torch.int64))
            return left_results, right_results, {}
        with torch.no_grad():
            rpn_proposals, _ = self.rpn(pts_input)
            if hasattr(self, "rcnn_net"):
                box, score, random = self.rcnn_net.refine(self.proposals_to_camera(rpn_proposals, pts_mean, rot_angle))
                left_results = combine_2d_3d(left_results, box, score, random)
            else:
                box3d = rpn_proposals["roi_boxes3d"].clone()
                B = box3d.shape[0]
                box3d[:, :, 0:3] = box3d[:, :, 0:3] + pts_mean[:, None, :]
                corners = Box3DList(box3d.reshape(-1, 7), (1, 1), "xyzhwl_ry").convert("corners").bbox_3d.view(B, -1, 3)
                corners = InstancePointCloud.rotate_back(corners, rot_angle).view(B, -1, 24)
                score_3d = rpn_proposals["roi_scores_raw"]
                idx = score_3d.argmax(dim=1)
                best = torch.gather(corners, 1, idx.view(B, 1, 1).expand(B, 1, 24))[:, 0]
                boxes = Box3DList(best, (1, 1), "corners").convert("xyzhwl_ry").bbox_3d
                scores = torch.gather(score_3d, 1, idx.view(B, 1))[:, 0].cpu()
                left_results = _attach(left_results, {"box3d": (boxes, lambda v, lr: Box3DList(v, (1, 1), "xyzhwl_ry")),
                                                      "scores_3d": (scores, None)})
        return left_results, right_results, {}

    def forward(self, left_inputs, right_inputs, targets=None):
        if self.training:
            raise NotImplementedError("PointRCNN: only the evaluation forward is implemented (no loss, no backward); call .eval()")
        return self._forward_val(left_inputs, right_inputs, targets)

"""PointRCNN: the 3D stage of Disp R-CNN (reference: point_rcnn/lib/net/point_rcnn.py) on HIP: the evaluation forward (`_forward_val`)
and the training forward (`_forward_train`).

2D results with per-ROI disparities and masks -> remove_empty_proposals -> InstancePointCloud (modeling/pointcloud.py) -> RPN ->
the RPN's clouds and proposals moved back to the camera frame (un-centred, rotated back; the proposals through their corners, as the
reference does) -> RCNNNet.refine -> the fields `box3d` ('ry_lhwxyz'), `scores_3d` and `random` on the left results, one box per
instance.  Without an instance the fields are empty (`random` too, which the reference omits there); with RCNN.ENABLED = False the best RPN proposal of each instance is returned
(`box3d` in 'xyzhwl_ry', `scores_3d`).  The reference writes that branch's fields to the first image only; here they are split over
the images as the RCNN branch's are, which is the same for its one-image batches.

The frame change between the networks is one kernel (`proposals_to_camera`; its torch composition is kept as
`proposals_to_camera_unfused`, the comparator).  From the RPN's output to the end of `refine` nothing reads the device; the fields are
then packed on the device and brought to the host in one copy (the reference's fields are CPU tensors too).

Training (reference :97-187, :244-284).  `process_input` turns the 2D results and the ground truth into the RPN's training input:
remove_empty_proposals, remove_too_right_proposals, the training clouds (InstancePointCloud.train_clouds: MASK_THRESH, no lower depth
clamp, draws from `rng`, scale / flip augmentation unless RPN.FIXED), the 2D matching of every left proposal to the ground truths of its
image (one kernel, layers/match2d.py; its indices reach the host in the same copy as the point counts, the step's only host read up to
the networks), the matched boxes scaled and flipped, their corners moved into the cloud frame (camera_to_rpn, the twin of the
frame-change kernel) and the per-point labels.  An image without ground truth contributes no cloud (the reference skips it and then
fails on the shape mismatch); calibrations are paired by image, as in evaluation.
  RPN not FIXED, RCNN disabled or RCNN.TRAIN false (rpn.yaml): the return is the RPN's training forward on that input.
  RPN FIXED, RCNN enabled and RCNN.TRAIN (rcnn.yaml): the RPN runs its evaluation forward under no_grad (it is put in eval mode, as the
    reference does), its dict and the targets' corners go back to the camera frame, unmatched clouds are dropped
    (filter_unmatched_idxs, on the host copy of the indices) and RCNNNet's training step gives {'loss_box3d'}.  The reference rotates
    back only matched_targets[0], with the means of all images -- the same thing for its one-image batches; here every image's are.
  RPN not FIXED with the RCNN training: the reference fails with a KeyError (the RPN's training dict has no proposals); here
    NotImplementedError.
  No cloud left: the config's loss keys as zeros that still reach every parameter of the stage that trains, so data-parallel ranks never
    skip a step (the convention of DispRCNN3D._forward_train).
The points kernels have no backward: no gradient flows from the 3D losses into the disparities.

The state-dict keys are the reference's (`rpn.*`, `rcnn_net.*`).
"""
import numpy as np
import torch
import torch.nn as nn

from disprcnn_amd.layers.match2d import camera_to_rpn, match_targets
from disprcnn_amd.layers.pointrcnn_loss import rpn_point_labels
from disprcnn_amd.layers.rpn_proposals import points_depth, rpn_to_camera
from disprcnn_amd.modeling.pointcloud import InstancePointCloud
from disprcnn_amd.structures.bounding_box import BoxList
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


def remove_too_right_proposals(left_results, right_results):
    """Keep the pairs whose left box starts right of the right box (positive disparity) or at the image border (left x1 == 0)."""
    ret_left, ret_right = [], []
    for lr, rr in zip(left_results, right_results):
        keep = (lr.bbox[:, 0] > rr.bbox[:, 0]) | (lr.bbox[:, 0] == 0)
        ret_left.append(lr[keep])
        ret_right.append(rr[keep])
    return ret_left, ret_right


def _index_target(target, item):
    """A matched-targets BoxList indexed per instance: its tensors and its `box3d`; `calib` is per image."""
    out = BoxList(target.bbox[item].reshape(-1, 4), target.size, target.mode)
    for k in target.fields():
        v = target.get_field(k)
        out.add_field(k, v[item] if torch.is_tensor(v) or isinstance(v, Box3DList) else v)
    return out


def filter_unmatched_idxs(proposals, matched_targets):
    """Drop the clouds whose proposal matched no ground truth (matched_idxs < 0) from every entry of `proposals` and from the targets.
    `matched_idxs` is the host tensor process_input left on the targets, so the device is not read."""
    matched_idxs = torch.cat([t.get_field("matched_idxs") for t in matched_targets]).cpu()
    keep = matched_idxs >= 0
    if bool(keep.all()):
        ret_proposals = dict(proposals)
    else:
        idx = torch.nonzero(keep).squeeze(1)
        ret_proposals = {k: v[idx.to(v.device)] for k, v in proposals.items()}
    ret_targets = [_index_target(t, k) for k, t in zip(torch.split(keep, [len(a) for a in matched_targets]), matched_targets)]
    return ret_proposals, ret_targets


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
        self.masker_threshold = float(getattr(self.cfg, "MASK_THRESH", 0.7))
        self.train_pointcloud = InstancePointCloud(npoints=self.cfg.RPN.NPOINTS, mask_threshold=self.masker_threshold, mask_padding=1)
        heads = getattr(getattr(cfg, "MODEL", None), "ROI_HEADS", None)                  # Matcher(FG, BG, allow_low_quality_matches=False)
        self.fg_iou_threshold = float(getattr(heads, "FG_IOU_THRESHOLD", 0.5))
        self.bg_iou_threshold = float(getattr(heads, "BG_IOU_THRESHOLD", 0.5))
        self.pts_mean = self.rot_angle = None
        self.aug_scale, self.aug_flip = 1.0, False

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

    # ------------------------------------------------------------------ training: reference :87-187
    def process_input(self, left_inputs, right_inputs, targets, rng=None):
        """-> pts (R,NPOINTS,3), cls_label (R,NPOINTS), reg_label (R,NPOINTS,7), matched_targets: per image with ground truth a BoxList of
        its proposals' matched targets with `box3d` ('corners', in the cloud frame), `calib` and `matched_idxs` (a host tensor).  Keeps
        `pts_mean` (R,3) and `rot_angle` (R, fp64, signed) for the way back, and the augmentation drawn as `aug_scale`, `aug_flip`.
        rng: numpy.random (default) or a RandomState."""
        left_inputs, right_inputs = remove_empty_proposals(left_inputs, right_inputs)
        left_inputs, right_inputs = remove_too_right_proposals(left_inputs, right_inputs)
        kept = [i for i, t in enumerate(targets[:len(left_inputs)]) if len(t) != 0]
        left = [left_inputs[i] for i in kept]
        right = [right_inputs[i] for i in kept]
        tgts = [targets[i] for i in kept]
        counts = [len(a) for a in left]
        R = sum(counts)
        npoints = self.cfg.RPN.NPOINTS
        dev = left[0].bbox.device if left else torch.device("cuda")
        gt3d = [t.get_field("box3d").convert("xyzhwl_ry") for t in tgts]
        if R == 0:
            self.pts_mean = torch.empty(0, 3, device=dev)
            self.rot_angle = torch.empty(0, dtype=torch.float64, device=dev)
            matched_targets = [self._matched_target(t, b, torch.empty(0, dtype=torch.int64), torch.empty(0, 24)) for t, b in zip(tgts, gt3d)]
            return (torch.empty(0, npoints, 3, device=dev), torch.empty(0, npoints, device=dev), torch.empty(0, npoints, 7, device=dev),
                    matched_targets)
        boxes = torch.cat([a.bbox for a in left]).to(dev).float().contiguous()
        gt = torch.cat([t.bbox for t in tgts]).to(dev).float().contiguous()
        gt_rows = torch.cat([b.bbox_3d for b in gt3d]).to(dev).float().contiguous()
        first = np.cumsum([0] + [len(t) for t in tgts])
        span = np.concatenate([np.tile(np.array([[first[i], len(t)]], np.int32), (c, 1)) for i, (t, c) in enumerate(zip(tgts, counts))])
        span = torch.from_numpy(span).pin_memory().to(dev, non_blocking=True)
        rows = []

        def match(view):
            rows.append(match_targets(boxes, span, gt, gt_rows, self.fg_iou_threshold, self.bg_iou_threshold, matched=view)[1])

        calibs = [t.get_field("calib") for t in tgts]
        pts, pts_mean, rot_angle, scale, flip, matched_idxs = self.train_pointcloud.train_clouds(
            left, right, calibs, rng=rng, augment=not self.cfg.RPN.FIXED, tail=R, fill_tail=match)
        self.pts_mean, self.rot_angle, self.aug_scale, self.aug_flip = pts_mean, rot_angle, scale, flip
        # the matched boxes: scaled and flipped as the clouds were, then through their corners into the cloud frame
        box7 = rows[0]
        if scale != 1.0:
            box7 = torch.cat([box7[:, 0:6] * scale, box7[:, 6:7]], dim=1)
        if flip:
            ry = box7[:, 6]
            box7 = torch.cat([-box7[:, 0:1], box7[:, 1:6], (torch.sign(ry) * np.pi - ry)[:, None]], dim=1)
        corners = Box3DList(box7, (1, 1), "xyzhwl_ry").convert("corners").bbox_3d.view(R, 8, 3)
        corners = camera_to_rpn(corners, pts_mean, rot_angle).view(R, 24)
        matched_targets = [self._matched_target(t, b, m, c) for t, b, m, c in
                           zip(tgts, gt3d, torch.split(matched_idxs, counts), torch.split(corners, counts))]
        cls_label, reg_label = generate_rpn_training_labels(pts, matched_targets)
        return pts, cls_label, reg_label, matched_targets

    @staticmethod
    def _matched_target(target, box3d, matched_idxs, corners):
        """target[matched_idxs.clamp(min=0)] with the fields box3d (the given corners), calib and matched_idxs (reference :92-94)."""
        out = BoxList(target.bbox[matched_idxs.clamp(min=0).to(target.bbox.device)].reshape(-1, 4), target.size, target.mode)
        out.add_field("box3d", Box3DList(corners, box3d.size, "corners"))
        out.add_field("calib", target.get_field("calib"))
        out.add_field("matched_idxs", matched_idxs)
        return out

    def targets_to_camera(self, matched_targets, pts_mean, rot_angle):
        """The matched targets' corners from the cloud frame back to the camera frame: the frame-change kernel on (R,8,3) points without
        boxes, for every image (reference :260-264 does it for matched_targets[0] with the means of all images, the same thing for its
        one-image batches).  New BoxLists; the inputs are left alone."""
        counts = [len(t) for t in matched_targets]
        corners = torch.cat([t.get_field("box3d").convert("corners").bbox_3d for t in matched_targets]).view(-1, 8, 3)
        back = rpn_to_camera(corners, corners.new_zeros((corners.shape[0], 0, 7)), pts_mean, rot_angle)[0].view(-1, 24)
        out = []
        for t, c in zip(matched_targets, torch.split(back, counts)):
            n = _index_target(t, slice(None))
            n.add_field("box3d", Box3DList(c, t.get_field("box3d").size, "corners"))
            out.append(n)
        return out

    def _zero_losses(self, rcnn_trains):
        """No cloud on this rank: the step's loss keys as zeros that reach every parameter of the stage that trains."""
        stage = self.rcnn_net if rcnn_trains else self.rpn
        zero = sum(p.sum() for p in stage.parameters() if p.requires_grad) * 0.0
        keys = ("loss_box3d",) if rcnn_trains else ("rpn_loss_cls", "rpn_loss_reg")
        return {k: zero for k in keys}

    def _forward_train(self, left_inputs, right_inputs, targets, rng=None):
        rpn_trains = not self.cfg.RPN.FIXED
        rcnn_trains = bool(self.cfg.RCNN.ENABLED and getattr(self.cfg.RCNN, "TRAIN", True))
        if rpn_trains and rcnn_trains:
            raise NotImplementedError("PointRCNN: training the RPN and the RCNN in one step (RPN.FIXED false with RCNN.ENABLED and RCNN.TRAIN): "
                                      "the RPN's training dict carries no proposals for the RCNN -- the reference fails there with a "
                                      "KeyError; train the RPN first (RCNN.ENABLED or RCNN.TRAIN false), then the RCNN with RPN.FIXED")
        if self.cfg.RPN.FIXED:
            self.rpn.eval()                                  # reference :251-252
        pts_input, rpn_cls_label, rpn_reg_label, matched_targets = self.process_input(left_inputs, right_inputs, targets, rng=rng)
        if rpn_trains:
            if pts_input.shape[0] == 0:
                return {}, self._zero_losses(False)
            return self.rpn(pts_input, rpn_cls_label, rpn_reg_label, matched_targets)
        if pts_input.shape[0] == 0:
            return {}, (self._zero_losses(True) if rcnn_trains else {})
        with torch.no_grad():
            proposals, _ = self.rpn(pts_input)
        if not rcnn_trains:
            return proposals, {}
        proposals = self.proposals_to_camera(proposals, self.pts_mean, self.rot_angle)
        matched_targets = self.targets_to_camera(matched_targets, self.pts_mean, self.rot_angle)
        proposals, matched_targets = filter_unmatched_idxs(proposals, matched_targets)
        if proposals["roi_boxes3d"].shape[0] == 0:
            return {}, self._zero_losses(True)
        return self.rcnn_net(proposals, matched_targets)

    def forward(self, left_inputs, right_inputs, targets=None, rng=None):
        if self.training:
            if targets is None:
                raise ValueError("PointRCNN: in training mode `targets` must not be None")
            return self._forward_train(left_inputs, right_inputs, targets, rng=rng)
        return self._forward_val(left_inputs, right_inputs, targets)

"""The mask head's loss evaluator (reference: modeling/roi_heads/mask_head/loss.py) on HIP.

    make_roi_mask_loss_evaluator(cfg)(proposals, mask_logits, targets) -> loss_mask

proposals: per image the BoxList the mask head ran on (keep_only_positive_boxes of the box head's sample); targets: per image a BoxList
with 'labels' and 'masks', the latter a uint8 [G,H,W] device tensor or an object with such a `.masks` tensor, like the reference's
BinaryMaskList (polygon masks raise: no shipped dataset makes them).  Two steps, nothing read back: the proposals are matched to the
targets again (Matcher(FG, BG), no low-quality matches; the matching kernel of layers/det2d_loss.py), then one workgroup per ROI crops
the matched instance's mask as BinaryMaskList.crop does, resizes it to M x M as torch's CPU bilinear interpolate does, truncates it to
0 / 1 and evaluates binary_cross_entropy_with_logits on the ROI's class plane with its gradient.  Proposals that come out non-positive
drop out on the device; without a positive ROI the loss is 0.  `last_targets` keeps the [P,M,M] targets of the last call.  The flat
module name stands for the reference's `mask_head.loss`: mask_head.py is a module here, not a package.
"""
import torch

from ...layers import det2d_loss as D
from ..matcher import Matcher


def keep_only_positive_boxes(boxes):
    """(reference mask_head.py:14-37) per image the boxes with label > 0, and the masks that selected them"""
    positive_boxes, positive_inds = [], []
    for boxes_per_image in boxes:
        inds_mask = boxes_per_image.get_field("labels") > 0
        positive_boxes.append(boxes_per_image[inds_mask.nonzero().squeeze(1)])
        positive_inds.append(inds_mask)
    return positive_boxes, positive_inds


def _mask_tensor(field):
    t = field if torch.is_tensor(field) else getattr(field, "masks", None)
    if not torch.is_tensor(t):
        raise NotImplementedError("MaskRCNNLossComputation: a uint8 [G,H,W] mask tensor (or an object with one as .masks) is expected; "
                                  "polygon masks are not built")
    return t.to(torch.uint8)


class MaskRCNNLossComputation(object):
    def __init__(self, proposal_matcher, discretization_size):
        if proposal_matcher.allow_low_quality_matches:
            raise NotImplementedError("MaskRCNNLossComputation: the mask head matches without low-quality matches")
        self.proposal_matcher = proposal_matcher
        self.discretization_size = discretization_size
        self.last_targets = None

    def __call__(self, proposals, mask_logits, targets):
        m = self.proposal_matcher
        if mask_logits.shape[-1] != self.discretization_size:
            raise RuntimeError(f"mask_logits of side {mask_logits.shape[-1]} for RESOLUTION {self.discretization_size}")
        dev = mask_logits.device
        boxes = torch.cat([p.bbox for p in proposals], dim=0).to(dev, torch.float32)
        roi_counts = [len(p) for p in proposals]
        gt = torch.cat([t.bbox for t in targets], dim=0).to(dev, torch.float32)
        gt_labels = torch.cat([t.get_field("labels") for t in targets], dim=0).to(dev, torch.int64)
        masks = [_mask_tensor(t.get_field("masks")).to(dev) for t in targets]
        for t, mt in zip(targets, masks):
            if tuple(mt.shape) != (len(t), t.size[1], t.size[0]):
                raise RuntimeError(f"MaskRCNNLossComputation: masks {tuple(mt.shape)} for {len(t)} ground truths of an image of (h, w) = "
                                   f"{(t.size[1], t.size[0])}")
        flat, table, inst_counts = D.pack_masks(masks)
        # an image without a proposal or a ground truth raises ValueError here, as the reference's Matcher does
        matched, _, _ = D.match_label_encode(boxes, roi_counts, gt, gt, inst_counts, m.high_threshold, m.low_threshold, False, gt_labels=gt_labels)
        loss, _, self.last_targets, _ = D.mask_loss(mask_logits, boxes, roi_counts, matched, gt_labels, flat, table, inst_counts)
        return loss


def make_roi_mask_loss_evaluator(cfg):
    matcher = Matcher(cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD, cfg.MODEL.ROI_HEADS.BG_IOU_THRESHOLD, allow_low_quality_matches=False)
    return MaskRCNNLossComputation(matcher, cfg.MODEL.ROI_MASK_HEAD.RESOLUTION)

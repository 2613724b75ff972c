"""The Stereo RPN's loss evaluator (reference: modeling/rpn/stereo_rpn/loss.py) on HIP.

    make_srpn_loss_evaluator(cfg, box_coder)(anchors, objectness, box_regression, left_targets, right_targets, draws=None)
        -> (loss_objectness, loss_rpn_box_reg)

anchors: per image a list of per-level BoxLists with a 'visibility' field (AnchorGenerator's output); `objectness`: the per-level RAW
cls_logits maps [N,2A,H,W], because the HIP head keeps them raw (the reference's head hands over the pair-softmax probabilities; the
kernel applies that softmax itself and differentiates through it); box_regression: the per-level [N,6A,H,W] maps.  Three steps, each one
launch for all images and nothing read back: match + label + encode, the balanced sample (its randomness is the `draws` input, see
layers/det2d_loss.py), and the two losses with their gradients.  A batch with no sampled anchor gives zero losses where the reference
gives NaN.  The flat module name stands for the reference's `stereo_rpn.loss`: stereo_rpn.py is a module here, not a package.
"""
import torch

from ...layers import det2d_loss as D
from ..balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
from ..matcher import Matcher


def generate_rpn_labels(matched_targets):
    return matched_targets.get_field("matched_idxs") >= 0


class SRPNLossComputation(object):
    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder, generate_labels_func):
        if generate_labels_func is not generate_rpn_labels:
            raise NotImplementedError("SRPNLossComputation: only generate_rpn_labels is built into the matching kernel")
        self.proposal_matcher = proposal_matcher
        self.fg_bg_sampler = fg_bg_sampler
        self.box_coder = box_coder
        self.copied_fields = ['original_lr_bbox']
        self.generate_labels_func = generate_labels_func
        self.discard_cases = ['not_visibility', 'between_thresholds']

    def prepare_targets(self, anchors, left_targets, right_targets):
        """-> (matched [R] int64, labels [R] fp32, regression_targets [R,6], per-image anchor counts), the images concatenated."""
        m = self.proposal_matcher
        per_image = [torch.cat([lvl.bbox for lvl in a], dim=0) for a in anchors]
        vis = torch.cat([lvl.get_field("visibility") for a in anchors for lvl in a], dim=0)
        dev = per_image[0].device
        counts = [int(b.shape[0]) for b in per_image]
        gl = torch.cat([t.bbox for t in left_targets], dim=0).to(dev, torch.float32)
        gr = torch.cat([t.bbox for t in right_targets], dim=0).to(dev, torch.float32)
        if [len(t) for t in left_targets] != [len(t) for t in right_targets]:
            raise ValueError("SRPNLossComputation: the two views hold different numbers of ground truths")
        matched, labels, reg = D.match_label_encode(torch.cat(per_image, dim=0), counts, gl, gr, [len(t) for t in left_targets],
                                                    m.high_threshold, m.low_threshold, m.allow_low_quality_matches, self.box_coder.weights,
                                                    visibility=vis.to(dev))
        return matched, labels, reg, counts

    def __call__(self, anchors, objectness, box_regression, left_targets, right_targets, draws=None):
        _, labels, reg, counts = self.prepare_targets(anchors, left_targets, right_targets)
        pos, neg, n_sampled, _ = self.fg_bg_sampler.sample(labels, counts, draws)
        loss_obj, loss_box, _ = D.srpn_loss(objectness, box_regression, pos, neg, reg, n_sampled, beta=1.0 / 9)
        return loss_obj, loss_box


def make_srpn_loss_evaluator(cfg, box_coder):
    matcher = Matcher(cfg.MODEL.RPN.FG_IOU_THRESHOLD, cfg.MODEL.RPN.BG_IOU_THRESHOLD, allow_low_quality_matches=True)
    fg_bg_sampler = BalancedPositiveNegativeSampler(cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE, cfg.MODEL.RPN.POSITIVE_FRACTION)
    return SRPNLossComputation(matcher, fg_bg_sampler, box_coder, generate_rpn_labels)

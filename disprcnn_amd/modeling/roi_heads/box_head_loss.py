"""The stereo box head's loss evaluator (reference: modeling/roi_heads/box_head/loss.py, the double-view branch) on HIP.

    ev = make_roi_box_loss_evaluator(cfg)
    left, right = ev.subsample({'left': [...], 'right': [...]}, {'left': [...], 'right': [...]}, draws=None)
    loss_classifier, loss_box_reg = ev(class_logits, box_regression)

subsample joins each image's two views into 6-coordinate boxes (x1 y1 x2 y2 x1' x2'), matches the proposals to the targets by the union
boxes of expand_left_right_box, labels them, codes the targets' original boxes against the proposals' (..._fromboxes6, BBOX_REG_WEIGHTS)
and draws the balanced sample -- three launches for all images (layers/det2d_loss.py).  It makes ONE host read, of the N sampled counts,
which the returned BoxLists' lengths need.  The sampled lists keep the order nonzero(pos | neg) gives and carry 'labels' and
'regression_targets'; the right list's boxes are (x1', y1, x2', y2) of the joint box, as retrive_left_right_proposals_from_joint makes
them.  The flat module name stands for the reference's `box_head.loss`: box_head.py is a module here, not a package.
"""
import torch

from ...layers import det2d_loss as D
from ..balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
from ..box_coder import BoxCoder
from ..matcher import Matcher


def _joint(left, right):
    return torch.cat((left.bbox, right.bbox[:, [0, 2]]), dim=1)


class FastRCNNLossComputation(object):
    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder, cls_agnostic_bbox_reg=False):
        if cls_agnostic_bbox_reg:
            raise NotImplementedError("CLS_AGNOSTIC_BBOX_REG is off in the shipped configs")
        self.proposal_matcher = proposal_matcher
        self.fg_bg_sampler = fg_bg_sampler
        self.box_coder = box_coder
        self.cls_agnostic_bbox_reg = cls_agnostic_bbox_reg

    def prepare_double_view_targets(self, joint_proposals, joint_targets, target_labels):
        """joint_proposals / joint_targets: per image [P,6] / [G,6]; target_labels: per image [G] -> (matched, labels int64, targets
        [R,6], proposal counts), the images concatenated."""
        m = self.proposal_matcher
        counts = [int(p.shape[0]) for p in joint_proposals]
        cand = torch.cat(joint_proposals, dim=0).to(torch.float32)
        gt = torch.cat(joint_targets, dim=0).to(cand.device, torch.float32)
        gl, gr = gt[:, 0:4], gt[:, [4, 1, 5, 3]]                                   # box6_to_box4s
        gt_labels = torch.cat(list(target_labels), dim=0).to(cand.device, torch.int64)
        matched, labels, reg = D.match_label_encode(cand, counts, gl, gr, [int(g.shape[0]) for g in joint_targets], m.high_threshold,
                                                    m.low_threshold, m.allow_low_quality_matches, self.box_coder.weights, gt_labels=gt_labels)
        return matched, labels, reg, counts

    def subsample(self, proposals, targets, draws=None):
        if not isinstance(proposals, dict):
            raise NotImplementedError("FastRCNNLossComputation.subsample: the single-view form is not used by the stereo box head")
        lp, rp, lt, rt = proposals['left'], proposals['right'], targets['left'], targets['right']
        joint = [_joint(a, b) for a, b in zip(lp, rp)]
        _, labels, reg, counts = self.prepare_double_view_targets(joint, [_joint(a, b) for a, b in zip(lt, rt)],
                                                                  [t.get_field("labels") for t in lt])
        _, _, n_sampled, idx = self.fg_bg_sampler.sample(labels, counts, draws, want_indices=True)
        n_sampled = n_sampled.sum(dim=1).tolist()                                  # the one host read: N counts
        left_out, right_out, all_labels, all_reg, first = [], [], [], [], 0
        for n, (a, j, cnt) in enumerate(zip(lp, joint, n_sampled)):
            keep = idx[n, :cnt]
            lab, tgt, jb = labels[first + keep], reg[first + keep], j[keep]
            left = a[keep]
            left.bbox = jb[:, 0:4]
            left.add_field("labels", lab)
            left.add_field("regression_targets", tgt)
            right = left.copy_with_fields(left.fields())
            right.bbox = jb[:, [4, 1, 5, 3]]
            left_out.append(left)
            right_out.append(right)
            all_labels.append(lab)
            all_reg.append(tgt)
            first += counts[n]
        self._proposals = left_out
        self._labels, self._regression_targets = torch.cat(all_labels, dim=0), torch.cat(all_reg, dim=0)
        return left_out, right_out

    def __call__(self, class_logits, box_regression):
        if not hasattr(self, "_proposals"):
            raise RuntimeError("subsample needs to be called before")
        class_logits = torch.cat(list(class_logits), dim=0) if not torch.is_tensor(class_logits) else class_logits
        box_regression = torch.cat(list(box_regression), dim=0) if not torch.is_tensor(box_regression) else box_regression
        loss_cls, loss_box, _ = D.fastrcnn_loss(class_logits, box_regression, self._labels, self._regression_targets)
        return loss_cls, loss_box


def make_roi_box_loss_evaluator(cfg):
    matcher = Matcher(cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD, cfg.MODEL.ROI_HEADS.BG_IOU_THRESHOLD, allow_low_quality_matches=False)
    box_coder = BoxCoder(weights=cfg.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS)
    fg_bg_sampler = BalancedPositiveNegativeSampler(cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE, cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
    return FastRCNNLossComputation(matcher, fg_bg_sampler, box_coder, cfg.MODEL.CLS_AGNOSTIC_BBOX_REG)

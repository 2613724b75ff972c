"""ProposalTargetLayer of PointRCNN's RCNN stage (reference: point_rcnn/lib/rpn/proposal_target_layer.py) on HIP: the ROIs one training
step of RCNNNet sees, sampled from the RPN's proposals, with their pooled points and labels.  Two kernels, no host read
(layers/proposal_target.py, pts/proposal_target.hip).

    ProposalTargetLayer(cfg, total_cfg)
    forward(input_dict, gt_boxes3d, draws=None, generator=None) -> the reference's dict: sampled_pts (R,S,3), pts_feature (R,S,E+C),
        cls_label (R) int64, reg_valid_mask (R) int64, gt_of_rois (R,7), gt_iou (R), roi_boxes3d (R,7); R = B * ROI_PER_IMAGE
    sample(input_dict, gt_boxes3d, draws=None, generator=None) -> the network's form: xyz (R,S,3), pts (R,3+E,S), feat (R,C,S) in the
        layouts the shared MLPs read, the same labels, plus empty_flag, src_index, n_iter and counts of the sampler

input_dict: roi_boxes3d (B,M,7), rpn_xyz (B,N,3), seg_mask (B,N), pts_depth (B,N) with RCNN.USE_DEPTH, and backbone_features (B,C,N) or
rpn_features (B,N,C), as RCNNNet.pool.  gt_boxes3d (B,N_gt,7 or 8).

Where the reference draws from torch's and numpy's generators in a data-dependent order, this layer reads `draws`
(layers/proposal_target.proposal_draws; one torch.rand call when not given): the same decisions with the same distributions
(DESIGN.md §1).  A cloud without a foreground and without a background candidate, where the reference raises, gets cls_label -1 and
reg_valid_mask 0 on all its slots and counts[b, 4] = 1.  RCNN.REG_AUG_METHOD = 'normal' raises NotImplementedError: the reference's
branch cannot run.  The point-major sampled_pts / pts_feature of `forward` are built only there; RCNNNet uses `sample`.
"""
import torch
import torch.nn as nn

from disprcnn_amd.layers import proposal_target as PT


class ProposalTargetLayer(nn.Module):
    def __init__(self, cfg, total_cfg):
        super().__init__()
        self.cfg = cfg
        self.total_cfg = total_cfg

    def sample(self, input_dict, gt_boxes3d, draws=None, generator=None):
        cfg, rc = self.cfg, self.cfg.RCNN
        if rc.REG_AUG_METHOD == "normal":
            raise NotImplementedError("RCNN.REG_AUG_METHOD = 'normal': the reference's branch calls torch.rand() without a size and cannot run")
        if rc.USE_INTENSITY:
            raise NotImplementedError("RCNN.USE_INTENSITY: the RPN carries no intensity")
        aug_data = bool(getattr(cfg, "AUG_DATA", True))                     # the reference's defaults where a cfg leaves them out
        aug_rot_range = getattr(cfg, "AUG_ROT_RANGE", 18)
        roi_boxes3d = input_dict["roi_boxes3d"]
        B, M = roi_boxes3d.shape[0], roi_boxes3d.shape[1]
        P, T = int(rc.ROI_PER_IMAGE), int(rc.ROI_FG_AUG_TIMES)
        with torch.no_grad():
            if draws is None:
                draws = PT.proposal_draws(B, M, P, T, roi_boxes3d.device, generator=generator)
            sampled = PT.rcnn_sample_rois(roi_boxes3d, gt_boxes3d, draws, P, rc.FG_RATIO, rc.REG_FG_THRESH, rc.CLS_FG_THRESH, rc.CLS_BG_THRESH,
                                          rc.CLS_BG_THRESH_LO, rc.HARD_BG_RATIO, T, rc.REG_AUG_METHOD)
            feats = input_dict.get("backbone_features")
            if feats is None:                              # a dict in the reference's form only
                feats = input_dict["rpn_features"].permute(0, 2, 1)
            out = PT.rcnn_pool_target(input_dict["rpn_xyz"], feats, input_dict["seg_mask"], input_dict["pts_depth"] if rc.USE_DEPTH else None,
                                      sampled, draws if aug_data else None, rc.POOL_EXTRA_WIDTH, rc.REG_FG_THRESH, rc.CLS_FG_THRESH,
                                      rc.CLS_BG_THRESH, sampled_pt_num=rc.NUM_POINTS, aug_data=aug_data, aug_rot_range=aug_rot_range,
                                      num_candidates=M, fg_aug_times=T)
        out["gt_iou"] = sampled["roi_iou"].view(-1)
        out["src_index"], out["n_iter"], out["counts"] = sampled["src_index"], sampled["n_iter"], sampled["counts"]
        return out

    def forward(self, input_dict, gt_boxes3d, draws=None, generator=None):
        s = self.sample(input_dict, gt_boxes3d, draws=draws, generator=generator)
        pts_feature = torch.cat([s["pts"][:, 3:].transpose(1, 2), s["feat"].transpose(1, 2)], dim=2)
        return {"sampled_pts": s["xyz"], "pts_feature": pts_feature, "cls_label": s["cls_label"], "reg_valid_mask": s["reg_valid_mask"],
                "gt_of_rois": s["gt_of_rois"], "gt_iou": s["gt_iou"], "roi_boxes3d": s["roi_boxes3d"]}

"""RPN: the first network of PointRCNN's 3D stage (reference: point_rcnn/lib/net/rpn.py) on HIP.

instance point cloud (B,N,3) -> Pointnet2MSG backbone -> per-point classification and box-regression heads -> ProposalLayer.
The state-dict keys equal the reference's for the same cfg (the Dropout at index 1 of each head keeps the indices), so a reference
checkpoint loads with strict=True.

Training (the reference's _forward_train): forward(pts_input, rpn_cls_label, rpn_reg_label, matched_targets) ->
({'rpn_cls', 'rpn_reg', 'backbone_xyz', 'backbone_features'}, {'rpn_loss_cls', 'rpn_loss_reg'}).  The backbone and the heads run their
training forms (BatchNorm on the statistics of the batch: the RPN opts in with pytorch_utils.enable_bn_training), the heads' Dropout is
torch's, the loss is PointRCNNLossComputation.  matched_targets: one object per image with len() instances and, optionally, the field
'matched_idxs' (default zeros), concatenated to one entry per cloud.  Missing labels and RPN.FIXED raise NotImplementedError.
"""
import math

import torch
import torch.nn as nn

from disprcnn_amd.layers.rpn_proposals import points_depth

from ..pointnet2_lib.pointnet2 import pytorch_utils as pt_utils
from disprcnn_amd.layers import pn2_mlp

from ..rpn.proposal_layer import ProposalLayer
from .pointnet2_msg import Pointnet2MSG
from .rpn_loss import PointRCNNLossComputation


class RPN(nn.Module):
    def __init__(self, cfg, total_cfg=None, use_xyz=True):
        super().__init__()
        self.cfg = cfg
        self.total_cfg = total_cfg
        self.backbone_net = Pointnet2MSG(cfg, input_channels=0, use_xyz=use_xyz)
        rpn = cfg.RPN

        def head(widths, out_channels):
            layers, pre = [], rpn.FP_MLPS[0][-1]
            for w in widths:
                layers.append(pt_utils.Conv1d(pre, w, bn=rpn.USE_BN))
                pre = w
            layers.append(pt_utils.Conv1d(pre, out_channels, activation=None))
            if rpn.DP_RATIO >= 0:
                layers.insert(1, nn.Dropout(rpn.DP_RATIO))
            return nn.Sequential(*layers)

        per_loc_bin_num = int(rpn.LOC_SCOPE / rpn.LOC_BIN_SIZE) * 2
        reg_channel = per_loc_bin_num * (4 if rpn.LOC_XZ_FINE else 2) + rpn.NUM_HEAD_BIN * 2 + 3 + 1
        self.rpn_cls_layer = head(rpn.CLS_FC, 1)
        self.rpn_reg_layer = head(rpn.REG_FC, reg_channel)
        self.proposal_layer = ProposalLayer(cfg, total_cfg)
        try:
            self.loss_evaluator = PointRCNNLossComputation(cfg)
        except NotImplementedError:                        # a LOSS_CLS the eval network accepts: raised again when training starts
            self.loss_evaluator = None
        self.init_weights()
        pt_utils.enable_bn_training(self)

    def init_weights(self):
        if self.cfg.RPN.LOSS_CLS in ["SigmoidFocalLoss"]:
            prior = 0.01                                   # focal loss: start from a 1 % foreground prior
            nn.init.constant_(self.rpn_cls_layer[2].conv.bias, -math.log((1 - prior) / prior))
        nn.init.normal_(self.rpn_reg_layer[-1].conv.weight, mean=0, std=0.001)

    @staticmethod
    def _head(layers, x):
        for layer in layers:
            if not isinstance(layer, nn.Dropout):          # evaluation: dropout is the identity
                x = layer(x)
        return x

    def _forward_train(self, pts_input, rpn_cls_label, rpn_reg_label, matched_targets):
        if rpn_cls_label is None or rpn_reg_label is None or matched_targets is None:
            raise NotImplementedError("RPN: the training forward needs rpn_cls_label, rpn_reg_label and matched_targets "
                                      "(PointRCNN.generate_rpn_training_labels); without them only the evaluation forward runs: call .eval()")
        if self.cfg.RPN.FIXED:
            raise NotImplementedError("RPN.FIXED: a fixed RPN is not trained; call .eval()")
        if self.loss_evaluator is None:
            PointRCNNLossComputation(self.cfg)             # raises with the reason
        with pn2_mlp.batch_counters():
            backbone_xyz, backbone_features = self.backbone_net(pts_input)
            rpn_cls = self.rpn_cls_layer(backbone_features).transpose(1, 2).contiguous()
            rpn_reg = self.rpn_reg_layer(backbone_features).transpose(1, 2).contiguous()
        ret_dict = {"rpn_cls": rpn_cls, "rpn_reg": rpn_reg, "backbone_xyz": backbone_xyz, "backbone_features": backbone_features}
        dev = rpn_cls.device
        matched_idxs = torch.cat([a.get_field("matched_idxs").to(dev) if a.has_field("matched_idxs")
                                  else torch.zeros(len(a), dtype=torch.long, device=dev) for a in matched_targets])
        return ret_dict, self.loss_evaluator(rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label, matched_idxs)

    def forward(self, pts_input, rpn_cls_label=None, rpn_reg_label=None, matched_targets=None):
        if self.training:
            return self._forward_train(pts_input, rpn_cls_label, rpn_reg_label, matched_targets)
        with torch.no_grad():
            backbone_xyz, backbone_features = self.backbone_net(pts_input)                         # (B,N,3), (B,C,N)
            rpn_cls = self._head(self.rpn_cls_layer, backbone_features).transpose(1, 2).contiguous()   # (B,N,1)
            rpn_reg = self._head(self.rpn_reg_layer, backbone_features).transpose(1, 2).contiguous()   # (B,N,R)
            rpn_scores_raw = rpn_cls[:, :, 0]
            seg_mask = (torch.sigmoid(rpn_scores_raw) > self.cfg.RPN.SCORE_THRESH).float()
            pts_depth = points_depth(backbone_xyz)
            rois, roi_scores_raw = self.proposal_layer(rpn_scores_raw, rpn_reg, backbone_xyz)
        ret_dict = {"rpn_cls": rpn_cls, "rpn_reg": rpn_reg, "backbone_xyz": backbone_xyz, "backbone_features": backbone_features,
                    "rpn_xyz": backbone_xyz, "rpn_features": backbone_features.permute((0, 2, 1)), "seg_mask": seg_mask,
                    "roi_boxes3d": rois, "roi_scores_raw": roi_scores_raw, "pts_depth": pts_depth}
        return ret_dict, {}

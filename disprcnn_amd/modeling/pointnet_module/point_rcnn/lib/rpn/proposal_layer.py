"""ProposalLayer of PointRCNN's RPN (reference: point_rcnn/lib/rpn/proposal_layer.py), score-based proposals on HIP.

Two things the reference does are reproduced although they look like accidents: `mode` is always 'TRAIN' (so cfg.TRAIN's
RPN_PRE_NMS_TOP_N / RPN_POST_NMS_TOP_N / RPN_NMS_THRESH are used in evaluation too and cfg.TEST's are never read, except for the
RPN_DISTANCE_BASED_PROPOSE flag), and both top-N values are divided by the batch size.  The NMS is the rotated one whatever
RPN.NMS_TYPE says, as score_based_proposal's.
"""
import torch
import torch.nn as nn

from disprcnn_amd.layers.rpn_proposals import decode_rpn_boxes, propose


class ProposalLayer(nn.Module):
    def __init__(self, cfg, total_cfg=None):
        super().__init__()
        self.cfg = cfg
        self.total_cfg = total_cfg
        self.mode = "TRAIN"
        self.MEAN_SIZE = tuple(float(v) for v in cfg.MEAN_SIZE[0])          # h, w, l

    def forward(self, rpn_scores, rpn_reg, xyz):
        """rpn_scores (B,N), rpn_reg (B,N,R), xyz (B,N,3) -> rois (B,M,7), roi scores (B,M); M = RPN_POST_NMS_TOP_N // B."""
        if self.cfg.TEST.RPN_DISTANCE_BASED_PROPOSE:
            raise NotImplementedError("RPN_DISTANCE_BASED_PROPOSE: only the score-based proposal is implemented")
        rpn = self.cfg.RPN
        batch_size = xyz.shape[0]
        with torch.no_grad():
            boxes, bev = decode_rpn_boxes(xyz, rpn_reg, self.MEAN_SIZE, rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE, rpn.NUM_HEAD_BIN, rpn.LOC_XZ_FINE)
            mode = self.cfg[self.mode]
            return propose(rpn_scores.contiguous(), boxes, bev, mode.RPN_PRE_NMS_TOP_N // batch_size, mode.RPN_POST_NMS_TOP_N // batch_size,
                           mode.RPN_NMS_THRESH)

"""RCNNNet: the second network of PointRCNN's 3D stage (reference: point_rcnn/lib/net/rcnn_net.py) on HIP: the evaluation forward, and
the training step on already sampled ROIs.

RPN output -> per ROI: the points inside the enlarged proposal in its canonical frame ++ mask ++ depth ++ RPN features (one fused
pooling kernel, layers/roipool3d.roipool3d_canonical) -> xyz_up / merge_down shared MLPs -> three single-scale SA levels, the last one
GroupAll -> classification and box-regression heads -> Box3DPointRCNNPostProcess.

The pooled data never takes the reference's point-major [R,S,3+E+C] form: the kernel writes the canonical xyz [R,S,3], the
[R,3+E,S] input of xyz_up and the [R,C,S] RPN features separately, and merge_down reads (xyz_up's output, features) as two inputs, so
the 256-channel concat is not built either.  The heads see one column per ROI and run as one [1,C,R] problem.  Folded, K-major
weights are cached by the parameter holders (pytorch_utils).

The state-dict keys equal the reference's for the same cfg (the Dropout at index 1 of each head keeps the indices), so a reference
checkpoint loads with strict=True.

Training (RCNN.USE_BN = False; a BatchNorm layer in training raises): with RCNN.ROI_SAMPLE_JIT = False `proposals` carries the sampled
ROIs (pts_input, roi_boxes3d, cls_label, reg_valid_mask, gt_boxes3d_ct), the network runs with autograd on the training forms of
layers/pn2_mlp.py (the eval arithmetic with the raw weights, activations in HBM, HIP backward) and the loss is
PointRCNNBox3dLossComputation.  With ROI_SAMPLE_JIT = True (the reference's real step) `targets` carries each cloud's ground-truth box:
ProposalTargetLayer samples, pools and labels the ROIs under no_grad (rpn/proposal_target_layer.py; its random draws may be passed as
proposals['draws'], else they come from torch's default generator), then the same network and loss run on them.  Without `targets` that
path raises NotImplementedError.  The coordinates are constants of the graph (FPS, ball query and the grouped coordinates carry no
gradient).

    forward(proposals) -> (list of BoxList, {})                       evaluation: the reference's interface
    forward(proposals) -> (proposals, {'loss_box3d': loss})           training, ROI_SAMPLE_JIT = False
    forward(proposals, targets) -> (proposals, {'loss_box3d': loss})  training, ROI_SAMPLE_JIT = True
    refine(proposals)  -> (box (B,7) 'ry_lhwxyz', score (B), random (B))    what combine_2d_3d keeps of those lists; no host sync
"""
import torch
import torch.nn as nn

from disprcnn_amd.layers import pn2_mlp
from disprcnn_amd.layers.rcnn_boxes import reg_channels
from disprcnn_amd.layers.roipool3d import roipool3d_canonical

from ..pointnet2_lib.pointnet2 import pytorch_utils as pt_utils
from ..pointnet2_lib.pointnet2.pointnet2_modules import PointnetSAModule
from ..rpn.proposal_target_layer import ProposalTargetLayer
from .rcnn_inference import Box3DPointRCNNPostProcess
from .rcnn_loss import PointRCNNBox3dLossComputation


class RCNNNet(nn.Module):
    def __init__(self, cfg, total_cfg=None, num_classes=2, input_channels=128, use_xyz=True):
        super().__init__()
        self.cfg = cfg
        self.total_cfg = total_cfg
        rcnn = cfg.RCNN
        if num_classes != 2:
            raise NotImplementedError("RCNNNet: one foreground class (num_classes = 2) is supported")
        if rcnn.USE_INTENSITY:
            raise NotImplementedError("RCNN.USE_INTENSITY: the RPN carries no intensity")
        if not rcnn.USE_MASK:
            raise NotImplementedError("RCNN.USE_MASK = False: the reference feeds seg_mask whatever the flag says, so its layers do not fit")
        if rcnn.LOSS_CLS not in ("SigmoidFocalLoss", "BinaryCrossEntropy", "CrossEntropy"):
            raise NotImplementedError(f"RCNN.LOSS_CLS {rcnn.LOSS_CLS!r}")

        self.SA_modules = nn.ModuleList()
        channel_in = input_channels
        if rcnn.USE_RPN_FEATURES:
            self.rcnn_input_channel = 3 + int(rcnn.USE_INTENSITY) + int(rcnn.USE_MASK) + int(rcnn.USE_DEPTH)
            self.xyz_up_layer = pt_utils.SharedMLP([self.rcnn_input_channel] + list(rcnn.XYZ_UP_LAYER), bn=rcnn.USE_BN)
            c_out = rcnn.XYZ_UP_LAYER[-1]
            self.merge_down_layer = pt_utils.SharedMLP([c_out * 2, c_out], bn=rcnn.USE_BN)
        sa = rcnn.SA_CONFIG
        for k in range(len(sa.NPOINTS)):
            mlps = [channel_in] + list(sa.MLPS[k])
            self.SA_modules.append(PointnetSAModule(npoint=sa.NPOINTS[k] if sa.NPOINTS[k] != -1 else None, radius=sa.RADIUS[k],
                                                    nsample=sa.NSAMPLE[k], mlp=mlps, use_xyz=use_xyz, bn=rcnn.USE_BN))
            channel_in = mlps[-1]

        def head(widths, out_channels):
            layers, pre = [], channel_in
            for w in widths:
                layers.append(pt_utils.Conv1d(pre, w, bn=rcnn.USE_BN))
                pre = w
            layers.append(pt_utils.Conv1d(pre, out_channels, activation=None))
            if rcnn.DP_RATIO >= 0:
                layers.insert(1, nn.Dropout(rcnn.DP_RATIO))
            return nn.Sequential(*layers)

        self.cls_layer = head(rcnn.CLS_FC, 1)
        self.reg_layer = head(rcnn.REG_FC, reg_channels(rcnn.LOC_SCOPE, rcnn.LOC_BIN_SIZE, rcnn.NUM_HEAD_BIN, rcnn.LOC_Y_BY_BIN,
                                                        rcnn.LOC_Y_SCOPE, rcnn.LOC_Y_BIN_SIZE))
        self.proposal_target_layer = ProposalTargetLayer(cfg, total_cfg)        # no parameters: the state dict is the reference's
        self.init_weights()
        self.inference = Box3DPointRCNNPostProcess(cfg)
        try:
            self.loss = PointRCNNBox3dLossComputation(cfg)
        except NotImplementedError:                        # a config the eval network accepts (LOSS_CLS = 'CrossEntropy'): raised again
            self.loss = None                               # by the first training forward

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layer[-1].conv.weight, mean=0, std=0.001)

    def _head(self, layers, x):
        for layer in layers:
            if self.training or not isinstance(layer, nn.Dropout):          # evaluation: dropout is the identity
                x = layer(x)
        return x

    def pool(self, proposals):
        """-> xyz (R,S,3), pts (R,3+E,S), feat (R,C,S): the network's input in the layouts its layers read."""
        rcnn = self.cfg.RCNN
        if rcnn.ROI_SAMPLE_JIT:
            feats = proposals.get("backbone_features")
            if feats is None:                              # a dict in the reference's form only
                feats = proposals["rpn_features"].permute(0, 2, 1)
            xyz, pts, feat, _ = roipool3d_canonical(proposals["rpn_xyz"].contiguous(), feats, proposals["seg_mask"],
                                                    proposals["pts_depth"] if rcnn.USE_DEPTH else None, proposals["roi_boxes3d"],
                                                    rcnn.POOL_EXTRA_WIDTH, sampled_pt_num=rcnn.NUM_POINTS)
            return xyz, pts, feat
        pts_input = proposals["pts_input"]                 # (R,S,3+E+C), already pooled and canonical
        n_in = self.rcnn_input_channel if rcnn.USE_RPN_FEATURES else 3
        return (pts_input[..., 0:3].contiguous(), pts_input[..., 0:n_in].transpose(1, 2).contiguous(),
                pts_input[..., n_in:].transpose(1, 2).contiguous())

    def backbone(self, xyz, pts, feat):
        """-> [xyz_up output, merge_down output, SA level outputs ...]; the last one is (R, C, 1)."""
        levels = []
        if self.cfg.RCNN.USE_RPN_FEATURES:
            x = pts
            merge = self.merge_down_layer[0]
            if self.training:
                for layer in self.xyz_up_layer:
                    x = pn2_mlp.pointwise_mlp_train(x, None, *layer.train_layer(), layer.relu)
                features = pn2_mlp.pointwise_mlp_train(x, feat, *merge.train_layer(), merge.relu)
            else:
                for layer in self.xyz_up_layer:
                    x = pn2_mlp.pointwise_mlp(x, None, layer.folded(), None, layer.relu)
                features = pn2_mlp.pointwise_mlp(x, feat, merge.folded(), None, merge.relu)
            levels.append(x)
            levels.append(features)
        else:
            features = feat if feat.shape[1] else None
        for module in self.SA_modules:
            xyz, features = module(xyz, features)
            levels.append(features)
        return levels

    def network(self, proposals, pooled=None):
        """-> {'rcnn_cls': (R,1), 'rcnn_reg': (R, reg channels)}, R = B * M; pooled: (xyz, pts, feat) when ProposalTargetLayer made them"""
        xyz, pts, feat = self.pool(proposals) if pooled is None else pooled
        R = xyz.shape[0]
        if R == 0:
            n_reg = self.reg_layer[-1].conv.weight.shape[0]
            return {"rcnn_cls": xyz.new_zeros((0, 1)), "rcnn_reg": xyz.new_zeros((0, n_reg))}
        last = self.backbone(xyz, pts, feat)[-1]
        cols = last[:, :, 0].t().unsqueeze(0).contiguous()                      # (1, C, R): one column per ROI
        rcnn_cls = self._head(self.cls_layer, cols)[0].t().contiguous()          # (R, 1)
        rcnn_reg = self._head(self.reg_layer, cols)[0].t().contiguous()          # (R, reg channels)
        return {"rcnn_cls": rcnn_cls, "rcnn_reg": rcnn_reg}

    @staticmethod
    def get_box3d_batch(boxlist):
        return torch.cat([t.get_field("box3d").convert("xyzhwl_ry").bbox_3d for t in boxlist])

    def forward(self, proposals, targets=None):
        if self.training:
            if self.cfg.RCNN.ROI_SAMPLE_JIT and targets is None:               # before `proposals` is read
                raise NotImplementedError("RCNNNet: training with RCNN.ROI_SAMPLE_JIT = True samples its ROIs with ProposalTargetLayer, which "
                                          "needs the ground-truth boxes: pass `targets`, or sample the ROIs beforehand (ROI_SAMPLE_JIT = "
                                          "False), or call .eval()")
            if self.loss is None:
                self.loss = PointRCNNBox3dLossComputation(self.cfg)
            pooled = None
            if self.cfg.RCNN.ROI_SAMPLE_JIT:
                with torch.no_grad():
                    gt = self.get_box3d_batch(targets).unsqueeze(1)
                    t = self.proposal_target_layer.sample(proposals, gt, draws=proposals.get("draws"))
                pooled = (t["xyz"], t["pts"], t["feat"])
                # the loss reads pts_input's row count only: the point-major tensor is not built
                target_dict = {"pts_input": t["xyz"], "roi_boxes3d": t["roi_boxes3d"], "cls_label": t["cls_label"],
                               "reg_valid_mask": t["reg_valid_mask"], "gt_of_rois": t["gt_of_rois"]}
            else:
                target_dict = {"pts_input": proposals["pts_input"], "roi_boxes3d": proposals["roi_boxes3d"], "cls_label": proposals["cls_label"],
                               "reg_valid_mask": proposals["reg_valid_mask"], "gt_of_rois": proposals["gt_boxes3d_ct"]}
            with torch.enable_grad():
                ret_dict = self.network(proposals, pooled)
                loss_box3d = self.loss(ret_dict, proposals, target_dict, targets)
            return proposals, dict(loss_box3d=loss_box3d)
        with torch.no_grad():
            ret_dict = self.network(proposals)
            return self.inference(ret_dict, proposals), {}

    def refine(self, proposals):
        """-> (box (B,7) 'ry_lhwxyz', score (B), random (B)): the arg-max entry of each cloud's BoxList, without a host sync."""
        if self.training:
            raise NotImplementedError("RCNNNet.refine: evaluation only; call .eval()")
        with torch.no_grad():
            return self.inference.best(self.network(proposals), proposals)

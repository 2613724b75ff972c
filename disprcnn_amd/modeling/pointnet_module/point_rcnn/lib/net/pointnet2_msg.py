"""Pointnet2MSG: the PointNet++ backbone of PointRCNN's RPN (reference: point_rcnn/lib/net/pointnet2_msg.py).  It trains, with
BatchNorm on the statistics of the batch, once pytorch_utils.enable_bn_training was called on a module above it (the RPN does)."""
import torch.nn as nn

from ..pointnet2_lib.pointnet2.pointnet2_modules import PointnetFPModule, PointnetSAModuleMSG


class Pointnet2MSG(nn.Module):
    def __init__(self, cfg, input_channels=6, use_xyz=True):
        super().__init__()
        sa = cfg.RPN.SA_CONFIG
        self.SA_modules = nn.ModuleList()
        channel_in = input_channels
        skip_channels = [input_channels]
        for k in range(len(sa.NPOINTS)):
            mlps = [[channel_in] + list(m) for m in sa.MLPS[k]]
            channel_out = sum(m[-1] for m in mlps)
            self.SA_modules.append(PointnetSAModuleMSG(npoint=sa.NPOINTS[k], radii=list(sa.RADIUS[k]), nsamples=list(sa.NSAMPLE[k]),
                                                       mlps=mlps, use_xyz=use_xyz, bn=cfg.RPN.USE_BN))
            skip_channels.append(channel_out)
            channel_in = channel_out
        fp = cfg.RPN.FP_MLPS
        self.FP_modules = nn.ModuleList()
        for k in range(len(fp)):
            pre_channel = fp[k + 1][-1] if k + 1 < len(fp) else channel_out
            self.FP_modules.append(PointnetFPModule(mlp=[pre_channel + skip_channels[k]] + list(fp[k])))

    @staticmethod
    def _break_up_pc(pc):
        """(B,N,3+C) -> coordinates (B,N,3) and channel-major features (B,C,N), None when C = 0"""
        extra = pc.size(-1) - 3
        return pc[..., :3].contiguous(), (pc[..., 3:].transpose(1, 2).contiguous() if extra > 0 else None)

    def forward(self, pointcloud, return_levels=False):
        """pointcloud (B,N,3+C) -> xyz (B,N,3), features (B,FP_MLPS[0][-1],N).  return_levels: also the per-level coordinates and
        features (the SA outputs, with the FP outputs written over the levels they refine, as the reference's lists end up)."""
        xyz, features = self._break_up_pc(pointcloud)
        l_xyz, l_features = [xyz], [features]
        sa_features = []
        for sa in self.SA_modules:
            li_xyz, li_features = sa(l_xyz[-1], l_features[-1])
            l_xyz.append(li_xyz)
            l_features.append(li_features)
            sa_features.append(li_features)
        for i in range(-1, -(len(self.FP_modules) + 1), -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])
        if return_levels:
            return l_xyz[0], l_features[0], {"xyz": l_xyz, "sa": sa_features, "fp": l_features[:len(self.FP_modules)]}
        return l_xyz[0], l_features[0]

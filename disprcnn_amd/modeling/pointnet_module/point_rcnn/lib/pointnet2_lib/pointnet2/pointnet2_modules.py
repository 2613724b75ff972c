"""PointNet++ set-abstraction and feature-propagation modules (reference: pointnet2_lib/pointnet2/pointnet2_modules.py) on the HIP
kernels: the index ops of layers/pointnet2.py and the fused shared MLPs of layers/pn2_mlp.py.

An SA module is FPS -> gather -> per scale: ball query -> one fused group / MLP / max kernel that writes its scale's channels into
the module's output, so neither the grouped tensor nor a torch.cat exists.  With npoint=None (GroupAll, the RCNN's last level) the one
neighbourhood is the whole cloud: the same kernel with new_xyz = 0 (x - 0 is exact, so the raw coordinates are fed as GroupAll does),
M = 1 and idx = 0..N-1; the cloud must fit one neighbourhood (N <= 64).  An FP module is three_nn -> weights -> three_interpolate
-> the MLP, whose first layer reads the interpolated and the skip features as two inputs.  FPS and ball query read coordinates only,
so every index equals the reference's.

In training mode an SA module without BatchNorm takes the materialising route (pn2_mlp.sa_mlp_max_train per scale, torch.cat over the
scales) with autograd through the features and the layers' parameters; FPS, gather and ball query stay under no_grad, so the
coordinates are constants of the graph.  A BatchNorm layer in training, and PointnetFPModule in training, raise, unless
pytorch_utils.enable_bn_training was called on a module above them: then each layer is conv -> BatchNorm on the batch statistics -> ReLU
(over all B * npoint * nsample grouped columns of an SA scale, as the reference's BatchNorm2d counts them), and the FP module is
three_nn and the weights under no_grad -> three_interpolate with its backward -> the MLP, whose first layer takes its two inputs.
"""
from typing import List

import torch
import torch.nn as nn

from disprcnn_amd.layers import pn2_mlp
from disprcnn_amd.layers import pointnet2 as pointnet2_utils
from . import pytorch_utils as pt_utils


class PointnetSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping."""

    def __init__(self, *, npoint: int, radii: List[float], nsamples: List[int], mlps: List[List[int]], bn: bool = True,
                 use_xyz: bool = True, pool_method="max_pool", instance_norm=False):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        if pool_method != "max_pool":
            raise NotImplementedError(f"pool_method {pool_method!r}: the fused kernel takes the max over the neighbourhood")
        if instance_norm:
            raise NotImplementedError("instance_norm is not supported by the HIP shared-MLP kernels")
        if not use_xyz:
            raise NotImplementedError("use_xyz=False: the fused kernel always feeds the relative coordinates")
        self.npoint = npoint
        self.pool_method = pool_method
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            spec = list(spec)
            spec[0] += 3
            self.mlps.append(pt_utils.SharedMLP(spec, bn=bn, instance_norm=instance_norm))

    def forward(self, xyz, features=None, new_xyz=None):
        """xyz (B,N,3), features (B,C,N) or None -> new_xyz (B,npoint,3), new_features (B, sum of the scales' widths, npoint)."""
        train = [m.train_layers() for m in self.mlps] if self.training else None          # raises for a BatchNorm layer that is not enabled
        if self.npoint is None:
            return None, self._forward_group_all(xyz, features, train)
        with torch.no_grad():
            if new_xyz is None:
                fps_idx = pointnet2_utils.furthest_point_sample(xyz, self.npoint)
                new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), fps_idx).transpose(1, 2).contiguous()
            if train is not None:
                idxs = [pointnet2_utils.ball_query(g.radius, g.nsample, xyz, new_xyz) for g in self.groupers]
        if train is not None:
            outs = [pn2_mlp.sa_mlp_max_train(xyz, new_xyz, features, idx, layers) for idx, layers in zip(idxs, train)]
            return new_xyz, torch.cat(outs, dim=1)
        with torch.no_grad():
            folded = [m.folded() for m in self.mlps]
            out = torch.empty((xyz.shape[0], sum(f[-1].cout for f in folded), new_xyz.shape[1]), dtype=torch.float32, device=xyz.device)
            c_off = 0
            for grouper, layers in zip(self.groupers, folded):
                idx = pointnet2_utils.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
                pn2_mlp.sa_mlp_max(xyz, new_xyz, features, idx, layers, out=out, c_off=c_off)
                c_off += layers[-1].cout
        return new_xyz, out

    def _forward_group_all(self, xyz, features, train=None):
        """GroupAll: (B,N,3), (B,C,N) -> (B, sum of the widths, 1), the max over all N points of the MLP of raw xyz ++ features."""
        B, N = xyz.shape[0], xyz.shape[1]
        if not 1 <= N <= 64:
            raise NotImplementedError(f"PointnetSAModuleMSG with npoint=None: the fused kernel holds one neighbourhood of at most 64 points, "
                                      f"got {N}")
        with torch.no_grad():
            key = (B, N, xyz.device)
            if getattr(self, "_group_all", (None,))[0] != key:      # constants of the shape: made once, not per call
                self._group_all = (key, torch.zeros((B, 1, 3), dtype=torch.float32, device=xyz.device),
                                   torch.arange(N, dtype=torch.int32, device=xyz.device).view(1, 1, N).expand(B, 1, N).contiguous())
            _, origin, idx = self._group_all
        if train is not None:
            return torch.cat([pn2_mlp.sa_mlp_max_train(xyz, origin, features, idx, layers) for layers in train], dim=1)
        with torch.no_grad():
            folded = [m.folded() for m in self.mlps]
            out = torch.empty((B, sum(f[-1].cout for f in folded), 1), dtype=torch.float32, device=xyz.device)
            c_off = 0
            for layers in folded:
                pn2_mlp.sa_mlp_max(xyz, origin, features, idx, layers, out=out, c_off=c_off)
                c_off += layers[-1].cout
        return out


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction with one scale."""

    def __init__(self, *, mlp: List[int], npoint: int = None, radius: float = None, nsample: int = None, bn: bool = True,
                 use_xyz: bool = True, pool_method="max_pool", instance_norm=False):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz,
                         pool_method=pool_method, instance_norm=instance_norm)


class PointnetFPModule(nn.Module):
    """Feature propagation: three-nearest-neighbour interpolation of the coarser level's features, then a shared MLP."""

    def __init__(self, *, mlp: List[int], bn: bool = True):
        super().__init__()
        self.mlp = pt_utils.SharedMLP(mlp, bn=bn)
        self._bn_train = False                              # set by pytorch_utils.enable_bn_training

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B,n,3), known (B,m,3), unknow_feats (B,C1,n) or None, known_feats (B,C2,m) -> (B, mlp[-1], n)."""
        if self.training:
            if not self._bn_train:
                raise NotImplementedError("PointnetFPModule: the HIP forward is inference only; call .eval()")
            return self._forward_train(unknown, known, unknow_feats, known_feats)
        with torch.no_grad():
            if known is not None:
                dist, idx = pointnet2_utils.three_nn(unknown, known)
                inv = 1.0 / (dist + 1e-8)                      # inverse-distance weights, normalised over the three neighbours
                weight = inv / inv.sum(dim=2, keepdim=True)
                x = pointnet2_utils.three_interpolate(known_feats.contiguous(), idx, weight)
            else:
                x = known_feats.expand(*known_feats.size()[0:2], unknown.size(1)).contiguous()
            skip = unknow_feats
            for layer in self.mlp:
                x = pn2_mlp.pointwise_mlp(x, skip, layer.folded(), None, layer.relu)
                skip = None
        return x

    def _forward_train(self, unknown, known, unknow_feats, known_feats):
        layers = self.mlp.train_layers()
        if known is not None:
            with torch.no_grad():
                dist, idx = pointnet2_utils.three_nn(unknown, known)
                inv = 1.0 / (dist + 1e-8)
                weight = inv / inv.sum(dim=2, keepdim=True)
            x = pointnet2_utils.three_interpolate(known_feats.contiguous(), idx, weight)
        else:
            x = known_feats.expand(*known_feats.size()[0:2], unknown.size(1)).contiguous()
        skip = unknow_feats
        for holder, layer in zip(self.mlp, layers):
            x = pn2_mlp.train_layer_apply(x, skip, layer, holder.relu)
            skip = None
        return x

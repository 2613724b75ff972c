"""Parameter holders of PointRCNN's shared MLPs (reference: pointnet2_lib/pointnet2/pytorch_utils.py).

`SharedMLP`, `Conv1d` and `Conv2d` keep the reference's submodule names (`layer<i>.conv`, `layer<i>.bn.bn`, `conv`, `bn.bn`), so a
reference state dict loads with strict=True.  They do not run torch convolutions: `folded()` gives the layer as the HIP kernels of
layers/pn2_mlp.py read it (BatchNorm folded in fp64 on the host, K-major on the device), cached and made again when a parameter or
buffer changes.  Calling a holder directly does its one layer through `pointwise_mlp`.

In training mode a layer without BatchNorm runs through `pn2_mlp.pointwise_mlp_train` with its raw parameters as autograd inputs (the
eval arithmetic, plus the HIP backward).  A layer with BatchNorm raises, unless `enable_bn_training` has been called on a module above
it: then the layer is conv -> BatchNorm on the statistics of the batch (-> ReLU) through `pn2_mlp.pointwise_bn_train`, which updates
the running statistics.  Batch-stat training is opt-in because only the RPN is trained that way; RCNNNet with USE_BN still refuses.
"""
import torch.nn as nn

from disprcnn_amd.layers import pn2_mlp


class _BNBase(nn.Module):
    def __init__(self, in_size, batch_norm):
        super().__init__()
        self.bn = batch_norm(in_size)


class BatchNorm1d(_BNBase):
    def __init__(self, in_size):
        super().__init__(in_size, nn.BatchNorm1d)


class BatchNorm2d(_BNBase):
    def __init__(self, in_size):
        super().__init__(in_size, nn.BatchNorm2d)


class _ConvBase(nn.Module):
    """1x1 conv (+ BatchNorm) (+ ReLU).  The conv has a bias only without BatchNorm, as the reference's."""

    def __init__(self, conv, batch_norm, in_size, out_size, activation, bn, bias, preact, instance_norm):
        super().__init__()
        if instance_norm:
            raise NotImplementedError("instance_norm is not supported by the HIP shared-MLP kernels")
        if preact:
            raise NotImplementedError("preact layers are not supported by the HIP shared-MLP kernels")
        if not (activation is None or activation == "relu" or isinstance(activation, nn.ReLU)):
            raise NotImplementedError("the HIP shared-MLP kernels apply ReLU or no activation")
        self.conv = conv(in_size, out_size, kernel_size=1, bias=bias and not bn)
        nn.init.kaiming_normal_(self.conv.weight)
        if self.conv.bias is not None:
            nn.init.constant_(self.conv.bias, 0)
        if bn:
            self.bn = batch_norm(out_size)
        self.relu = activation is not None
        self._fold = None
        self._bn_train = False                              # set by enable_bn_training

    def _tensors(self):
        ts = [self.conv.weight, self.conv.bias]
        if hasattr(self, "bn"):
            b = self.bn.bn
            ts += [b.weight, b.bias, b.running_mean, b.running_var]
        return ts

    def folded(self):
        """The layer as a pn2_mlp.Packed on the weight's device; folded again when any tensor of the layer was changed or replaced."""
        key = tuple((t.data_ptr(), t._version, t.device) if t is not None else None for t in self._tensors())
        if self._fold is None or self._fold[0] != key:
            w, cb = self.conv.weight, self.conv.bias
            if hasattr(self, "bn"):
                b = self.bn.bn
                if self.bn.training or b.training:
                    raise NotImplementedError("BatchNorm in training mode: the HIP shared MLPs are inference only")
                wf, bf = pn2_mlp.fold_bn(w, cb, b.weight, b.bias, b.running_mean, b.running_var, b.eps)
            else:
                wf = w.detach().reshape(w.shape[0], -1).float()
                bf = cb.detach().float() if cb is not None else w.new_zeros(w.shape[0])
            self._fold = (key, pn2_mlp.pack(wf.to(w.device), bf.to(w.device)))
        return self._fold[1]

    def train_layer(self):
        """(weight, bias), or (weight, None, bn) for a BatchNorm layer under enable_bn_training: the raw parameters, as the training forms
        of layers/pn2_mlp.py take them.  A BatchNorm layer's fold is dropped: the training kernels write the running statistics through
        raw pointers, which `folded()`'s version check cannot see."""
        if hasattr(self, "bn"):
            if not self._bn_train:
                raise NotImplementedError("BatchNorm in training mode: the HIP shared MLPs train without BatchNorm only (USE_BN = False)")
            self._fold = None
            return self.conv.weight, None, self.bn.bn
        if self.conv.bias is None:
            raise NotImplementedError("a layer without bias in training mode is not supported by the HIP shared-MLP kernels")
        return self.conv.weight, self.conv.bias

    def forward(self, x):
        squeeze = x.dim() == 4
        if squeeze:
            if x.shape[3] != 1:
                raise NotImplementedError("a shared MLP over grouped points runs through layers.pn2_mlp.sa_mlp_max")
            x = x.squeeze(3)
        if self.training:
            y = pn2_mlp.train_layer_apply(x, None, self.train_layer(), self.relu)
        else:
            y = pn2_mlp.pointwise_mlp(x, None, self.folded(), None, self.relu)
        return y.unsqueeze(3) if squeeze else y


class Conv1d(_ConvBase):
    def __init__(self, in_size, out_size, *, activation="relu", bn=False, bias=True, preact=False, instance_norm=False):
        super().__init__(nn.Conv1d, BatchNorm1d, in_size, out_size, activation, bn, bias, preact, instance_norm)


class Conv2d(_ConvBase):
    def __init__(self, in_size, out_size, *, activation="relu", bn=False, bias=True, preact=False, instance_norm=False):
        super().__init__(nn.Conv2d, BatchNorm2d, in_size, out_size, activation, bn, bias, preact, instance_norm)


def enable_bn_training(module):
    """Let every conv holder and every PointnetFPModule below `module` (itself included) train with BatchNorm on batch statistics.
    -> module."""
    for m in module.modules():
        if hasattr(m, "_bn_train"):
            m._bn_train = True
    return module


class SharedMLP(nn.Sequential):
    def __init__(self, args, *, bn=False, activation="relu", preact=False, first=False, name="", instance_norm=False):
        super().__init__()
        for i in range(len(args) - 1):
            self.add_module(name + "layer{}".format(i),
                            Conv2d(args[i], args[i + 1], bn=bn, activation=activation, preact=preact, instance_norm=instance_norm))

    def folded(self):
        return [layer.folded() for layer in self]

    def train_layers(self):
        return [layer.train_layer() for layer in self]

"""build_backbone(cfg) -- drop-in for disprcnn.modeling.backbone.build_backbone (reference backbone/backbone.py:23-45,74-79).

Returns an ``nn.Sequential(OrderedDict(body=ResNet, fpn=FPN))`` subclass with ``.out_channels`` and the reference's
state-dict keys (``body.*``, ``fpn.*``); calling it runs ResNet-FPN on the HIP engine and returns the tuple of 5 maps.  In training
mode it runs only with the body frozen and in eval (``freeze_body()``): the FPN then trains through ``fpn_train``'s autograd Function."""
from collections import OrderedDict

from torch import nn

from .fpn import FPN
from .resnet import ResNet

_REGISTERED = ("R-50-FPN", "R-101-FPN", "R-152-FPN")


class ResNetFPNBackbone(nn.Sequential):
    def __init__(self, arch, res2_out=256, out_channels=256):
        body = ResNet(arch, res2_out=res2_out)
        super().__init__(OrderedDict([("body", body), ("fpn", FPN(body.stage_channels, out_channels))]))
        self.out_channels = out_channels
        self._rt = None
        self._body_frozen = False

    def freeze_body(self):
        """Train the FPN behind a frozen ResNet body (the reference's fix_model pattern, one level down): body.* stops requiring grad,
        body goes to eval and STAYS there through later .train() calls of this module or of a parent.  -> self."""
        self.body.requires_grad_(False)
        self._body_frozen = True
        self.body.eval()
        return self

    def train(self, mode=True):
        super().train(mode)
        if getattr(self, "_body_frozen", False):
            self.body.eval()
        return self

    def forward(self, x):
        from .runtime import BackboneRuntime
        if self.training:
            if self.body.training:
                raise NotImplementedError("training-mode BatchNorm / backward are not built on the HIP engine yet")
            if any(p.requires_grad for p in self.body.parameters()):
                raise NotImplementedError("the ResNet body's backward is not built on the HIP engine yet: the FPN trains behind a frozen body "
                                          "(freeze_body())")
        if self._rt is None or self._rt.device != x.device:
            self._rt = BackboneRuntime(self, x.device)
        if self.training:
            return self._rt.forward_fpn_train(x)
        return self._rt.forward(x)


def build_backbone(cfg):
    name = cfg.MODEL.BACKBONE.CONV_BODY
    if name not in _REGISTERED:
        raise NotImplementedError(f"CONV_BODY {name!r}: only {_REGISTERED} are built on MI355X")
    return ResNetFPNBackbone(name[:-4], getattr(cfg.MODEL.RESNETS, "RES2_OUT_CHANNELS", 256),
                             cfg.MODEL.RESNETS.BACKBONE_OUT_CHANNELS)

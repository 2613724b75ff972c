"""build_backbone(cfg) -- drop-in for disprcnn.modeling.backbone.build_backbone (reference backbone/backbone.py:23-45,74-79).

Returns an ``nn.Sequential(OrderedDict(body=ResNet, fpn=FPN))`` subclass with ``.out_channels`` and the reference's
state-dict keys (``body.*``, ``fpn.*``); calling it runs ResNet-FPN on the HIP engine and returns the tuple of 5 maps.  In training
mode it runs with the body frozen and in eval (``freeze_body()``): the FPN then trains through ``fpn_train``'s autograd Function -- or,
after the opt-in ``enable_body_training(freeze_at)``, with the body in its training form (``body_train``: batch-statistics BatchNorm and
the bottleneck backward).  A trainable body that was not opted in is refused, as before."""
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
        self._body_training = False

    def freeze_body(self):
        """Train the FPN behind a frozen ResNet body (the reference's fix_model pattern, one level down): body.* stops requiring grad,
        body goes to eval and STAYS there through later .train() calls of this module or of a parent.  -> self."""
        self.body.requires_grad_(False)
        self._body_frozen = True
        self._body_training = False
        self.body.eval()
        return self

    def enable_body_training(self, freeze_at=2):
        """Opt in to training the ResNet body on the HIP engine (the reference's _freeze_backbone(FREEZE_CONV_BODY_AT), resnet.py:126-135):
        the stem and layer1..layer{freeze_at - 1} stop requiring grad, the rest of the body requires it, and in training mode forward()
        runs the body with batch-statistics BatchNorm (backbone/body_train.py) -- every BatchNorm whose module is in training mode, the
        frozen stages' included, as in the reference.  Without this call a trainable body is still refused.  freeze_body() undoes it.
        -> self."""
        if freeze_at == 0:
            raise NotImplementedError("enable_body_training(freeze_at=0): the stem's weight gradient (the 7x7 convolution runs as a 4x4 one over "
                                      "the pixel-unshuffled image) and the max-pool adjoint are not built on the HIP engine")
        if freeze_at not in (1, 2, 3, 4, 5):
            raise ValueError("enable_body_training: freeze_at in 1..5")
        self.body.requires_grad_(True)
        self.body.stem.requires_grad_(False)
        for li in range(1, freeze_at):
            getattr(self.body, f"layer{li}").requires_grad_(False)
        self._body_training, self._body_frozen = True, False
        self.body.train(self.training)                                  # (a body frozen earlier was held in eval)
        return self

    def train(self, mode=True):
        super().train(mode)
        if getattr(self, "_body_frozen", False):
            self.body.eval()
        return self

    def forward(self, x):
        from .runtime import BackboneRuntime
        body_training = self.training and getattr(self, "_body_training", False)
        if self.training and not body_training:
            if self.body.training:
                raise NotImplementedError("training-mode BatchNorm / backward are not built on the HIP engine yet")
            if any(p.requires_grad for p in self.body.parameters()):
                raise NotImplementedError("the ResNet body's backward is not built on the HIP engine yet: the FPN trains behind a frozen body "
                                          "(freeze_body())")
        if self._rt is None or self._rt.device != x.device:
            self._rt = BackboneRuntime(self, x.device)
        if body_training:
            return self._rt.forward_body_train(x)
        if self.training:
            return self._rt.forward_fpn_train(x)
        return self._rt.forward(x)


def build_backbone(cfg):
    name = cfg.MODEL.BACKBONE.CONV_BODY
    if name not in _REGISTERED:
        raise NotImplementedError(f"CONV_BODY {name!r}: only {_REGISTERED} are built on MI355X")
    return ResNetFPNBackbone(name[:-4], getattr(cfg.MODEL.RESNETS, "RES2_OUT_CHANNELS", 256),
                             cfg.MODEL.RESNETS.BACKBONE_OUT_CHANNELS)

"""PointRCNNLossComputation: the RPN's training loss (reference: point_rcnn/lib/net/rpn_loss.py) on HIP.

    PointRCNNLossComputation(cfg)(rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label, matched_idxs, tb_dict=None)
        -> {"rpn_loss_cls", "rpn_loss_reg"}        (0-dim fp32 device tensors, differentiable in rpn_cls and rpn_reg)

One reduction for the classification loss and one for the regression loss, each with one gradient kernel; the reference's foreground
selection `[fg_mask]` and its `matched_idxs >= 0` masks are masks the kernels read, so nothing is compacted and nothing is read back.
With no foreground point the regression loss is a zero whose gradient into rpn_reg is a zero tensor (the reference's is
`rpn_loss_cls * 0`, which reaches rpn_cls instead).

tb_dict: the reference fills its `tb_dict={}` default on every call, each entry a host synchronisation.  Here the terms always stay on
the device as `last_terms` (names in TERM_NAMES) and are copied to the host, in one copy, only when the caller passes a dict.
BinaryCrossEntropy is evaluated from the logit (see layers/pointrcnn_loss.py and DESIGN.md): no clamp at 100 with a dead gradient.
"""
import torch

from disprcnn_amd.layers.pointrcnn_loss import bin_reg_loss, point_cls_loss


class PointRCNNLossComputation(object):
    TERM_NAMES = ("rpn_loss_cls", "rpn_loss_reg", "rpn_loss", "rpn_fg_sum", "rpn_loss_loc", "rpn_loss_angle", "rpn_loss_size",
                  "rpn_loss_cls_pos", "rpn_loss_cls_neg")

    def __init__(self, cfg):
        self.cfg = cfg
        self.MEAN_SIZE = tuple(float(v) for v in cfg.MEAN_SIZE[0])          # h, w, l
        if cfg.RPN.LOSS_CLS not in ("DiceLoss", "SigmoidFocalLoss", "BinaryCrossEntropy"):
            raise NotImplementedError(f"RPN.LOSS_CLS = {cfg.RPN.LOSS_CLS!r}")
        self._anchor = {}
        self.last_terms = None

    def _mean_size(self, device):
        if device not in self._anchor:
            self._anchor[device] = torch.tensor(self.MEAN_SIZE, dtype=torch.float32, device=device)
        return self._anchor[device]

    def __call__(self, rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label, matched_idxs, tb_dict=None):
        rpn = self.cfg.RPN
        matched = (matched_idxs >= 0).unsqueeze(-1).repeat(1, rpn.NPOINTS).view(-1)
        labels = rpn_cls_label.reshape(-1)
        kind = rpn.LOSS_CLS
        if kind == "DiceLoss":                     # the reference applies no matched mask here
            loss_cls, cls_terms = point_cls_loss(kind, rpn_cls, labels)
        elif kind == "SigmoidFocalLoss":
            loss_cls, cls_terms = point_cls_loss(kind, rpn_cls, labels, matched, alpha=rpn.FOCAL_ALPHA[0], gamma=rpn.FOCAL_GAMMA)
        else:
            loss_cls, cls_terms = point_cls_loss(kind, rpn_cls, labels, matched, fg_weight=rpn.FG_WEIGHT)
        point_num = rpn_reg.size(0) * rpn_reg.size(1)
        loss_loc, loss_angle, loss_size, reg_terms = bin_reg_loss(
            rpn_reg.reshape(point_num, -1), rpn_reg_label.reshape(point_num, 7), labels > 0, rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE,
            rpn.NUM_HEAD_BIN, self._mean_size(rpn_reg.device), get_xz_fine=rpn.LOC_XZ_FINE, get_y_by_bin=False, get_ry_fine=False,
            loss_mask=matched)
        loss_size = 3 * loss_size  # consistent with old codes
        rpn_loss_reg = loss_loc + loss_angle + loss_size
        rpn_loss_cls = loss_cls * rpn.LOSS_WEIGHT[0]
        rpn_loss_reg = rpn_loss_reg * rpn.LOSS_WEIGHT[1]
        with torch.no_grad():
            self.last_terms = torch.stack([rpn_loss_cls, rpn_loss_reg, rpn_loss_cls + rpn_loss_reg, reg_terms[12], loss_loc, loss_angle,
                                           loss_size, cls_terms[1], cls_terms[2]])
        if tb_dict is not None:
            v = dict(zip(self.TERM_NAMES, self.last_terms.tolist()))
            v["rpn_fg_sum"] = int(v["rpn_fg_sum"])
            if kind != "SigmoidFocalLoss":
                del v["rpn_loss_cls_pos"], v["rpn_loss_cls_neg"]
            tb_dict.update(v)
        return {"rpn_loss_cls": rpn_loss_cls, "rpn_loss_reg": rpn_loss_reg}

"""DiceLoss, SigmoidFocalClassificationLoss and get_reg_loss under the reference's names (point_rcnn/lib/utils/loss_utils.py), on the HIP
kernels of layers/pointrcnn_loss.py.

The loss evaluators (net/rpn_loss.py, net/rcnn_loss.py) do not go through these: they call the fused reductions with all rows and a
selection mask.  These are for callers that hold the reference's calling convention:
    DiceLoss(ignore_target)(input, target)                       -> 0-dim loss
    SigmoidFocalClassificationLoss(gamma, alpha)(x, t, weights)  -> the UNREDUCED loss, as the reference returns it
    get_reg_loss(pred_reg, reg_label, ...)                       -> (loc_loss, angle_loss, size_loss, reg_loss_dict) over rows the caller
                                                                    has already selected (`pred_reg[fg_mask]`)
One difference: reg_loss_dict's per-term values are 0-dim device tensors, not Python floats; the reference's `.item()` on each of them is
a host synchronisation per term, and float(v) gives the number to whoever wants it.
"""
import torch.nn as nn

from disprcnn_amd.layers.pointrcnn_loss import bin_reg_loss, focal_loss_elementwise, point_cls_loss


class DiceLoss(nn.Module):
    def __init__(self, ignore_target=-1):
        super().__init__()
        self.ignore_target = ignore_target

    def forward(self, input, target):
        """input (N) logits, target (N) in {0, 1, ignore_target} -> 1 - sum min(p, t) / clamp(sum max(p, t), 1)"""
        return point_cls_loss("DiceLoss", input.reshape(-1), target.reshape(-1), ignore_target=self.ignore_target)[0]


class SigmoidFocalClassificationLoss(nn.Module):
    def __init__(self, gamma=2.0, alpha=0.25):
        super().__init__()
        if alpha is None:
            raise NotImplementedError("SigmoidFocalClassificationLoss: alpha = None (no class balancing) is not built")
        self._alpha = alpha
        self._gamma = gamma

    def forward(self, prediction_tensor, target_tensor, weights):
        return focal_loss_elementwise(prediction_tensor, target_tensor, weights, alpha=self._alpha, gamma=self._gamma or 0.0)


def get_reg_loss(pred_reg, reg_label, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True, get_y_by_bin=False,
                 loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False, loss_mask=None):
    """Bin-based 3D box regression loss over pred_reg (N,C), reg_label (N,7) [dx, dy, dz, h, w, l, ry]; anchor_size (3) or (N,3)."""
    loc, angle, size, terms = bin_reg_loss(pred_reg, reg_label, None, loc_scope, loc_bin_size, num_head_bin, anchor_size,
                                           get_xz_fine=get_xz_fine, get_y_by_bin=get_y_by_bin, loc_y_scope=loc_y_scope,
                                           loc_y_bin_size=loc_y_bin_size, get_ry_fine=get_ry_fine, loss_mask=loss_mask)
    d = {"loss_x_bin": terms[0], "loss_z_bin": terms[1]}
    if get_xz_fine:
        d.update(loss_x_res=terms[2], loss_z_res=terms[3])
    if get_y_by_bin:
        d.update(loss_y_bin=terms[4], loss_y_res=terms[5])
    else:
        d["loss_y_offset"] = terms[4]
    d.update(loss_ry_bin=terms[6], loss_ry_res=terms[7], loss_loc=loc, loss_angle=angle, loss_size=size)
    return loc, angle, size, d

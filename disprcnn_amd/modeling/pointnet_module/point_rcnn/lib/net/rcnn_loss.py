"""PointRCNNBox3dLossComputation: the RCNN stage's training loss (reference: point_rcnn/lib/net/rcnn_loss.py) on HIP.

    PointRCNNBox3dLossComputation(cfg)(end_points, proposals, labels, targets, matched_idxs=None, tb_dict=None) -> rcnn_loss (0-dim)

end_points: {'rcnn_cls' (R,1), 'rcnn_reg' (R,C)}; labels: {'cls_label' (R) in {1, 0, -1}, 'reg_valid_mask' (R), 'gt_of_rois' (R,7),
'roi_boxes3d' (R,7), 'pts_input' (R,...)}.  As the reference's: the classification loss takes no loss mask, the regression loss is
get_reg_loss with get_xz_fine and get_ry_fine over the rows with reg_valid_mask > 0 (a row mask here, not a selection), anchored on the
ROI's own size with RCNN.SIZE_RES_ON_ROI, 3 x loss_size.  `proposals`, `targets` and `matched_idxs` are accepted and unused, as there.

LOSS_CLS 'CrossEntropy' raises NotImplementedError: the reference's branch reads a variable it never defines.  BinaryCrossEntropy
expects the hard labels ProposalTargetLayer makes (its target is label > 0) and is evaluated from the logit.
tb_dict as in net/rpn_loss.py: `last_terms` (TERM_NAMES) stays on the device; a dict is filled, with one copy to the host, only when given.
"""
import torch

from disprcnn_amd.layers.pointrcnn_loss import bin_reg_loss, point_cls_loss


class PointRCNNBox3dLossComputation(object):
    TERM_NAMES = ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size", "rpn_loss_cls_pos",
                  "rpn_loss_cls_neg", "rcnn_cls_fg", "rcnn_cls_bg", "rcnn_reg_fg", "loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res",
                  "loss_y_offset|loss_y_bin", "loss_y_res", "loss_ry_bin", "loss_ry_res", "loss_size")

    def __init__(self, cfg):
        self.cfg = cfg
        if cfg.RCNN.LOSS_CLS == "CrossEntropy":
            raise NotImplementedError("RCNN.LOSS_CLS = 'CrossEntropy': the reference's branch reads an undefined cls_valid_mask")
        if cfg.RCNN.LOSS_CLS not in ("SigmoidFocalLoss", "BinaryCrossEntropy"):
            raise NotImplementedError(f"RCNN.LOSS_CLS = {cfg.RCNN.LOSS_CLS!r}")
        self.MEAN_SIZE = tuple(float(v) for v in cfg.MEAN_SIZE[0])          # h, w, l
        self._anchor = {}
        self.last_terms = None

    def _mean_size(self, device):
        if device not in self._anchor:
            self._anchor[device] = torch.tensor(self.MEAN_SIZE, dtype=torch.float32, device=device)
        return self._anchor[device]

    def __call__(self, end_points, proposals, labels, targets, matched_idxs=None, tb_dict=None):
        rc = self.cfg.RCNN
        rcnn_cls, rcnn_reg = end_points["rcnn_cls"], end_points["rcnn_reg"]
        cls_label = labels["cls_label"].float().reshape(-1)
        reg_valid_mask = labels["reg_valid_mask"].reshape(-1)
        roi_boxes3d = labels["roi_boxes3d"]
        batch_size = labels["pts_input"].shape[0]
        if rc.LOSS_CLS == "SigmoidFocalLoss":
            loss_cls, cls_terms = point_cls_loss("SigmoidFocalLoss", rcnn_cls, cls_label, alpha=rc.FOCAL_ALPHA[0], gamma=rc.FOCAL_GAMMA)
        else:
            loss_cls, cls_terms = point_cls_loss("BinaryCrossEntropy", rcnn_cls, cls_label, fg_weight=1.0)
        anchor = roi_boxes3d.reshape(batch_size, 7)[:, 3:6] if rc.SIZE_RES_ON_ROI else self._mean_size(rcnn_reg.device)
        loss_loc, loss_angle, loss_size, reg_terms = bin_reg_loss(
            rcnn_reg.reshape(batch_size, -1), labels["gt_of_rois"].reshape(batch_size, 7), reg_valid_mask > 0, rc.LOC_SCOPE, rc.LOC_BIN_SIZE,
            rc.NUM_HEAD_BIN, anchor, get_xz_fine=True, get_y_by_bin=rc.LOC_Y_BY_BIN, loc_y_scope=rc.LOC_Y_SCOPE,
            loc_y_bin_size=rc.LOC_Y_BIN_SIZE, get_ry_fine=True)
        loss_size = 3 * loss_size  # consistent with old codes
        rcnn_loss_reg = loss_loc + loss_angle + loss_size
        rcnn_loss = loss_cls + rcnn_loss_reg
        with torch.no_grad():
            counts = torch.stack([(cls_label > 0).sum(), (cls_label == 0).sum(), reg_valid_mask.sum()]).float()
            self.last_terms = torch.cat([torch.stack([loss_cls, rcnn_loss_reg, rcnn_loss, loss_loc, loss_angle, loss_size, cls_terms[1],
                                                      cls_terms[2]]), counts, reg_terms[:9]])
        if tb_dict is not None:
            v = dict(zip(self.TERM_NAMES, self.last_terms.tolist()))
            for k in ("rcnn_cls_fg", "rcnn_cls_bg", "rcnn_reg_fg"):
                v[k] = int(v[k])
            if rc.LOSS_CLS != "SigmoidFocalLoss":
                del v["rpn_loss_cls_pos"], v["rpn_loss_cls_neg"]
            y = v.pop("loss_y_offset|loss_y_bin")
            y_res = v.pop("loss_y_res")
            if rc.LOC_Y_BY_BIN:
                v["loss_y_bin"], v["loss_y_res"] = y, y_res
            else:
                v["loss_y_offset"] = y
            if v["rcnn_reg_fg"] == 0:              # the reference reports no regression term without a foreground ROI
                for k in [k for k in v if k.startswith("loss_")]:
                    del v[k]
            else:
                v.update(loss_loc=v["rcnn_loss_loc"], loss_angle=v["rcnn_loss_angle"])
            tb_dict.update(v)
        return rcnn_loss

"""Box3DPointRCNNPostProcess: RCNNNet's outputs -> one BoxList of refined 3D boxes per cloud (reference: point_rcnn/lib/net/
rcnn_inference.py), on HIP.

`__call__` returns the reference's lists: per cloud, the boxes scoring above RCNN.SCORE_THRESH after a rotated NMS at RCNN.NMS_THRESH in
descending raw-score order (fields `box3d` in 'ry_lhwxyz', `box3d_score`, `labels`, `iou_score`, `random` = 0); a cloud without such a
box gets the RPN's best proposal (`roi_scores_raw.argmax()` over all slots, zero padding included) with `box3d_score` 0, `labels` 1 and
`random` = 1.  In that branch the reference sizes the 2D placeholder boxes and `random` by the 7 values of the chosen proposal, so the
BoxList has 7 rows around one 3D box; that is kept.  One decode launch, one batched NMS for all clouds and one host sync to size the
lists (the reference syncs per cloud).

`best` is what `combine_2d_3d` keeps of those lists -- the arg-max box of each cloud -- without the lists, the NMS or a host sync: greedy
NMS always keeps its top-scoring input, so it is the best-scoring box above the threshold or else the fallback.  Ties resolve to the
lower ROI index, as the stable sort in front of the NMS does.
"""
import torch

from disprcnn_amd.layers.iou3d import nms_gpu_batched
from disprcnn_amd.layers.rcnn_boxes import decode_rcnn_boxes
from disprcnn_amd.structures.bounding_box import BoxList
from disprcnn_amd.structures.bounding_box_3d import Box3DList

SIZE = (1280, 720)          # the reference's placeholder image size


class Box3DPointRCNNPostProcess(object):
    def __init__(self, cfg):
        self.cfg = cfg
        if cfg.RCNN.SIZE_RES_ON_ROI:
            raise NotImplementedError("RCNN.SIZE_RES_ON_ROI is not supported (the reference asserts on it)")
        self.MEAN_SIZE = tuple(float(v) for v in cfg.MEAN_SIZE[0])          # h, w, l

    def decode(self, output_dict, proposals):
        """-> roi (B,M,7), boxes (B,M,7), bev (B,M,5), raw (B,M), norm (B,M)"""
        roi = proposals["roi_boxes3d"]
        B, M = roi.shape[0], roi.shape[1]
        rcnn_cls, rcnn_reg = output_dict["rcnn_cls"], output_dict["rcnn_reg"]
        if rcnn_cls.dim() != 2 or rcnn_cls.shape[1] != 1:
            raise NotImplementedError("Box3DPointRCNNPostProcess: one class logit per ROI (num_classes = 2) is supported")
        r = self.cfg.RCNN
        boxes, bev, norm = decode_rcnn_boxes(roi.reshape(-1, 7), rcnn_reg.reshape(B * M, -1), rcnn_cls.reshape(-1), self.MEAN_SIZE, r.LOC_SCOPE,
                                             r.LOC_BIN_SIZE, r.NUM_HEAD_BIN, r.LOC_Y_BY_BIN, r.LOC_Y_SCOPE, r.LOC_Y_BIN_SIZE)
        return roi, boxes.view(B, M, 7), bev.view(B, M, 5), rcnn_cls.reshape(B, M), norm.view(B, M)

    @staticmethod
    def _first_argmax(v):
        """(B,M) -> (B) index of the first maximum of each row"""
        M = v.shape[1]
        pos = torch.arange(M, device=v.device).view(1, M)
        return torch.where(v == v.max(dim=1, keepdim=True)[0], pos, torch.full_like(pos, M)).min(dim=1)[0].clamp(max=M - 1)

    def best(self, output_dict, proposals):
        """-> box (B,7) 'ry_lhwxyz', score (B), random (B) int64: the arg-max entry of each cloud's list.  No host sync."""
        with torch.no_grad():
            roi, boxes, _, raw, norm = self.decode(output_dict, proposals)
            B, M = raw.shape
            dev = raw.device
            if B == 0 or M == 0:
                return torch.empty((0, 7), device=dev), torch.empty((0,), device=dev), torch.empty((0,), dtype=torch.int64, device=dev)
            valid = norm > self.cfg.RCNN.SCORE_THRESH
            any_valid = valid.any(dim=1)
            idx = self._first_argmax(torch.where(valid, raw, torch.full_like(raw, float("-inf"))))
            fb = self._first_argmax(proposals["roi_scores_raw"])
            take = lambda t, i: torch.gather(t, 1, i.view(B, 1, 1).expand(B, 1, 7))[:, 0]
            box = torch.where(any_valid.view(B, 1), take(boxes, idx), take(roi, fb))
            score = torch.where(any_valid, torch.gather(raw, 1, idx.view(B, 1))[:, 0], torch.zeros_like(raw[:, 0]))
            return Box3DList(box, SIZE, "xyzhwl_ry").convert("ry_lhwxyz").bbox_3d, score, (~any_valid).long()

    def __call__(self, output_dict, proposals):
        with torch.no_grad():
            roi, boxes, bev, raw, norm = self.decode(output_dict, proposals)
            B, M = raw.shape
            dev = raw.device
            if B == 0:
                return []
            if M == 0:
                raise RuntimeError("Box3DPointRCNNPostProcess: no ROI slot (M = 0): there is no proposal to fall back to")
            inds = norm > self.cfg.RCNN.SCORE_THRESH
            # the boxes above the threshold first, in index order, as `pred_boxes3d[k, cur_inds]` compacts them
            perm = torch.sort((~inds).to(torch.int8), dim=1, stable=True)[1]
            counts = inds.sum(dim=1)
            cbev = torch.gather(bev, 1, perm.unsqueeze(2).expand(B, M, 5)).contiguous()
            craw = torch.gather(raw, 1, perm).contiguous()
            keep, num = nms_gpu_batched(cbev, craw, counts, float(self.cfg.RCNN.NMS_THRESH))
            orig = torch.gather(perm, 1, keep.clamp(min=0))                                     # ROI index of every kept position
            fb = self._first_argmax(proposals["roi_scores_raw"])
            host = torch.stack([counts, num, fb]).cpu()                                         # the one sync
            results = []
            for k in range(B):
                if int(host[0, k]) == 0:
                    b3d = roi[k][int(host[2, k])]
                    bbox = BoxList(torch.tensor([0, 0, SIZE[0], SIZE[1]], dtype=torch.float32, device=dev).repeat(b3d.shape[0], 1), SIZE,
                                   mode="xyxy")
                    bbox.add_field("box3d", Box3DList(b3d, SIZE, "xyzhwl_ry").convert("ry_lhwxyz"))
                    bbox.add_field("box3d_score", torch.zeros(1, device=dev))
                    bbox.add_field("labels", 1)
                    bbox.add_field("random", torch.ones(len(bbox), dtype=torch.int64, device=dev))
                    results.append(bbox)
                    continue
                sel = orig[k, :int(host[1, k])]
                scores = raw[k, sel]
                bbox = BoxList(torch.tensor([0, 0, SIZE[0], SIZE[1]], dtype=torch.float32, device=dev).repeat(sel.shape[0], 1), SIZE,
                               mode="xyxy")
                bbox.add_field("box3d", Box3DList(boxes[k, sel], SIZE, "xyzhwl_ry").convert("ry_lhwxyz"))
                bbox.add_field("box3d_score", scores)
                bbox.add_field("labels", torch.ones(sel.shape[0], dtype=torch.int64, device=dev))     # every kept box is above the threshold
                bbox.add_field("iou_score", scores)
                bbox.add_field("random", torch.zeros(len(bbox), dtype=torch.int64, device=dev))
                results.append(bbox)
            return results

#!/usr/bin/env python3
"""Golden fixture for PointRCNN's RPN inference, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rpn.py    -> rpn_ref_golden.npz, rpn_cfg_car.json

Reference code exercised (its own Python on torch-CPU): RPN (net/rpn.py) with Pointnet2MSG, the SA / FP modules, pytorch_utils,
pointnet2_utils, ProposalLayer, decode_bbox_target, iou3d_utils.nms_gpu, kitti_utils.boxes3d_to_bev_torch, under the reference's
config defaults with configs/kitti/car/vob/rpn.yaml's POINTRCNN overrides.  Harness-only stand-ins: stubbed yacs / torch._six,
`Tensor.cuda` = identity, torch.cuda.IntTensor / FloatTensor -> CPU tensors, `pointnet2_cuda` served by tests/pn2_oracle.py and
`iou3d_cuda.nms_gpu` by tests/box3d_oracle.nms_sorted.  Only inputs' seeds, settings and recorded outputs are written.

Weights and clouds are not stored: tests/rpn_oracle.py builds both from seeds (random_state, make_batch).  Every run is recorded
twice: from the fp32 module, and from module.double() with dtype-preserving gather / group / interpolate stand-ins (indices still
from the fp32 oracle, so both runs use identical neighbourhoods).  Their difference is the reference's own fp32 rounding error and is
stored per tensor as err32_max_* / err32_mean_* (over both batches): the yardstick of the tests' tolerances.

To stay under the repository's file-size limit the fp64 tensors are stored on recorded subsets of points (`pts_*`), the per-level
outputs for the B = 2 batch only, and the fp32 rpn_reg on the pre-NMS top-N points (`top_*`): the only rows a proposal depends on.

Checked before writing: no IoU the NMS walk compares lies within 1e-4 of the threshold, and no two bins competing in an argmax of a
pre-NMS top-N point lie within 1e-4 of each other; otherwise the weight seed moves on.
"""
import copy
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("DISPRCNN_REFERENCE", "/root/reference"))
sys.dont_write_bytecode = True

from tests import box3d_oracle as BO  # noqa: E402
from tests import pn2_oracle as PO  # noqa: E402
from tests import rpn_oracle as RO  # noqa: E402

for name in ("cv2", "pycocotools", "pycocotools.mask", "roipool3d_cuda", "tensorboardX", "termcolor", "numba", "zarr", "fastai",
             "matplotlib", "matplotlib.pyplot", "dl_ext", "dl_ext.primitive", "dl_ext.vision_ext", "dl_ext.vision_ext.datasets",
             "dl_ext.vision_ext.datasets.kitti", "dl_ext.vision_ext.datasets.kitti.structures", "disprcnn._C", "PIL", "PIL.Image", "tqdm",
             "scipy", "scipy.spatial", "skimage", "shapely", "shapely.geometry"):
    sys.modules.setdefault(name, MagicMock())


class CfgNode(dict):
    def __init__(self, init=None, *a, **k):
        super().__init__(init or {})

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self):
        return copy.deepcopy(self)


yacs, yc = types.ModuleType("yacs"), types.ModuleType("yacs.config")
yc.CfgNode = CfgNode
yacs.config = yc
sys.modules["yacs"], sys.modules["yacs.config"] = yacs, yc
torch._six = types.SimpleNamespace(PY3=True, PY37=True, string_classes=(str,), int_classes=(int,),
                                   container_abcs=__import__("collections").abc)
sys.modules["torch._six"] = torch._six
np.float, np.int, np.bool = float, int, bool
torch.Tensor.cuda = lambda self, *a, **k: self

DTYPE = [torch.float32]                 # the dtype of the run in progress
torch.cuda.FloatTensor = lambda *s: torch.empty(*s, dtype=DTYPE[0])
torch.cuda.IntTensor = lambda *s: torch.empty(*s, dtype=torch.int32)


def _np32(t):
    return t.detach().to(torch.float32).numpy()


def _take(p, idx):
    """p (B,C,N), idx (B,K) -> (B,C,K) in p's dtype"""
    return torch.gather(p, 2, idx.long().unsqueeze(1).expand(-1, p.shape[1], -1))


pn2 = types.ModuleType("pointnet2_cuda")
pn2.furthest_point_sampling_wrapper = lambda B, N, m, xyz, temp, out: out.copy_(torch.from_numpy(PO.fps(_np32(xyz), m)))
pn2.ball_query_wrapper = lambda B, N, m, r, ns, new_xyz, xyz, idx: idx.copy_(torch.from_numpy(PO.ball_query(r, ns, _np32(xyz), _np32(new_xyz))))
pn2.gather_points_wrapper = lambda B, C, N, m, p, idx, out: out.copy_(_take(p, idx))
pn2.group_points_wrapper = lambda B, C, N, m, ns, p, idx, out: out.copy_(_take(p, idx.reshape(B, -1)).reshape(B, C, m, ns))


def _three_nn(B, N, m, unknown, known, dist2, idx):
    d, i = PO.three_nn(_np32(unknown), _np32(known))
    dist2.copy_(torch.from_numpy(d))
    idx.copy_(torch.from_numpy(i))


def _three_interpolate(B, c, m, n, p, idx, w, out):
    out.copy_(w[:, None, :, 0] * _take(p, idx[:, :, 0]) + w[:, None, :, 1] * _take(p, idx[:, :, 1]) + w[:, None, :, 2] * _take(p, idx[:, :, 2]))


pn2.three_nn_wrapper = _three_nn
pn2.three_interpolate_wrapper = _three_interpolate
sys.modules["pointnet2_cuda"] = pn2

iou3d = types.ModuleType("iou3d_cuda")


def _nms_gpu(boxes, keep, thresh):
    k = BO.nms_sorted(_np32(boxes), thresh)
    keep[:len(k)] = torch.from_numpy(k)
    return len(k)


iou3d.nms_gpu = _nms_gpu
sys.modules["iou3d_cuda"] = iou3d

from disprcnn.config import cfg as ref_cfg  # noqa: E402  (the reference)
from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.rpn import RPN  # noqa: E402  (the reference)

CAR = {"MASK_THRESH": 0.5, "AUG_DATA": True, "MEAN_SIZE": [[1.52563191462, 1.62856739989, 3.88311640418]],
       "RPN": {"LOSS_CLS": "BinaryCrossEntropy", "SA_CONFIG": {"NPOINTS": [768, 512, 256, 64]}}}       # configs/kitti/car/vob/rpn.yaml
N_LEVEL_PTS, N_OUT_PTS = 8, 16


def merge(node, over):
    for k, v in over.items():
        if isinstance(v, dict):
            merge(node[k], v)
        else:
            node[k] = v


def plain(node):
    if isinstance(node, dict):
        return {k: plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [plain(v) for v in node]
    return node


def run(model, pts, dtype):
    """-> ret_dict, {'sa<k>': ..., 'fp<k>': ...} from forward hooks, the pre-NMS decoded boxes"""
    DTYPE[0] = dtype
    levels, hooks = {}, []
    for k, m in enumerate(model.backbone_net.SA_modules):
        hooks.append(m.register_forward_hook(lambda mod, i, o, k=k: levels.__setitem__(f"sa{k}", o[1].detach().clone())))
    for k, m in enumerate(model.backbone_net.FP_modules):
        hooks.append(m.register_forward_hook(lambda mod, i, o, k=k: levels.__setitem__(f"fp{k}", o.detach().clone())))
    with torch.no_grad():
        ret, _ = model(torch.from_numpy(pts).to(dtype))
    for h in hooks:
        h.remove()
    return ret, levels


def main():
    pr = ref_cfg.MODEL.POINTRCNN.clone()
    merge(pr, CAR)
    sub = {"RPN": plain(pr.RPN), "MEAN_SIZE": plain(pr.MEAN_SIZE), "TRAIN": plain(pr.TRAIN), "TEST": plain(pr.TEST)}
    cfg = RO.make_cfg(sub)
    model = RPN(pr, ref_cfg).eval()
    keys = list(model.state_dict().keys())
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    rpn = cfg.RPN
    thresh = cfg.TRAIN.RPN_NMS_THRESH

    for wseed in range(1, 50):
        sd = RO.random_state(shapes, wseed)
        out = {"state_dict_keys": np.array(keys), "weight_seed": np.int64(wseed)}
        errs, ok = {}, True
        for tag, (kinds, seed) in RO.BATCHES.items():
            pts = RO.make_batch(kinds, seed)
            B = pts.shape[0]
            model.float().load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            r32, l32 = run(model, pts, torch.float32)
            model.double()
            r64, l64 = run(model, pts, torch.float64)
            assert r32["rpn_reg"].dtype == torch.float32 and r64["rpn_reg"].dtype == torch.float64
            assert r64["backbone_features"].dtype == torch.float64 and all(v.dtype == torch.float64 for v in l64.values())
            pre, post = cfg.TRAIN.RPN_PRE_NMS_TOP_N // B, cfg.TRAIN.RPN_POST_NMS_TOP_N // B
            cls32, reg32 = r32["rpn_cls"].numpy(), r32["rpn_reg"].numpy()
            top = np.stack([np.argsort(-cls32[b, :, 0], kind="stable")[:pre] for b in range(B)])
            reg_top = np.stack([reg32[b, top[b]] for b in range(B)])
            # margins: the argmax groups of the top rows, and every IoU the walk compares
            boxes_top = np.stack([RO.decode(pts[b][top[b]], reg_top[b], cfg.MEAN_SIZE[0], rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE, rpn.NUM_HEAD_BIN,
                                            rpn.LOC_XZ_FINE) for b in range(B)])
            am = min(RO.argmax_margin(reg_top[b], rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE, rpn.NUM_HEAD_BIN) for b in range(B))
            wm = min(RO.nms_walk(BO.boxes3d_to_bev(boxes_top[b]), thresh)[1] for b in range(B))
            print(f"weight seed {wseed} {tag}: argmax margin {am:.3g}, NMS walk margin {wm:.3g}, scores [{cls32.min():.3f}, {cls32.max():.3f}], "
                  f"reg [{reg32.min():.2f}, {reg32.max():.2f}], proposals {[(r32['roi_scores_raw'][b] != 0).sum().item() for b in range(B)]}")
            if am < 1e-4 or wm < 1e-4:
                ok = False
                break
            # the reference's own decode of the same rows (its ProposalLayer's first half), for the pre-NMS boxes
            from disprcnn.modeling.pointnet_module.point_rcnn.lib.utils.bbox_transform import decode_bbox_target
            DTYPE[0] = torch.float32
            ref_boxes = []
            for b in range(B):
                p = decode_bbox_target(torch.from_numpy(pts[b][top[b]]), torch.from_numpy(reg_top[b]), anchor_size=model.proposal_layer.MEAN_SIZE.float(),
                                       loc_scope=rpn.LOC_SCOPE, loc_bin_size=rpn.LOC_BIN_SIZE, num_head_bin=rpn.NUM_HEAD_BIN,
                                       get_xz_fine=rpn.LOC_XZ_FINE, get_y_by_bin=False, get_ry_fine=False)
                p[:, 1] = p[:, 1] + p[:, 3] / 2
                ref_boxes.append(p.numpy())
            rs = np.random.RandomState(7)
            N = pts.shape[1]
            pts_out = np.sort(rs.choice(N, N_OUT_PTS, replace=False))
            out.update({
                f"{tag}_top_idx": top.astype(np.int32), f"{tag}_top_reg": reg_top, f"{tag}_top_boxes": np.stack(ref_boxes),
                f"{tag}_rpn_cls": cls32, f"{tag}_rpn_cls64": r64["rpn_cls"].numpy(),
                f"{tag}_pts_out": pts_out.astype(np.int32),
                f"{tag}_rpn_reg64": r64["rpn_reg"].numpy()[:, pts_out], f"{tag}_backbone_features64": r64["backbone_features"].numpy()[:, :, pts_out],
                f"{tag}_roi_boxes3d": r32["roi_boxes3d"].numpy(), f"{tag}_roi_scores_raw": r32["roi_scores_raw"].numpy(),
                f"{tag}_seg_mask": r32["seg_mask"].numpy().astype(np.uint8), f"{tag}_pts_depth": r32["pts_depth"].numpy(),
                f"{tag}_backbone_xyz_equals_input": np.bool_(np.array_equal(r32["backbone_xyz"].numpy(), pts)),
            })
            for name, a, b in [("rpn_cls", r32["rpn_cls"], r64["rpn_cls"]), ("rpn_reg", r32["rpn_reg"], r64["rpn_reg"]),
                               ("backbone_features", r32["backbone_features"], r64["backbone_features"])] + \
                              [(k, l32[k], l64[k]) for k in sorted(l32)]:
                d = (a.double() - b).abs()
                errs.setdefault(name, []).append((d.max().item(), d.mean().item(), b.abs().max().item()))
            if tag == "b2":
                for k in sorted(l64):
                    n = l64[k].shape[2]
                    sel = np.sort(rs.choice(n, min(N_LEVEL_PTS, n), replace=False))
                    out[f"{tag}_pts_{k}"] = sel.astype(np.int32)
                    out[f"{tag}_{k}64"] = l64[k].numpy()[:, :, sel]
        if ok:
            break
    else:
        raise SystemExit("no weight seed met the margins")
    for name, e in errs.items():
        out[f"err32_max_{name}"] = np.float64(max(x[0] for x in e))
        out[f"err32_mean_{name}"] = np.float64(np.mean([x[1] for x in e]))
        out[f"absmax_{name}"] = np.float64(max(x[2] for x in e))
        print(f"{name}: err32 max {out[f'err32_max_{name}']:.3g} mean {out[f'err32_mean_{name}']:.3g} |v| <= {out[f'absmax_{name}']:.3g}")
    with open(os.path.join(HERE, "rpn_cfg_car.json"), "w") as f:
        json.dump(sub, f, indent=1, sort_keys=True)
        f.write("\n")
    path = os.path.join(HERE, "rpn_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

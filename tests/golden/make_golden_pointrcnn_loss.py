#!/usr/bin/env python3
"""Golden fixture for PointRCNN's training labels and losses, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointrcnn_loss.py    -> pointrcnn_loss_golden.npz

Reference code exercised (its own Python on torch-CPU): utils/loss_utils.py (get_reg_loss, DiceLoss, SigmoidFocalClassificationLoss),
net/rpn_loss.py (PointRCNNLossComputation), net/rcnn_loss.py (PointRCNNBox3dLossComputation), net/point_rcnn.py
(generate_rpn_training_labels, filter_bbox_3d) and structures/bounding_box_3d.py (Box3DList.convert, enlarge_box3d), backward included.
Harness-only stand-ins: the import stubs of make_golden_rpn.py, `Tensor.cuda` = identity, torch.cuda.FloatTensor -> a CPU tensor of the
run's dtype, and, for the fp64 run, `Tensor.float` follows the run's dtype (the reference's .float() calls otherwise mix dtypes).
F.cross_entropy is wrapped for the duration of a call to record the integer bin labels get_reg_loss hands it.

Every case is run in fp32 and in fp64.  Stored per case: the fp64 losses / terms / gradients, the reference's own fp32 error per output
(`*_e32`: |fp32 run - fp64 run|, the yardstick of the GPU tests' tolerance) and the fp32 run's bin labels.  Inputs are not stored:
tests/pointrcnn_loss_oracle.py rebuilds them from the seed recorded here.  A seed is moved on until the fp32 and fp64 runs put every row
in the same bins.  The multi-block cases keep every 16th gradient row.  Point labels: a point is flagged `near_face` when the fp32 and
fp64 inside tests differ or a dot product lies within 1e-5 |v|^2 of a bound; at most 0.5 % of a case's points may be (asserted).
"""
import copy
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

from tests import pointrcnn_loss_oracle as O  # noqa: E402

for name in ("cv2", "pycocotools", "pycocotools.mask", "pointnet2_cuda", "iou3d_cuda", "roipool3d_cuda", "tensorboardX", "termcolor",
             "numba", "zarr", "fastai", "matplotlib", "matplotlib.pyplot", "dl_ext", "dl_ext.primitive", "dl_ext.vision_ext",
             "dl_ext.vision_ext.datasets", "dl_ext.vision_ext.datasets.kitti", "dl_ext.vision_ext.datasets.kitti.structures",
             "disprcnn._C", "PIL", "PIL.Image", "tqdm", "scipy", "scipy.spatial", "skimage", "shapely", "shapely.geometry"):
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
_float = torch.Tensor.float
torch.Tensor.float = lambda self, *a, **k: self.to(DTYPE[0])

import torch.nn.functional as TF  # noqa: E402
from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import filter_bbox_3d, generate_rpn_training_labels  # noqa: E402
from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.rcnn_loss import PointRCNNBox3dLossComputation  # noqa: E402
from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.rpn_loss import PointRCNNLossComputation  # noqa: E402
from disprcnn.modeling.pointnet_module.point_rcnn.lib.utils.loss_utils import get_reg_loss  # noqa: E402
from disprcnn.structures.bounding_box_3d import Box3DList  # noqa: E402

RPN_VALS = ("rpn_loss_cls", "rpn_loss_reg", "rpn_loss", "rpn_fg_sum", "rpn_loss_loc", "rpn_loss_angle", "rpn_loss_size", "rpn_loss_cls_pos",
            "rpn_loss_cls_neg")
RCNN_VALS = ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size", "rpn_loss_cls_pos",
             "rpn_loss_cls_neg", "rcnn_cls_fg", "rcnn_cls_bg", "rcnn_reg_fg", "loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res",
             "loss_y_offset", "loss_y_bin", "loss_y_res", "loss_ry_bin", "loss_ry_res", "loss_loc", "loss_angle", "loss_size")
REG_DICT = ("loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res", "loss_y", "loss_y_res", "loss_ry_bin", "loss_ry_res")


class capture_bins:
    """records the targets of every F.cross_entropy call"""

    def __enter__(self):
        self.targets, self.orig = [], TF.cross_entropy

        def wrapped(inp, target, *a, **k):
            self.targets.append(target.detach().numpy().copy())
            return self.orig(inp, target, *a, **k)
        TF.cross_entropy = wrapped
        return self

    def __exit__(self, *a):
        TF.cross_entropy = self.orig


def t(a, dtype):
    a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(dtype) if a.dtype.is_floating_point else a


def num(v):
    return float(v.item()) if isinstance(v, torch.Tensor) else float(v)


def ref_bins(reg_label, anchor, lay, dtype):
    """the bin labels the reference derives for every row: (rows,4) x, z, y (-1 when not binned), ry"""
    DTYPE[0] = dtype
    rows = reg_label.shape[0]
    with capture_bins() as cap, torch.no_grad():
        get_reg_loss(torch.zeros(rows, O.channels(lay), dtype=dtype), t(reg_label, dtype), anchor_size=t(anchor, dtype), **lay)
    b = cap.targets
    assert len(b) == (4 if lay["get_y_by_bin"] else 3)
    y = b[2] if lay["get_y_by_bin"] else np.full(rows, -1, np.int64)
    return np.stack([b[0], b[1], y, b[-1]], 1)


def ref_reg(inp, lay, dtype):
    DTYPE[0] = dtype
    sel = inp["row_mask"]
    rows, C = inp["pred"].shape
    terms, grad = np.zeros(12), np.zeros((rows, C))
    if sel.sum() == 0:                                    # the reference's callers do not call get_reg_loss without a row
        return terms, grad
    pred = t(inp["pred"], dtype).requires_grad_()
    s = torch.from_numpy(sel)
    anchor = t(inp["anchor"], dtype)
    loc, angle, size, d = get_reg_loss(pred[s], t(inp["reg_label"], dtype)[s], anchor_size=anchor[s] if anchor.dim() == 2 else anchor,
                                       loss_mask=None if inp["loss_mask"] is None else torch.from_numpy(inp["loss_mask"])[s], **lay)
    g = O.GRAD_WEIGHTS
    (g[0] * loc + g[1] * angle + g[2] * size).backward()
    d = dict(d)
    d["loss_y"] = d.get("loss_y_bin", d.get("loss_y_offset"))
    for i, k in enumerate(REG_DICT):
        terms[i] = num(d.get(k, 0.0))
    terms[8], terms[9], terms[10], terms[11] = num(size), num(loc), num(angle), num(size)
    return terms, pred.grad.double().numpy()


def ref_rpn(case, inp, dtype):
    DTYPE[0] = dtype
    ev = PointRCNNLossComputation(O.cfg_for(case))
    cls, reg = t(inp["rpn_cls"], dtype).requires_grad_(), t(inp["rpn_reg"], dtype).requires_grad_()
    tb = {}
    out = ev(cls, reg, t(inp["cls_label"], dtype), t(inp["reg_label"], dtype), torch.from_numpy(inp["matched"]), tb_dict=tb)
    assert sorted(out) == ["rpn_loss_cls", "rpn_loss_reg"]
    (out["rpn_loss_cls"] + out["rpn_loss_reg"]).backward()
    vals = np.array([num(tb.get(k, 0.0)) for k in RPN_VALS])
    assert abs(vals[0] - num(out["rpn_loss_cls"])) == 0 and abs(vals[1] - num(out["rpn_loss_reg"])) == 0
    gc = cls.grad.double().numpy().reshape(-1) if cls.grad is not None else np.zeros(cls.numel())
    gr = reg.grad.double().numpy().reshape(-1, reg.shape[-1]) if reg.grad is not None else np.zeros((cls.numel(), reg.shape[-1]))
    return vals, gc, gr, sorted(tb)


def ref_rcnn(case, inp, dtype):
    DTYPE[0] = dtype
    ev = PointRCNNBox3dLossComputation(O.cfg_for(case))
    cls, reg = t(inp["rcnn_cls"], dtype).requires_grad_(), t(inp["rcnn_reg"], dtype).requires_grad_()
    labels = {"cls_label": t(inp["cls_label"], dtype), "reg_valid_mask": torch.from_numpy(inp["reg_valid_mask"]),
              "roi_boxes3d": t(inp["roi_boxes3d"], dtype), "gt_of_rois": t(inp["gt_of_rois"], dtype),
              "pts_input": torch.zeros(cls.shape[0], 1)}
    tb = {}
    loss = ev({"rcnn_cls": cls, "rcnn_reg": reg}, None, labels, None, None, tb_dict=tb)
    loss.backward()
    vals = np.array([num(tb.get(k, 0.0)) for k in RCNN_VALS])
    assert vals[2] == num(loss)
    return vals, cls.grad.double().numpy().reshape(-1), reg.grad.double().numpy(), sorted(tb)


def bins_agree(reg_label, anchor, lay):
    b32, b64 = ref_bins(reg_label, anchor, lay, torch.float32), ref_bins(reg_label, anchor, lay, torch.float64)
    return b32, np.array_equal(b32, b64)


class Target:
    def __init__(self, box3d):
        self.box3d = box3d

    def get_field(self, name):
        assert name == "box3d"
        return self.box3d


def main():
    out = {"rpn_vals": np.array(RPN_VALS), "rcnn_vals": np.array(RCNN_VALS)}
    # ---- get_reg_loss
    for ci, (name, case) in enumerate(O.REG_CASES.items()):
        lay = O.LAYOUTS[case["layout"]]
        for seed in range(1000 + 100 * ci, 1100 + 100 * ci):
            inp = O.make_reg_case(case, seed)
            b32, ok = bins_agree(inp["reg_label"], inp["anchor"], lay)
            if ok:
                break
            print(f"{name}: seed {seed} puts a row in different fp32 / fp64 bins, moving on")
        else:
            raise SystemExit(f"{name}: no seed")
        t32, g32 = ref_reg(inp, lay, torch.float32)
        t64, g64 = ref_reg(inp, lay, torch.float64)
        keep = O.stored_rows(case)
        out.update({f"{name}_seed": np.int64(seed), f"{name}_bins": b32.astype(np.int8), f"{name}_terms": t64, f"{name}_terms_e32": np.abs(t32 - t64),
                    f"{name}_grad": g64[keep], f"{name}_grad_e32": np.float64(np.abs(g32 - g64).max())})
        print(f"{name}: seed {seed}, selected {int(inp['row_mask'].sum())}, loc {t64[9]:.6f} angle {t64[10]:.6f} size {t64[8]:.6f}, "
              f"e32 terms {np.abs(t32 - t64).max():.3g} grad {np.abs(g32 - g64).max():.3g} (|g| <= {np.abs(g64).max():.3g})")
    # ---- bins on the edges (the fp32 run's; the fp64 run may differ there, which is the point)
    for lname, lay in O.LAYOUTS.items():
        lab = O.make_edge_rows(lay)
        b32 = ref_bins(lab, np.array(O.MEAN_SIZE, np.float32), lay, torch.float32)
        out[f"edge_{lname}_bins"] = b32.astype(np.int8)
        print(f"edge_{lname}: {len(lab)} rows, fp32 vs fp64 bins differ on "
              f"{int((b32 != ref_bins(lab, np.array(O.MEAN_SIZE, np.float32), lay, torch.float64)).any(1).sum())}")
    # ---- the RPN evaluator and, through it, the classification losses
    for ci, (name, case) in enumerate(O.RPN_CASES.items()):
        cfg = O.cfg_for(case)
        lay = O.rpn_layout(cfg)
        for seed in range(20000 + 100 * ci, 20100 + 100 * ci):
            inp = O.make_rpn_case(case, seed)
            fg = inp["cls_label"].reshape(-1) > 0
            if bins_agree(inp["reg_label"].reshape(-1, 7)[fg], np.array(O.MEAN_SIZE, np.float32), lay)[1] if fg.any() else True:
                break
        else:
            raise SystemExit(f"{name}: no seed")
        v32, gc32, gr32, _ = ref_rpn(case, inp, torch.float32)
        v64, gc64, gr64, keys = ref_rpn(case, inp, torch.float64)
        e = case.get("every", 1)
        out.update({f"{name}_seed": np.int64(seed), f"{name}_vals": v64, f"{name}_vals_e32": np.abs(v32 - v64), f"{name}_keys": np.array(keys),
                    f"{name}_gcls": gc64[e - 1::e], f"{name}_gcls_e32": np.float64(np.abs(gc32 - gc64).max())})
        if name.startswith("ev_"):
            out.update({f"{name}_greg": gr64, f"{name}_greg_e32": np.float64(np.abs(gr32 - gr64).max())})
        print(f"{name}: seed {seed}, cls {v64[0]:.6f} reg {v64[1]:.6f} fg {int(v64[3])}, e32 vals {np.abs(v32 - v64).max():.3g} "
              f"gcls {np.abs(gc32 - gc64).max():.3g} greg {np.abs(gr32 - gr64).max():.3g}")
    # ---- the RCNN evaluator
    for ci, (name, case) in enumerate(O.RCNN_CASES.items()):
        cfg = O.cfg_for(case)
        lay = O.rcnn_layout(cfg)
        for seed in range(40000 + 100 * ci, 40100 + 100 * ci):
            inp = O.make_rcnn_case(case, seed)
            anchor = inp["roi_boxes3d"][:, 3:6] if cfg.RCNN.SIZE_RES_ON_ROI else np.array(O.MEAN_SIZE, np.float32)
            b32, ok = bins_agree(inp["gt_of_rois"], anchor, lay)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed")
        v32, gc32, gr32, _ = ref_rcnn(case, inp, torch.float32)
        v64, gc64, gr64, keys = ref_rcnn(case, inp, torch.float64)
        out.update({f"{name}_seed": np.int64(seed), f"{name}_vals": v64, f"{name}_vals_e32": np.abs(v32 - v64), f"{name}_keys": np.array(keys),
                    f"{name}_bins": b32.astype(np.int8), f"{name}_gcls": gc64, f"{name}_gcls_e32": np.float64(np.abs(gc32 - gc64).max()),
                    f"{name}_greg": gr64, f"{name}_greg_e32": np.float64(np.abs(gr32 - gr64).max())})
        print(f"{name}: seed {seed}, loss {v64[2]:.6f}, e32 vals {np.abs(v32 - v64).max():.3g} gcls {np.abs(gc32 - gc64).max():.3g} "
              f"greg {np.abs(gr32 - gr64).max():.3g}")
    # ---- point labels
    DTYPE[0] = torch.float32
    for ci, name in enumerate(O.LABEL_CASES):
        seed = 60000 + ci
        pts, boxes7 = O.make_label_case(name, seed)
        targets = [Target(Box3DList(torch.from_numpy(boxes7[b:b + 1]), (1242, 375), mode="xyzhwl_ry")) for b in range(len(boxes7))]
        cls32, reg32 = generate_rpn_training_labels(torch.from_numpy(pts), targets)
        corners = torch.cat([x.box3d.convert("corners").bbox_3d.view(-1, 8, 3) for x in targets]).numpy()
        large = torch.cat([x.box3d.enlarge_box3d(0.2).convert("corners").bbox_3d.view(-1, 8, 3) for x in targets]).numpy()
        gt7 = torch.cat([x.box3d.convert("xyzhwl_ry").bbox_3d for x in targets]).numpy()
        assert np.array_equal(gt7, boxes7)
        near = np.zeros(pts.shape[:2], bool)
        for b in range(len(boxes7)):
            for c in (corners[b], large[b]):
                d32 = filter_bbox_3d(torch.from_numpy(c), torch.from_numpy(pts[b]))[2].numpy()
                d64 = filter_bbox_3d(torch.from_numpy(c).double(), torch.from_numpy(pts[b]).double())[2].numpy()
                near[b] |= (d32 != d64) | (O.inside_margin(pts[b], c)[1] < 1e-5)
        assert near.mean() <= 0.005, (name, near.mean())
        cls64, reg64 = O.point_labels(pts, boxes7, corners, large)
        assert np.array_equal(cls64[~near], cls32.numpy()[~near])
        fg = cls32.numpy() == 1
        out.update({f"{name}_seed": np.int64(seed), f"{name}_corners": corners, f"{name}_corners_large": large,
                    f"{name}_cls": cls32.numpy().astype(np.int8), f"{name}_near_face": near, f"{name}_reg32_sub": reg32.numpy()[:, ::8],
                    f"{name}_reg_e32": np.float64(np.abs(reg32.numpy().astype(np.float64) - reg64)[fg & ~near].max() if (fg & ~near).any() else 0.0)})
        print(f"{name}: inside {int(fg.sum())} ignored {int((cls32.numpy() == -1).sum())} of {fg.size}, per cloud inside "
              f"{fg.sum(1).tolist()}, near_face {int(near.sum())}, reg e32 {out[f'{name}_reg_e32']:.3g}")
    path = os.path.join(HERE, "pointrcnn_loss_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

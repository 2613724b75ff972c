#!/usr/bin/env python3
"""Golden fixture for RCNNNet's training step, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rcnn_train.py    -> rcnn_train_golden.npz

Reference code exercised (its own Python on torch-CPU, autograd included): RCNNNet.forward in training mode with RCNN.ROI_SAMPLE_JIT =
False (net/rcnn_net.py), its SA modules, pytorch_utils and pointnet2_utils (forward and backward), PointRCNNBox3dLossComputation
(net/rcnn_loss.py) with loss_utils.get_reg_loss and SigmoidFocalClassificationLoss.  Config: make_golden_rcnn.py's car config with
ROI_SAMPLE_JIT off and LOSS_CLS = SigmoidFocalLoss -- the car file's BinaryCrossEntropy branch cannot be recorded with the ignore label -1
that this fixture must contain (F.binary_cross_entropy refuses a target outside [0, 1]).  The harness stand-ins are make_golden_rpn.py's
(through make_golden_rcnn.py), plus `group_points_grad_wrapper` / `gather_points_grad_wrapper` served by tests/pn2_oracle.scatter_grad, and
`Tensor.float` keeping the dtype of the run in progress (the loss calls .float() on its labels and on MEAN_SIZE), as
make_golden_pointrcnn_loss.py does; the loss evaluator is initialised again at the start of each run, because it makes its MEAN_SIZE
tensor when it is constructed.

Inputs and weights are not stored: tests/rcnn_train_oracle.py builds them from the seeds recorded here (R = 4 ROIs, NUM_POINTS = 512:
level 0 samples 128 centroids).  The step runs once as .double() and once in fp32 on the same fp32 pts_input: both see identical
coordinates, hence identical FPS / ball-query indices, and their difference is the reference's own fp32 rounding error, stored per tensor
on exactly the stored entries as err32_max_* / err32_mean_* (and err32_sum_* / err32_asum_* for the stored sums).

Stored: the fp64 loss; for every parameter the fp64 gradient -- whole under 4096 elements, else a recorded random subset of 2048 entries
plus the fp64 sum and absolute sum of the whole tensor; the fp64 gradient with respect to pts_input on a recorded subset of its feature
channels (index 3 on: the product treats the coordinates as constants of the graph, the reference also differentiates the grouped
coordinates, so channels 0..2 differ by design and are not recorded).

Checked before writing, else the label seed moves on: no gt_boxes3d_ct component within 1e-4 of a bin edge, and the fp32 and fp64 runs
agree on every bin label.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_rcnn as MC  # noqa: E402  (installs the stand-ins, imports the reference)
from tests.golden import make_golden_rpn as MR  # noqa: E402
from tests import pn2_oracle as PO  # noqa: E402
from tests import pointrcnn_loss_oracle as LO  # noqa: E402
from tests import rcnn_oracle as CO  # noqa: E402
from tests import rcnn_train_oracle as TO  # noqa: E402
from tests import rpn_oracle as RO  # noqa: E402

import torch.nn.functional as TF  # noqa: E402

torch.Tensor.float = lambda self, *a, **k: self.to(MR.DTYPE[0])


def _group_grad(B, C, N, npoint, nsample, grad_out, idx, grad_features):
    g = PO.scatter_grad(grad_out.detach().double().numpy().reshape(B, C, npoint * nsample), idx.numpy().reshape(B, -1), N)
    grad_features.copy_(torch.from_numpy(g).to(grad_features.dtype))


def _gather_grad(B, C, N, npoint, grad_out, idx, grad_features):
    g = PO.scatter_grad(grad_out.detach().double().numpy().reshape(B, C, npoint), idx.numpy().reshape(B, -1), N)
    grad_features.copy_(torch.from_numpy(g).to(grad_features.dtype))


MR.pn2.group_points_grad_wrapper = _group_grad
MR.pn2.gather_points_grad_wrapper = _gather_grad

WHOLE_BELOW, N_SUBSET = 4096, 2048
T = torch.from_numpy


class capture_bins:
    def __enter__(self):
        self.targets, self.orig = [], TF.cross_entropy

        def wrapped(inp, target, *a, **k):
            self.targets.append(target.detach().numpy().copy())
            return self.orig(inp, target, *a, **k)
        TF.cross_entropy = wrapped
        return self

    def __exit__(self, *a):
        TF.cross_entropy = self.orig


def run(model, sd, prop, dtype):
    """one training step of the reference -> loss, {name: grad}, d loss / d pts_input, the bin labels its loss derived"""
    MR.DTYPE[0] = dtype
    model.loss.__init__(model.loss.cfg)      # its MEAN_SIZE tensor is made with .float() at construction: made again in this run's dtype
    model.to(dtype).load_state_dict({k: T(v).to(dtype) for k, v in sd.items()}, strict=True)
    model.train()
    model.zero_grad()
    for p in model.parameters():
        p.grad = None
    pin = T(prop["pts_input"]).to(dtype).requires_grad_()
    d = {"pts_input": pin, "roi_boxes3d": T(prop["roi_boxes3d"]).to(dtype), "cls_label": T(prop["cls_label"]).to(dtype),
         "reg_valid_mask": T(prop["reg_valid_mask"]), "gt_boxes3d_ct": T(prop["gt_boxes3d_ct"]).to(dtype)}
    with capture_bins() as cap:
        ret, losses = model(d)
    assert ret is d and sorted(losses) == ["loss_box3d"]
    loss = losses["loss_box3d"]
    assert loss.dtype == dtype
    loss.backward()
    grads = {k: p.grad.detach().double().numpy().copy() for k, p in model.named_parameters()}
    assert all(p.grad.dtype == dtype for p in model.parameters())
    return float(loss.item()), grads, pin.grad.detach().double().numpy().copy(), [t.tolist() for t in cap.targets]


def edge_margin_ok(gt, lay, valid):
    """no component of a regression label within 1e-4 of a bin edge: the bins do not move when any component does by 1e-4"""
    base, _ = LO.bin_targets(gt[valid], LO.MEAN_SIZE, lay, np.float64)
    for col in (0, 1, 2, 6):
        for s in (-1e-4, 1e-4):
            g = gt[valid].astype(np.float64).copy()
            g[:, col] += s
            if not np.array_equal(LO.bin_targets(g, LO.MEAN_SIZE, lay, np.float64)[0], base):
                return False
    return True


def main():
    pr = MR.ref_cfg.MODEL.POINTRCNN.clone()
    MR.merge(pr, MC.CAR)
    MR.merge(pr, {"RCNN": {"ROI_SAMPLE_JIT": False, "LOSS_CLS": "SigmoidFocalLoss"}})
    sub = {"RPN": MR.plain(pr.RPN), "RCNN": MR.plain(pr.RCNN), "MEAN_SIZE": MR.plain(pr.MEAN_SIZE), "TRAIN": MR.plain(pr.TRAIN),
           "TEST": MR.plain(pr.TEST), "MASK_THRESH": pr.MASK_THRESH}
    cfg = RO.make_cfg(sub)
    assert cfg.RCNN.NUM_POINTS == 512 and not cfg.RCNN.USE_BN and cfg.RCNN.DP_RATIO == 0.0
    base = np.load(os.path.join(HERE, "rcnn_ref_golden.npz"))
    wseed, bump = int(base["weight_seed"]), int(base["input_bump"])
    model = MC.RCNNNet(pr, MR.ref_cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = CO.random_state(shapes, wseed)
    lay = LO.rcnn_layout(cfg)
    for gt_seed in range(1, 40):
        prop = TO.make_train_inputs(cfg, bump, gt_seed)
        valid = prop["reg_valid_mask"] > 0
        if not edge_margin_ok(prop["gt_boxes3d_ct"], lay, valid):
            print(f"label seed {gt_seed}: a label lies within 1e-4 of a bin edge")
            continue
        l64, g64, p64, b64 = run(model, sd, prop, torch.float64)
        l32, g32, p32, b32 = run(model, sd, prop, torch.float32)
        print(f"label seed {gt_seed}: loss fp64 {l64:.9g} fp32 {l32:.9g}; bins {b64}")
        if b64 != b32:
            print("  the fp32 and fp64 runs disagree on a bin label")
            continue
        break
    else:
        raise SystemExit("no label seed met the margins")
    assert sorted(set(prop["cls_label"].tolist())) == [-1.0, 0.0, 1.0] and sorted(set(prop["reg_valid_mask"].tolist())) == [0, 1]
    out = {"weight_seed": np.int64(wseed), "input_bump": np.int64(bump), "gt_seed": np.int64(gt_seed), "rois": np.array(TO.TRAIN_ROIS, np.int32),
           "loss64": np.float64(l64), "err32_loss": np.float64(abs(l32 - l64)), "param_names": np.array(sorted(g64))}
    rs = np.random.RandomState(11)
    for name in sorted(g64):
        a64, a32 = g64[name].reshape(-1), g32[name].reshape(-1)
        if a64.size < WHOLE_BELOW:
            sel = np.arange(a64.size)
        else:
            sel = np.sort(rs.choice(a64.size, N_SUBSET, replace=False))
            out[f"gi_{name}"] = sel.astype(np.int32)
            out[f"gsum_{name}"], out[f"gasum_{name}"] = np.float64(a64.sum()), np.float64(np.abs(a64).sum())
            out[f"err32_sum_{name}"] = np.float64(abs(a32.sum() - a64.sum()))
            out[f"err32_asum_{name}"] = np.float64(abs(np.abs(a32).sum() - np.abs(a64).sum()))
        out[f"g_{name}"] = a64[sel]
        d = np.abs(a32[sel] - a64[sel])
        out[f"err32_max_{name}"], out[f"err32_mean_{name}"] = np.float64(d.max()), np.float64(d.mean())
        print(f"{name}: |g| <= {np.abs(a64).max():.3g}, err32 max {d.max():.3g} mean {d.mean():.3g}")
    # d loss / d pts_input on its feature channels
    R, S, Cp = p64.shape
    feat64, feat32 = p64[..., 3:].reshape(-1), p32[..., 3:].reshape(-1)
    sel = np.sort(rs.choice(feat64.size, N_SUBSET, replace=False))
    d = np.abs(feat32[sel] - feat64[sel])
    out.update(gi_pts_input=sel.astype(np.int32), g_pts_input=feat64[sel], err32_max_pts_input=np.float64(d.max()),
               err32_mean_pts_input=np.float64(d.mean()))
    print(f"pts_input[..., 3:]: |g| <= {np.abs(feat64).max():.3g}, err32 max {d.max():.3g} mean {d.mean():.3g}; nonzero {np.count_nonzero(feat64)}")
    path = os.path.join(HERE, "rcnn_train_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden fixture for the stereo box head's TRAINING step, recorded from the IMPORTED REFERENCE (authoring container only).

    python oracle/build_ref.py && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_roi_heads_train.py

Reference code exercised (its own Python on torch-CPU, train mode): ROIBoxHead.forward_double_view (roi_heads/box_head/box_head.py) =
FastRCNNLossComputation.subsample (its own seeded BalancedPositiveNegativeSampler) + StereoFPN2MLPFeatureExtractor (Pooler / ROIAlign =
disprcnn._C.roi_align_forward, the reference's CPU kernel built by oracle/build_ref.py; Dropout(0.2) twice) + StereoFPNPredictor + the
double-view loss, then autograd for the gradients of the parameter tensors.  The pyramids do not require grad: the reference's CPU ROIAlign
has no backward.  Forward hooks on the two Dropout modules capture the keep masks (output != 0 or input == 0).
The import harness (stand-in modules, the config) is tests/golden/make_golden_det.py's.  Small dims: in_channels 8, MLP_HEAD_DIM 72, two
images of 96 x 160, BATCH_SIZE_PER_IMAGE 8.  The pyramid variant and torch seed are the first for which the recorded case keeps every ReLU input of the fp64
oracle (tests/roi_heads_train_oracle.py) at least 1e-4 of the largest away from zero.
Inputs (pyramids, weights, boxes) come from disprcnn_amd.utils.synth / tests/roi_heads_train_cases.py and are rebuilt by the tests.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_det as MD  # noqa: E402  (the harness: stand-ins, reference imports, make_cfg)

from disprcnn.modeling.roi_heads.box_head.box_head import ROIBoxHead  # noqa: E402  (the reference)
from disprcnn.structures.bounding_box import BoxList  # noqa: E402

from disprcnn_amd.utils import synth  # noqa: E402
from tests import roi_heads_train_cases as CS  # noqa: E402
from tests import roi_heads_train_oracle as TO  # noqa: E402

C_IN, DIM, BATCH, H, W = CS.BOX_C, CS.BOX_DIM, CS.BOX_BATCH, CS.BOX_IMG[1], CS.BOX_IMG[0]


def golden_inputs(variant):
    """what the tests rebuild: pyramids (tag variant), weights, proposals and ground truths (tests/roi_heads_train_cases.py: the box_full
    case's boxes)"""
    c = CS.box_full_case()
    fl, fr = synth.synth_pyramid(2, H, W, c=C_IN, tag=f"rht:golden:{variant}")
    return c, fl, fr


def boxlist(b, **fields):
    out = BoxList(torch.from_numpy(np.asarray(b, np.float32)), (W, H), mode="xyxy")
    for k, v in fields.items():
        out.add_field(k, torch.from_numpy(v))
    return out


def record(seed, variant):
    cfg = MD.make_cfg()
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = DIM
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE, cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION = BATCH, 0.25
    head = ROIBoxHead(cfg, C_IN).train()
    state = synth.synth_det_state({k: v for k, v in head.state_dict().items()}, gain={"predictor.cls_score.weight": 3.0, "predictor.bbox_pred.weight": 2.0})
    head.load_state_dict(state, strict=True)
    c, fl, fr = golden_inputs(variant)
    masks = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: masks.append(((out != 0) | (inp[0] == 0)).numpy().reshape(out.shape[0], -1)))
             for m in head.feature_extractor.RCNN_top if isinstance(m, torch.nn.Dropout)]
    torch.manual_seed(seed)
    props = {"left": [boxlist(p) for p in c.left_props], "right": [boxlist(p) for p in c.right_props]}
    tgts = {"left": [boxlist(g, labels=l) for g, l in zip(c.gt_left, c.gt_labels)], "right": [boxlist(g, labels=l) for g, l in zip(c.gt_right, c.gt_labels)]}
    x, left, right, losses = head({"left": fl, "right": fr}, props, tgts)
    (losses["loss_classifier"] + losses["loss_box_reg"]).backward()
    for h in hooks:
        h.remove()
    out = {"seed": np.array(seed), "variant": np.array(variant), "loss_classifier": losses["loss_classifier"].detach().numpy(), "loss_box_reg": losses["loss_box_reg"].detach().numpy(),
           "keep": np.stack(masks).astype(np.uint8), "counts": np.array([len(b) for b in left])}
    out["left_boxes"] = np.concatenate([b.bbox.numpy() for b in left])
    out["right_boxes"] = np.concatenate([b.bbox.numpy() for b in right])
    out["labels"] = np.concatenate([b.get_field("labels").numpy() for b in left])
    out["regression_targets"] = np.concatenate([b.get_field("regression_targets").numpy() for b in left])
    for k, v in head.named_parameters():
        out["grad:" + k] = v.grad.numpy()
    return out, state, (fl, fr)


def margin(out, state, feats):
    counts = np.cumsum([0] + list(out["counts"]))
    lb = [out["left_boxes"][a:b] for a, b in zip(counts[:-1], counts[1:])]
    rb = [out["right_boxes"][a:b] for a, b in zip(counts[:-1], counts[1:])]
    r = TO.box_step([f.numpy() for f in feats[0][:4]], [f.numpy() for f in feats[1][:4]], lb, rb, H, {k: v.numpy() for k, v in state.items()},
                    out["labels"], out["regression_targets"], out["keep"].astype(bool), 0.2)
    return r


def main():
    for variant, seed in ((v, s) for v in range(16) for s in range(12)):
        out, state, feats = record(seed, variant)
        r = margin(out, state, feats)
        print("variant", variant, "seed", seed, "R", int(out["counts"].sum()), "pre_lo", r["pre_lo"], "pre_hi", r["pre_hi"], "loss", float(out["loss_classifier"]),
              r["loss_classifier"], float(out["loss_box_reg"]), r["loss_box_reg"])
        if r["pre_lo"] >= 2e-4 * r["pre_hi"] and (out["labels"] > 0).sum() >= 2:
            break
    else:
        raise SystemExit("no seed keeps the ReLU inputs away from zero")
    path = os.path.join(HERE, "roi_heads_train_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()

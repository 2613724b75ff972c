#!/usr/bin/env python3
"""Golden fixture for the Stereo RPN's TRAINING step, recorded from the IMPORTED REFERENCE (authoring container only).

    python oracle/build_ref.py && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_srpn_train.py

Reference code exercised (its own Python on torch-CPU, train mode): StereoRPN.forward -> SRPNHead, AnchorGenerator, _forward_train =
box_selector_train (SRPNPostProcessor.forward with the TRAIN limits) + SRPNLossComputation (Matcher, its own seeded
BalancedPositiveNegativeSampler, BoxCoder.encode, smooth_l1_loss, cross_entropy), then autograd for the six parameter gradients.  The
sampler is wrapped to capture its masks, which the host test feeds to tests/srpn_train_oracle.py.  The import harness (stand-in modules,
the config) is tests/golden/make_golden_det.py's.  Inputs are the `full` case's of tests/srpn_train_cases.py (pyramids, weights, ground
truths) and are rebuilt by the tests; PRE_NMS_TOP_N_TRAIN 60 (below the anchor count) and POST_NMS_TOP_N_TRAIN 20, so both cuts act.
The torch seed is the first for which the recorded sample keeps every hidden pre-activation at an active pixel at least 2e-4 of the
largest away from zero in the fp64 oracle.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_det as MD  # noqa: E402  (the harness: stand-ins, reference imports, make_cfg)

from disprcnn.modeling.rpn.stereo_rpn.srpn import StereoRPN  # noqa: E402  (the reference)
from disprcnn.structures.bounding_box import BoxList  # noqa: E402
from disprcnn.structures.image_list import ImageList  # noqa: E402

from tests import srpn_train_cases as CS  # noqa: E402

PRE, POST = 60, 20


def record(seed):
    c = CS.cached("full")
    cfg = MD.make_cfg()
    r = cfg.MODEL.RPN
    r.PRE_NMS_TOP_N_TRAIN, r.POST_NMS_TOP_N_TRAIN, r.BATCH_SIZE_PER_IMAGE, r.POSITIVE_FRACTION = PRE, POST, CS.BATCH, CS.FRACTION
    assert (r.FG_IOU_THRESHOLD, r.BG_IOU_THRESHOLD, r.STRADDLE_THRESH, r.NMS_THRESH, r.MIN_SIZE) == (0.7, 0.3, 0, 0.7, 0)
    rpn = StereoRPN(cfg, c.c).train()
    state = rpn.state_dict()
    for k, v in c.params.items():
        state[k] = torch.from_numpy(v)
    rpn.load_state_dict(state, strict=True)
    masks = {}
    sampler = rpn.loss_evaluator.fg_bg_sampler

    def capturing(labels):
        pos, neg = sampler(labels)
        masks["pos"], masks["neg"] = torch.cat(pos).numpy().astype(np.uint8), torch.cat(neg).numpy().astype(np.uint8)
        return pos, neg
    rpn.loss_evaluator.fg_bg_sampler = capturing
    W, H = CS.IMG
    images = ImageList(torch.zeros(c.n, 3, H, W), [(H, W)] * c.n)
    fl, fr = [torch.from_numpy(f) for f in c.feats_left], [torch.from_numpy(f) for f in c.feats_right]
    lt = [BoxList(torch.from_numpy(g), (W, H), mode="xyxy") for g in c.gt_left]
    rt = [BoxList(torch.from_numpy(g), (W, H), mode="xyxy") for g in c.gt_right]
    torch.manual_seed(seed)
    lp, rp, losses = rpn(images, images, fl, fr, lt, rt)
    (losses["loss_objectness"] + losses["loss_rpn_box_reg"]).backward()
    out = {"seed": np.array(seed), "pre_nms": np.array(PRE), "post_nms": np.array(POST), "pos": masks["pos"], "neg": masks["neg"],
           "loss_objectness": losses["loss_objectness"].detach().numpy(), "loss_rpn_box_reg": losses["loss_rpn_box_reg"].detach().numpy()}
    with torch.no_grad():
        objectness, regression = rpn.head(fl, fr)
    for lvl in range(len(fl)):
        MD.samples(out, f"obj{lvl}", objectness[lvl], 512)
        MD.samples(out, f"reg{lvl}", regression[lvl], 512)
    for i in range(c.n):
        out[f"prop_left{i}"], out[f"prop_right{i}"] = lp[i].bbox.numpy(), rp[i].bbox.numpy()
        out[f"prop_score{i}"] = lp[i].get_field("objectness").numpy()
    for k, v in rpn.named_parameters():
        out["grad:" + k] = v.grad.numpy()
    return out


def main():
    c = CS.cached("full")
    for seed in range(32):
        out = record(seed)
        r = CS.oracle(c, 64, feat_grad=False, pos=out["pos"], neg=out["neg"])
        print("seed", seed, "pos", int(out["pos"].sum()), "neg", int(out["neg"].sum()), "pre_lo", r["pre_lo"], "pre_hi", r["pre_hi"], "loss",
              float(out["loss_objectness"]), r["loss_objectness"], float(out["loss_rpn_box_reg"]), r["loss_rpn_box_reg"],
              "proposals", [len(out[f"prop_score{i}"]) for i in range(c.n)])
        if r["pre_lo"] >= 2e-4 * r["pre_hi"]:
            break
    else:
        raise SystemExit("no seed keeps the ReLU inputs away from zero")
    path = os.path.join(HERE, "srpn_train_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()

"""The cases of tests/test_hip_roi_heads_train.py, built on the host so that tests/test_roi_heads_train_host.py can hold every one of them
to the ReLU-margin condition (smallest |pre-activation| >= 1e-4 * largest in the fp64 oracle) before the GPU sees it.

Box-head cases use a small sample (R <= 16 ROIs, 72 features: ~2 300 ReLU inputs), for which a seed with that margin exists; the seeds
below were searched on the CPU (python -m tests.roi_heads_train_cases).  The mask head has 250 000 ReLU inputs for five ROIs, where no seed
can give the margin, so its cases take their biases from roi_heads_train_oracle.margin_mask_params: +-B per channel, B above the layer's
largest response, so that a channel is wholly on or wholly off.
"""
import functools
from types import SimpleNamespace

import numpy as np

from . import det2d_loss_oracle as DO
from . import roi_heads_train_oracle as TO

F32 = np.float32
P_DROP = 0.2
BOX_SHAPES = [(24, 40), (12, 20), (6, 10), (3, 5)]            # image 96 x 160
BOX_IMG = (160, 96)                                           # (width, height)
BOX_C, BOX_DIM, BOX_BATCH = 8, 72, 8
MASK_SHAPES = [(64, 128), (32, 64), (16, 32), (8, 16)]        # image 256 x 512
MASK_IMG = (512, 256)
MASK_C, MASK_NCLS, MASK_M = 32, 2, 28
SEEDS = {"box_full": 27, "box_one": 0, "combined": 21}


def uniform(key, shape, lo, hi):
    from disprcnn_amd.utils.synth import hash_uniform
    return hash_uniform(key, shape, lo, hi).numpy()


def box_params(tag, c=BOX_C, dim=BOX_DIM, ncls=2, res=7):
    shapes = {TO.BOX_PARAMS[0]: (dim, 2 * c, res, res), TO.BOX_PARAMS[1]: (dim,), TO.BOX_PARAMS[2]: (dim, dim, 1, 1), TO.BOX_PARAMS[3]: (dim,),
              TO.BOX_PARAMS[4]: (ncls, dim), TO.BOX_PARAMS[5]: (ncls,), TO.BOX_PARAMS[6]: (6 * ncls, dim), TO.BOX_PARAMS[7]: (6 * ncls,)}
    out = {}
    for k, s in shapes.items():
        if k.endswith("bias"):
            out[k] = uniform(f"{tag}:{k}", s, -0.1, 0.1)
        else:
            a = np.sqrt(3.0 / np.prod(s[1:])) * (3.0 if "predictor" in k else 1.0)
            out[k] = uniform(f"{tag}:{k}", s, -a, a)
    return out


def real_pyramid(tag, n, shapes, c):
    a = np.sqrt(3.0)
    left = [uniform(f"{tag}:L{l}", (n, c, h, w), -a, a) for l, (h, w) in enumerate(shapes)]
    right = [(0.8 * np.roll(f, -1, 3) + 0.2 * uniform(f"{tag}:R{l}", f.shape, -a, a)).astype(F32) for l, f in enumerate(left)]
    return left, right


# ---- the box head's full forward: proposals on every level of both images, ground truths, sample draws, dropout draws
BOX_GT = [np.array([[10, 12, 40, 44], [60, 20, 150, 90]], F32), np.array([[-150, -180, 330, 290], [30, 30, 75, 70], [-60, -40, 200, 180]], F32)]
BOX_GT_SHIFT = [np.array([-4, 0, -5, 0], F32), np.array([-7, 0, -6, 0], F32)]      # the right view's boxes: x moved by the disparity


BOX_FAR = [np.array([[100, 60, 124, 80], [-30, -20, 60, 50], [20, -120, 250, 80], [100, 60, 530, 460], [5, 70, 40, 95]], F32),
           np.array([[120, 10, 144, 30], [70, 40, 160, 110], [150, 60, 380, 260], [200, 150, 630, 550], [100, 5, 135, 30]], F32)]


def box_full_case(seed=None):
    seed = SEEDS["box_full"] if seed is None else seed
    tag = f"rht:box_full:{seed}"
    gl = BOX_GT
    gr = [g + s for g, s in zip(gl, BOX_GT_SHIFT)]
    labels = [np.ones(len(g), np.int64) for g in gl]
    lp, rp = [], []
    for i, (a, b) in enumerate(zip(gl, gr)):
        jit = uniform(f"{tag}:jit{i}", (3,) + a.shape, -3.0, 3.0)
        far = BOX_FAR[i] + uniform(f"{tag}:far{i}", (5, 4), -2.0, 2.0)         # negatives: one per pyramid level and one more
        lp.append(np.concatenate([a] + [a + j for j in jit] + [far]).astype(F32))
        rp.append(np.concatenate([b] + [b + j * np.array([1, 0, 1, 0], F32) for j in jit] + [far - np.array([3, 0, 3, 0], F32)]).astype(F32))
        rp[-1][:, [1, 3]] = lp[-1][:, [1, 3]]                          # a joint box shares its rows between the views
    total = sum(len(p) for p in lp)
    draws = uniform(f"{tag}:sample", (total,), 0.0, 1.0)
    smp = TO.sampled(lp, rp, gl, gr, labels, draws, BOX_BATCH, 0.25)
    R = sum(len(s[0]) for s in smp)
    fl, fr = real_pyramid(tag, 2, BOX_SHAPES, BOX_C)
    return SimpleNamespace(tag=tag, left_props=lp, right_props=rp, gt_left=gl, gt_right=gr, gt_labels=labels, sample_draws=draws, sampled=smp, R=R,
                           feats_left=fl, feats_right=fr, params=box_params(tag), dropout=uniform(f"{tag}:drop", (2, R, BOX_DIM), 0.0, 1.0),
                           img=BOX_IMG, shapes=BOX_SHAPES)


def box_one_case(seed=None):
    """one image, one proposal (a positive): R = 1"""
    seed = SEEDS["box_one"] if seed is None else seed
    tag = f"rht:box_one:{seed}"
    gl, gr = [BOX_GT[0][:1]], [BOX_GT[0][:1] + BOX_GT_SHIFT[0]]
    lp, rp = [gl[0] + np.array([1, -1, 2, 1], F32)], [gr[0] + np.array([1, -1, 2, 1], F32)]
    labels = [np.ones(1, np.int64)]
    draws = uniform(f"{tag}:sample", (1,), 0.0, 1.0)
    smp = TO.sampled(lp, rp, gl, gr, labels, draws, BOX_BATCH, 0.25)
    fl, fr = real_pyramid(tag, 1, BOX_SHAPES, BOX_C)
    return SimpleNamespace(tag=tag, left_props=lp, right_props=rp, gt_left=gl, gt_right=gr, gt_labels=labels, sample_draws=draws, sampled=smp, R=1,
                           feats_left=fl, feats_right=fr, params=box_params(tag), dropout=uniform(f"{tag}:drop", (2, 1, BOX_DIM), 0.0, 1.0),
                           img=BOX_IMG, shapes=BOX_SHAPES)


def box_oracle(c, dtype, feat_grad=True):
    import torch
    lb = [s[3][:, :4] for s in c.sampled]
    rb = [s[3][:, [4, 1, 5, 3]] for s in c.sampled]
    return TO.box_step(c.feats_left, c.feats_right, lb, rb, c.img[1], c.params, np.concatenate([s[1] for s in c.sampled]),
                       np.concatenate([s[2] for s in c.sampled]), TO.dropout_keep(c.dropout, P_DROP), P_DROP,
                       torch.float64 if dtype == 64 else torch.float32, feat_grad)


# ---- the mask head: one box per pyramid level and more
MASK_BOXES = [np.array([[40, 60, 68, 88],            # 28 x 28      -> P2, bin 1/2
                        [120, 32, 232, 88],          # 112 x 56     -> P3, bins 1, 1/2
                        [272, 16, 496, 240]], F32),  # 224 x 224    -> P4, bin 1
              np.array([[16, 96, 72, 208],           # 56 x 112     -> P3
                        [32, -96, 480, 352]], F32)]  # 448 x 448    -> P5, bin 1, hangs over the image's top and bottom


def _gt_masks(boxes, tag):
    W, H = MASK_IMG
    out = np.zeros((len(boxes), H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for g, b in enumerate(boxes):
        cx, cy, rx, ry = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, (b[2] - b[0]) / 2.5, (b[3] - b[1]) / 2.5
        out[g] = (((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0).astype(np.uint8)
    return out


def mask_case(which):
    """which: 5 (two images, 3 + 2 positives), 1 (one image, one positive), 0 (two images, no positive among their proposals)"""
    tag = f"rht:mask:{which}"
    if which == 5:
        boxes = MASK_BOXES
    elif which == 1:
        boxes = [MASK_BOXES[0][1:2]]
    else:
        boxes = [np.zeros((0, 4), F32), np.zeros((0, 4), F32)]
    n = len(boxes)
    gt = MASK_BOXES[:n]
    gt_labels = [np.ones(len(g), np.int64) for g in gt]
    masks = [_gt_masks(g, tag) for g in gt]
    cls = np.concatenate([np.ones(len(b), np.int64) for b in boxes])
    targets = [DO.mask_target(masks[i][g], b, MASK_M) for i, bs in enumerate(boxes) for g, b in enumerate(bs)] if which == 5 else \
        [DO.mask_target(masks[0][1], boxes[0][0], MASK_M)] if which == 1 else []
    negatives = [np.array([[300, 100, 330, 140], [5, 5, 25, 30]], F32) + 7 * i for i in range(n)]      # label 0: the head drops them
    feats = real_pyramid(tag, n, MASK_SHAPES, MASK_C)[0]
    return SimpleNamespace(tag=tag, boxes=boxes, negatives=negatives, gt=gt, gt_labels=gt_labels, masks=masks, cls=cls,
                           targets=np.stack(targets) if targets else np.zeros((0, MASK_M, MASK_M), np.uint8), feats=feats,
                           params=TO.margin_mask_params(tag, feats, boxes, MASK_IMG[1], MASK_C, MASK_NCLS), img=MASK_IMG, shapes=MASK_SHAPES)


def mask_oracle(c, dtype, feat_grad=True):
    import torch
    return TO.mask_step(c.feats, c.boxes, c.img[1], c.params, c.cls, c.targets, torch.float64 if dtype == 64 else torch.float32, feat_grad)


# ---- both heads: the mask case's image and ground truths; proposals = the ground truths (aligned, IoU 1) and negatives
def combined_case(seed=None):
    seed = SEEDS["combined"] if seed is None else seed
    tag = f"rht:combined:{seed}"
    gl = [b[:2] for b in MASK_BOXES]                                   # two ground truths per image: at most 2 positives are sampled of 8
    gr = [g + np.array([-8, 0, -8, 0], F32) for g in gl]
    labels = [np.ones(len(g), np.int64) for g in gl]
    masks = [_gt_masks(g, tag) for g in gl]
    lp, rp = [], []
    for i, (a, b) in enumerate(zip(gl, gr)):
        far = uniform(f"{tag}:far{i}", (8, 4), 0.0, 1.0) * np.array([380, 60, 380, 60], F32)
        far[:, 0] += 100 * (i == 1)
        far[:, 1] += 130 * (i == 0)
        far[:, 2:] = far[:, :2] + 10 + far[:, 2:] * 0.4
        lp.append(np.concatenate([a, far]).astype(F32))
        rp.append(np.concatenate([b, far - np.array([5, 0, 5, 0], F32)]).astype(F32))
    total = sum(len(p) for p in lp)
    draws = uniform(f"{tag}:sample", (total,), 0.0, 1.0)
    smp = TO.sampled(lp, rp, gl, gr, labels, draws, BOX_BATCH, 0.25)
    R = sum(len(s[0]) for s in smp)
    fl, fr = real_pyramid(tag, 2, MASK_SHAPES, MASK_C)
    pos = [s[3][s[1] > 0][:, :4] for s in smp]
    tg = [DO.mask_target(masks[i][int(np.nonzero((gl[i] == b).all(1))[0][0])], b, MASK_M) for i, bs in enumerate(pos) for b in bs]
    return SimpleNamespace(tag=tag, left_props=lp, right_props=rp, gt_left=gl, gt_right=gr, gt_labels=labels, masks=masks, sample_draws=draws,
                           sampled=smp, R=R, feats_left=fl, feats_right=fr, box_params=box_params(tag, c=MASK_C),
                           mask_params=TO.margin_mask_params(tag, fl, pos, MASK_IMG[1], MASK_C, MASK_NCLS), dropout=uniform(f"{tag}:drop", (2, R, BOX_DIM), 0.0, 1.0),
                           pos_boxes=pos, mask_cls=np.concatenate([np.ones(len(b), np.int64) for b in pos]), mask_targets=np.stack(tg),
                           img=MASK_IMG, shapes=MASK_SHAPES)


def combined_oracle(c, dtype, box_params=None, mask_params=None, feat_grad=False):
    """-> (box_step dict, mask_step dict) at the case's parameters or at the given ones"""
    import torch
    dt = torch.float64 if dtype == 64 else torch.float32
    lb = [s[3][:, :4] for s in c.sampled]
    rb = [s[3][:, [4, 1, 5, 3]] for s in c.sampled]
    box = TO.box_step(c.feats_left, c.feats_right, lb, rb, c.img[1], box_params or c.box_params, np.concatenate([s[1] for s in c.sampled]),
                      np.concatenate([s[2] for s in c.sampled]), TO.dropout_keep(c.dropout, P_DROP), P_DROP, dt, feat_grad)
    mask = TO.mask_step(c.feats_left, c.pos_boxes, c.img[1], mask_params or c.mask_params, c.mask_cls, c.mask_targets, dt, feat_grad)
    return box, mask


@functools.lru_cache(maxsize=None)
def cached(name, *args):
    return globals()[name](*args)


def margins():
    """name -> (pre_lo, pre_hi) of every case in the fp64 oracle"""
    out = {}
    for name in ("box_full_case", "box_one_case"):
        r = box_oracle(cached(name), 64, feat_grad=False)
        out[name] = (r["pre_lo"], r["pre_hi"])
    for which in (5, 1):
        r = mask_oracle(cached("mask_case", which), 64, feat_grad=False)
        out[f"mask_case[{which}]"] = (r["pre_lo"], r["pre_hi"])
    b, m = combined_oracle(cached("combined_case"), 64)
    out["combined_case box"] = (b["pre_lo"], b["pre_hi"])
    out["combined_case mask"] = (m["pre_lo"], m["pre_hi"])
    return out


if __name__ == "__main__":                                # the seed search: python -m tests.roi_heads_train_cases
    for name, oracle in (("box_full", lambda s: box_oracle(box_full_case(s), 64, False)), ("box_one", lambda s: box_oracle(box_one_case(s), 64, False)),
                         ("combined", lambda s: combined_oracle(combined_case(s), 64)[0])):
        for seed in range(64):
            r = oracle(seed)
            ok = r["pre_lo"] >= 1e-4 * r["pre_hi"]
            print(name, seed, r["pre_lo"], r["pre_hi"], "OK" if ok else "")
            if ok:
                break
    for k, v in margins().items():
        print(k, v, v[0] >= 1e-4 * v[1])

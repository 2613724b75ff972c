"""The cases of tests/test_hip_srpn_train.py, built on the host so that tests/test_srpn_train_host.py can hold every one of them to the
ReLU-margin condition -- every hidden pre-activation at an active pixel at least 1e-4 of the largest away from zero in the fp64 oracle --
before the GPU sees it, so that no gradient element is ever excluded from a comparison.

Image 96 x 160, pyramid (24,40), (12,20), (6,10), (3,5), (2,3), A = 3 (the shipped anchor sizes and strides):
    full   N = 2, C = 8, BATCH_SIZE_PER_IMAGE 16, the ground truths of roi_heads_train_cases.BOX_GT (one hangs over the image), the right
           view's boxes shifted by the disparity
    wide   N = 1, C = 24
    none   N = 2, C = 8 in images so small (16 x 16, the pyramid kept) that no anchor is visible: nothing is sampled
The seeds were searched on the CPU (python -m tests.srpn_train_cases); a seed moves the pyramids, the weights and the sampler's draws.  The
search asks for 5e-4 where the tests assert 1e-4: the step recorded from the reference (tests/golden/make_golden_srpn_train.py) runs the
`full` case's inputs with the reference's own sample, and shares the positives' pixels.
"""
import functools
from types import SimpleNamespace

import numpy as np

from . import roi_heads_train_cases as RC
from . import srpn_train_oracle as TO

F32 = np.float32
IMG = (160, 96)                                               # (width, height)
SHAPES = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]
A = 3
BATCH, FRACTION = 16, 0.5
SEEDS = {"full": 4, "wide": 1, "none": 0}
GT_LEFT = RC.BOX_GT
GT_RIGHT = [g + s for g, s in zip(RC.BOX_GT, RC.BOX_GT_SHIFT)]


def uniform(key, shape, lo, hi):
    from disprcnn_amd.utils.synth import hash_uniform
    return hash_uniform(key, shape, lo, hi).numpy()


def head_params(tag, c):
    shapes = {TO.PARAMS[0]: (2 * c, c, 3, 3), TO.PARAMS[1]: (2 * c,), TO.PARAMS[2]: (2 * A, 4 * c, 1, 1), TO.PARAMS[3]: (2 * A,),
              TO.PARAMS[4]: (6 * A, 4 * c, 1, 1), TO.PARAMS[5]: (6 * A,)}
    out = {}
    for k, s in shapes.items():
        if k.endswith("bias"):
            out[k] = uniform(f"{tag}:{k}", s, -0.1, 0.1)
        else:
            a = np.sqrt(3.0 / np.prod(s[1:])) * (1.0 if "conv." in k else 2.0)
            out[k] = uniform(f"{tag}:{k}", s, -a, a)
    return out


def pyramid(tag, n, c):
    from disprcnn_amd.utils.synth import synth_pyramid
    fl, fr = synth_pyramid(n, IMG[1], IMG[0], c=c, tag=tag)
    assert [tuple(f.shape[2:]) for f in fl] == SHAPES
    return [f.numpy() for f in fl], [f.numpy() for f in fr]


def case(name, seed=None):
    seed = SEEDS[name] if seed is None else seed
    tag = f"srpn:{name}:{seed}"
    n, c = {"full": (2, 8), "wide": (1, 24), "none": (2, 8)}[name]
    img_whs = [(16, 16)] * n if name == "none" else [IMG] * n
    gl, gr = GT_LEFT[:n], GT_RIGHT[:n]
    fl, fr = pyramid(tag, n, c)
    total = sum(h * w for h, w in SHAPES) * A
    draws = uniform(f"{tag}:sample", (n * total,), 0.0, 1.0)
    labels, reg, pos, neg = TO.targets_and_sample(SHAPES, img_whs, gl, gr, draws, BATCH, FRACTION)
    return SimpleNamespace(name=name, tag=tag, n=n, c=c, img_whs=img_whs, gt_left=gl, gt_right=gr, feats_left=fl, feats_right=fr,
                           params=head_params(tag, c), draws=draws, labels=labels, reg=reg, pos=pos, neg=neg, total=total, shapes=SHAPES)


def oracle(c, dtype, feat_grad=True, pos=None, neg=None):
    import torch
    return TO.train_step(c.params, c.feats_left, c.feats_right, c.labels, c.reg, c.pos if pos is None else pos, c.neg if neg is None else neg,
                         torch.float64 if dtype == 64 else torch.float32, feat_grad)


@functools.lru_cache(maxsize=None)
def cached(name):
    return case(name)


@functools.lru_cache(maxsize=None)
def cached_oracle(name, dtype):
    """computed once and shared: the tests read it and leave it unchanged"""
    return oracle(cached(name), dtype)


def margins():
    out = {}
    for name in ("full", "wide"):
        r = oracle(cached(name), 64, feat_grad=False)
        out[name] = (r["pre_lo"], r["pre_hi"])
    return out


if __name__ == "__main__":                                    # the seed search: python -m tests.srpn_train_cases
    for name in ("full", "wide"):
        for seed in range(64):
            c = case(name, seed)
            r = oracle(c, 64, feat_grad=False)
            ok = r["pre_lo"] >= 5e-4 * r["pre_hi"]
            print(name, seed, "pos", int(c.pos.sum()), "neg", int(c.neg.sum()), "active pixels", r["n_active"], r["pre_lo"], r["pre_hi"], "OK" if ok else "")
            if ok:
                break
    c = case("none")
    print("none", int(c.pos.sum()), int(c.neg.sum()))

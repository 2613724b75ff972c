"""Records tests/golden/input_nearest_tables.npz from Pillow: the source index of every output row / column of
`Image.resize(size, NEAREST)` for eight shapes, read off a resized image whose pixels hold their own coordinate.  Arrays only.

    python tests/golden/make_golden_input.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
# (in_w, in_h, out_w, out_h)
SHAPES = [(1242, 375, 1987, 600), (1224, 370, 1984, 600), (37, 11, 57, 17), (100, 30, 50, 15), (7, 5, 7, 5), (123, 37, 196, 59),
          (9, 5, 31, 13), (375, 1242, 600, 1987)]


def pillow_tables(in_w, in_h, out_w, out_h):
    nearest = getattr(Image, "Resampling", Image).NEAREST
    xs = np.broadcast_to(np.arange(in_w, dtype=np.int32)[None, :], (in_h, in_w))
    ys = np.broadcast_to(np.arange(in_h, dtype=np.int32)[:, None], (in_h, in_w))
    rx = np.asarray(Image.fromarray(np.ascontiguousarray(xs), mode="I").resize((out_w, out_h), nearest))
    ry = np.asarray(Image.fromarray(np.ascontiguousarray(ys), mode="I").resize((out_w, out_h), nearest))
    assert (rx == rx[:1]).all() and (ry == ry[:, :1]).all()
    return ry[:, 0].astype(np.int32), rx[0].astype(np.int32)


if __name__ == "__main__":
    out = {"shapes": np.asarray(SHAPES, dtype=np.int32)}
    for k, s in enumerate(SHAPES):
        out[f"y{k}"], out[f"x{k}"] = pillow_tables(*s)
    np.savez_compressed(os.path.join(HERE, "input_nearest_tables.npz"), **out)

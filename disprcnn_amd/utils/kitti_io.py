"""KITTI object label lines of one image's prediction (reference: data/datasets/evaluation/kitti/kitti_eval.py:17-36, the text
`write_txt` hands to the KITTI evaluator).

    kitti_label_lines(prediction, label="Car") -> ["Car -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score", ...]

With a `box3d` field: the box converted to 'xyzhwl_ry' (through its corners, as every Box3DList conversion), alpha = ry + arctan(-x / z),
the score is `scores_3d`.  Without: the 2D form `label -1 -1 -10 x1 y1 x2 y2 0 0 0 0 0 0 0 score` with `scores`.  Numbers are written as
Python formats the floats of `.tolist()`, as the reference does.  No resize, no dataset, no evaluator: the caller passes the prediction
at the image size it wants and writes the lines where it wants ('\\n'.join(lines), one file per image).
"""
import numpy as np


def kitti_label_lines(prediction, label="Car"):
    lines = []
    bbox = prediction.bbox.tolist()
    if prediction.has_field("box3d"):
        bbox3d = prediction.get_field("box3d").convert("xyzhwl_ry").bbox_3d.tolist()
        scores_3d = prediction.get_field("scores_3d").tolist()
        for b, b3d, sc in zip(bbox, bbox3d, scores_3d):
            x1, y1, x2, y2 = b
            x, y, z, h, w, l, ry = b3d
            alpha = ry + np.arctan(-x / z)
            lines.append(f"{label} -1 -1 {alpha} {x1} {y1} {x2} {y2} {h} {w} {l} {x} {y} {z} {ry} {sc}")
    else:
        scores = prediction.get_field("scores").tolist()
        for b, s in zip(bbox, scores):
            x1, y1, x2, y2 = b
            lines.append(f"{label} -1 -1 -10 {x1} {y1} {x2} {y2} 0 0 0 0 0 0 0 {s}")
    return lines

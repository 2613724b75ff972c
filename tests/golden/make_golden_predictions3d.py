#!/usr/bin/env python3
"""Manifest of the reference's `predictions.pth` with 3D results, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predictions3d.py

The reference's own BoxList / Box3DList (disprcnn/structures/bounding_box.py, structures/bounding_box_3d.py) are filled with two images
of synthetic detections that carry what its 3D stage attaches (`box3d`, `scores_3d`, `random`; point_rcnn.py:combine_2d_3d) and saved the
way engine/inference.py:132-133 saves them (plain torch.save).  Recorded -- DATA ONLY, no pickled reference class travels: the class paths
and helper globals the file names, the instance-dict keys of a Box3DList, dtype, shape and values of every tensor, the KITTI label lines
the reference's write_txt expression (data/datasets/evaluation/kitti/kitti_eval.py:17-36) gives for the left lists, and two cross-checks
run here: this package's reader loads the reference's file, and the reference's own classes load the file this package writes.

Image 0 carries its boxes in 'ry_lhwxyz' (what the RCNN branch writes: the label lines then pass through the reference's corner
conversion), image 1 in 'xyzhwl_ry' (the conversion is the identity: the lines hold the stored floats themselves)."""
import json
import os
import pickletools
import sys
import tempfile
import zipfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True
for name in ("cv2", "pycocotools", "pycocotools.mask", "disprcnn._C"):
    sys.modules[name] = MagicMock()

from disprcnn.structures.bounding_box import BoxList as RefBoxList  # noqa: E402  (the reference)
from disprcnn.structures.bounding_box_3d import Box3DList as RefBox3DList  # noqa: E402

from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.structures.bounding_box_3d import Box3DList  # noqa: E402
from disprcnn_amd.utils import synth  # noqa: E402
from disprcnn_amd.utils.kitti_io import kitti_label_lines  # noqa: E402
from disprcnn_amd.utils.predictions_io import load_predictions, save_predictions  # noqa: E402

W, H = 1242, 375
ROIS = (3, 4)
MODES = ("ry_lhwxyz", "xyzhwl_ry")


def boxes3d(tag, r, mode):
    u = lambda k, lo, hi: synth.hash_uniform(f"{tag}:{k}", (r, 1), lo, hi)
    ry, l, h, w = u("ry", -3.1, 3.1), u("l", 3.0, 4.5), u("h", 1.3, 1.8), u("w", 1.4, 1.9)
    x, y, z = u("x", -12.0, 12.0), u("y", 1.0, 2.0), u("z", 6.0, 60.0)
    return torch.cat((ry, l, h, w, x, y, z) if mode == "ry_lhwxyz" else (x, y, z, h, w, l, ry), dim=1)


def build(cls_box, cls_box3d):
    out = {"left": [], "right": []}
    for side in ("left", "right"):
        for img, r in enumerate(ROIS):
            tag = f"pred3d:{side}{img}"
            b = cls_box(synth.hash_uniform(tag, (r, 4), 0.0, 300.0), (W, H))
            b.add_field("scores", synth.hash_uniform(tag + ":s", (r,), 0.0, 1.0))
            if side == "left":
                b.add_field("box3d", cls_box3d(boxes3d(tag, r, MODES[img]), size=(W, H), mode=MODES[img]))
                b.add_field("scores_3d", synth.hash_uniform(tag + ":s3", (r,), -4.0, 4.0))
                b.add_field("random", (synth.hash_uniform(tag + ":r", (r,), 0.0, 1.0) < 0.3).to(torch.int64))
            out[side].append(b)
    return out


def globals_of(path):
    z = zipfile.ZipFile(path)
    data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    return sorted({a for op, a, _ in pickletools.genops(data) if op.name == "GLOBAL"})


def tensor(t):
    return {"dtype": str(t.dtype), "shape": list(t.shape), "values": t.tolist()}


def plain(v):
    return str(v) if isinstance(v, torch.device) else list(v) if isinstance(v, tuple) else v


def describe(preds):
    d = {}
    for side, lst in preds.items():
        d[side] = []
        for b in lst:
            fields = {}
            for k, v in b.extra_fields.items():
                if torch.is_tensor(v):
                    fields[k] = tensor(v)
                else:
                    fields[k] = {"class": type(v).__name__, "state_keys": sorted(v.__dict__), "bbox_3d": tensor(v.bbox_3d),
                                 "state": {n: plain(x) for n, x in v.__dict__.items() if n != "bbox_3d"}}
            d[side].append({"size": list(b.size), "mode": b.mode, "bbox": tensor(b.bbox), "state_keys": sorted(b.__dict__),
                            "mask_thresh": b.mask_thresh, "fields": fields})
    return d


def reference_lines(prediction, label="Car"):
    """write_txt's per-image expression on the reference's own objects (without its dataset lookup, resize and evaluator call)"""
    lines = []
    bbox = prediction.bbox.tolist()
    bbox3d = prediction.get_field("box3d").convert("xyzhwl_ry").bbox_3d.tolist()
    scores_3d = prediction.get_field("scores_3d").tolist()
    scores = prediction.get_field("scores").tolist()
    for b, b3d, s3d, s in zip(bbox, bbox3d, scores_3d, scores):
        sc = s3d
        x1, y1, x2, y2 = b
        x, y, z, h, w, l, ry = b3d
        alpha = ry + np.arctan(-x / z)
        lines.append(f"{label} -1 -1 {alpha} {x1} {y1} {x2} {y2} {h} {w} {l} {x} {y} {z} {ry} {sc}")
    return lines


def same(a, b):
    for side in a:
        for x, y in zip(a[side], b[side]):
            assert tuple(x.size) == tuple(y.size) and x.mode == y.mode and torch.equal(x.bbox, y.bbox)
            assert list(x.extra_fields) == list(y.extra_fields)
            for k in x.extra_fields:
                u, v = x.extra_fields[k], y.extra_fields[k]
                if torch.is_tensor(u):
                    assert torch.equal(u, v) and u.dtype == v.dtype, k
                else:
                    assert u.mode == v.mode and tuple(u.size) == tuple(v.size) and torch.equal(u.bbox_3d, v.bbox_3d), k
    return True


def main():
    tmp = tempfile.mkdtemp()
    ref_preds = build(RefBoxList, RefBox3DList)
    ref_path = os.path.join(tmp, "predictions_ref.pth")
    torch.save(ref_preds, ref_path)                                   # engine/inference.py:132-133
    ours = build(BoxList, Box3DList)
    our_path = os.path.join(tmp, "predictions_ours.pth")
    save_predictions(ours, our_path)
    got = load_predictions(ref_path)                                  # our reader on the reference's file
    assert type(got["left"][0]) is BoxList and type(got["left"][0].get_field("box3d")) is Box3DList and same(got, ref_preds)
    back = torch.load(our_path, map_location="cpu", weights_only=False)   # the reference's classes on our file
    b3 = back["left"][0].get_field("box3d")
    assert type(back["left"][0]) is RefBoxList and type(b3) is RefBox3DList and same(back, ours)
    assert sorted(b3.__dict__) == sorted(ref_preds["left"][0].get_field("box3d").__dict__)
    lines = [reference_lines(b) for b in ref_preds["left"]]
    assert lines == [reference_lines(b) for b in back["left"]]        # the reference's expression on our file, loaded by its classes
    assert lines == [kitti_label_lines(b) for b in ours["left"]] == [kitti_label_lines(b) for b in got["left"]]
    manifest = {"reference_globals": globals_of(ref_path), "our_globals": globals_of(our_path), "layout": describe(ref_preds),
                "kitti_lines": lines, "our_reader_loads_reference_file": True, "reference_classes_load_our_file": True,
                "generator": "synth.hash_uniform tags pred3d:{left,right}{0,1}[:s|:s3|:r|:ry|:l|:h|:w|:x|:y|:z]; ROI counts (3, 4); "
                             "box3d modes (ry_lhwxyz, xyzhwl_ry)"}
    with open(os.path.join(HERE, "predictions3d_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest["reference_globals"]), "\n", json.dumps(manifest["our_globals"]), "\n", "\n".join(sum(lines, [])))


if __name__ == "__main__":
    main()

"""The 3D stage's way out of the process and into the detector, on the CPU: `box3d` through the predictions file (pinned by
tests/golden/predictions3d_manifest.json, which tests/golden/make_golden_predictions3d.py recorded from the reference's own BoxList /
Box3DList), the KITTI label lines, DispRCNN3D's construction with MODEL.DET3D_ON / MODEL.DISPNET_ON, and the C ABI of the frame-change
kernel."""
import copy
import json
import os
import pickle
import pickletools
import re
import sys
import types
import zipfile

import numpy as np
import pytest
import torch

from disprcnn_amd.structures.bounding_box import BoxList
from disprcnn_amd.structures.bounding_box_3d import Box3DList
from disprcnn_amd.utils import predictions_io as PIO
from disprcnn_amd.utils import synth
from disprcnn_amd.utils.kitti_io import kitti_label_lines
from disprcnn_amd.utils.predictions_io import load_predictions, save_predictions
from tests import rpn_oracle as RO

from .conftest import GOLDEN, ROOT

W, H = 1242, 375
with open(os.path.join(GOLDEN, "predictions3d_manifest.json")) as _f:
    MANIFEST = json.load(_f)
BOX3D_PATH = "disprcnn.structures.bounding_box_3d Box3DList"


def _build():
    out = {"left": [], "right": []}
    for side in ("left", "right"):
        for img, r in enumerate((3, 0, 5)):
            tag = f"p3:{side}{img}"
            b = BoxList(synth.hash_uniform(tag, (r, 4), 0.0, 300.0), (W, H))
            b.add_field("scores", synth.hash_uniform(tag + ":s", (r,), 0.0, 1.0))
            if side == "left":
                b7 = torch.cat([synth.hash_uniform(tag + ":ry", (r, 1), -3.1, 3.1), synth.hash_uniform(tag + ":lhw", (r, 3), 1.0, 5.0),
                                synth.hash_uniform(tag + ":xyz", (r, 3), -40.0, 40.0)], 1)
                b.add_field("box3d", Box3DList(b7, (W, H), "ry_lhwxyz"))
                b.add_field("scores_3d", synth.hash_uniform(tag + ":s3", (r,), -4.0, 4.0))
                b.add_field("random", (synth.hash_uniform(tag + ":r", (r,), 0.0, 1.0) < 0.3).to(torch.int64))
            out[side].append(b)
    return out


def _pickle_of(path):
    z = zipfile.ZipFile(path)
    return z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])


def _globals_of(path):
    return sorted({a for op, a, _ in pickletools.genops(_pickle_of(path)) if op.name == "GLOBAL"})


def _same_field(a, b):
    if torch.is_tensor(b):
        return torch.is_tensor(a) and a.dtype == b.dtype and a.device.type == "cpu" and torch.equal(a, b)
    return type(a) is Box3DList and a.mode == b.mode and a.size == b.size and a.bbox_3d.device.type == "cpu" and \
        a.bbox_3d.dtype == torch.float32 and torch.equal(a.bbox_3d, b.bbox_3d)


# ---- 1. round trip
def test_predictions_with_box3d_round_trip(tmp_path):
    path = str(tmp_path / "predictions.pth")
    preds = _build()
    save_predictions(preds, path)
    names = _globals_of(path)
    assert BOX3D_PATH in names and not any("disprcnn_amd" in n for n in names)
    back = load_predictions(path)
    assert sorted(back) == ["left", "right"]
    for side in preds:
        assert len(back[side]) == len(preds[side])
        for b, src in zip(back[side], preds[side]):
            assert type(b) is BoxList and b.size == src.size and b.mode == src.mode and torch.equal(b.bbox, src.bbox)
            assert sorted(b.fields()) == sorted(src.fields())
            for k in src.fields():
                assert _same_field(b.get_field(k), src.get_field(k)), (side, k)
    b3 = back["left"][2].get_field("box3d")
    assert b3.mode == "ry_lhwxyz" and b3.size == (W, H) and len(b3) == 5 and len(back["left"][1].get_field("box3d")) == 0
    assert b3.convert("xyzhwl_ry").bbox_3d.shape == (5, 7)                # a working object, not a bag of attributes
    evil = str(tmp_path / "evil.pth")
    torch.save({"left": [types.SimpleNamespace(a=1)]}, evil)              # a class path outside the format is still refused
    with pytest.raises(pickle.UnpicklingError):
        load_predictions(evil)


# ---- 2. the reference's own layout
def _tensor(d):
    t = torch.tensor(d["values"], dtype=getattr(torch, d["dtype"].split(".")[1])).reshape(d["shape"])
    assert str(t.dtype) == d["dtype"]
    return t


def _write_reference_layout(path):
    """A file of the layout the reference wrote (the manifest), from stand-in classes at the reference's class paths and plain torch.save."""
    saved, stubs = {}, {}
    try:
        for module, name in PIO._REF.values():
            parts = module.split(".")
            for i in range(1, len(parts) + 1):
                m = ".".join(parts[:i])
                if m not in saved:
                    saved[m] = sys.modules.get(m)
                    sys.modules[m] = types.ModuleType(m)
            stubs[name] = PIO._stub(module, name)
            setattr(sys.modules[module], name, stubs[name])
        out = {}
        for side, lst in MANIFEST["layout"].items():
            out[side] = []
            for want in lst:
                b = object.__new__(stubs["BoxList"])
                fields = {}
                for k, v in want["fields"].items():
                    if "class" in v:
                        o = object.__new__(stubs[v["class"]])
                        st = dict(v["state"])
                        st["device"], st["size"] = torch.device(st["device"]), tuple(st["size"])
                        o.__dict__.update(st, bbox_3d=_tensor(v["bbox_3d"]))
                        assert sorted(o.__dict__) == v["state_keys"]
                        fields[k] = o
                    else:
                        fields[k] = _tensor(v)
                b.__dict__.update(bbox=_tensor(want["bbox"]), size=tuple(want["size"]), mode=want["mode"], extra_fields=fields,
                                  PixelWise_map={}, mask_thresh=want["mask_thresh"])
                assert sorted(b.__dict__) == want["state_keys"]
                out[side].append(b)
        torch.save(out, path)
    finally:
        for m, old in saved.items():
            if old is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = old


def _box3d_state_keys():
    return next(v["state_keys"] for b in MANIFEST["layout"]["left"] for v in b["fields"].values() if "class" in v)


def test_reader_loads_the_reference_layout_and_writer_reproduces_it(tmp_path):
    assert MANIFEST["our_reader_loads_reference_file"] and MANIFEST["reference_classes_load_our_file"]
    assert BOX3D_PATH in MANIFEST["reference_globals"] and MANIFEST["our_globals"] == MANIFEST["reference_globals"]
    assert _box3d_state_keys() == ["bbox_3d", "device", "frame", "mode", "pose", "ry", "size"]
    ref_path = str(tmp_path / "ref_layout.pth")
    _write_reference_layout(ref_path)
    assert _globals_of(ref_path) == MANIFEST["reference_globals"]
    got = load_predictions(ref_path)
    n3d = 0
    for side, lst in MANIFEST["layout"].items():
        assert len(got[side]) == len(lst)
        for b, want in zip(got[side], lst):
            assert type(b) is BoxList and list(b.size) == want["size"] and b.mode == want["mode"] and torch.equal(b.bbox, _tensor(want["bbox"]))
            assert sorted(b.__dict__) == want["state_keys"] and list(b.extra_fields) == list(want["fields"])
            for k, v in want["fields"].items():
                f = b.get_field(k)
                if "class" in v:
                    n3d += 1
                    assert type(f) is Box3DList and sorted(f.__dict__) == v["state_keys"] and f.mode == v["state"]["mode"]
                    assert list(f.size) == v["state"]["size"] and f.frame == v["state"]["frame"]
                    assert [str(f.bbox_3d.dtype), list(f.bbox_3d.shape)] == [v["bbox_3d"]["dtype"], v["bbox_3d"]["shape"]]
                    assert torch.equal(f.bbox_3d, _tensor(v["bbox_3d"]))
                else:
                    assert [str(f.dtype), list(f.shape)] == [v["dtype"], v["shape"]] and torch.equal(f, _tensor(v))
    assert n3d == 2
    # what save_predictions writes for the loaded lists: the manifest's GLOBAL names and instance-dict keys, read from the raw pickle with
    # stand-ins (no class of this package takes part)
    our_path = str(tmp_path / "ours.pth")
    save_predictions(got, our_path)
    assert _globals_of(our_path) == MANIFEST["reference_globals"]

    class Raw(pickle.Unpickler):
        def find_class(self, module, name):
            if module.startswith("disprcnn."):
                return type(name, (object,), {"__module__": module})
            return super().find_class(module, name)

    raw = torch.load(our_path, map_location="cpu", weights_only=False,
                     pickle_module=types.SimpleNamespace(Unpickler=Raw, load=lambda f, **kw: Raw(f, **kw).load(), __name__="raw"))
    for side, lst in MANIFEST["layout"].items():
        for b, want in zip(raw[side], lst):
            assert type(b).__name__ == "BoxList" and sorted(b.__dict__) == want["state_keys"]
            for k, v in want["fields"].items():
                if "class" in v:
                    f = b.extra_fields[k]
                    assert type(f).__name__ == "Box3DList" and type(f).__module__ == "disprcnn.structures.bounding_box_3d"
                    assert sorted(f.__dict__) == v["state_keys"] and f.pose is None and f.ry is None and f.device == torch.device("cpu")
                    assert isinstance(f.size, tuple) and torch.equal(f.bbox_3d, _tensor(v["bbox_3d"]))


# ---- 3. KITTI lines
def _reference_line(label, b, b3d, sc):
    """kitti_eval.py:22-29 on `.tolist()` values"""
    x1, y1, x2, y2 = b
    x, y, z, h, w, l, ry = b3d
    alpha = ry + np.arctan(-x / z)
    return f"{label} -1 -1 {alpha} {x1} {y1} {x2} {y2} {h} {w} {l} {x} {y} {z} {ry} {sc}"


def _is_float_token(s):
    return re.fullmatch(r"-?\d+\.\d+(e[-+]?\d+)?|-?\d+e[-+]?\d+", s) is not None


@pytest.mark.parametrize("mode", ["ry_lhwxyz", "xyzhwl_ry"])
def test_kitti_lines_equal_the_reference_expression(mode):
    # depths from 3 m to 75 m, angles over the circle incl. negative ones, a box on the optical axis (x = 0), one behind it on the left
    xyzhwl_ry = torch.tensor([[0.0, 1.6, 12.0, 1.5, 1.6, 3.9, -1.2], [-7.5, 1.7, 3.0, 1.4, 1.7, 4.2, 0.3], [15.25, 2.1, 75.0, 1.6, 1.5, 3.5, 3.0],
                              [2.0, 1.5, 30.5, 1.7, 1.8, 4.4, -3.1], [-0.125, 1.4, 48.0, 1.3, 1.9, 3.3, 1.5707964]])
    n = len(xyzhwl_ry)
    b7 = xyzhwl_ry if mode == "xyzhwl_ry" else xyzhwl_ry[:, [6, 5, 3, 4, 0, 1, 2]]
    p = BoxList(synth.hash_uniform("kitti:b", (n, 4), 0.0, 370.0), (W, H))
    p.add_field("scores", synth.hash_uniform("kitti:s", (n,), 0.0, 1.0))
    lines2d = kitti_label_lines(p)
    assert lines2d == [f"Car -1 -1 -10 {b[0]} {b[1]} {b[2]} {b[3]} 0 0 0 0 0 0 0 {s}" for b, s in zip(p.bbox.tolist(), p.get_field("scores").tolist())]
    p.add_field("box3d", Box3DList(b7, (W, H), mode))
    p.add_field("scores_3d", synth.hash_uniform("kitti:s3", (n,), -5.0, 5.0))
    lines = kitti_label_lines(p, label="Pedestrian")
    conv = p.get_field("box3d").convert("xyzhwl_ry").bbox_3d.tolist()
    want = [_reference_line("Pedestrian", b, b3, s) for b, b3, s in zip(p.bbox.tolist(), conv, p.get_field("scores_3d").tolist())]
    assert lines == want and len(lines) == n
    for ln, b3 in zip(lines, conv):
        tok = ln.split(" ")
        assert len(tok) == 16 and tok[:3] == ["Pedestrian", "-1", "-1"] and all(_is_float_token(t_) for t_ in tok[3:])
        assert float(tok[14]) == b3[6] and abs(float(tok[3]) - (b3[6] + np.arctan2(-b3[0], b3[2]))) < 1e-12       # z > 0: arctan = arctan2
    assert float(lines[0].split(" ")[3]) == conv[0][6]                     # x = 0: alpha is ry
    assert any(c[6] < 0 for c in conv)
    empty = BoxList(torch.zeros(0, 4), (W, H))
    empty.add_field("scores", torch.zeros(0))
    assert kitti_label_lines(empty) == []
    empty.add_field("box3d", Box3DList(torch.zeros(0, 7), (W, H), "ry_lhwxyz"))
    empty.add_field("scores_3d", torch.zeros(0))
    assert kitti_label_lines(empty) == []


def test_kitti_lines_equal_the_reference_recording(tmp_path):
    """The lines the reference's write_txt expression gave for the manifest's fixture.  Image 1 stores 'xyzhwl_ry': no arithmetic but the
    double-precision arctan lies between the stored floats and the text, and the lines must be equal.  Image 0 stores 'ry_lhwxyz', so the
    reference's numbers went through its fp32 corner conversion (cos, sin, a 3x3 product, norms, atan2 from torch's CPU kernels): every
    token that is not a float is equal, every float within 4 eps32 * 64 = 3.1e-5 (|coordinate| < 64; a product sum of three terms and a
    difference of two such values).  On the recording host the lines were equal (the recorder asserts that).  The bound instead of
    equality is a precaution, not an observation: torch dispatches those CPU kernels by the host's vector units and no second kind of
    host was at hand to see whether the last bits move.  Exactness of the text itself is held by the in-test comparison above and by
    image 1."""
    ref_path = str(tmp_path / "ref_layout.pth")
    _write_reference_layout(ref_path)
    left = load_predictions(ref_path)["left"]
    assert [len(kitti_label_lines(b)) for b in left] == [len(b) for b in left] == [len(x) for x in MANIFEST["kitti_lines"]]
    assert left[1].get_field("box3d").mode == "xyzhwl_ry" and kitti_label_lines(left[1]) == MANIFEST["kitti_lines"][1]
    assert left[0].get_field("box3d").mode == "ry_lhwxyz"
    for got, want in zip(kitti_label_lines(left[0]), MANIFEST["kitti_lines"][0]):
        g, w_ = got.split(" "), want.split(" ")
        assert len(g) == len(w_) == 16 and g[:3] == w_[:3]
        for a, b in zip(g[3:], w_[3:]):
            print(a, b)
            assert _is_float_token(a) and abs(float(a) - float(b)) <= 4 * float(np.finfo(np.float32).eps) * 64
        assert g[4:8] == w_[4:8] and g[15] == w_[15]                       # the 2D box and the score are stored values


# ---- 4. construction and state dict
def _pointrcnn_cfg(rcnn=True, trained=""):
    with open(os.path.join(GOLDEN, "rcnn_cfg_car.json")) as f:
        c = json.load(f)
    c["RCNN"]["ENABLED"] = rcnn
    c["TRAINED_MODEL"] = trained
    return RO.make_cfg(c)


def _cfg(dispnet=True, rcnn=True, trained=""):
    from disprcnn_amd.modeling.detector.disprcnn3d import default_cfg
    cfg = default_cfg()
    cfg.MODEL.DET3D_ON, cfg.MODEL.DISPNET_ON, cfg.MODEL.POINTRCNN = True, dispnet, _pointrcnn_cfg(rcnn, trained)
    return cfg


def test_disprcnn3d_with_det3d_state_dict_keys_and_trained_model(tmp_path):
    from disprcnn_amd.modeling.detector import build_detection_model
    from disprcnn_amd.modeling.detector.disprcnn3d import DispRCNN3D, default_cfg
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN
    alone = PointRCNN(_cfg())
    want = {"pcnet." + k for k in alone.state_dict()}
    assert any(k.startswith("pcnet.rpn.") for k in want) and any(k.startswith("pcnet.rcnn_net.") for k in want)
    plain = set(DispRCNN3D(default_cfg()).state_dict())
    assert plain and all(k.startswith("dispnet.") for k in plain)
    both = build_detection_model(_cfg())
    assert type(both) is DispRCNN3D and set(both.state_dict()) == plain | want
    offline = DispRCNN3D(_cfg(dispnet=False))
    assert not hasattr(offline, "dispnet") and set(offline.state_dict()) == want
    rpn_only = DispRCNN3D(_cfg(dispnet=False, rcnn=False))
    keys = set(rpn_only.state_dict())
    assert keys and all(k.startswith("pcnet.rpn.") for k in keys) and keys == {k for k in want if k.startswith("pcnet.rpn.")}
    # MODEL.POINTRCNN.TRAINED_MODEL: a checkpoint of the wrapped stand-alone network; keys without 'module.' do not count
    g = torch.Generator().manual_seed(5)
    sd = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone() + 3) for k, v in alone.state_dict().items()}
    ckpt = {"module." + k: v for k, v in sd.items()}
    first = next(iter(sd))
    ckpt[first] = torch.full_like(sd[first], 77.0)                         # same name without the prefix: ignored
    ckpt["optimizer_step"] = torch.zeros(1)
    path = str(tmp_path / "pointrcnn.pth")
    torch.save({"model": ckpt}, path)
    m = DispRCNN3D(_cfg(dispnet=False, trained=path))
    got = m.pcnet.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    # a whole-detector checkpoint is loaded first, then TRAINED_MODEL wins again (reference :317-323)
    m.load_state_dict({k: torch.zeros_like(v) for k, v in m.state_dict().items()})
    got = m.pcnet.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    m.train()
    with pytest.raises(NotImplementedError, match="PointRCNN"):
        m({"left": None, "right": None}, {"left": [], "right": []}, {"left": []})
    both.train()
    with pytest.raises(NotImplementedError, match="PointRCNN"):
        both({"left": None, "right": None}, {"left": [], "right": []}, {"left": []})
    with pytest.raises(ValueError):
        offline.eval()({"left": None, "right": None}, {"left": [], "right": []})      # evaluation without lr_targets
    # neither stage: nothing to train, said so instead of failing on a missing attribute
    cfg = default_cfg()
    cfg.MODEL.DISPNET_ON = False
    bare = DispRCNN3D(cfg)
    assert not list(bare.state_dict())
    with pytest.raises(NotImplementedError, match="DISPNET_ON"):
        bare.train()({"left": None, "right": None}, {"left": [], "right": []}, {"left": []})
    assert bare.eval()({"left": None, "right": None}, {"left": [], "right": []}) == {"left": [], "right": []}


# ---- 5. C ABI
def test_frame_change_entry_is_declared_bound_and_built():
    from disprcnn_amd.pts import _lib, build
    name = "drc_rpn_to_camera_fwd"
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    src_name = next(s for s in build.SOURCES if name in open(os.path.join(ROOT, "disprcnn_amd", "pts", s)).read())
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", src_name)).read()
    assert name in _lib.EXPORTED_SYMBOLS
    decl = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    defn = re.search(r'extern "C" int\s+%s\s*\(([^{]*?)\)\s*\{' % name, src, re.S)
    assert decl and defn
    norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]
    assert norm(decl.group(1)) == norm(defn.group(1)) and len(norm(decl.group(1))) == len(_lib._SIGS[name][1]) == 11
    assert "const double* rot" in decl.group(1)
    assert "asm" not in src and "__shared__" not in src                   # plain C++, no LDS

"""Host tests of the KITTI scoring: tests/kitti_eval_oracle.py (the NumPy restatement the GPU tests lean on) is held to what the KITTI
evaluator programs wrote (tests/golden/kitti_eval_golden.npz), the fixtures are checked for the cases the GPU tests need, and the host
half of layers/kitti_eval.py (label parser, threshold selection, stats files) and the C ABI's three descriptions are checked.  No GPU."""
import os
import re

import numpy as np
import pytest

from . import kitti_eval_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SETS = ("main_car", "main_pedestrian", "main_cyclist", "empty_frames", "empty_difficulty", "few_matches", "equal_scores", "limits", "classes",
        "no_aos", "only_2d", "dontcare", "det_counts", "frames_1", "frames_2", "frames_257", "write_txt_car", "write_txt_car_2d")


@pytest.fixture(scope="module")
def G():
    path = os.path.join(HERE, "golden", "kitti_eval_golden.npz")
    assert os.path.getsize(path) < (1 << 20)
    return np.load(path)


def test_fixture_sets_are_the_ones_the_tests_name(G):
    assert tuple(sorted(SETS)) == tuple(O.golden_sets(G))


@pytest.mark.parametrize("name", SETS)
def test_oracle_reproduces_the_evaluator_programs(G, name):
    """The programs print %f: a recorded value is within 5e-7 of the true one, and the oracle is fp64 like them."""
    _, gt, det = O.golden_frames(G, name)
    for program in O.PROGRAMS:
        for cls in O.CLASS_NAMES:
            want = O.golden_stats(G, name, program, cls)
            got = O.evaluate(gt, det, cls, program)
            assert set(got) == set(want), (program, cls)
            for k in want:
                assert np.abs(got[k] - want[k]).max() <= 1e-6, (program, cls, k)


def test_fixtures_hold_the_cases_the_checks_need(G):
    from disprcnn_amd.layers import kitti_eval as K
    for name in ("main_car", "main_pedestrian", "main_cyclist"):
        for program in O.PROGRAMS:
            st = O.golden_stats(G, name, program, name[5:])
            assert set(st) == set(O.STATS) and all((a != 0).any(axis=1).all() for a in st.values()), (name, program)
    assert np.any(np.diff(G["main_cyclist/frames"]) > 1)                                            # sparse frame indices
    car = lambda name, program=0.7: O.golden_stats(G, name, program, "car")
    assert (car("empty_difficulty")["detection"][0] == 0).all() and (car("empty_difficulty")["detection"][1] != 0).any()
    assert (car("few_matches")["detection"][:, -1] == 0).all() and (car("few_matches")["detection"][:, 0] != 0).all()
    assert set(car("no_aos")) == {"detection", "detection_ground", "detection_3d"} and set(car("only_2d")) == {"detection"}
    assert O.golden_stats(G, "empty_frames", 0.7, "pedestrian") == {}
    counts = G["empty_frames/gt_count"].tolist(), G["empty_frames/det_count"].tolist()
    pairs = list(zip(*counts))
    assert any(g == 0 and d > 0 for g, d in pairs) and any(g > 0 and d == 0 for g, d in pairs) and (0, 0) in pairs
    _, gt, _ = O.golden_frames(G, "empty_frames")
    assert any(f and all(x.startswith("DontCare") for x in f) for f in gt)
    assert G["det_counts/det_count"].tolist() == [63, 64, 65, 256]
    assert [len(G[f"frames_{n}/frames"]) for n in (1, 2, 257)] == [1, 2, 257]
    # limit values in the ground truth and the detections, equal scores, the classes of the class-handling set
    _, gt, det = O.golden_frames(G, "limits")
    g = np.concatenate([K.parse_label_lines(f, "gt")[1] for f in gt])
    d = np.concatenate([K.parse_label_lines(f, "det")[1] for f in det])
    assert {25.0, 40.0} <= set((g[:, 6] - g[:, 4]).round(6)) and {25.0, 40.0} <= set((d[:, 4] - d[:, 2]).round(6))
    assert {0.15, 0.3, 0.5} <= set(g[:, 0]) and {0, 1, 2, 3} <= set(g[:, 1])
    _, _, det = O.golden_frames(G, "equal_scores")
    scores = np.concatenate([K.parse_label_lines(f, "det")[1][:, 12] for f in det])
    assert len(set(scores)) < len(scores) // 4
    _, gt, det = O.golden_frames(G, "classes")
    assert {"Van", "Person_sitting", "car", "PEDESTRIAN"} <= {x.split()[0] for f in gt for x in f}
    assert {"Truck", "Tram", "CAR"} <= {x.split()[0] for f in det for x in f}
    # a DontCare region absorbs a detection: without the DontCare rows the recorded precision is not reached
    _, gt, det = O.golden_frames(G, "dontcare")
    without = O.evaluate([[x for x in f if not x.startswith("DontCare")] for f in gt], det, "car", 0.7)["detection"]
    assert (without < car("dontcare")["detection"] - 1e-3).any()


def test_label_parser():
    from disprcnn_amd.layers import kitti_eval as K
    lines = ["Car 0.15 2 -1.57 10.00 20.00 110.50 80.25 1.50 1.60 3.90 -2.00 1.65 20.00 0.30", "",
             "DontCare -1 -1 -10 1.00 2.00 3.00 4.00 -1 -1 -1 -1000 -1000 -1000 -10"]
    types, v = K.parse_label_lines(lines, "gt")
    assert types == ["Car", "DontCare"] and v.shape == (2, 14) and v.dtype == np.float64
    assert v[0].tolist() == [0.15, 2.0, -1.57, 10.0, 20.0, 110.5, 80.25, 1.5, 1.6, 3.9, -2.0, 1.65, 20.0, 0.3]
    assert v[1].tolist() == [-1, -1, -10, 1, 2, 3, 4, -1, -1, -1, -1000, -1000, -1000, -10]
    types, v = K.parse_label_lines(["car -1 -1 0.1 1 2 3 4 1.5 1.6 3.9 0.5 1.6 20 -0.2 0.875"], "det")
    assert types == ["car"] and v.tolist() == [[0.1, 1, 2, 3, 4, 1.5, 1.6, 3.9, 0.5, 1.6, 20, -0.2, 0.875]]
    assert K.parse_label_lines([], "det")[1].shape == (0, 13) and K.parse_label_lines(["", " "], "gt")[1].shape == (0, 14)
    with pytest.raises(ValueError):
        K.parse_label_lines(["Car -1 -1 0.1 1 2 3 4 1.5 1.6 3.9 0.5 1.6 20 -0.2"], "det")       # a ground-truth line: no score
    with pytest.raises(ValueError):
        K.parse_label_lines([], "other")
    assert K.gt_class_codes(["Car", "VAN", "dontcare", "Person_sitting", "Truck"], "car").tolist() == [0, 1, 2, 3, 3]
    assert K.gt_class_codes(["Pedestrian", "Van", "DontCare", "person_Sitting"], "Pedestrian").tolist() == [0, 3, 2, 1]
    assert K.gt_class_codes(["Cyclist", "Van", "Person_sitting"], "cyclist").tolist() == [0, 3, 3]
    assert K.det_class_codes(["CAR", "Van", "car"], "Car").tolist() == [0, 1, 0]
    det = [K.parse_label_lines(["Car -1 -1 0.1 1 2 3 4 1.5 1.6 3.9 0.5 1.6 20 -0.2 0.9"], "det"),
           K.parse_label_lines(["Pedestrian -1 -1 -10 1 2 3 4 0 0 0 0 0 0 0 0.5"], "det")]
    assert K.load_flags(det, "car") == (False, True, True, True) and K.load_flags(det, "pedestrian") == (False, True, False, False)
    assert K.load_flags(det[:1], "car")[0] is True and K.load_flags(det, "cyclist") == (False, False, False, False)


def test_threshold_selection_is_the_devkit_walk():
    from disprcnn_amd.layers import kitti_eval as K
    rs = np.random.RandomState(5)
    for n_gt, n in [(1, 1), (7, 3), (40, 40), (41, 41), (100, 37), (1000, 640), (5000, 5000), (300, 1)]:
        v = np.sort(np.round(rs.uniform(0, 1, n), 2))[::-1]                   # rounded: ties
        want = O.get_thresholds(list(v), n_gt)
        got = K.select_thresholds(v, n_gt)
        assert got.tolist() == want and len(got) <= 41
    assert K.select_thresholds(np.zeros(0), 5).shape == (0,)


def test_stats_files_round_trip(tmp_path, G):
    from disprcnn_amd.layers import kitti_eval as K
    st = O.golden_stats(G, "main_car", 0.7, "car")
    K.write_stats_files(str(tmp_path), "Car", {k: st[k] for k in ("detection", "detection_3d")})
    assert sorted(os.listdir(tmp_path)) == ["stats_car_detection.txt", "stats_car_detection_3d.txt"]
    text = open(tmp_path / "stats_car_detection.txt").read()
    assert text.count("\n") == 3 and text.split("\n")[0].endswith(" ") and len(text.split("\n")[0].split()) == 41
    assert re.fullmatch(r"(\d+\.\d{6} ){41}", text.split("\n")[1])
    assert np.array_equal(K.read_stats_file(str(tmp_path / "stats_car_detection.txt")), st["detection"])      # %f of a %f value
    K.write_stats_files(str(tmp_path), "car", {"detection": st["detection"]})                                 # a stale file goes
    assert os.listdir(tmp_path) == ["stats_car_detection.txt"]
    assert K.format_stats(np.full((3, 41), 1 / 3)).split()[0] == "0.333333"


def test_min_overlap_tables():
    from disprcnn_amd.layers import kitti_eval as K
    assert K._min_overlaps("Car", 0.7) == (0.7, 0.7, 0.7) and K._min_overlaps("car", 0.5) == (0.5, 0.5, 0.5)
    assert K._min_overlaps("pedestrian", 0.7) == (0.5, 0.5, 0.5) and K._min_overlaps("Cyclist", 0.7) == (0.5, 0.5, 0.5)
    assert K._min_overlaps("car", (0.7, 0.5, 0.25)) == (0.7, 0.5, 0.25)
    with pytest.raises(ValueError):
        K._min_overlaps("car", 0.6)


def test_evaluate_dispatches_by_class_name(monkeypatch):
    from disprcnn_amd.data.datasets import evaluation as E
    from disprcnn_amd.data.datasets.evaluation.kitti import kitti_eval as KE
    calls = []
    monkeypatch.setattr(KE, "write_txt", lambda dataset, predictions, output_folder, label="Car": calls.append((predictions, output_folder, label)) or label)
    kw = dict(class2type=None, box_only=False, iou_types=("bbox",), expected_results=[], expected_results_sigma_tol=4, eval_bbox3d=True)
    for cls_name, label in (("KITTIObjectDatasetCar", "Car"), ("KITTIObjectDatasetPedestrian", "Pedestrian"), ("KITTIObjectDatasetCyclist", "Cyclist")):
        ds = type(cls_name, (), {})()
        assert E.evaluate(ds, {"left": "L", "right": "R"}, "out", **kw) == label
        assert calls[-1] == ("L", "out", label)
    sub = type("Mine", (type("KITTIObjectDatasetCyclist", (), {}),), {})()
    assert E.evaluate(sub, {"left": "L", "right": "R"}, "out", **kw) == "Cyclist"
    with pytest.raises(NotImplementedError):
        E.evaluate(object(), {"left": "L", "right": "R"}, "out", **kw)
    from disprcnn.data.datasets.evaluation import evaluate
    assert evaluate is E.evaluate
    assert KE.DEFAULT_GT_DIR == os.path.join(ROOT, "data/kitti/object/training/label_2")


def test_header_symbols_and_sources_agree_for_the_new_entries():
    from disprcnn_amd.pts import _lib, build
    header = open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "kitti_eval.hip")).read()
    assert "kitti_eval.hip" in build.SOURCES
    names = [n for n in _lib.EXPORTED_SYMBOLS if n.startswith("drc_kitti_eval_")]
    assert sorted(names) == sorted(set(re.findall(r'extern "C" int\s+(drc_kitti_eval_\w+)', src))) and len(names) == 7
    ctype = {"int": _lib._I, "int64_t": _lib._L, "double": _lib._D}
    for name in names:
        decl = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r'extern "C" int\s+%s\s*\(([^{]*?)\)\s*\{' % name, src, re.S)
        assert decl and defn, name
        norm = lambda s: [" ".join(p.split()) for p in s.split(",") if p.strip() not in ("", "void")]
        assert norm(decl.group(1)) == norm(defn.group(1)), name
        want = [_lib._P if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in norm(decl.group(1))]
        assert want == _lib._SIGS[name][1], name
    assert "drc_kitti_eval_max_det() = %d" % int(re.search(r"kMaxDet = (\d+)", src).group(1)) in header
    assert "drc_kitti_eval_max_gt() = %d" % int(re.search(r"kMaxGt = (\d+)", src).group(1)) in header

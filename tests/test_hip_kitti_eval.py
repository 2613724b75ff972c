"""The KITTI scoring on the MI355X (disprcnn_amd/layers/kitti_eval.py over pts/kitti_eval.hip) against what the KITTI evaluator programs
wrote for the same label files (tests/golden/kitti_eval_golden.npz, see tests/golden/make_golden_kitti_eval.py), the overlap kernel alone
against the NumPy oracle (tests/kitti_eval_oracle.py), and the reference's entry points (write_txt, evaluate) on stub datasets.

Tolerances.  The programs print %f, so a recorded value is within 5e-7 of the value they computed; precision is a ratio of integer counts
and the orientation similarity an fp64 sum of at most a few hundred terms, so 1e-6 covers the print alone.  The overlaps are fp64 on both
sides from differently ordered operations on coordinates below 1e3: 1e-9 absolute is four orders above their rounding.  The image overlap
is the same expression in the same order and is compared bit for bit.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import kitti_eval_oracle as O
from tests.test_kitti_eval_host import SETS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "kitti_eval_golden.npz"))


def write_label_dirs(root, frames, gt, det):
    res, gtd = os.path.join(str(root), "res"), os.path.join(str(root), "gt")
    os.makedirs(res)
    os.makedirs(gtd)
    for f, g, d in zip(frames, gt, det):
        with open(os.path.join(gtd, "%06d.txt" % f), "w") as fh:
            fh.write("\n".join(g))
        with open(os.path.join(res, "%06d.txt" % f), "w") as fh:
            fh.write("\n".join(d))
    return res, gtd


def stats_files(res, cls):
    return {s for s in O.STATS if os.path.exists(os.path.join(res, f"stats_{cls}_{s}.txt"))}


# ---- 1. the recorded programs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_eval_label_dirs_reproduces_the_evaluator_programs(G, tmp_path, name):
    """Every fixture set through both overlap tables and all three classes: the same metrics present, every value within 1e-6, and the
    stats files written in the programs' format."""
    from disprcnn_amd.layers import kitti_eval as K
    frames, gt, det = O.golden_frames(G, name)
    res, gtd = write_label_dirs(tmp_path, frames, gt, det)
    worst = 0.0
    for program in O.PROGRAMS:
        for cls in O.CLASS_NAMES:
            want = O.golden_stats(G, name, program, cls)
            got = K.eval_label_dirs(res, gtd, cls=cls, min_overlap=program)
            assert set(got) == set(want) == stats_files(res, cls), (program, cls, sorted(got), sorted(want))
            for k in want:
                assert got[k].shape == (3, 41) and got[k].dtype == np.float64
                err = np.abs(got[k] - want[k]).max()
                worst = max(worst, err)
                assert err <= 1e-6, (program, cls, k, err)
                on_disk = K.read_stats_file(os.path.join(res, f"stats_{cls}_{k}.txt"))
                assert np.abs(on_disk - want[k]).max() <= 1e-6 and np.abs(on_disk - got[k]).max() <= 5.0000001e-7
    print(f"{name}: max |stats - recorded| = {worst:.3e}")


def test_a_frame_above_the_detection_limit_raises(G):
    from disprcnn_amd.layers import kitti_eval as K
    from disprcnn_amd.pts import _lib
    limit = _lib.lib().drc_kitti_eval_max_det()
    assert limit >= 128 and _lib.lib().drc_kitti_eval_max_gt() >= 64
    _, gt, det = O.golden_frames(G, "det_counts")
    assert len(det[3]) == limit                                         # the frame at the limit is part of the golden match above
    gt_frames = [K.parse_label_lines(f, "gt") for f in gt]
    det_frames = [K.parse_label_lines(f, "det") for f in det[:3]] + [K.parse_label_lines(det[3] + det[0][:1], "det")]
    with pytest.raises(RuntimeError, match="at most"):
        K.kitti_eval_stats(gt_frames, det_frames, "car", 0.7)
    # the library itself: a negative status, nothing launched
    L = _lib.lib()
    null = None
    st = L.drc_kitti_eval_pass1(1, 1, limit + 1, limit + 1, 1, limit + 1, null, null, null, null, null, null, null, null, null, 7, 0.7, 0.7, 0.7,
                                null, null, null)
    assert st == -3
    st = L.drc_kitti_eval_pass2(1, 1, limit + 1, limit + 1, 1, limit + 1, null, null, null, null, null, null, null, null, null, 7, 0.7, 0.7, 0.7,
                                1, null, null, null, null, null)
    assert st == -3
    assert L.drc_kitti_eval_overlaps(1, 4, null, null, null, null, null, null, 7, null, null) == -1
    assert L.drc_kitti_eval_overlaps(1, 4, null, null, null, null, null, null, 8, null, null) == -2


# ---- 2. the overlap kernel alone ------------------------------------------------------------------------------------------------------------
def gt_row(typ, box, h, w, l, t1, t2, t3, ry):
    return (typ, 0.0, 0, 0.0) + tuple(float(x) for x in box) + tuple(float(x) for x in (h, w, l, t1, t2, t3, ry))


def det_row(box, h, w, l, t1, t2, t3, ry):
    return ("Car", 0.0) + tuple(float(x) for x in box) + tuple(float(x) for x in (h, w, l, t1, t2, t3, ry)) + (0.5,)


def gpu_overlaps(gt_rows, det_rows):
    from disprcnn_amd.layers import kitti_eval as K
    gt = ([r[0] for r in gt_rows], np.array([r[1:] for r in gt_rows], np.float64).reshape(-1, 14))
    det = ([r[0] for r in det_rows], np.array([r[1:] for r in det_rows], np.float64).reshape(-1, 13))
    out = K.frame_overlaps(gt, det, "car")
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (3, len(gt_rows), len(det_rows))
    return out.cpu().numpy()


def oracle_overlaps(gt_rows, det_rows):
    return np.stack([O.pair_overlaps(gt_rows, det_rows, m) for m in range(3)])


def test_overlaps_match_the_oracle_on_random_pairs():
    rs = np.random.RandomState(11)

    def boxes(n):
        x1, y1 = rs.uniform(0, 300, n), rs.uniform(0, 100, n)
        return np.stack([x1, y1, x1 + rs.uniform(5, 200, n), y1 + rs.uniform(5, 120, n)], 1)

    def dims(n):
        return (rs.uniform(1, 2.5, n), rs.uniform(0.5, 3, n), rs.uniform(0.5, 6, n), rs.uniform(-3, 3, n), rs.uniform(1, 2.5, n),
                rs.uniform(-3, 3, n), rs.uniform(-2 * math.pi, 2 * math.pi, n))

    nG, nD = 37, 70                                                   # 2590 pairs: more than one workgroup, not a multiple of it
    gb, db, gd, dd = boxes(nG), boxes(nD), dims(nG), dims(nD)
    gt_rows = [gt_row("DontCare" if i % 5 == 4 else "Car", gb[i], *[a[i] for a in gd]) for i in range(nG)]
    gt_rows[4] = ("DontCare", -1.0, -1, -10.0) + tuple(gb[4]) + (-1.0, -1.0, -1.0, -1000.0, -1000.0, -1000.0, -10.0)   # KITTI's own form
    det_rows = [det_row(db[i], *[a[i] for a in dd]) for i in range(nD)]
    got, want = gpu_overlaps(gt_rows, det_rows), oracle_overlaps(gt_rows, det_rows)
    assert (want[1] > 0.05).sum() > 200 and (want[2] > 0.05).sum() > 100 and (want[1] == 0).sum() > 50
    assert np.array_equal(got[0], want[0])                            # the image overlap: bit for bit
    err = np.abs(got - want).max(axis=(1, 2))
    print("max |overlap - oracle|: image %.1e  ground %.1e  3d %.1e" % tuple(err))
    assert (err <= 1e-9).all()
    assert (got[1:, 4] == 0).all()                                    # nothing reaches a DontCare row's placeholder box at -1000


def test_overlaps_on_the_hard_geometric_cases():
    img = (10.0, 10.0, 60.0, 50.0)
    s2 = math.sqrt(2.0)
    # name, ground truth (h, w, l, t1, t2, t3, ry), detection, expected ground and 3d overlap
    cases = [
        ("identical", (1.5, 1.6, 3.9, 2.0, 1.7, 20.0, 0.4), (1.5, 1.6, 3.9, 2.0, 1.7, 20.0, 0.4), 1.0, 1.0),
        ("ry and ry + pi", (1.5, 1.6, 3.9, 2.0, 1.7, 20.0, 0.4), (1.5, 1.6, 3.9, 2.0, 1.7, 20.0, 0.4 + math.pi), 1.0, 1.0),
        ("square turned by 90 degrees", (2.0, 3.0, 3.0, -1.0, 1.5, 12.0, 0.7), (2.0, 3.0, 3.0, -1.0, 1.5, 12.0, 0.7 + math.pi / 2), 1.0, 1.0),
        ("one inside the other", (2.0, 4.0, 6.0, 0.0, 2.0, 10.0, 0.3), (1.0, 1.0, 2.0, 0.5, 1.5, 10.2, 1.1), 2.0 / 24.0, 2.0 / 48.0),
        ("sharing an edge", (1.0, 2.0, 2.0, 1.0, 1.0, 1.0, 0.0), (1.0, 2.0, 2.0, 3.0, 1.0, 1.0, 0.0), 0.0, 0.0),
        ("sharing an edge, both turned", (1.0, 2.0, 2.0, 1.0, 1.0, 1.0, math.pi / 2), (1.0, 2.0, 2.0, 1.0, 1.0, 3.0, math.pi / 2), 0.0, 0.0),
        ("sharing a corner", (1.0, 2.0, 2.0, 1.0, 1.0, 1.0, 0.0), (1.0, 2.0, 2.0, 3.0, 1.0, 3.0, 0.0), 0.0, 0.0),
        ("corner of a diamond on an edge", (1.0, 2.0, 2.0, 0.0, 1.0, 0.0, 0.0), (1.0, 2.0, 2.0, 1.0 + s2, 1.0, 0.0, math.pi / 4), 0.0, 0.0),
        ("disjoint", (1.5, 1.6, 3.9, 0.0, 1.7, 10.0, 0.2), (1.5, 1.6, 3.9, 30.0, 1.7, 40.0, -1.0), 0.0, 0.0),
        ("no height overlap, full ground overlap", (1.5, 1.6, 3.9, 2.0, 1.7, 20.0, 0.4), (1.5, 1.6, 3.9, 2.0, 3.2, 20.0, 0.4), 1.0, 0.0),
        ("half the height", (2.0, 1.6, 3.9, 2.0, 2.0, 20.0, 0.4), (2.0, 1.6, 3.9, 2.0, 1.0, 20.0, 0.4), 1.0, 1.0 / 3.0),
    ]
    gt_rows = [gt_row("Car", img, *c[1]) for c in cases]
    det_rows = [det_row(img, *c[2]) for c in cases]
    got, want = gpu_overlaps(gt_rows, det_rows), oracle_overlaps(gt_rows, det_rows)
    assert np.array_equal(got[0], want[0]) and (got[0] == 1.0).all()
    assert np.abs(got - want).max() <= 1e-9
    for i, (name, _, _, ground, vol) in enumerate(cases):
        assert abs(got[1, i, i] - ground) <= 1e-9 and abs(got[2, i, i] - vol) <= 1e-9, (name, got[1, i, i], got[2, i, i])
        assert abs(want[1, i, i] - ground) <= 1e-9 and abs(want[2, i, i] - vol) <= 1e-9, name
    # criterion 0 on a DontCare row: over the detection's own area / volume
    dc = [gt_row("DontCare", (0.0, 0.0, 100.0, 100.0), 2.0, 4.0, 6.0, 0.0, 2.0, 10.0, 0.3)]
    dets = [det_row((50.0, 50.0, 150.0, 150.0), 1.0, 1.0, 2.0, 0.5, 1.5, 10.2, 1.1)]
    got = gpu_overlaps(dc, dets)
    assert got[0, 0, 0] == 0.25 and abs(got[1, 0, 0] - 1.0) <= 1e-9 and abs(got[2, 0, 0] - 1.0) <= 1e-9
    assert np.abs(got - oracle_overlaps(dc, dets)).max() <= 1e-9


# ---- 3. the reference's entry points ---------------------------------------------------------------------------------------------------------
def stub_dataset_and_predictions(G, with_3d):
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    frames = G["write_txt_car/frames"].tolist()
    size = tuple(int(x) for x in G["write_txt_car/image_size"])
    half = (size[0] // 2, size[1] // 2)
    edges = np.concatenate([[0], np.cumsum(G["write_txt_car/det_count"])])
    dataset = type("KITTIObjectDatasetCar", (), {})()
    dataset.ids = ["%06d" % f for f in frames]
    dataset.infos = {f: {"size": size} for f in frames}
    preds = []
    for a, b in zip(edges[:-1], edges[1:]):
        p = BoxList(torch.from_numpy(G["write_txt_car/pred_bbox"][a:b]), half)
        p.add_field("scores", torch.from_numpy(G["write_txt_car/pred_scores"][a:b]))
        if with_3d:
            p.add_field("box3d", Box3DList(torch.from_numpy(G["write_txt_car/pred_box3d"][a:b]), half, "xyzhwl_ry"))
            p.add_field("scores_3d", torch.from_numpy(G["write_txt_car/pred_scores_3d"][a:b]))
        preds.append(p)
    return dataset, preds


@pytest.mark.parametrize("with_3d", [True, False], ids=["box3d", "2d_only"])
def test_write_txt_scores_a_stub_dataset_like_the_programs(G, tmp_path, capsys, with_3d):
    from disprcnn.data.datasets.evaluation import evaluate
    from disprcnn_amd.data.datasets.evaluation.kitti import kitti_eval as KE
    name = "write_txt_car" if with_3d else "write_txt_car_2d"
    frames, gt, det = O.golden_frames(G, name)
    gtd = tmp_path / "label_2"
    os.makedirs(gtd)
    for f, g in zip(frames, gt):
        (gtd / ("%06d.txt" % f)).write_text("\n".join(g))
    dataset, preds = stub_dataset_and_predictions(G, with_3d)
    out = tmp_path / "out"
    msg = KE.write_txt(dataset, preds, str(out), gt_dir=str(gtd))
    want = "".join(KE.ap_message(p, O.golden_stats(G, name, p, "car")) for p in (0.7, 0.5))
    assert msg == want and msg in capsys.readouterr().out
    assert msg.count("AP ") == (8 if with_3d else 2) and msg.startswith("0.7\nAP 2d ") and "\n0.5\nAP 2d " in msg
    txt = out / "txt"
    assert stats_files(str(txt), "car") == (set(O.STATS) if with_3d else {"detection"})
    for f, d in zip(frames, det):                                     # the label files: the lines the programs were given
        lines = (txt / ("%06d.txt" % f)).read_text().split("\n") if d else []
        assert len(lines) == len(d)
        for got_line, want_line in zip(lines, d):
            a, b = got_line.split(), want_line.split()
            assert a[:3] == b[:3] and np.allclose([float(x) for x in a[3:]], [float(x) for x in b[3:]], rtol=1e-5, atol=1e-5)
    # the dispatcher reaches the same function through the reference's import path; the ground truth directory is the default there
    assert evaluate.__module__ == "disprcnn_amd.data.datasets.evaluation"
    with pytest.raises(NotImplementedError):
        evaluate(object(), {"left": preds, "right": preds}, str(out))


def test_evaluate_runs_the_car_evaluation_for_a_car_dataset(G, tmp_path, monkeypatch):
    from disprcnn.data.datasets.evaluation import evaluate
    from disprcnn_amd.data.datasets.evaluation.kitti import kitti_eval as KE
    frames, gt, _ = O.golden_frames(G, "write_txt_car")
    for f, g in zip(frames, gt):
        (tmp_path / ("%06d.txt" % f)).write_text("\n".join(g))
    monkeypatch.setattr(KE, "DEFAULT_GT_DIR", str(tmp_path))
    dataset, preds = stub_dataset_and_predictions(G, True)
    msg = evaluate(dataset, {"left": preds, "right": None}, str(tmp_path / "out"), class2type=None, box_only=False, iou_types=("bbox",),
                   expected_results=[], expected_results_sigma_tol=4, eval_bbox3d=True)
    assert msg == "".join(KE.ap_message(p, O.golden_stats(G, "write_txt_car", p, "car")) for p in (0.7, 0.5))


# ---- 4. the build against itself -------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_reproducible_byte_for_byte(G):
    from disprcnn_amd.layers import kitti_eval as K
    _, gt, det = O.golden_frames(G, "frames_257")
    gt_frames, det_frames = [K.parse_label_lines(f, "gt") for f in gt], [K.parse_label_lines(f, "det") for f in det]
    a = K.kitti_eval_stats(gt_frames, det_frames, "car", 0.7)
    b = K.kitti_eval_stats(gt_frames, det_frames, "car", 0.7)
    assert list(a) == list(O.STATS) == list(b)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert (a["orientation"] > 0).any() and (a["orientation"] <= a["detection"]).all()

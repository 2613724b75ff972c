#!/usr/bin/env python3
"""Golden fixture of the KITTI object scoring, recorded from the REFERENCE'S EVALUATOR PROGRAMS (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kitti_eval.py [REFERENCE_ROOT]    -> kitti_eval_golden.npz

The reference scores by running tools/kitti_object/kitti_evaluation_lib/evaluate_object_0.7 and evaluate_object_0.5 (the KITTI devkit's
evaluate_object.cpp, built with MIN_OVERLAP {0.7, 0.5, 0.5} and 0.5).  For every case set below this script writes the label files of a
seeded generator, copies each program to a temporary directory, runs it as `prog RESULT_DIR GT_DIR` and records

    <set>/frames                      the frame indices (the %06d of the file names)
    <set>/gt_lines,  <set>/gt_count   the ground-truth label lines as written, and how many each frame holds
    <set>/det_lines, <set>/det_count  the same for the detections
    <set>/<program>/<class>/<stats>   the [3,41] array of stats_<class>_<stats>.txt; a file the program did not write has no entry

Only data is stored; the programs are not.  One run writes the statistics of all three classes, so every set goes through both programs
for car, pedestrian and cyclist.  Checked before writing: in the main sets no recorded row is all zero.
"""
import os
import shutil
import stat
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kitti_eval_golden.npz")
PROGRAMS = ("0.7", "0.5")
CLASSES = ("car", "pedestrian", "cyclist")
STATS = ("detection", "orientation", "detection_ground", "detection_3d")
DIMS = {"Car": (1.5, 1.6, 3.9), "Van": (2.2, 1.9, 5.0), "Pedestrian": (1.75, 0.6, 0.8), "Person_sitting": (1.3, 0.6, 0.8),
        "Cyclist": (1.7, 0.6, 1.8), "Truck": (3.2, 2.6, 10.0), "Tram": (3.5, 2.5, 15.0), "Misc": (1.9, 1.5, 3.5)}
MAX_DET = 256                                   # include/disprcnn_pts.h: drc_kitti_eval_max_det()


def gt_line(typ, trunc, occ, alpha, box, dims, loc, ry):
    v = [trunc, alpha, *box, *dims, *loc, ry]
    return "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (typ, v[0], occ, *v[1:])


def dontcare_line(box):
    return "DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10" % tuple(box)


def det_line(typ, alpha, box, dims, loc, ry, score):
    vals = [alpha, *box, *dims, *loc, ry, score]
    return f"{typ} -1 -1 " + " ".join(repr(float(x)) for x in vals)


def det2d_line(typ, box, score):
    return f"{typ} -1 -1 -10 " + " ".join(repr(float(x)) for x in box) + f" 0 0 0 0 0 0 0 {float(score)!r}"


def random_object(rng, typ, min_h=18.0, max_h=140.0, easy=False):
    h2d = rng.uniform(45.0, max_h) if easy else rng.uniform(min_h, max_h)
    w2d = h2d * rng.uniform(0.5, 2.0)
    x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 220)
    occ = 0 if easy else int(rng.choice([0, 0, 0, 1, 1, 2, 3]))
    trunc = 0.0 if easy or rng.random() < 0.6 else rng.uniform(0, 0.6)
    dims = np.array(DIMS[typ]) * rng.uniform(0.9, 1.1, 3)
    loc = (rng.uniform(-20, 20), rng.uniform(1.2, 2.0), rng.uniform(6, 60))
    return dict(typ=typ, trunc=trunc, occ=occ, alpha=rng.uniform(-3.1, 3.1), box=(x1, y1, x1 + w2d, y1 + h2d), dims=tuple(dims), loc=loc,
                ry=rng.uniform(-3.1, 3.1))


def rounded(o):
    """the object as its %.2f label line states it: detections are perturbations of what the evaluator reads"""
    r2 = lambda t: tuple(float("%.2f" % x) for x in t)
    return dict(o, trunc=float("%.2f" % o["trunc"]), alpha=float("%.2f" % o["alpha"]), box=r2(o["box"]), dims=r2(o["dims"]), loc=r2(o["loc"]),
                ry=float("%.2f" % o["ry"]))


def perturbed(rng, o, typ=None, level=None):
    level = rng.choice([0.01, 0.04, 0.12]) if level is None else level
    x1, y1, x2, y2 = o["box"]
    w, h = x2 - x1, y2 - y1
    box = (x1 + rng.normal(0, level) * w, y1 + rng.normal(0, level) * h, x2 + rng.normal(0, level) * w, y2 + rng.normal(0, level) * h)
    dims = tuple(np.array(o["dims"]) * (1 + rng.normal(0, level, 3)))
    loc = tuple(np.array(o["loc"]) + rng.normal(0, level * 2, 3))
    ry = o["ry"] + rng.normal(0, level * 2) + (np.pi if rng.random() < 0.1 else 0.0)
    return det_line(typ or o["typ"], o["alpha"] + rng.normal(0, 0.3), box, dims, loc, ry, rng.uniform(0.05, 1.0))


def as_gt(o):
    return gt_line(o["typ"], o["trunc"], o["occ"], o["alpha"], o["box"], o["dims"], o["loc"], o["ry"])


def main_set(seed, n_frames, weights, first=0, step=1):
    rng = np.random.default_rng(seed)
    names = list(DIMS)
    p = np.array([weights.get(n, 0.4) for n in names])
    frames, gts, dets = [], [], []
    for f in range(n_frames):
        g, d = [], []
        for k in range(int(rng.integers(3, 9))):
            typ = str(rng.choice(names, p=p / p.sum()))
            o = rounded(random_object(rng, typ, easy=rng.random() < 0.4))
            g.append(as_gt(o))
            if rng.random() < 0.85:
                d.append(perturbed(rng, o, typ=typ if typ in ("Car", "Pedestrian", "Cyclist") else str(rng.choice(["Car", "Pedestrian"]))))
            if rng.random() < 0.15:                                     # a second detection of the same object
                d.append(perturbed(rng, o, typ=typ if typ in ("Car", "Pedestrian", "Cyclist") else "Car"))
        for k in range(int(rng.integers(0, 3))):
            x1, y1 = rng.uniform(0, 1000), rng.uniform(80, 200)
            box = (x1, y1, x1 + rng.uniform(40, 200), y1 + rng.uniform(30, 100))
            g.append(dontcare_line(box))
            for _ in range(int(rng.integers(0, 3))):                    # detections that lie (mostly) in the DontCare region
                bw, bh = (box[2] - box[0]) * rng.uniform(0.3, 0.9), max((box[3] - box[1]) * rng.uniform(0.5, 0.95), 26.0)
                bx, by = rng.uniform(box[0] - 0.2 * bw, box[2] - 0.8 * bw), rng.uniform(box[1], max(box[1], box[3] - bh))
                fp = random_object(rng, str(rng.choice(["Car", "Pedestrian", "Cyclist"])))
                d.append(det_line(fp["typ"], fp["alpha"], (bx, by, bx + bw, by + bh), fp["dims"], fp["loc"], fp["ry"], rng.uniform(0.05, 1.0)))
        for k in range(int(rng.integers(0, 4))):                        # plain false positives
            fp = random_object(rng, str(rng.choice(["Car", "Pedestrian", "Cyclist"])))
            d.append(det_line(fp["typ"], fp["alpha"], fp["box"], fp["dims"], fp["loc"], fp["ry"], rng.uniform(0.05, 0.9)))
        order = rng.permutation(len(d))
        frames.append(first + f * step)
        gts.append(g)
        dets.append([d[i] for i in order])
    return frames, gts, dets


def simple_frames(seed, n_frames, n_obj=2, typ="Car"):
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    for f in range(n_frames):
        objs = [rounded(random_object(rng, typ, easy=k == 0)) for k in range(n_obj)]
        gts.append([as_gt(o) for o in objs])
        dets.append([perturbed(rng, o, level=0.02) for o in objs if rng.random() < 0.9] +
                    [perturbed(rng, rounded(random_object(rng, typ)), level=0.02) for _ in range(int(rng.integers(0, 2)))])
    return list(range(n_frames)), gts, dets


def edge_sets():
    sets = {}
    rng = np.random.default_rng(77)
    car = lambda **kw: rounded(random_object(rng, "Car", **kw))
    # frames without ground truth, without detections, without either, with DontCare only; two ordinary frames around them
    fr, g, d = simple_frames(1, 2)
    o = car(easy=True)
    g += [[], [as_gt(o), as_gt(car())], [], [dontcare_line((100, 100, 300, 200))]]
    d += [[perturbed(rng, o, level=0.02), perturbed(rng, car(), level=0.02)], [], [],
          [det_line("Car", 0.3, (120, 110, 200, 180), (1.5, 1.6, 3.9), (1.0, 1.5, 20.0), 0.1, 0.8), perturbed(rng, car(), level=0.02)]]
    sets["empty_frames"] = (list(range(6)), g, d)
    # a difficulty without a valid ground truth: nothing as tall as 40 px, so the easy line is all zero
    g, d = [], []
    for f in range(4):
        objs = [rounded(random_object(rng, "Car", min_h=26.0, max_h=38.0)) for _ in range(3)]
        for o in objs:
            o["occ"], o["trunc"] = min(o["occ"], 2), 0.0
        g.append([as_gt(o) for o in objs])
        d.append([perturbed(rng, o, level=0.02) for o in objs])
    sets["empty_difficulty"] = (list(range(4)), g, d)
    # fewer matched detections than recall samples (one detection is its ground truth exactly)
    fr, g, d = simple_frames(3, 3, n_obj=3)
    o = car(easy=True)
    g[0].append(as_gt(o))
    d[0].append(det_line("Car", o["alpha"], o["box"], o["dims"], o["loc"], o["ry"], 0.77))
    sets["few_matches"] = (fr, g, d)
    # equal scores, within a frame (two detections of one object) and across frames
    g, d = [], []
    for f in range(8):
        objs = [car(easy=k < 2) for k in range(4)]
        g.append([as_gt(o) for o in objs])
        dd = []
        for k, o in enumerate(objs):
            for rep in range(2 if k % 2 == 0 else 1):
                line = perturbed(rng, o, level=0.02).split()
                line[-1] = repr([0.5, 0.5, 0.75, 0.25][(f + k) % 4])
                dd.append(" ".join(line))
        fp = perturbed(rng, car(), level=0.02).split()
        fp[-1] = "0.5"
        d.append(dd + [" ".join(fp)])
    sets["equal_scores"] = (list(range(8)), g, d)
    # limit values: heights of exactly 25.00 and 40.00 px (and just below), occlusion and truncation exactly at the levels' limits
    g, d = [], []
    for f, (hgt, dh) in enumerate([(25.0, 25.0), (40.0, 40.0), (24.99, 24.99), (39.99, 39.99), (40.0, 25.5), (25.0, 40.0), (60.0, 39.99), (60.0, 25.0),
                                (60.0, 60.0), (40.01, 40.0), (25.01, 25.0)]):
        gg, dd = [], []
        for k, (occ, trunc) in enumerate([(0, 0.15), (1, 0.3), (2, 0.5), (0, 0.16), (1, 0.31), (2, 0.51), (3, 0.0), (0, 0.0)]):
            o = car()
            x1, y1 = 20.0 + 150.0 * k, 120.0 + f
            o.update(occ=occ, trunc=trunc, box=(x1, y1, x1 + 90.0, y1 + hgt))
            gg.append(as_gt(o))
            line = perturbed(rng, o, level=0.004).split()
            line[4:8] = [repr(x1), repr(y1), repr(x1 + 90.0), repr(y1 + dh)]
            dd.append(" ".join(line))
        g.append(gg)
        d.append(dd)
    sets["limits"] = (list(range(len(g))), g, d)
    # class handling: Van beside Car, Person_sitting beside Pedestrian, foreign classes among the detections, names in another case
    g, d = [], []
    for f in range(8):
        gg, dd = [], []
        for typ, det_typ in [("Car", "Car"), ("Van", "Car"), ("Pedestrian", "Pedestrian"), ("Person_sitting", "Pedestrian"), ("Cyclist", "Cyclist"),
                             ("Truck", "Car"), ("Car", "Truck"), ("car", "CAR"), ("Pedestrian", "Tram"), ("Tram", "Cyclist"), ("Cyclist", "Van"),
                             ("Misc", "Misc"), ("PEDESTRIAN", "pedestrian")]:
            o = rounded(random_object(rng, typ.capitalize() if typ.capitalize() in DIMS else "Car", easy=rng.random() < 0.6))
            o["typ"] = typ
            gg.append(as_gt(o))
            dd.append(perturbed(rng, o, typ=det_typ, level=0.015))
        g.append(gg)
        d.append(dd)
    sets["classes"] = (list(range(8)), g, d)
    # disabled metrics: one detection without an orientation (alpha -10) switches AOS off for every class
    fr, g, d = main_set(5, 6, {"Car": 3.0, "Pedestrian": 1.5, "Cyclist": 1.5})
    line = d[2][0].split()
    line[3] = "-10"
    d[2][0] = " ".join(line)
    sets["no_aos"] = (fr, g, d)
    # 2D-only detections: the detection file alone
    fr, g, d = main_set(6, 8, {"Car": 3.0, "Pedestrian": 1.5, "Cyclist": 1.5})
    d = [[det2d_line(x.split()[0], x.split()[4:8], x.split()[-1]) for x in dd] for dd in d]
    sets["only_2d"] = (fr, g, d)
    # detections swallowed by DontCare regions: inside, mostly inside, mostly outside, and one that also matches an ignored ground truth
    g, d = [], []
    for f in range(6):
        o, o2 = car(easy=True), car(easy=True)
        region = (300.0, 100.0, 600.0 + 10 * f, 260.0)
        gg = [as_gt(o), dontcare_line(region), as_gt(o2), dontcare_line((700.0, 120.0, 900.0, 200.0))]
        dd = [perturbed(rng, o, level=0.02)]
        for (x1, y1, x2, y2) in [(320, 110, 420, 180), (550, 120, 650, 200), (200, 150, 330, 230), (590 + 10 * f, 130, 640 + 10 * f, 190),
                                 (710, 125, 800, 190), (650, 120, 760, 190), (330, 120, 380, 140)]:
            fp = car()
            dd.append(det_line("Car", fp["alpha"], (x1, y1, x2, y2), fp["dims"], fp["loc"], fp["ry"], rng.uniform(0.1, 1.0)))
        dd.append(perturbed(rng, o2, level=0.02))
        g.append(gg)
        d.append(dd)
    sets["dontcare"] = (list(range(6)), g, d)
    # per-frame detection counts around the 64-bit words of the assigned set, and the documented limit
    g, d = [], []
    for n_det in (63, 64, 65, MAX_DET):
        objs = [car(easy=k % 3 == 0) for k in range(24)]
        gg = [as_gt(o) for o in objs]
        dd = [perturbed(rng, objs[k % len(objs)], level=0.02) for k in range(n_det)]
        dd = [dd[i] for i in rng.permutation(n_det)]
        g.append(gg)
        d.append(dd)
    sets["det_counts"] = ([0, 1, 2, 3], g, d)
    # total frame counts: 1, 2 and one more than the 256 frames a workgroup takes
    sets["frames_1"] = simple_frames(11, 1, n_obj=4)
    sets["frames_2"] = simple_frames(12, 2, n_obj=3)
    sets["frames_257"] = simple_frames(13, 257, n_obj=2)
    return sets


def write_txt_sets():
    """Predictions as the detector hands them over (BoxList + Box3DList at half the image size), their label lines as the project's own
    kitti_label_lines writes them after the resize -- with the 3D boxes and without -- and the arrays the test rebuilds the predictions from"""
    import torch
    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    from disprcnn_amd.utils.kitti_io import kitti_label_lines
    frames, gts, dets = main_set(104, 24, {"Car": 4.0, "Van": 1.0})
    size, half = (1280, 384), (640, 192)
    rng = np.random.default_rng(105)
    lines3d, lines2d, arrays = [], [], {"bbox": [], "box3d": [], "scores_3d": [], "scores": []}
    for d in dets:
        v = np.array([[float(x) for x in line.split()[3:16]] for line in d], np.float64).reshape(-1, 13)
        bbox = (v[:, 1:5] / 2).astype(np.float32)
        box3d = v[:, [8, 9, 10, 5, 6, 7, 11]].astype(np.float32)                    # x, y, z, h, w, l, ry
        scores_3d, scores = v[:, 12].astype(np.float32), rng.uniform(0.05, 1.0, len(v)).astype(np.float32)
        pred = BoxList(torch.from_numpy(bbox), half)
        pred.add_field("scores", torch.from_numpy(scores))
        lines2d.append(kitti_label_lines(pred.resize(size), "Car"))
        pred.add_field("box3d", Box3DList(torch.from_numpy(box3d), half, "xyzhwl_ry"))
        pred.add_field("scores_3d", torch.from_numpy(scores_3d))
        lines3d.append(kitti_label_lines(pred.resize(size), "Car"))
        for k, a in zip(arrays, (bbox, box3d, scores_3d, scores)):
            arrays[k].append(a)
    extra = {f"write_txt_car/pred_{k}": np.concatenate(a) for k, a in arrays.items()}
    extra["write_txt_car/image_size"] = np.array(size, np.int32)
    return {"write_txt_car": (frames, gts, lines3d), "write_txt_car_2d": (frames, gts, lines2d)}, extra


def case_sets():
    sets = {"main_car": main_set(101, 50, {"Car": 4.0, "Van": 1.0}),
            "main_pedestrian": main_set(102, 50, {"Pedestrian": 4.0, "Person_sitting": 1.0}),
            "main_cyclist": main_set(103, 50, {"Cyclist": 4.0}, first=3, step=7)}          # sparse frame indices
    sets.update(edge_sets())
    return sets


def run_program(prog_src, frames, gts, dets):
    """-> {(class, stats): [3,41]} of the files the program wrote"""
    with tempfile.TemporaryDirectory() as tmp:
        prog = os.path.join(tmp, "evaluate_object")
        shutil.copyfile(prog_src, prog)
        os.chmod(prog, os.stat(prog).st_mode | stat.S_IXUSR)
        res, gtd = os.path.join(tmp, "res"), os.path.join(tmp, "gt")
        os.makedirs(res)
        os.makedirs(gtd)
        for f, g, d in zip(frames, gts, dets):
            with open(os.path.join(gtd, "%06d.txt" % f), "w") as fh:
                fh.write("\n".join(g))
            with open(os.path.join(res, "%06d.txt" % f), "w") as fh:
                fh.write("\n".join(d))
        r = subprocess.run([prog, res, gtd], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        out = {}
        for c in CLASSES:
            for s in STATS:
                path = os.path.join(res, f"stats_{c}_{s}.txt")
                if os.path.exists(path):
                    with open(path) as fh:
                        rows = [list(map(float, line.split())) for line in fh.read().splitlines()]
                    arr = np.array(rows, np.float64)
                    assert arr.shape == (3, 41), (path, arr.shape, r.stdout[-2000:])
                    out[(c, s)] = arr
        return out, r.stdout


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    lib = os.path.join(ref, "tools", "kitti_object", "kitti_evaluation_lib")
    sets = case_sets()
    wt_sets, store = write_txt_sets()
    sets.update(wt_sets)
    for name, (frames, gts, dets) in sets.items():
        assert len(frames) == len(gts) == len(dets)
        store[f"{name}/frames"] = np.array(frames, np.int32)
        store[f"{name}/gt_lines"] = np.array([x for g in gts for x in g] or [""])[:sum(map(len, gts))]
        store[f"{name}/gt_count"] = np.array([len(g) for g in gts], np.int32)
        store[f"{name}/det_lines"] = np.array([x for d in dets for x in d] or [""])[:sum(map(len, dets))]
        store[f"{name}/det_count"] = np.array([len(d) for d in dets], np.int32)
        for p in PROGRAMS:
            out, log = run_program(os.path.join(lib, "evaluate_object_" + p), frames, gts, dets)
            for (c, s), arr in out.items():
                store[f"{name}/{p}/{c}/{s}"] = arr
                if name == "main_" + c:
                    assert (arr != 0).any(axis=1).all(), (name, p, c, s, "a recorded row is all zero")
            print(f"{name:18s} {p}: " + ", ".join(f"{c}/{s} {arr[:, ::4].mean(1).round(3).tolist()}" for (c, s), arr in sorted(out.items())))
            if name.startswith("main_"):
                assert all((name[5:], s) in out for s in STATS), (name, p, sorted(out), log[-2000:])
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()

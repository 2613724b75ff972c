"""kitti_eval -- the KITTI object benchmark's scoring (the devkit's evaluate_object.cpp, which the reference runs as the prebuilt programs
tools/kitti_object/kitti_evaluation_lib/evaluate_object_0.7 and _0.5) on the HIP kernels of libdisprcnn_pts.so (pts/kitti_eval.hip).

    kitti_eval_stats(gt_frames, det_frames, cls, min_overlap) -> {'detection', 'orientation', 'detection_ground', 'detection_3d': [3,41]}
    eval_label_dirs(result_dir, gt_dir, cls='car', min_overlap=0.7) -> the same dict, and RESULT_DIR/stats_<cls>_*.txt as the programs write

Each array holds, per difficulty (easy, moderate, hard), the precision (for 'orientation' the orientation similarity) at the 41 recall
samples; the reference's 11-point AP is `a[:, ::4].mean(1)`.  A metric the programs would not evaluate is absent: AOS when any detection of
the run has alpha == -10, BEV / 3D when no detection of the class carries a valid location and positive extents.

What runs where: the text is parsed and the class names are resolved (case-insensitively) on the host; the overlaps of every (ground truth,
detection) pair of a frame -- image, BEV, 3D -- are computed once on the GPU and both passes of the greedy assignment read them; the
per-frame counts are summed on the GPU in a fixed order.  Between the passes the matched scores are sorted (torch.sort) and the recall
thresholds are picked on the host, where the result is needed anyway.  All arithmetic is fp64 like the devkit's.  The arrays live on the
current GPU; there is no CPU path.
"""
import os
import re
import time

import numpy as np

N_SAMPLE_PTS = 41
CLASS_NAMES = ("car", "pedestrian", "cyclist")
NEIGHBOUR = {"car": "van", "pedestrian": "person_sitting"}
METRICS = ("detection", "detection_ground", "detection_3d")               # METRIC IMAGE, GROUND, BOX3D
STATS = ("detection", "orientation", "detection_ground", "detection_3d")
# MIN_OVERLAP[metric][class] of the two programs, keyed by the suffix of the program's name
MIN_OVERLAP = {0.7: ((0.7, 0.5, 0.5), (0.7, 0.5, 0.5), (0.7, 0.5, 0.5)), 0.5: ((0.5, 0.5, 0.5),) * 3}
GT_COLS, DET_COLS = 14, 13
_FRAME_FILE = re.compile(r"^\d{6}\.txt$")


# ---- host side: label text <-> arrays -----------------------------------------------------------------------------------------------------
def parse_label_lines(lines, kind):
    """Label lines of one frame -> (types, values).  kind 'gt': values [n,14] = truncation, occlusion, alpha, x1, y1, x2, y2, h, w, l,
    t1, t2, t3, ry; kind 'det': values [n,13] = alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score (the two fields after the type
    are not read, as in the devkit).  Blank lines are skipped; a line with too few fields raises."""
    if kind not in ("gt", "det"):
        raise ValueError(f"kind must be 'gt' or 'det', got {kind!r}")
    need = 15 if kind == "gt" else 16
    types, rows = [], []
    for line in lines:
        p = line.split()
        if not p:
            continue
        if len(p) < need:
            raise ValueError(f"a {kind} label line needs {need} fields, got {len(p)}: {line!r}")
        types.append(p[0])
        if kind == "gt":
            rows.append([float(p[1]), float(int(float(p[2])))] + [float(x) for x in p[3:15]])
        else:
            rows.append([float(x) for x in p[3:16]])
    cols = GT_COLS if kind == "gt" else DET_COLS
    return types, np.asarray(rows, np.float64).reshape(len(rows), cols)


def read_label_file(path, kind):
    with open(path) as f:
        return parse_label_lines(f.read().splitlines(), kind)


def gt_class_codes(types, cls):
    """0 the class itself, 1 its neighbour class (ignored, but may absorb a detection), 2 DontCare, 3 any other"""
    cls = cls.lower()
    code = {cls: 0, "dontcare": 2}
    if cls in NEIGHBOUR:
        code[NEIGHBOUR[cls]] = 1
    return np.asarray([code.get(t.lower(), 3) for t in types], np.int32)


def det_class_codes(types, cls):
    cls = cls.lower()
    return np.asarray([0 if t.lower() == cls else 1 for t in types], np.int32)


def load_flags(det_frames, cls):
    """loadDetections' switches: (compute_aos, eval_image, eval_ground, eval_3d).  compute_aos looks at every detection of the run,
    whatever its class; the other three at the detections of `cls`."""
    types = [t for ts, _ in det_frames for t in ts]
    if not types:
        return True, False, False, False
    v = np.concatenate([np.asarray(a, np.float64).reshape(-1, DET_COLS) for _, a in det_frames])
    own = v[det_class_codes(types, cls) == 0]
    h, w, l, t1, t2, t3 = (own[:, k] for k in range(5, 11))
    ground = (t1 != -1000) & (t3 != -1000) & (w > 0) & (l > 0)
    return (not bool((v[:, 0] == -10).any()), bool((own[:, 1] >= 0).any()), bool(ground.any()),
            bool((ground & (t2 != -1000) & (h > 0)).any()))


def format_stats(a):
    """[3,41] -> the text of a stats_*.txt file: '%f ' per value, one line per difficulty"""
    return "".join("".join("%f " % x for x in row) + "\n" for row in np.asarray(a, np.float64))


def read_stats_file(path):
    with open(path) as f:
        return np.asarray([[float(x) for x in line.split()] for line in f.read().splitlines()], np.float64)


def write_stats_files(result_dir, cls, stats):
    """stats_<cls>_<name>.txt for the metrics present; a file of an earlier run whose metric is absent now is removed"""
    for name in STATS:
        path = os.path.join(result_dir, f"stats_{cls.lower()}_{name}.txt")
        if name in stats:
            with open(path, "w") as f:
                f.write(format_stats(stats[name]))
        elif os.path.exists(path):
            os.remove(path)


def select_thresholds(v_sorted, n_gt):
    """getThresholds on scores already in descending order: for each recall sample in turn, the first score (after the last one taken)
    that the devkit's walk does not skip.  While `current_recall` stands still the skip test is monotonic in i, so the walk's next stop is
    the first i that fails it."""
    n = len(v_sorted)
    if n == 0:
        return np.zeros(0, np.float64)
    i = np.arange(n, dtype=np.float64)
    l_recall = (i + 1) / float(n_gt)
    r_recall = (i + 2) / float(n_gt)
    r_recall[-1] = l_recall[-1]
    last = np.arange(n) == n - 1
    out, start, current = [], 0, 0.0
    while start < n:
        skip = ((r_recall[start:] - current) < (current - l_recall[start:])) & ~last[start:]
        k = start + int(np.argmin(skip))                 # the last index is never skipped, so there is a False
        out.append(v_sorted[k])
        current += 1.0 / (N_SAMPLE_PTS - 1.0)
        start = k + 1
    return np.asarray(out, np.float64)


def _running_max_from_right(a, n):
    """the devkit's `a[i] = *max_element(a.begin() + i, a.end())` for i < n, over all 41 entries"""
    for i in range(n):
        best = a[i]
        for x in a[i + 1:]:
            if best < x:
                best = x
        a[i] = best


def _min_overlaps(cls, min_overlap):
    c = CLASS_NAMES.index(cls.lower())
    if np.ndim(min_overlap) == 0:
        key = float(min_overlap)
        if key not in MIN_OVERLAP:
            raise ValueError(f"min_overlap names the program: 0.7 or 0.5 (or give the three per-metric values), got {min_overlap!r}")
        return tuple(float(MIN_OVERLAP[key][m][c]) for m in range(3))
    if len(min_overlap) != 3:
        raise ValueError("min_overlap: a program's suffix (0.7 / 0.5) or three values (image, ground, 3d)")
    return tuple(float(x) for x in min_overlap)


# ---- GPU side -------------------------------------------------------------------------------------------------------------------------------
class _Packed:
    """The frames of a run as the kernels read them (CSR over the frames), on the current GPU."""

    def __init__(self, gt_frames, det_frames, cls):
        import torch
        if len(gt_frames) != len(det_frames):
            raise ValueError(f"{len(gt_frames)} ground-truth frames but {len(det_frames)} detection frames")
        if not torch.cuda.is_available():
            raise RuntimeError("kitti_eval: needs a GPU (MI355X); the HIP path has no CPU fallback")
        self.F = len(gt_frames)
        g_n = np.asarray([len(t) for t, _ in gt_frames], np.int64)
        d_n = np.asarray([len(t) for t, _ in det_frames], np.int64)
        self.max_gt, self.max_det = int(g_n.max(initial=0)), int(d_n.max(initial=0))
        gt_off = np.concatenate([[0], np.cumsum(g_n)])
        det_off = np.concatenate([[0], np.cumsum(d_n)])
        pair_off = np.concatenate([[0], np.cumsum(g_n * d_n)])
        self.NG, self.ND, self.NP = int(gt_off[-1]), int(det_off[-1]), int(pair_off[-1])
        if self.NG >= 2 ** 31 or self.ND >= 2 ** 31:
            raise ValueError("kitti_eval: too many label rows")
        gt = np.concatenate([v.reshape(-1, GT_COLS) for _, v in gt_frames] + [np.zeros((0, GT_COLS))])
        det = np.concatenate([v.reshape(-1, DET_COLS) for _, v in det_frames] + [np.zeros((0, DET_COLS))])
        gt_cls = gt_class_codes([t for ts, _ in gt_frames for t in ts], cls)
        det_cls = det_class_codes([t for ts, _ in det_frames for t in ts], cls)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)
        self.gt, self.det = put(gt, np.float64), put(det, np.float64)
        self.gt_cls, self.det_cls = put(gt_cls, np.int32), put(det_cls, np.int32)
        self.gt_off, self.det_off, self.pair_off = put(gt_off, np.int32), put(det_off, np.int32), put(pair_off, np.int64)
        self.gt_off_host = gt_off


def _limits_check(L, p):
    if p.max_det > L.drc_kitti_eval_max_det() or p.max_gt > L.drc_kitti_eval_max_gt():
        raise RuntimeError(f"kitti_eval: a frame holds {p.max_det} detections / {p.max_gt} ground-truth rows; the kernels take at most "
                           f"{L.drc_kitti_eval_max_det()} / {L.drc_kitti_eval_max_gt()} per frame")


def _overlaps(L, p, metric_mask):
    import torch
    from ..engine import _ptr, _stream_ptr
    from ..pts import _lib
    ov = torch.empty((3, p.NP), dtype=torch.float64, device=p.dev)
    st = L.drc_kitti_eval_overlaps(p.F, p.NP, _ptr(p.gt), _ptr(p.gt_cls), _ptr(p.det), _ptr(p.gt_off), _ptr(p.det_off), _ptr(p.pair_off),
                                   metric_mask, _ptr(ov), _stream_ptr(p.dev))
    _lib.check(st, "drc_kitti_eval_overlaps")
    return ov


def frame_overlaps(gt_frame, det_frame, cls="car"):
    """[3, G, D] fp64 tensor on the GPU: image, BEV and 3D overlap of every pair of ONE frame, as the evaluation uses them (IoU; for a
    DontCare row the intersection over the detection's own area / volume)."""
    from ..pts import _lib
    L = _lib.lib()
    p = _Packed([gt_frame], [det_frame], cls)
    return _overlaps(L, p, 7).view(3, p.NG, p.ND)


def kitti_eval_stats(gt_frames, det_frames, cls, min_overlap, timings=None):
    """gt_frames / det_frames: per frame the (types, values) pair of parse_label_lines; cls: 'car', 'pedestrian' or 'cyclist' (any case);
    min_overlap: 0.7 or 0.5, naming the program whose MIN_OVERLAP table is used, or the three values (image, ground, 3d) themselves.
    -> {'detection', 'orientation', 'detection_ground', 'detection_3d'}: [3,41] float64 arrays; a metric that is not evaluated is absent.
    `timings`, when a dict, receives the milliseconds between the stages' HIP events ('thresholds_ms' is the sort, the copies to the
    host and the selection) and 'host_ms': the call's wall time less the four kernel stages."""
    import torch
    from ..engine import _ptr, _stream_ptr
    from ..pts import _lib
    if cls.lower() not in CLASS_NAMES:
        raise ValueError(f"cls must be one of {CLASS_NAMES}, got {cls!r}")
    t_host = time.perf_counter()
    mo = _min_overlaps(cls, min_overlap)
    compute_aos, ev_image, ev_ground, ev_3d = load_flags(det_frames, cls)
    metric_mask = int(ev_image) | int(ev_ground) << 1 | int(ev_3d) << 2
    if metric_mask == 0:
        return {}
    L = _lib.lib()
    p = _Packed(gt_frames, det_frames, cls)
    _limits_check(L, p)
    dev, stream = p.dev, _stream_ptr(p.dev)
    T = N_SAMPLE_PTS
    marks = []

    def mark(name):
        if timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            marks.append((name, e))

    mark("start")
    gt_ign = torch.empty((3, p.NG), dtype=torch.int8, device=dev)
    det_ign = torch.empty((3, p.ND), dtype=torch.int8, device=dev)
    _lib.check(L.drc_kitti_eval_clean(p.NG, p.ND, _ptr(p.gt), _ptr(p.gt_cls), _ptr(p.det), _ptr(p.det_cls), _ptr(gt_ign), _ptr(det_ign), stream),
               "drc_kitti_eval_clean")
    ov = _overlaps(L, p, metric_mask)
    mark("overlaps_ms")
    v = torch.empty((9, p.NG), dtype=torch.float64, device=dev)
    matched = torch.zeros((9, p.NG), dtype=torch.int8, device=dev)
    common = (p.F, p.NG, p.ND, p.NP, p.max_gt, p.max_det, _ptr(p.gt), _ptr(p.gt_cls), _ptr(p.det), _ptr(p.gt_off), _ptr(p.det_off),
              _ptr(p.pair_off), _ptr(gt_ign), _ptr(det_ign), _ptr(ov), metric_mask, mo[0], mo[1], mo[2])
    _lib.check(L.drc_kitti_eval_pass1(*common, _ptr(v), _ptr(matched), stream), "drc_kitti_eval_pass1")
    mark("pass1_ms")
    # threshold selection: the matched scores of each (difficulty, metric) in descending order, then at most 41 of them
    n_gt = (gt_ign == 0).sum(1).cpu().numpy()                                    # per difficulty: the recall's denominator
    hit = matched.bool()
    v_sorted = torch.sort(torch.where(hit, v, torch.full_like(v, float("-inf"))), dim=1, descending=True)[0].cpu().numpy()
    n_hit = hit.sum(1).cpu().numpy()
    t_sel = time.perf_counter()
    thr = np.zeros((3, 3, T), np.float64)
    n_thr = np.zeros((3, 3), np.int32)
    for d in range(3):
        for m in range(3):
            if (metric_mask >> m) & 1 and n_gt[d] > 0:
                t = select_thresholds(v_sorted[d * 3 + m, :int(n_hit[d * 3 + m])], int(n_gt[d]))
                assert len(t) <= T
                thr[d, m, :len(t)], n_thr[d, m] = t, len(t)
    t_sel = time.perf_counter() - t_sel
    thr_d, n_thr_d = torch.from_numpy(thr).to(dev), torch.from_numpy(n_thr).to(dev)
    mark("thresholds_ms")
    counts = torch.empty((9 * T, 3, p.F), dtype=torch.int16, device=dev)
    sim = torch.empty((9 * T, p.F), dtype=torch.float64, device=dev)
    _lib.check(L.drc_kitti_eval_pass2(*common, int(compute_aos), _ptr(thr_d), _ptr(n_thr_d), _ptr(counts), _ptr(sim), stream),
               "drc_kitti_eval_pass2")
    mark("pass2_ms")
    out_counts = torch.empty((3, 3, T, 3), dtype=torch.int64, device=dev)
    out_sim = torch.empty((3, 3, T), dtype=torch.float64, device=dev)
    _lib.check(L.drc_kitti_eval_reduce(p.F, _ptr(counts), _ptr(sim), _ptr(out_counts), _ptr(out_sim), stream), "drc_kitti_eval_reduce")
    mark("reduce_ms")
    c, s = out_counts.cpu().numpy(), out_sim.cpu().numpy()
    # the curves: precision = tp / (tp + fp), aos = similarity / (tp + fp), each replaced by its running maximum from the right
    stats = {}
    for m in range(3):
        if not (metric_mask >> m) & 1:
            continue
        aos_on = compute_aos and m == 0
        prec, aos = np.zeros((3, T), np.float64), np.zeros((3, T), np.float64)
        for d in range(3):
            n = int(n_thr[d, m])
            tp, fp = c[d, m, :n, 0].astype(np.float64), c[d, m, :n, 1].astype(np.float64)
            with np.errstate(all="ignore"):
                prec[d, :n] = tp / (tp + fp)
                if aos_on:
                    aos[d, :n] = s[d, m, :n] / (tp + fp)
            _running_max_from_right(prec[d], n)
            if aos_on:
                _running_max_from_right(aos[d], n)
        stats[METRICS[m]] = prec
        if aos_on:
            stats["orientation"] = aos
    if timings is not None:
        torch.cuda.synchronize(dev)
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            timings[name] = e0.elapsed_time(e1)
        timings["select_host_ms"] = t_sel * 1e3
        timings["host_ms"] = (time.perf_counter() - t_host) * 1e3 - sum(timings[k] for k in ("overlaps_ms", "pass1_ms", "pass2_ms", "reduce_ms"))
    return {k: stats[k] for k in STATS if k in stats}


def read_label_dirs(result_dir, gt_dir):
    """The frames of a run: every RESULT_DIR/%06d.txt with the GT_DIR file of the same name -> (frame ids, gt_frames, det_frames)"""
    names = sorted(n for n in os.listdir(result_dir) if _FRAME_FILE.match(n))
    gt_frames, det_frames = [], []
    for n in names:
        gt_path = os.path.join(gt_dir, n)
        if not os.path.exists(gt_path):
            raise FileNotFoundError(f"no ground truth for {n}: {gt_path}")
        gt_frames.append(read_label_file(gt_path, "gt"))
        det_frames.append(read_label_file(os.path.join(result_dir, n), "det"))
    return [n[:-4] for n in names], gt_frames, det_frames


def eval_label_dirs(result_dir, gt_dir, cls="car", min_overlap=0.7):
    """What `evaluate_object_<min_overlap> RESULT_DIR GT_DIR` does for one class: parse the label files, score them on the GPU, write
    RESULT_DIR/stats_<cls>_{detection,orientation,detection_ground,detection_3d}.txt for the metrics evaluated, return the dict."""
    _, gt_frames, det_frames = read_label_dirs(result_dir, gt_dir)
    stats = kitti_eval_stats(gt_frames, det_frames, cls, min_overlap)
    write_stats_files(result_dir, cls, stats)
    return stats

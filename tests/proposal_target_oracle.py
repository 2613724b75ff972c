"""NumPy restatement of PointRCNN's ProposalTargetLayer (rpn/proposal_target_layer.py) consuming explicit random draws, plus the shared
pieces of its fixtures: the cases, the seeded inputs and the seeded draws.

Every random decision reads one fp32 uniform of `draws` (per cloud: key[M] | pick[P] | noise[P][T][9] | aug[P][3]).  Two
modes: dtype float32 evaluates the reference's fp32 expressions in their order, float64 is the exact-input evaluation.  Trigonometry is
evaluated in double and rounded once (tests/rcnn_oracle.py does the same), so the fp32 mode does not depend on a libm's fp32 functions.
Index decisions (picks, the range row) multiply in fp32 in both modes, as the kernels do.  IoU and pooling come from
tests/box3d_oracle.py: the fp32 mode uses its restatement of the rotated-overlap kernel, the fp64 mode its independent polygon clip.

Shared by tests/golden/make_golden_proposal_target.py (which records the imported reference), tests/test_proposal_target_host.py
(which pins this file to the recording) and tests/test_hip_proposal_target.py (which checks the HIP path against both).
"""
import copy

import numpy as np

from . import box3d_oracle as BO
from . import rcnn_oracle as CO
from . import rpn_oracle as RO

F = np.float32
D = np.float64

# M candidates, P slots, N ground-truth boxes, T noise iterations; pts points per cloud, S pooled points, C feature channels
CASES = {
    "a": dict(M=70, P=16, N=1, T=10, pts=300, S=64, C=8, depth=True, method="multiple", aug=True, seed=101),
    "b": dict(M=130, P=64, N=3, T=10, pts=257, S=1, C=0, depth=False, method="single", aug=True, seed=102),
    "c": dict(M=63, P=5, N=3, T=1, pts=300, S=48, C=5, depth=True, method="multiple", aug=False, seed=103),
    "d": dict(M=1, P=5, N=1, T=0, pts=257, S=48, C=5, depth=False, method="multiple", aug=True, seed=104),
}
B = 6
# the class mix of each cloud's candidates: (fg, hard bg, easy bg, in-between) shares; the last cloud has no fg and no bg candidate
CLOUDS = ("fg+hard+easy", "fg", "hard", "easy", "hard+easy", "none")
NONE_CLOUD = 5
RANGE = ((0.2, 0.1, np.pi / 12, 0.7), (0.3, 0.15, np.pi / 12, 0.6), (0.5, 0.15, np.pi / 9, 0.5), (0.8, 0.15, np.pi / 6, 0.3),
         (1.0, 0.15, np.pi / 3, 0.2))
CLASS_RANGE = {"fg": (0.56, 1.0), "hard": (0.06, 0.44), "easy": (0.0, 0.04), "mid": (0.46, 0.54)}
MEAN_SIZE = (1.52563191462, 1.62856739989, 3.88311640418)          # h, w, l


# ---- settings
def case_cfg(cfg_json, case):
    """the car cfg of the RCNN fixtures with one case's settings (ROI_SAMPLE_JIT on, as the car file has it)"""
    c = copy.deepcopy(cfg_json)
    k = CASES[case]
    c["RCNN"].update(ROI_PER_IMAGE=k["P"], ROI_FG_AUG_TIMES=k["T"], NUM_POINTS=k["S"], USE_DEPTH=k["depth"], REG_AUG_METHOD=k["method"],
                     ROI_SAMPLE_JIT=True)
    c["AUG_DATA"] = k["aug"]
    c["AUG_ROT_RANGE"] = 18
    return RO.make_cfg(c)


def settings(cfg):
    rc = cfg.RCNN
    return dict(P=int(rc.ROI_PER_IMAGE), T=int(rc.ROI_FG_AUG_TIMES), fg_ratio=rc.FG_RATIO, reg_fg=rc.REG_FG_THRESH, cls_fg=rc.CLS_FG_THRESH,
                cls_bg=rc.CLS_BG_THRESH, cls_bg_lo=rc.CLS_BG_THRESH_LO, hard_ratio=rc.HARD_BG_RATIO, method=rc.REG_AUG_METHOD,
                S=int(rc.NUM_POINTS), extra=rc.POOL_EXTRA_WIDTH, depth=bool(rc.USE_DEPTH), aug=bool(getattr(cfg, "AUG_DATA", True)),
                rot_range=getattr(cfg, "AUG_ROT_RANGE", 18))


# ---- draws
def blocks(M, P, T):
    return {"key": 0, "pick": M, "noise": M + P, "aug": M + P + 9 * P * T, "len": M + P + 9 * P * T + 3 * P}


def split_draws(d, M, P, T):
    """one cloud's draws -> key (M), pick (P), noise (P,T,9), aug (P,3)"""
    o = blocks(M, P, T)
    assert d.shape == (o["len"],)
    return d[:M], d[M:M + P], d[o["noise"]:o["aug"]].reshape(P, T, 9), d[o["aug"]:].reshape(P, 3)


def pick_index(u, n):
    return int(min(max(np.floor(F(u) * F(n)), 0), n - 1))


# ---- IoU
def iou3d(a7, b7, dtype):
    """boxes_iou3d_gpu of (Na,7) x (Nb,7) in the run's precision"""
    if dtype is F:
        return BO.iou3d(a7, b7)
    a7, b7 = np.asarray(a7, D).reshape(-1, 7), np.asarray(b7, D).reshape(-1, 7)

    def bev(b):
        return [b[0] - b[5] / 2, b[2] - b[4] / 2, b[0] + b[5] / 2, b[2] + b[4] / 2, b[6]]
    out = np.zeros((a7.shape[0], b7.shape[0]), D)
    for i, a in enumerate(a7):
        for j, b in enumerate(b7):
            ov = BO.clip_overlap64(bev(a), bev(b))
            oh = max(min(a[1], b[1]) - max(a[1] - a[3], b[1] - b[3]), 0.0)
            o3 = ov * oh
            out[i, j] = o3 / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - o3, 1e-7)
    return out


def _cs(ang, dtype):
    return dtype(np.cos(D(ang))), dtype(np.sin(D(ang)))


def _atan2(y, x, dtype):
    return dtype(np.arctan2(D(y), D(x)))


def _rot(x, z, cosa, sina, dtype):
    """rotate_pc_along_y_torch of (x, z), scalars or arrays"""
    r = lambda v: np.asarray(v).astype(dtype)              # each operation rounds to the run's precision (np.float64(a) would drop a length-1 axis)
    return r(r(x * cosa) + r(z * (-sina))), r(r(x * sina) + r(z * cosa))


# ---- sample_rois_for_rcnn
def random_aug_box3d(roi, u, method, dtype):
    """roi (7) dtype, u (9) one iteration's draws (fp32 values) -> the noised box"""
    c = (lambda v: dtype(F(v))) if dtype is F else D
    u = np.asarray(u, F).astype(dtype)
    h = dtype(0.5)
    out = np.array(roi, dtype)
    if method == "multiple":
        r = RANGE[pick_index(u[1], 5)]
        out[0:3] = roi[0:3] + ((u[2:5] - h) / h) * c(r[0])
        out[3:6] = roi[3:6] * (((u[5:8] - h) / h) * c(r[1]) + dtype(1.0))
        out[6] = roi[6] + ((u[8] - h) / h) * c(r[2])
    elif method == "single":
        out[0:3] = roi[0:3] + (u[2:5] - h)
        out[3:6] = roi[3:6] * ((u[5:8] - h) / c(0.5 / 0.15) + dtype(1.0))
        out[6] = roi[6] + (u[8] - h) / c(0.5 / (np.pi / 12))
    else:
        raise NotImplementedError(method)
    return out.astype(dtype)


def sample_rois(st, cand, gt, draws, dtype=F):
    """cand (B,M,7), gt (B,N,7), draws (B,len) fp32 -> dict: rois (B,P,7), gt_of_rois (B,P,7), roi_iou (B,P), src_index, n_iter (B,P) int32,
    counts (B,5) int32, kept (B,P) bool (the last iteration kept the original box), margin: the smallest distance of a compared IoU to the
    threshold it was compared with (classes, the loop's stop test)."""
    cand, gt, draws = np.asarray(cand, F), np.asarray(gt, F), np.asarray(draws, F)
    Bn, M, _ = cand.shape
    P, T = st["P"], st["T"]
    c = (lambda v: F(v)) if dtype is F else D
    fg_thresh = c(min(st["reg_fg"], st["cls_fg"]))
    bg, bg_lo = c(st["cls_bg"]), c(st["cls_bg_lo"])
    fg_per_image = int(np.round(st["fg_ratio"] * P))
    out = {"rois": np.zeros((Bn, P, 7), dtype), "gt_of_rois": np.zeros((Bn, P, 7), dtype), "roi_iou": np.zeros((Bn, P), dtype),
           "src_index": np.zeros((Bn, P), np.int32), "n_iter": np.zeros((Bn, P), np.int32), "counts": np.zeros((Bn, 5), np.int32),
           "kept": np.ones((Bn, P), bool)}
    margin = np.inf
    for b in range(Bn):
        key, pick, noise, _ = split_draws(draws[b], M, P, T)
        iou = iou3d(cand[b], gt[b], dtype)
        asg = iou.argmax(1)                                # the first maximum
        mx = iou[np.arange(M), asg]
        margin = min(margin, float(np.abs(mx[:, None].astype(D) - np.array([fg_thresh, bg, bg_lo], D)[None]).min()))
        fg = np.nonzero(mx >= fg_thresh)[0]
        easy = np.nonzero(mx < bg_lo)[0]
        hard = np.nonzero((mx < bg) & (mx >= bg_lo))[0]
        n_bg = hard.size + easy.size
        none = fg.size == 0 and n_bg == 0
        fg_taken = (min(fg_per_image, fg.size) if n_bg > 0 else P) if fg.size > 0 else 0
        bg_slots = P - fg_taken
        hard_slots = int(bg_slots * st["hard_ratio"]) if hard.size and easy.size else (bg_slots if hard.size else 0)
        out["counts"][b] = [fg.size, hard.size, easy.size, fg_taken, int(none)]
        by_key = fg[np.argsort(key[fg], kind="stable")] if fg.size else fg
        for j in range(P):
            if none:
                src = j % M
            elif j < fg_taken:
                src = by_key[j] if n_bg > 0 else fg[pick_index(pick[j], fg.size)]
            elif j < fg_taken + hard_slots:
                src = hard[pick_index(pick[j], hard.size)]
            else:
                src = easy[pick_index(pick[j], easy.size)]
            times = 0 if none else (T if j < fg_taken else min(T, 1))
            roi = cand[b, src].astype(dtype)
            g = gt[b, asg[src]].astype(dtype)
            aug, temp, cnt, keep = roi, dtype(0), 0, True
            while temp < fg_thresh and cnt < times:
                if D(noise[j, cnt, 0]) < 0.2:
                    aug, keep = roi, True
                else:
                    aug, keep = random_aug_box3d(roi, noise[j, cnt], st["method"], dtype), False
                temp = dtype(iou3d(aug[None], g[None], dtype)[0, 0])
                margin = min(margin, abs(float(temp) - float(fg_thresh)))
                cnt += 1
            out["rois"][b, j], out["gt_of_rois"][b, j] = aug, g
            out["roi_iou"][b, j] = mx[src] if (cnt == 0 or keep) else temp
            out["src_index"][b, j], out["n_iter"][b, j], out["kept"][b, j] = src, cnt, keep
    out["margin"] = margin
    return out


# ---- pooling, data augmentation, canonical transform, labels
def _sign(v):
    return np.sign(v)


def augment_box(r, g, u, rot_range, dtype):
    """data_augmentation of one ROI r and its ground truth g (7, dtype) with draws u (3): -> r, g, (cosa, sina, scale, flip factor), the smallest |ry| whose sign the
    flip read"""
    c = (lambda v: dtype(F(v))) if dtype is F else D
    u = np.asarray(u, F).astype(dtype)
    pi, two = c(np.pi), dtype(2)
    r, g = np.array(r, dtype), np.array(g, dtype)
    margin = np.inf
    angle = dtype((u[0] - dtype(1.0)) * c(np.pi / rot_range))          # (rand - 0.5 / 0.5) * (pi / AUG_ROT_RANGE), as the reference evaluates it
    ca, sa = _cs(angle, dtype)
    for v in (g, r):
        beta = _atan2(v[2], v[0], dtype)
        alpha = dtype(dtype(dtype(dtype(-_sign(beta) * pi) / two) + beta) + v[6])
        v[0], v[2] = _rot(v[0], v[2], ca, sa, dtype)
        beta = _atan2(v[2], v[0], dtype)
        v[6] = dtype(dtype(dtype(dtype(_sign(beta) * pi) / two) + alpha) - beta)
    scale = dtype(dtype(dtype((u[1] - dtype(0.5)) / dtype(0.5)) * c(0.05)) + dtype(1.0))
    flip = _sign(dtype(u[2] - dtype(0.5)))
    fx = dtype(-1.0) if flip == -1 else dtype(1.0)         # u == 0.5 exactly counts as no flip
    for v in (g, r):
        margin = min(margin, abs(float(v[6])))             # the flip reads the sign of ry
        v[0:6] = (v[0:6] * scale).astype(dtype)
        v[0] = dtype(v[0] * fx)
        if flip == -1:
            v[6] = dtype(dtype(_sign(v[6]) * pi) - v[6])
    return r, g, (ca, sa, scale, fx), margin


def pool_target(st, inp, sampled, draws, num_candidates, dtype=F):
    """inp: rpn_xyz (B,N,3), backbone_features (B,C,N), seg_mask (B,N), pts_depth (B,N); sampled: sample_rois' dict (same dtype); draws
    (B,len) -> dict: idx (R,S), count (R), empty_flag (R) int32, xyz (R,S,3), pts (R,3+E,S), feat (R,C,S), roi_boxes3d (R,7),
    gt_of_rois (R,7), cls_label, reg_valid_mask (R) int64, margin (of any near point to a face of its enlarged box), ry_margin (of an
    angle to a value where its sign or its modulo flips)."""
    xyz, feats, mask, depth = np.asarray(inp["rpn_xyz"], F), inp["backbone_features"], inp["seg_mask"], inp["pts_depth"]
    Bn, N = xyz.shape[:2]
    P, T, S, C = st["P"], st["T"], st["S"], feats.shape[1]
    E = 2 if st["depth"] else 1
    R = Bn * P
    c = (lambda v: dtype(F(v))) if dtype is F else D
    out = {"idx": np.zeros((R, S), np.int64), "count": np.zeros(R, np.int64), "empty_flag": np.zeros(R, np.int32), "xyz": np.zeros((R, S, 3), dtype),
           "pts": np.zeros((R, 3 + E, S), dtype), "feat": np.zeros((R, C, S), dtype), "roi_boxes3d": np.zeros((R, 7), dtype),
           "gt_of_rois": np.zeros((R, 7), dtype), "cls_label": np.zeros(R, np.int64), "reg_valid_mask": np.zeros(R, np.int64)}
    dch = (depth.astype(dtype) / dtype(70.0) - dtype(0.5)).astype(dtype)
    margin = ry_margin = np.inf
    for b in range(Bn):
        rois = sampled["rois"][b].astype(dtype)
        big = rois.copy()                                  # enlarge_box3d in the run's precision; the selection is the fp32 kernel's
        big[:, 3:6] = big[:, 3:6] + c(st["extra"] * 2)
        big[:, 1] = big[:, 1] + c(st["extra"])
        big = big.astype(F)
        flags = BO.pts_in_boxes3d(xyz[b], big)
        idx, empty = BO.pooled_idx(flags, S)
        margin = min(margin, CO.face_margin(xyz[b], big))
        aug_u = split_draws(np.asarray(draws[b], F), num_candidates, P, T)[3] if st["aug"] else None
        for j in range(P):
            r_ = b * P + j
            out["idx"][r_], out["empty_flag"][r_], out["count"][r_] = idx[j], empty[j], flags[j].sum()
            r, g = rois[j].copy(), sampled["gt_of_rois"][b, j].astype(dtype)
            if empty[j]:
                p = np.zeros((S, 3), dtype)
            else:
                p = xyz[b][idx[j]].astype(dtype)
                out["pts"][r_, 3] = mask[b][idx[j]]
                if st["depth"]:
                    out["pts"][r_, 4] = dch[b][idx[j]]
                out["feat"][r_] = feats[b][:, idx[j]]
            if st["aug"]:
                r, g, (ca, sa, scale, fx), m_ry = augment_box(r, g, aug_u[j], st["rot_range"], dtype)
                ry_margin = min(ry_margin, m_ry)
                px, pz = _rot(p[:, 0], p[:, 2], ca, sa, dtype)
                p = np.stack([(px * scale).astype(dtype) * fx, (p[:, 1] * scale).astype(dtype), (pz * scale).astype(dtype)], 1).astype(dtype)
            d = (p - r[None, 0:3]).astype(dtype)
            cosr, sinr = _cs(r[6], dtype)
            x, z = _rot(d[:, 0], d[:, 2], cosr, sinr, dtype)
            out["xyz"][r_] = np.stack([x, d[:, 1], z], 1)
            out["pts"][r_, 0:3] = out["xyz"][r_].T
            roi_ry = dtype(np.mod(r[6], c(2 * np.pi)))
            ry_margin = min(ry_margin, float(roi_ry), 2 * np.pi - float(roi_ry))        # the wrap of the modulo
            gc = np.array(g, dtype)
            gc[0:3] = (g[0:3] - r[0:3]).astype(dtype)
            gc[6] = dtype(g[6] - roi_ry)
            cm, sm = _cs(roi_ry, dtype)
            gc[0], gc[2] = _rot(gc[0], gc[2], cm, sm, dtype)
            out["roi_boxes3d"][r_], out["gt_of_rois"][r_] = r, gc
            iou = sampled["roi_iou"][b, j]
            no_cand = bool(sampled["counts"][b, 4])
            cls = int(iou > c(st["cls_fg"]))
            if empty[j] or (iou > c(st["cls_bg"]) and iou < c(st["cls_fg"])) or no_cand:
                cls = -1
            out["cls_label"][r_] = cls
            out["reg_valid_mask"][r_] = int(iou > c(st["reg_fg"]) and not empty[j] and not no_cand)
    out["margin"], out["ry_margin"] = margin, ry_margin
    return out


def label_margin(st, sampled):
    """the smallest distance of a slot's IoU to a threshold the labels compare it with"""
    th = np.array([st["reg_fg"], st["cls_fg"], st["cls_bg"]], D)
    return float(np.abs(np.asarray(sampled["roi_iou"], D)[..., None] - th).min())


def layer(st, inp, draws, dtype=F):
    """the whole layer -> (sample_rois' dict, pool_target's dict)"""
    s = sample_rois(st, inp["roi_boxes3d"], inp["gt_boxes3d"], draws, dtype)
    return s, pool_target(st, inp, s, draws, inp["roi_boxes3d"].shape[1], dtype)


def reference_dict(pool, sampled):
    """pool_target's result in the reference's output form (point-major)"""
    return {"sampled_pts": pool["xyz"], "pts_feature": np.concatenate([np.transpose(pool["pts"][:, 3:], (0, 2, 1)), np.transpose(pool["feat"], (0, 2, 1))], 2),
            "cls_label": pool["cls_label"], "reg_valid_mask": pool["reg_valid_mask"], "gt_of_rois": pool["gt_of_rois"],
            "gt_iou": sampled["roi_iou"].reshape(-1), "roi_boxes3d": pool["roi_boxes3d"]}


# ---- seeded fixtures
def _box_near(rs, g, lo, hi, spread):
    """a box around ground truth g whose fp32 IoU3D with it lies in [lo, hi]: offsets of scale `spread` are drawn until one does"""
    for _ in range(200):
        n = 32
        s = rs.uniform(0.3, 1.0, (n, 1)) * spread
        off = rs.uniform(-1, 1, (n, 7)) * s * np.array([1.0, 0.15, 1.6, 0.1, 0.1, 0.2, 0.25])
        c = (np.asarray(g, D)[None] + off).astype(F)
        v = BO.iou3d(c, np.asarray(g, F)[None])[:, 0]
        ok = np.nonzero((v >= lo) & (v <= hi))[0]
        if ok.size:
            return c[ok[0]]
    raise RuntimeError(f"no candidate with IoU in [{lo}, {hi}]")


SPREAD = {"fg": 0.35, "hard": 1.3, "easy": 6.0, "mid": 0.7}


def make_inputs(case, bump=0):
    """One case's layer input from seeds: roi_boxes3d (B,M,7) built around the ground truth so that every candidate's class is known,
    gt_boxes3d (B,N,7), rpn_xyz (B,pts,3) scattered over the ground-truth boxes, backbone_features (B,C,pts), seg_mask, pts_depth, and
    `classes` (B,M) the designed class of each candidate."""
    k = CASES[case]
    M, N, npts, C = k["M"], k["N"], k["pts"], k["C"]
    rs = np.random.RandomState(k["seed"] + 1000 * bump)
    gt, cand = np.zeros((B, N, 7), F), np.zeros((B, M, 7), F)
    classes = np.zeros((B, M), "U4")
    xyz = np.zeros((B, npts, 3), F)
    for b in range(B):
        for n in range(N):
            size = np.array(MEAN_SIZE) * rs.uniform(0.9, 1.1, 3)
            gt[b, n] = [rs.uniform(-2, 2) + 9.0 * (n - (N - 1) / 2), rs.uniform(0.8, 1.8), rs.uniform(14, 30), size[0], size[1], size[2],
                        rs.uniform(-np.pi, np.pi)]
        kinds = {"fg+hard+easy": ("fg", "hard", "easy"), "fg": ("fg",), "hard": ("hard",), "easy": ("easy",), "hard+easy": ("hard", "easy"),
                 "none": ("mid",)}[CLOUDS[b]]
        if M == 1 and CLOUDS[b] == "fg+hard+easy":
            kinds = ("fg",)
        for m in range(M):
            if CLOUDS[b] == "fg+hard+easy" and M > 1:     # P = 16: more fg candidates than fg slots; P = 64: fewer
                kind = "fg" if m % 5 < 2 and m < 50 else kinds[1 + m % 2]
            else:
                kind = kinds[m % len(kinds)]
            classes[b, m] = kind
            cand[b, m] = _box_near(rs, gt[b, m % N], *CLASS_RANGE[kind], SPREAD[kind])
        which = rs.randint(0, N, npts)
        g = gt[b][which].astype(D)
        local = rs.uniform(-0.5, 0.5, (npts, 3)) * g[:, [5, 3, 4]] * np.array([1.1, 1.0, 1.1])        # along l, h, w
        ca, sa = np.cos(g[:, 6]), np.sin(g[:, 6])
        xyz[b, :, 0] = g[:, 0] + local[:, 0] * ca + local[:, 2] * sa
        xyz[b, :, 2] = g[:, 2] - local[:, 0] * sa + local[:, 2] * ca
        xyz[b, :, 1] = g[:, 1] - g[:, 3] / 2 + local[:, 1]
    feats = np.maximum(rs.normal(0.0, 0.6, (B, C, npts)), 0).astype(F)
    mask = (rs.uniform(size=(B, npts)) < 0.7).astype(F)
    depth = (np.sqrt((xyz.astype(D) ** 2).sum(2)) + 20.0).astype(F)
    return {"roi_boxes3d": cand, "gt_boxes3d": gt, "rpn_xyz": xyz, "backbone_features": feats, "seg_mask": mask, "pts_depth": depth,
            "classes": classes}


def make_draws(case, bump=0):
    """(B, len) fp32 uniforms in [0,1) from a seed, with a few slots of cloud 0 set by hand so that the loop's cases occur: slot 0 keeps
    the original box at its first iteration; slot 1 draws the widest noise at every iteration (it runs all T); slot 2 draws the widest
    noise three times and then keeps the original box."""
    k = CASES[case]
    M, P, T = k["M"], k["P"], k["T"]
    o = blocks(M, P, T)
    rs = np.random.RandomState(k["seed"] + 7 + 1000 * bump)
    d = rs.randint(0, 1 << 24, (B, o["len"])).astype(F) / F(1 << 24)          # 24-bit uniforms: exact in fp32, < 1
    if T >= 10:
        wide = np.array([0.9, 0.99, 0.01, 0.5, 0.99, 0.5, 0.5, 0.5, 0.99], F)
        noise = d[0, o["noise"]:o["aug"]].reshape(P, T, 9)
        noise[0, 0, 0] = 0.1
        noise[1, :] = wide
        noise[2, :3] = wide
        noise[2, 3, 0] = 0.05
    return d

"""NumPy restatement of PointRCNN's training labels and losses (net/point_rcnn.py:generate_rpn_training_labels + filter_bbox_3d,
utils/loss_utils.py:get_reg_loss / DiceLoss / SigmoidFocalClassificationLoss, and the glue of net/rpn_loss.py and net/rcnn_loss.py), in
fp64 with analytic gradients, plus the shared pieces of the fixtures: bin layouts, cfg values, case tables and the seeded input generators
(the fixture stores seeds and outputs, not inputs).

Shared by tests/golden/make_golden_pointrcnn_loss.py (which records the imported reference), tests/test_pointrcnn_loss_host.py (which pins
this file to those recordings) and tests/test_hip_pointrcnn_loss.py (which checks the HIP path against both).

bin_targets(..., dtype=np.float32) follows the reference's fp32 run operation by operation (each Python double it mixes in is rounded to
fp32 where it meets the tensor), so its bins are the fp32 reference's; with np.float64 it is the fp64 run.
"""
import math

import numpy as np

from .rpn_oracle import make_cfg

F = np.float32
MEAN_SIZE = [1.52563191462, 1.62856739989, 3.88311640418]            # h, w, l (configs/kitti/car)

LAYOUTS = {
    "rpn52": dict(loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, get_xz_fine=False, get_y_by_bin=False, loc_y_scope=0.5,
                  loc_y_bin_size=0.25, get_ry_fine=False),
    "rpn76": dict(loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
                  loc_y_bin_size=0.25, get_ry_fine=False),
    "rcnn46": dict(loc_scope=1.5, loc_bin_size=0.5, num_head_bin=9, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
                   loc_y_bin_size=0.25, get_ry_fine=True),
    "rcnn53": dict(loc_scope=1.5, loc_bin_size=0.5, num_head_bin=9, get_xz_fine=True, get_y_by_bin=True, loc_y_scope=0.5,
                   loc_y_bin_size=0.25, get_ry_fine=True),
}
TERMS = ("x_bin", "z_bin", "x_res", "z_res", "y", "y_res", "ry_bin", "ry_res", "size", "loc", "angle", "size_again")
GRAD_WEIGHTS = (1.0, 0.7, 3.0)         # the recorded gradient is that of loc + 0.7 angle + 3 size: three different paths


def channels(lay):
    P = int(lay["loc_scope"] / lay["loc_bin_size"]) * 2
    YB = int(lay["loc_y_scope"] / lay["loc_y_bin_size"]) * 2
    return P * (4 if lay["get_xz_fine"] else 2) + (2 * YB if lay["get_y_by_bin"] else 1) + 2 * lay["num_head_bin"] + 3


# ------------------------------------------------------------------------------------------------------------ bin targets
def bin_targets(reg_label, anchor, lay, dtype=np.float32):
    """-> bins (rows,4) int64: x, z, y (-1 when not binned), ry; res (rows,7) dtype: x, z, y (the offset itself when not binned), ry
    residual labels and the three size residuals"""
    T = dtype
    lab = np.asarray(reg_label).astype(T)
    anchor = np.asarray(anchor).astype(T)

    def c(v):
        return T(v)

    def loc(col, scope, bs):
        s = np.clip(lab[:, col] + c(scope), c(0), c(scope * 2 - 1e-3))
        b = np.floor(s / c(bs)).astype(np.int64)
        r = (s - (b.astype(T) * c(bs) + c(bs / 2))) / c(bs)
        return b, r

    xb, xr = loc(0, lay["loc_scope"], lay["loc_bin_size"])
    zb, zr = loc(2, lay["loc_scope"], lay["loc_bin_size"])
    if lay["get_y_by_bin"]:
        yb, yr = loc(1, lay["loc_y_scope"], lay["loc_y_bin_size"])
    else:
        yb, yr = np.full(lab.shape[0], -1, np.int64), lab[:, 1]
    H = lay["num_head_bin"]
    two_pi = c(2 * math.pi)
    if lay["get_ry_fine"]:
        apc = (math.pi / 2) / H
        r = np.remainder(lab[:, 6], two_pi)
        flag = (r > c(math.pi * 0.5)) & (r < c(math.pi * 1.5))
        r = np.where(flag, np.remainder(r + c(math.pi), two_pi), r)
        shift = np.remainder(r + c(math.pi * 0.5), two_pi)
        shift = np.clip(shift - c(math.pi * 0.25), c(1e-3), c(math.pi * 0.5 - 1e-3))
    else:
        apc = (2 * math.pi) / H
        heading = np.remainder(lab[:, 6], two_pi)
        shift = np.remainder(heading + c(apc / 2), two_pi)
    rb = np.floor(shift / c(apc)).astype(np.int64)
    rr = (shift - (rb.astype(T) * c(apc) + c(apc / 2))) / c(apc / 2)
    size = (lab[:, 3:6] - anchor) / anchor
    res = np.concatenate([np.stack([xr, zr, yr, rr], 1), np.broadcast_to(size, (lab.shape[0], 3))], 1).astype(T)
    return np.stack([xb, zb, yb, rb], 1), res


# ------------------------------------------------------------------------------------------------------------ get_reg_loss
def _ce(x, label):
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    loss = (m + np.log(s))[:, 0] - x[np.arange(x.shape[0]), label]
    g = e / s
    g[np.arange(x.shape[0]), label] -= 1.0
    return loss, g


def _sl1(d):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5), np.clip(d, -1.0, 1.0)


def reg_loss(pred, reg_label, row_mask, lay, anchor, loss_mask=None, g=GRAD_WEIGHTS):
    """get_reg_loss over the rows row_mask selects, fp64.  -> terms (12) in TERMS order (absent terms 0), grad (rows,C) of
    g[0] loc + g[1] angle + g[2] size, zero on unselected rows"""
    pred = np.asarray(pred, np.float64)
    rows, C = pred.shape
    assert C == channels(lay)
    sel = np.asarray(row_mask).astype(bool) if row_mask is not None else np.ones(rows, bool)
    idx = np.nonzero(sel)[0]
    n = len(idx)
    terms, grad = np.zeros(12), np.zeros((rows, C))
    anchor = np.asarray(anchor, np.float64)
    bins, res = bin_targets(np.asarray(reg_label)[idx], anchor[idx] if anchor.ndim == 2 else anchor, lay, np.float64)
    x = pred[idx]
    gx = np.zeros((n, C))
    masked = loss_mask is not None
    w = np.asarray(loss_mask)[idx].astype(np.float64) if masked else np.ones(n)
    cnt = w.sum() if masked else float(n)
    dm = cnt if cnt != 0 else 1.0
    dy = float(n) if n != 0 else 1.0
    P, H = int(lay["loc_scope"] / lay["loc_bin_size"]) * 2, lay["num_head_bin"]
    YB = int(lay["loc_y_scope"] / lay["loc_y_bin_size"]) * 2
    ar = np.arange(n)

    def ce_term(k, lo, width, label, weight, denom, gscale):
        v, gg = _ce(x[:, lo:lo + width], label)
        terms[k] = (v * weight).sum() / denom
        gx[:, lo:lo + width] += gscale * gg * (weight / denom)[:, None]

    def res_term(k, lo, label, target, weight, denom, gscale):
        v, gg = _sl1(x[ar, lo + label] - target)
        terms[k] = (v * weight).sum() / denom
        gx[ar, lo + label] += gscale * gg * weight / denom

    ce_term(0, 0, P, bins[:, 0], w, dm, g[0])
    ce_term(1, P, P, bins[:, 1], w, dm, g[0])
    off = 2 * P
    if lay["get_xz_fine"]:
        res_term(2, 2 * P, bins[:, 0], res[:, 0], w, dm, g[0])
        res_term(3, 3 * P, bins[:, 1], res[:, 1], w, dm, g[0])
        off = 4 * P
    one = np.ones(n)
    if lay["get_y_by_bin"]:
        ce_term(4, off, YB, bins[:, 2], one, dy, g[0])
        res_term(5, off + YB, bins[:, 2], res[:, 2], one, dy, g[0])
        off += 2 * YB
    else:
        res_term(4, off, np.zeros(n, np.int64), res[:, 2], w, dm, g[0])
        off += 1
    ce_term(6, off, H, bins[:, 3], w, dm, g[1])
    res_term(7, off + H, bins[:, 3], res[:, 3], w, dm, g[1])
    off += 2 * H
    v, gg = _sl1(x[:, off:off + 3] - res[:, 4:7])
    ds = dm if masked else 3.0 * dm
    terms[8] = (v * w[:, None]).sum() / ds
    gx[:, off:off + 3] += g[2] * gg * (w / ds)[:, None]
    terms[9] = terms[0] + terms[1] + terms[2] + terms[3] + terms[4] + terms[5]
    terms[10] = terms[6] + terms[7]
    terms[11] = terms[8]
    grad[idx] = gx
    return terms, grad


# ------------------------------------------------------------------------------------------------------------ classification
def _sigmoid(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def _bce_logits(x, t):
    return np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))


def cls_loss(kind, logits, labels, mask=None, fg_weight=15.0, alpha=0.25, gamma=2.0, ignore=-1):
    """-> dict(loss, pos, neg, norm, grad) in fp64.  BinaryCrossEntropy is the closed form from the logit, which is what
    F.binary_cross_entropy(sigmoid(x)) evaluates in exact arithmetic."""
    x = np.asarray(logits, np.float64).reshape(-1)
    lab = np.asarray(labels, np.float64).reshape(-1)
    m = np.ones(x.shape, bool) if mask is None else np.asarray(mask).astype(bool).reshape(-1)
    p = _sigmoid(x)
    out = dict(pos=0.0, neg=0.0)
    if kind == "BinaryCrossEntropy":
        valid = ((lab >= 0) & m).astype(np.float64)
        t = (lab > 0).astype(np.float64)
        wt = np.where(lab > 0, fg_weight, 1.0)
        norm = max(valid.sum(), 1.0)
        out.update(loss=(wt * _bce_logits(x, t) * valid).sum() / norm, norm=valid.sum(), grad=wt * (p - t) * valid / norm)
    elif kind == "SigmoidFocalLoss":
        pos, neg = ((lab > 0) & m).astype(np.float64), ((lab == 0) & m).astype(np.float64)
        norm = max(pos.sum(), 1.0)
        ce1, ce0 = _bce_logits(x, 1.0), _bce_logits(x, 0.0)
        f = pos * alpha * (1 - p) ** gamma * ce1 + neg * (1 - alpha) * p ** gamma * ce0
        d1 = alpha * (1 - p) ** gamma * (-gamma * p * ce1 - (1 - p))
        d0 = (1 - alpha) * p ** gamma * (gamma * (1 - p) * ce0 + p)
        out.update(loss=f.sum() / norm, pos=(f * pos).sum() / norm, neg=(f * neg).sum() / norm, norm=pos.sum(), grad=(pos * d1 + neg * d0) / norm)
    elif kind == "DiceLoss":
        keep = (lab != ignore).astype(np.float64)
        inter, union = (np.minimum(p, lab) * keep).sum(), (np.maximum(p, lab) * keep).sum()
        u = max(union, 1.0)
        dp = p * (1 - p) * keep
        di = np.where(p < lab, dp, 0.0)
        du = np.where(p > lab, dp, 0.0) if union >= 1.0 else np.zeros_like(dp)
        out.update(loss=1.0 - inter / u, norm=union, grad=-di / u + inter * du / (u * u))
    else:
        raise KeyError(kind)
    return out


# ------------------------------------------------------------------------------------------------------------ point labels
def inside_margin(pts, corners, dtype=np.float64):
    """filter_bbox_3d: pts (N,3), corners (8,3) -> inside (N) bool, margin (N): the smallest distance of a dot product to either of its
    bounds, relative to |v|^2"""
    c = np.asarray(corners).astype(dtype)
    p = np.asarray(pts).astype(dtype) - c[4]
    ok, margin = np.ones(len(p), bool), np.full(len(p), np.inf)
    for far in (5, 0, 7):
        v = c[far] - c[4]
        m, vv = p @ v, v @ v
        ok &= (0 < m) & (m < vv)
        margin = np.minimum(margin, np.minimum(np.abs(m), np.abs(m - vv)) / vv)
    return ok, margin


def point_labels(pts, boxes7, corners, corners_large, dtype=np.float64):
    """-> cls_label (B,N), reg_label (B,N,7) in dtype"""
    pts = np.asarray(pts).astype(dtype)
    boxes7 = np.asarray(boxes7).astype(dtype)
    B, N = pts.shape[:2]
    cls, reg = np.zeros((B, N), dtype), np.zeros((B, N, 7), dtype)
    for k in range(B):
        cs, _ = inside_margin(pts[k], corners[k], dtype)
        big, _ = inside_margin(pts[k], corners_large[k], dtype)
        cls[k][cs] = 1
        cls[k][big != cs] = -1
        centre = boxes7[k, :3].copy()
        centre[1] = centre[1] - boxes7[k, 3] / 2
        reg[k][cs, :3] = centre[None] - pts[k][cs]
        reg[k][cs, 3:] = boxes7[k, 3:]
    return cls, reg


# ------------------------------------------------------------------------------------------------------------ the evaluators
RPN_CFG = {"LOSS_CLS": "BinaryCrossEntropy", "FOCAL_ALPHA": [0.25, 0.75], "FOCAL_GAMMA": 2.0, "FG_WEIGHT": 15.0, "NPOINTS": 64,
           "LOC_SCOPE": 3.0, "LOC_BIN_SIZE": 0.5, "NUM_HEAD_BIN": 12, "LOC_XZ_FINE": False, "LOSS_WEIGHT": [1.0, 1.0]}
RCNN_CFG = {"LOSS_CLS": "SigmoidFocalLoss", "FOCAL_ALPHA": [0.25, 0.75], "FOCAL_GAMMA": 2.0, "ROI_PER_IMAGE": 64, "SIZE_RES_ON_ROI": False,
            "LOC_SCOPE": 1.5, "LOC_BIN_SIZE": 0.5, "NUM_HEAD_BIN": 9, "LOC_Y_BY_BIN": False, "LOC_Y_SCOPE": 0.5, "LOC_Y_BIN_SIZE": 0.25}


def cfg_for(case):
    rpn, rcnn = dict(RPN_CFG), dict(RCNN_CFG)
    rpn.update(case.get("rpn", {}))
    rcnn.update(case.get("rcnn", {}))
    if "N" in case:
        rpn["NPOINTS"] = case["N"]
    return make_cfg({"MEAN_SIZE": [MEAN_SIZE], "RPN": rpn, "RCNN": rcnn})


def rpn_layout(cfg):
    r = cfg.RPN
    return dict(loc_scope=r.LOC_SCOPE, loc_bin_size=r.LOC_BIN_SIZE, num_head_bin=r.NUM_HEAD_BIN, get_xz_fine=r.LOC_XZ_FINE, get_y_by_bin=False,
                loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False)


def rcnn_layout(cfg):
    r = cfg.RCNN
    return dict(loc_scope=r.LOC_SCOPE, loc_bin_size=r.LOC_BIN_SIZE, num_head_bin=r.NUM_HEAD_BIN, get_xz_fine=True, get_y_by_bin=r.LOC_Y_BY_BIN,
                loc_y_scope=r.LOC_Y_SCOPE, loc_y_bin_size=r.LOC_Y_BIN_SIZE, get_ry_fine=True)


def rpn_loss(cfg, inp):
    """PointRCNNLossComputation.__call__ in fp64 -> dict of values (the reference's tb_dict names) and the gradients of
    rpn_loss_cls + rpn_loss_reg with respect to rpn_cls and rpn_reg"""
    r = cfg.RPN
    B, N = inp["cls_label"].shape
    matched = np.repeat(np.asarray(inp["matched"]) >= 0, N)
    labels = inp["cls_label"].reshape(-1)
    kind = r.LOSS_CLS
    c = cls_loss(kind, inp["rpn_cls"], labels, None if kind == "DiceLoss" else matched, fg_weight=r.FG_WEIGHT, alpha=r.FOCAL_ALPHA[0],
                 gamma=r.FOCAL_GAMMA)
    lay = rpn_layout(cfg)
    gw = (r.LOSS_WEIGHT[1], r.LOSS_WEIGHT[1], 3 * r.LOSS_WEIGHT[1])
    t, g = reg_loss(inp["rpn_reg"].reshape(B * N, -1), inp["reg_label"].reshape(B * N, 7), labels > 0, lay, MEAN_SIZE, matched, gw)
    out = {"rpn_loss_cls": c["loss"] * r.LOSS_WEIGHT[0], "rpn_loss_reg": (t[9] + t[10] + 3 * t[8]) * r.LOSS_WEIGHT[1],
           "rpn_fg_sum": int((labels > 0).sum()), "rpn_loss_loc": t[9], "rpn_loss_angle": t[10], "rpn_loss_size": 3 * t[8]}
    out["rpn_loss"] = out["rpn_loss_cls"] + out["rpn_loss_reg"]
    if kind == "SigmoidFocalLoss":
        out.update(rpn_loss_cls_pos=c["pos"], rpn_loss_cls_neg=c["neg"])
    return out, c["grad"] * r.LOSS_WEIGHT[0], g


def rcnn_loss(cfg, inp):
    r = cfg.RCNN
    lab = inp["cls_label"].reshape(-1)
    c = cls_loss(r.LOSS_CLS, inp["rcnn_cls"], lab, None, fg_weight=1.0, alpha=r.FOCAL_ALPHA[0], gamma=r.FOCAL_GAMMA)
    lay = rcnn_layout(cfg)
    anchor = inp["roi_boxes3d"][:, 3:6] if r.SIZE_RES_ON_ROI else MEAN_SIZE
    t, g = reg_loss(inp["rcnn_reg"], inp["gt_of_rois"], inp["reg_valid_mask"] > 0, lay, anchor, None, (1.0, 1.0, 3.0))
    out = {"rcnn_loss_cls": c["loss"], "rcnn_loss_reg": t[9] + t[10] + 3 * t[8], "rcnn_loss_loc": t[9], "rcnn_loss_angle": t[10],
           "rcnn_loss_size": 3 * t[8], "rcnn_cls_fg": int((lab > 0).sum()), "rcnn_cls_bg": int((lab == 0).sum()),
           "rcnn_reg_fg": int(inp["reg_valid_mask"].sum())}
    out["rcnn_loss"] = out["rcnn_loss_cls"] + out["rcnn_loss_reg"]
    if r.LOSS_CLS == "SigmoidFocalLoss":
        out.update(rpn_loss_cls_pos=c["pos"], rpn_loss_cls_neg=c["neg"])
    return out, c["grad"], g


# ------------------------------------------------------------------------------------------------------------ cases and inputs
# regression: rows, layout, loss_mask (none / random / none_true), anchor per row, selection (all / random / none / last)
REG_CASES = {
    "r1_52m": dict(rows=1, layout="rpn52", mask="random_true", per_row=False, select="all"),
    "r63_76m": dict(rows=63, layout="rpn76", mask="random", per_row=False, select="all"),
    "r64_46": dict(rows=64, layout="rcnn46", mask=None, per_row=True, select="all"),
    "r65_53": dict(rows=65, layout="rcnn53", mask=None, per_row=True, select="random"),
    "r65_46m": dict(rows=65, layout="rcnn46", mask="random", per_row=False, select="random"),
    "r65_53m": dict(rows=65, layout="rcnn53", mask="random", per_row=True, select="all"),
    "r257_52": dict(rows=257, layout="rpn52", mask=None, per_row=False, select="random"),
    "r257_76m": dict(rows=257, layout="rpn76", mask="random", per_row=False, select="random"),
    "r257_none": dict(rows=257, layout="rpn52", mask="random", per_row=False, select="none"),
    "r257_allmasked": dict(rows=257, layout="rpn76", mask="none_true", per_row=False, select="random"),
    "r3840_76m": dict(rows=5 * 768, layout="rpn76", mask="random", per_row=False, select="random", every=16),
    "r3840_last": dict(rows=5 * 768, layout="rpn52", mask="random_true", per_row=False, select="last", every=16),
}


def stored_rows(case):
    """the gradient rows the fixture keeps: all, or every 16th counted so that the last row is one of them"""
    e = case.get("every", 1)
    return np.arange(e - 1, case["rows"], e)


def make_reg_labels(rs, rows, lay):
    s = lay["loc_scope"]
    lab = np.empty((rows, 7))
    lab[:, 0] = rs.uniform(-1.3 * s, 1.3 * s, rows)
    lab[:, 1] = rs.uniform(-0.8, 0.8, rows)
    lab[:, 2] = rs.uniform(-1.3 * s, 1.3 * s, rows)
    lab[:, 3:6] = np.array(MEAN_SIZE) * rs.uniform(0.8, 1.2, (rows, 3))
    lab[:, 6] = rs.uniform(-2 * math.pi, 3 * math.pi, rows)
    return lab.astype(F)


def make_reg_case(case, seed):
    rs = np.random.RandomState(seed)
    lay = LAYOUTS[case["layout"]]
    rows = case["rows"]
    pred = rs.normal(0.0, 1.5, (rows, channels(lay))).astype(F)
    lab = make_reg_labels(rs, rows, lay)
    sel = {"all": np.ones(rows, bool), "random": rs.uniform(size=rows) < 0.4, "none": np.zeros(rows, bool),
           "last": np.arange(rows) == rows - 1}[case["select"]]
    draw = rs.uniform(size=rows) < 0.7
    mask = {None: None, "random": draw, "random_true": np.ones(rows, bool), "none_true": np.zeros(rows, bool)}[case["mask"]]
    anchor = (np.array(MEAN_SIZE) * rs.uniform(0.9, 1.1, (rows, 3))).astype(F) if case["per_row"] else np.array(MEAN_SIZE, F)
    return dict(pred=pred, reg_label=lab, row_mask=sel, loss_mask=mask, anchor=anchor)


def make_edge_rows(lay):
    """reg_label rows on the bin edges: offsets -scope, 0, one bin, scope - 1e-3, scope, 2 scope on x (z and y take the next ones), crossed
    with ry = 0, +-pi, +-pi / num_head_bin, 2 pi + 0.1, pi / 2, 3 pi / 2"""
    s, b, ys, yb = lay["loc_scope"], lay["loc_bin_size"], lay["loc_y_scope"], lay["loc_y_bin_size"]
    offs = [-s, 0.0, b, s - 1e-3, s, 2 * s]
    yoffs = [-ys, 0.0, yb, ys - 1e-3, ys, 2 * ys]
    H = lay["num_head_bin"]
    rys = [0.0, math.pi, -math.pi, math.pi / H, -math.pi / H, 2 * math.pi + 0.1, math.pi / 2, 3 * math.pi / 2]
    rows = []
    for i in range(6):
        for ry in rys:
            rows.append([offs[i], yoffs[(i + 2) % 6], offs[(i + 1) % 6]] + MEAN_SIZE + [ry])
    return np.array(rows, F)


# the RPN evaluator (and, through it, the classification losses): B clouds of N points
_KINDS = {"bce": "BinaryCrossEntropy", "focal": "SigmoidFocalLoss", "dice": "DiceLoss"}
RPN_CASES = {}
for _k, _kind in _KINDS.items():
    RPN_CASES.update({
        f"c1_{_k}": dict(B=1, N=1, labels="one", matched=[0], rpn={"LOSS_CLS": _kind}),
        f"c65_{_k}": dict(B=1, N=65, labels="mixed", matched=[0], rpn={"LOSS_CLS": _kind}),
        f"c3840_{_k}": dict(B=5, N=768, labels="mixed", matched=[0, -1, 2, 0, 1], rpn={"LOSS_CLS": _kind}, every=16),
        f"c65_ign_{_k}": dict(B=1, N=65, labels="ignore", matched=[0], rpn={"LOSS_CLS": _kind}),
        f"c65_nopos_{_k}": dict(B=1, N=65, labels="nopos", matched=[0], rpn={"LOSS_CLS": _kind}),
        f"c65_maskfalse_{_k}": dict(B=1, N=65, labels="mixed", matched=[-1], rpn={"LOSS_CLS": _kind}),
    })
RPN_CASES.update({
    "ev_bce": dict(B=5, N=64, labels="mixed", matched=[0, -1, 1, 0, 2], rpn={"LOSS_CLS": "BinaryCrossEntropy", "LOSS_WEIGHT": [0.8, 1.2]}),
    "ev_focal": dict(B=5, N=64, labels="mixed", matched=[0, -1, 1, 0, 2],
                     rpn={"LOSS_CLS": "SigmoidFocalLoss", "LOSS_WEIGHT": [0.8, 1.2], "LOC_XZ_FINE": True}),
    "ev_dice": dict(B=5, N=64, labels="mixed", matched=[0, -1, 1, 0, 2], rpn={"LOSS_CLS": "DiceLoss", "LOSS_WEIGHT": [0.8, 1.2]}),
    "ev_nofg": dict(B=5, N=64, labels="nopos", matched=[0, -1, 1, 0, 2], rpn={"LOSS_CLS": "BinaryCrossEntropy", "LOSS_WEIGHT": [0.8, 1.2]}),
})
RCNN_CASES = {
    "rc16_focal": dict(R=16, rcnn={"LOSS_CLS": "SigmoidFocalLoss"}),
    # no -1 label here: F.binary_cross_entropy refuses a target outside [0, 1], so the reference's BCE branch cannot take one
    "rc65_bce": dict(R=65, no_ignore=True, rcnn={"LOSS_CLS": "BinaryCrossEntropy", "LOC_Y_BY_BIN": True, "SIZE_RES_ON_ROI": True}),
}


def make_rpn_case(case, seed):
    """logits within +-6 (the fp32 reference's log(1 - sigmoid) is well conditioned there)"""
    rs = np.random.RandomState(seed)
    cfg = cfg_for(case)
    B, N = case["B"], case["N"]
    C = channels(rpn_layout(cfg))
    u = rs.uniform(size=(B, N))
    lab = {"one": np.ones((B, N)), "mixed": np.where(u < 0.4, 1.0, np.where(u < 0.55, -1.0, 0.0)), "ignore": -np.ones((B, N)),
           "nopos": np.where(u < 0.3, -1.0, 0.0)}[case["labels"]]
    return dict(rpn_cls=rs.uniform(-6.0, 6.0, (B, N, 1)).astype(F), rpn_reg=rs.normal(0.0, 1.5, (B, N, C)).astype(F),
                cls_label=lab.astype(F), reg_label=make_reg_labels(rs, B * N, rpn_layout(cfg)).reshape(B, N, 7),
                matched=np.array(case["matched"], np.int64))


def make_rcnn_case(case, seed):
    rs = np.random.RandomState(seed)
    cfg = cfg_for(case)
    R = case["R"]
    lay = rcnn_layout(cfg)
    u = rs.uniform(size=R)
    cls_label = np.where(u < 0.4, 1.0, np.where(u < 0.55, 0.0 if case.get("no_ignore") else -1.0, 0.0)).astype(F)
    roi = np.concatenate([rs.uniform(-2, 2, (R, 3)), np.array(MEAN_SIZE) * rs.uniform(0.85, 1.15, (R, 3)), rs.uniform(-3, 3, (R, 1))], 1).astype(F)
    return dict(rcnn_cls=rs.uniform(-6.0, 6.0, (R, 1)).astype(F), rcnn_reg=rs.normal(0.0, 1.5, (R, channels(lay))).astype(F),
                cls_label=cls_label, reg_valid_mask=(rs.uniform(size=R) < 0.5).astype(np.int64), gt_of_rois=make_reg_labels(rs, R, lay),
                roi_boxes3d=roi)


# point labels: (B, N); cloud 1 (when there is one) has no point inside, cloud 2 lies entirely inside
LABEL_CASES = {"lb_1_1": (1, 1), "lb_3_65": (3, 65), "lb_16_768": (16, 768)}


def make_label_case(name, seed):
    B, N = LABEL_CASES[name]
    rs = np.random.RandomState(seed)
    boxes = np.empty((B, 7))
    boxes[:, :3] = rs.uniform(-0.5, 0.5, (B, 3)) + np.array([0.0, 0.8, 0.0])
    boxes[:, 3:6] = np.array(MEAN_SIZE) * rs.uniform(0.85, 1.15, (B, 3))
    boxes[:, 6] = (np.arange(B) % 4) * (math.pi / 2) - math.pi + rs.uniform(0.1, math.pi / 2 - 0.1, B)         # all four quadrants
    pts = np.empty((B, N, 3))
    for b in range(B):
        h, w, l, ry = boxes[b, 3:]
        scale = 1.6 if b != 2 else 0.45
        local = rs.uniform(-0.5, 0.5, (N, 3)) * np.array([l, h, w]) * scale
        if b == 1:
            local[:, 0] += 3 * l
        cs, sn = math.cos(ry), math.sin(ry)
        x = cs * local[:, 0] + sn * local[:, 2]
        z = -sn * local[:, 0] + cs * local[:, 2]
        pts[b] = np.stack([x, local[:, 1] - h / 2, z], 1) + boxes[b, :3]
    return pts.astype(F), boxes.astype(F)


# saturation: logits where the fp32 reference's log(1 - sigmoid(x)) has clamped; checked against cls_loss's closed form only
def make_saturation_case():
    x = np.array([20.0, -20.0, 50.0, -50.0, 100.0, -100.0] * 2, F)
    lab = np.array([1.0] * 6 + [0.0] * 6, F)
    return x, lab

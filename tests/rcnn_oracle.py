"""NumPy restatement of PointRCNN's RCNN stage (net/rcnn_net.py eval forward, net/rcnn_inference.py, utils/bbox_transform.py
decode_bbox_target in the RCNN form, structures/bounding_box_3d.py, point_rcnn.py:combine_2d_3d) on tests/rpn_oracle.py,
tests/pn2_oracle.py and tests/box3d_oracle.py, plus the shared pieces of the RCNN fixtures: the seeded inputs and weights.

Shared by tests/golden/make_golden_rcnn.py (which records the imported reference), tests/test_rcnn_host.py (which pins this file to
those recordings) and tests/test_hip_rcnn.py (which checks the HIP path against both).

Trigonometry of the fp32 paths is evaluated in double and rounded once, so the seeded fp32 inputs built here (`pool_canonical` with
dtype float32, which the network fixtures are fed with) do not depend on a libm's fp32 cos / sin.
"""
import numpy as np

from . import box3d_oracle as BO
from . import pn2_oracle as PO
from . import rpn_oracle as RO

F = np.float32
D = np.float64

# cases: cloud kinds, cloud seed, ROIs per cloud, input seed
BATCHES = {"b2": (("surface", "sparse"), 300, 16, 11), "b5": (("surface", "dup", "sparse", "surface", "surface"), 400, 16, 12)}
FALLBACK_CLOUD = {"b2": None, "b5": 3}       # the cloud whose post-process scores are pushed below SCORE_THRESH
N_FEAT = 128
POOL_EXTRA_WIDTH = 1.0       # RCNN.POOL_EXTRA_WIDTH of the fixtures' cfg
FACE_MARGIN = 2e-4


# ---- seeded fixtures
def random_state(shapes, seed):
    """rpn_oracle.random_state (He-normal weights, BN statistics) with conv biases ~N(0, 0.1): the RCNN runs without BatchNorm, so
    every conv has a bias, which the RPN rule leaves at 0."""
    sd = RO.random_state(shapes, seed)
    rs = np.random.RandomState(seed + 1000)
    for name in sorted(sd):
        if name.endswith("conv.bias"):
            sd[name] = rs.normal(0.0, 0.1, sd[name].shape).astype(F)
    return sd


def make_inputs(tag, bump=0):
    """What an RPN run hands to the RCNN, from seeds: rpn_xyz (B,N,3), backbone_features (B,C,N), seg_mask (B,N), pts_depth (B,N),
    roi_boxes3d (B,M,7), roi_scores_raw (B,M).  The ROIs are car-sized boxes scattered around each cloud; slot 1 lies far away (empty),
    slot 2 is a small box at the cloud's edge (fewer than S points), the last slot is an all-zero padding ROI with score 0.  In the
    fallback cloud every real proposal has a negative score, so the reference's argmax lands on the padding slot."""
    kinds, cseed, M, iseed = BATCHES[tag]
    rs = np.random.RandomState(iseed + 1000 * bump)
    base = RO.make_batch(kinds, cseed)
    B, N = base.shape[:2]
    feats = np.maximum(rs.normal(0.0, 0.6, (B, N_FEAT, N)), 0).astype(F)
    mask = (rs.uniform(size=(B, N)) < 0.7).astype(F)
    xyz, rois = np.zeros_like(base), np.zeros((B, M, 7), F)
    for b in range(B):
        # a cloud's offset and ROIs are drawn again until no point lies within FACE_MARGIN of a face of an enlarged ROI, so that the
        # in-box decisions do not hang on the last bits of a rotation
        g = np.random.RandomState(100 * iseed + b + 1000 * bump)
        for attempt in range(1000):
            xyz[b] = (base[b] + g.uniform(-0.3, 0.3, (1, 3)).astype(F)).astype(F)
            ctr = xyz[b].mean(0)
            for m in range(M - 1):
                c = ctr + g.normal(0.0, 0.5, 3) * np.array([1.0, 0.2, 1.6])
                size = np.array([1.5, 1.6, 3.9]) * g.uniform(0.85, 1.15, 3)
                rois[b, m] = [c[0], c[1] + size[0] / 2, c[2], size[0], size[1], size[2], g.uniform(-np.pi, np.pi)]
            rois[b, 1, [0, 2]] += 30.0
            rois[b, 2] = [ctr[0] - 1.9, ctr[1] + 0.2, ctr[2] + 2.6, 0.4, 0.5, 0.6, 0.3]
            if face_margin(xyz[b], BO.enlarge_box3d(rois[b], POOL_EXTRA_WIDTH)) >= FACE_MARGIN:
                break
        else:
            raise RuntimeError("make_inputs: no draw met the face margin")
    depth = np.sqrt((xyz[..., 0] * xyz[..., 0] + xyz[..., 1] * xyz[..., 1]).astype(F) + xyz[..., 2] * xyz[..., 2]).astype(F) + F(20.0)
    scores = rs.normal(0.0, 2.0, (B, M)).astype(F)
    scores[:, M - 1] = 0
    fb = FALLBACK_CLOUD[tag]
    if fb is not None:
        scores[fb, :M - 1] = -np.abs(scores[fb, :M - 1]) - F(0.1)
    return {"rpn_xyz": xyz, "backbone_features": feats, "seg_mask": mask, "pts_depth": depth.astype(F), "roi_boxes3d": rois,
            "roi_scores_raw": scores}


def post_cls(tag, rcnn_cls):
    """The class logits the post-process fixtures use: the network's own, spread out, and pushed down in the fallback cloud."""
    kinds, _, M, _ = BATCHES[tag]
    c = (np.asarray(rcnn_cls, F).reshape(len(kinds), M) * F(4.0)).astype(F)
    c = (c - np.sort(c, axis=1)[:, M // 2:M // 2 + 1] + F(-1.5)).astype(F)
    if FALLBACK_CLOUD[tag] is not None:
        c[FALLBACK_CLOUD[tag]] = (-np.abs(c[FALLBACK_CLOUD[tag]]) - F(4.0)).astype(F)
    return c.reshape(-1, 1)


# ---- pooling + canonical transform
def _cs(ang, dtype):
    a = np.asarray(ang, D)
    return np.cos(a).astype(dtype), np.sin(a).astype(dtype)


def pool_canonical(inp, extra_width, S, use_depth=True, dtype=D):
    """-> dict: idx (R,S) int64 selected point per slot, empty (R) int32, count (R) in-box points, xyz (R,S,3), pts (R,3+E,S),
    feat (R,C,S), margin (the smallest distance of any near point to a face of its enlarged box, in the rotated fp64 frame).
    dtype float32 evaluates the reference's fp32 expressions in order; float64 is the exact-input fp64 evaluation."""
    xyz, rois = np.asarray(inp["rpn_xyz"], F), np.asarray(inp["roi_boxes3d"], F)
    feats, mask, depth = inp["backbone_features"], inp["seg_mask"], inp["pts_depth"]
    B, N = xyz.shape[:2]
    M, C = rois.shape[1], feats.shape[1]
    E = 2 if use_depth else 1
    R = B * M
    out = {"idx": np.zeros((R, S), np.int64), "empty": np.zeros(R, np.int32), "count": np.zeros(R, np.int64),
           "xyz": np.zeros((R, S, 3), dtype), "pts": np.zeros((R, 3 + E, S), dtype), "feat": np.zeros((R, C, S), dtype)}
    margin = np.inf
    dch = (depth.astype(dtype) / dtype(70.0) - dtype(0.5)).astype(dtype)
    for b in range(B):
        big = BO.enlarge_box3d(rois[b], extra_width)
        flags = BO.pts_in_boxes3d(xyz[b], big)
        idx, empty = BO.pooled_idx(flags, S)
        margin = min(margin, face_margin(xyz[b], big))
        for m in range(M):
            r = b * M + m
            out["idx"][r], out["empty"][r], out["count"][r] = idx[m], empty[m], flags[m].sum()
            roi = rois[b, m]
            if empty[m]:
                p = np.zeros((S, 3), dtype)
            else:
                p = xyz[b][idx[m]].astype(dtype)
                out["pts"][r, 3] = mask[b][idx[m]]
                if use_depth:
                    out["pts"][r, 4] = dch[b][idx[m]]
                out["feat"][r] = feats[b][:, idx[m]]
            d = (p - roi[:3].astype(dtype)).astype(dtype)
            cosa, sina = _cs(roi[6], dtype)
            x = ((d[:, 0] * cosa).astype(dtype) + (d[:, 2] * (-sina)).astype(dtype)).astype(dtype)
            z = ((d[:, 0] * sina).astype(dtype) + (d[:, 2] * cosa).astype(dtype)).astype(dtype)
            out["xyz"][r] = np.stack([x, d[:, 1], z], 1)
            out["pts"][r, 0:3] = out["xyz"][r].T
    out["margin"] = margin
    return out


def face_margin(pts, big):
    """How far the in-box decision of any point is from flipping, in fp64: pts (N,3), big (M,7).  A point is inside when the largest of its
    signed slab distances (x, y, z of the rotated box, the two max_dis tests) is negative; the margin is the smallest magnitude of it."""
    p, b = np.asarray(pts, D), np.asarray(big, D)
    best = np.inf
    for m in range(b.shape[0]):
        cx, by, cz, h, w, l, ry = b[m]
        dx, dz = p[:, 0] - cx, p[:, 2] - cz
        sy = np.abs(p[:, 1] - (by - h / 2)) - h / 2
        sx = np.abs(dx * np.cos(ry) - dz * np.sin(ry)) - l / 2
        sz = np.abs(dx * np.sin(ry) + dz * np.cos(ry)) - w / 2
        s = np.maximum(np.maximum(np.maximum(sx, sy), sz), np.maximum(np.abs(dx), np.abs(dz)) - 10.0)
        best = min(best, float(np.abs(s).min()))
    return best


def pts_input_of(pool):
    """The reference's point-major (R,S,3+E+C) tensor from a pool_canonical result."""
    return np.concatenate([np.transpose(pool["pts"], (0, 2, 1)), np.transpose(pool["feat"], (0, 2, 1))], 2)


# ---- network
def _mlp_cols(x, layers, dtype):
    """x (Cin, cols) -> ReLU MLP (Cout, cols)"""
    for w, b in layers:
        x = np.maximum(w.astype(dtype) @ x + b.astype(dtype)[:, None], 0)
    return x


def network(sd, cfg, pts_input, dtype=D, chunk=8):
    """RCNNNet on the point-major input (R,S,3+E+C) -> {'xyz_up','merge_down','sa0','sa1','sa2'} (channel-major), rcnn_cls (R,1),
    rcnn_reg (R,reg).  Index ops (FPS, ball query) run on the fp32 coordinates, as the product's and the reference's do."""
    rc = cfg.RCNN
    n_in = 3 + 1 + int(rc.USE_DEPTH)
    pts_input = np.asarray(pts_input)
    R = pts_input.shape[0]
    xyz0 = np.ascontiguousarray(pts_input[..., :3]).astype(F)
    levels = {k: [] for k in ["xyz_up", "merge_down"] + [f"sa{k}" for k in range(len(rc.SA_CONFIG.NPOINTS))]}
    up = [RO.folded_layer(sd, p) for p in RO.mlp_prefixes(sd, "xyz_up_layer")]
    md = [RO.folded_layer(sd, p) for p in RO.mlp_prefixes(sd, "merge_down_layer")]
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(R, r0 + chunk))
        pin = pts_input[sl].astype(dtype)
        x = np.transpose(pin[..., :n_in], (0, 2, 1))
        for w, b in up:
            x = RO.pointwise_mlp(x, None, w, b, True, dtype)
        levels["xyz_up"].append(x)
        f = RO.pointwise_mlp(x, np.transpose(pin[..., n_in:], (0, 2, 1)), md[0][0], md[0][1], True, dtype)
        levels["merge_down"].append(f)
        cur = xyz0[sl]
        for k, npoint in enumerate(rc.SA_CONFIG.NPOINTS):
            layers = [RO.folded_layer(sd, p) for p in RO.mlp_prefixes(sd, f"SA_modules.{k}.mlps.0")]
            nb = cur.shape[0]
            if npoint == -1:
                new_xyz = np.zeros((nb, 1, 3), F)
                idx = np.broadcast_to(np.arange(cur.shape[1], dtype=np.int32), (nb, 1, cur.shape[1]))
            else:
                fidx = PO.fps(cur, npoint)
                new_xyz = np.stack([cur[i][fidx[i]] for i in range(nb)])
                idx = PO.ball_query(rc.SA_CONFIG.RADIUS[k], rc.SA_CONFIG.NSAMPLE[k], cur, new_xyz)
            outs = []
            for i in range(nb):                                 # per ROI: the grouped tensor of a chunk would not fit
                g = RO.grouped_input(cur[i:i + 1], new_xyz[i:i + 1], f[i:i + 1], idx[i:i + 1], dtype)[0]        # (3+C, M, ns)
                y = _mlp_cols(g.reshape(g.shape[0], -1), layers, dtype)
                outs.append(y.reshape(y.shape[0], g.shape[1], g.shape[2]).max(2))
            f = np.stack(outs)
            levels[f"sa{k}"].append(f)
            cur = new_xyz
    levels = {k: np.concatenate(v) for k, v in levels.items()}
    last = levels[f"sa{len(rc.SA_CONFIG.NPOINTS) - 1}"]
    cls, reg = heads(sd, last, dtype)
    return levels, cls, reg


def heads(sd, last, dtype=D):
    """last (R,C,1) -> rcnn_cls (R,1), rcnn_reg (R,reg)"""
    out = []
    x0 = np.ascontiguousarray(last[:, :, 0].T)[None]            # (1,C,R)
    for head in ("cls_layer", "reg_layer"):
        ids = sorted({int(k.split(".")[1]) for k in sd if k.startswith(head + ".")})
        x = x0
        for j, i in enumerate(ids):
            w, b = RO.folded_layer(sd, f"{head}.{i}")
            x = RO.pointwise_mlp(x, None, w, b, j + 1 < len(ids), dtype)
        out.append(np.ascontiguousarray(x[0].T))
    return out


# ---- decode
def reg_layout(rc):
    nb = int(rc.LOC_SCOPE / rc.LOC_BIN_SIZE) * 2
    ny = int(rc.LOC_Y_SCOPE / rc.LOC_Y_BIN_SIZE) * 2
    hb = int(rc.NUM_HEAD_BIN)
    y0 = 4 * nb
    a0 = y0 + (2 * ny if rc.LOC_Y_BY_BIN else 1)
    return dict(nb=nb, ny=ny, hb=hb, y0=y0, a0=a0, s0=a0 + 2 * hb, R=a0 + 2 * hb + 3)


def decode_bins(reg, rc):
    """-> (n,4) int: x, z, y (0 without LOC_Y_BY_BIN), ry bins by first-maximum argmax"""
    L = reg_layout(rc)
    reg = np.asarray(reg)
    yb = reg[:, L["y0"]:L["y0"] + L["ny"]].argmax(1) if rc.LOC_Y_BY_BIN else np.zeros(reg.shape[0], np.int64)
    return np.stack([reg[:, :L["nb"]].argmax(1), reg[:, L["nb"]:2 * L["nb"]].argmax(1), yb, reg[:, L["a0"]:L["a0"] + L["hb"]].argmax(1)], 1)


def argmax_margin(reg, rc):
    L = reg_layout(rc)
    groups = [(0, L["nb"]), (L["nb"], 2 * L["nb"]), (L["a0"], L["a0"] + L["hb"])] + ([(L["y0"], L["y0"] + L["ny"])] if rc.LOC_Y_BY_BIN else [])
    gaps = []
    for lo, hi in groups:
        s = np.sort(np.asarray(reg, D)[:, lo:hi], 1)
        gaps.append((s[:, -1] - s[:, -2]).min())
    return float(min(gaps))


def decode(roi, reg, rc, mean_size, dtype=F, bins=None):
    """decode_bbox_target (get_xz_fine, get_ry_fine, LOC_Y_BY_BIN as rc says): roi (n,7), reg (n,R) -> boxes (n,7) in `dtype`.
    float32: every operation rounded in the reference's order, constants as the Python doubles rounded at their use; float64 with the
    given bins: the exact-input evaluation."""
    T = dtype
    roi, reg = np.asarray(roi, F).astype(T), np.asarray(reg).astype(T)
    L = reg_layout(rc)
    assert reg.shape[1] == L["R"]
    bins = decode_bins(reg, rc) if bins is None else np.asarray(bins)
    rows = np.arange(reg.shape[0])
    nb = L["nb"]
    bs, hb_, sc = T(rc.LOC_BIN_SIZE), T(rc.LOC_BIN_SIZE / 2), T(rc.LOC_SCOPE)
    xb, zb, yb, rb = bins.T
    pos_x = ((xb.astype(T) * bs).astype(T) + hb_).astype(T) - sc
    pos_z = ((zb.astype(T) * bs).astype(T) + hb_).astype(T) - sc
    pos_x = (pos_x.astype(T) + (reg[rows, 2 * nb + xb] * bs).astype(T)).astype(T)
    pos_z = (pos_z.astype(T) + (reg[rows, 3 * nb + zb] * bs).astype(T)).astype(T)
    if rc.LOC_Y_BY_BIN:
        ybs, yh, ysc = T(rc.LOC_Y_BIN_SIZE), T(rc.LOC_Y_BIN_SIZE / 2), T(rc.LOC_Y_SCOPE)
        y_res = (reg[rows, L["y0"] + L["ny"] + yb] * ybs).astype(T)
        pos_y = ((((yb.astype(T) * ybs).astype(T) + yh).astype(T) - ysc).astype(T) + y_res).astype(T)
        pos_y = (pos_y + roi[:, 1]).astype(T)
    else:
        pos_y = (roi[:, 1] + reg[:, L["y0"]]).astype(T)
    apc = (np.pi / 2) / L["hb"]
    ry_res = (reg[rows, L["a0"] + L["hb"] + rb] * T(apc / 2)).astype(T)
    ry = ((((rb.astype(T) * T(apc)).astype(T) + T(apc / 2)).astype(T) + ry_res).astype(T) - T(np.pi / 4)).astype(T)
    anchor = np.asarray(mean_size, D).astype(F).astype(T)
    hwl = ((reg[:, L["s0"]:L["s0"] + 3] * anchor).astype(T) + anchor).astype(T)
    cosa, sina = _cs(-roi[:, 6], T)
    x = ((pos_x * cosa).astype(T) + (pos_z * (-sina)).astype(T)).astype(T)
    z = ((pos_x * sina).astype(T) + (pos_z * cosa).astype(T)).astype(T)
    ry = (ry + roi[:, 6]).astype(T)
    x, z = (x + roi[:, 0]).astype(T), (z + roi[:, 2]).astype(T)
    return np.stack([x, pos_y, z, hwl[:, 0], hwl[:, 1], hwl[:, 2], ry], 1).astype(T)


def sigmoid(x, dtype=F):
    x = np.asarray(x, dtype)
    return (dtype(1) / (dtype(1) + np.exp(-x))).astype(dtype)


# ---- Box3DList
def box_corners(b7, dtype=D, mode="xyzhwl_ry"):
    """(n,7) -> (n,24) rect-frame corners in the reference's order"""
    b = np.asarray(b7).astype(dtype).reshape(-1, 7)
    x, y, z, h, w, l, ry = (b[:, k] for k in range(7)) if mode == "xyzhwl_ry" else (b[:, k] for k in (4, 5, 6, 2, 3, 1, 0))
    z0 = np.zeros_like(h)
    xc = np.stack([-l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2], 1)
    yc = np.stack([z0, -h, -h, z0, z0, -h, -h, z0], 1)
    zc = np.stack([w / 2, w / 2, w / 2, w / 2, -w / 2, -w / 2, -w / 2, -w / 2], 1)
    c, s = _cs(ry, dtype)
    X = (c[:, None] * xc).astype(dtype) + (s[:, None] * zc).astype(dtype) + x[:, None]
    Z = (-s[:, None] * xc).astype(dtype) + (c[:, None] * zc).astype(dtype) + z[:, None]
    Y = yc + y[:, None]
    return np.stack([X, Y, Z], 2).astype(dtype).reshape(-1, 24)


def corners_to_box(c24, dtype=D, mode="xyzhwl_ry"):
    c = np.asarray(c24).astype(dtype).reshape(-1, 8, 3)
    dif = c[:, 3] - c[:, 0]
    ry = -np.arctan2(dif[:, 2], dif[:, 0])
    xyz = (c[:, 7] + c[:, 0]) / dtype(2)
    norm = lambda v: np.sqrt((v * v).sum(1))
    l, h, w = norm(c[:, 0] - c[:, 3]), norm(c[:, 0] - c[:, 1]), norm(c[:, 0] - c[:, 4])
    cols = [xyz[:, 0], xyz[:, 1], xyz[:, 2], h, w, l, ry] if mode == "xyzhwl_ry" else [ry, l, h, w, xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    return np.stack(cols, 1).astype(dtype)


def to_ry_lhwxyz(b7, dtype=D):
    return corners_to_box(box_corners(b7, dtype), dtype, "ry_lhwxyz")


def rotate_back(pts, mean, rot, dtype=D):
    """point_rcnn.py's un-centre + rotate_back of (B,n,3) points; rot (B) float64"""
    p = np.asarray(pts).astype(dtype) + np.asarray(mean).astype(dtype)[:, None, :]
    a = -np.asarray(rot, D)
    c, s = np.cos(a).astype(dtype)[:, None], np.sin(a).astype(dtype)[:, None]
    out = p.copy()
    out[..., 0] = (p[..., 0] * c).astype(dtype) + (p[..., 2] * (-s)).astype(dtype)
    out[..., 2] = (p[..., 0] * s).astype(dtype) + (p[..., 2] * c).astype(dtype)
    return out.astype(dtype)


def rois_to_camera(rois, mean, rot, dtype=D):
    """(B,M,7) proposals of the centred, rotated clouds -> camera frame through their corners (point_rcnn.py:303-312)"""
    B, M = rois.shape[:2]
    c = box_corners(rois.reshape(-1, 7), dtype).reshape(B, M * 8, 3)
    return corners_to_box(rotate_back(c, mean, rot, dtype).reshape(-1, 24), dtype).reshape(B, M, 7)


# ---- post-process
def postprocess(rc, mean_size, rois, roi_scores_raw, rcnn_cls, rcnn_reg):
    """Box3DPointRCNNPostProcess on fp32 inputs -> per cloud: dict(fallback, keep (ROI indices in list order), boxes (k,7) xyzhwl_ry,
    scores (k)), and the margins (score threshold, NMS walk).  Ties in the score order resolve to the lower ROI index."""
    B, M = rois.shape[:2]
    raw = np.asarray(rcnn_cls, F).reshape(B, M)
    norm = sigmoid(raw)
    boxes = decode(rois.reshape(-1, 7), rcnn_reg, rc, mean_size).reshape(B, M, 7)
    out = []
    m_score = float(np.abs(norm.astype(D) - D(F(rc.SCORE_THRESH))).min())
    m_nms = np.inf
    for b in range(B):
        sel = np.nonzero(norm[b] > F(rc.SCORE_THRESH))[0]
        if sel.size == 0:
            k = int(np.argmax(roi_scores_raw[b]))
            out.append(dict(fallback=True, keep=np.array([k]), boxes=rois[b, k][None], scores=np.zeros(1, F)))
            continue
        order = sel[np.argsort(-raw[b, sel], kind="stable")]
        keep, mg = RO.nms_walk(BO.boxes3d_to_bev(boxes[b, order]), rc.NMS_THRESH)
        m_nms = min(m_nms, mg)
        out.append(dict(fallback=False, keep=order[keep], boxes=boxes[b, order[keep]], scores=raw[b, order[keep]]))
    return out, m_score, m_nms


def best_of(lists):
    """combine_2d_3d: the arg-max entry of every cloud's list -> (ROI index, box xyzhwl_ry, score, random)"""
    res = []
    for d in lists:
        i = int(np.argmax(d["scores"]))
        res.append((int(d["keep"][i]), d["boxes"][i], float(d["scores"][i]), int(d["fallback"])))
    return res

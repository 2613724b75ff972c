"""NumPy restatement of PointRCNN's RPN inference (net/rpn.py, net/pointnet2_msg.py, pointnet2_modules.py, rpn/proposal_layer.py,
utils/bbox_transform.py:decode_bbox_target) on tests/pn2_oracle.py and tests/box3d_oracle.py for the ops, plus the shared pieces of
the RPN fixtures: the cfg object, the seeded weights and the seeded input clouds.

Shared by tests/golden/make_golden_rpn.py (which records the imported reference), tests/test_rpn_host.py (which pins this file to
those recordings) and tests/test_hip_rpn.py (which checks the HIP path against both).
"""
import math

import numpy as np

from . import box3d_oracle as BO
from . import pn2_oracle as PO

F = np.float32


# ---- cfg: attribute- and []-indexable, built from the values-only JSON the golden maker dumps
class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def make_cfg(d):
    return Cfg({k: make_cfg(v) if isinstance(v, dict) else v for k, v in d.items()})


# ---- seeded weights: the reference's initial state is useless for testing (BN statistics 0 / 1, last reg layer at std 0.001)
def random_state(shapes, seed):
    """shapes: {state-dict name: shape} -> {name: array}, drawn in sorted-name order from RandomState(seed).  Conv weights are He-normal;
    BN running means ~N(0, 0.1), variances and gamma in [0.75, 1.25], beta ~N(0, 0.1); the last classification layer has std 0.2, the
    last regression layer std 0.05 with bias std 0.5."""
    rs = np.random.RandomState(seed)
    last = {}
    for name in shapes:
        head = name.split(".")[0]
        if head in ("rpn_cls_layer", "rpn_reg_layer"):
            last[head] = max(last.get(head, 0), int(name.split(".")[1]))
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        parts = name.split(".")
        is_last = parts[0] in last and int(parts[1]) == last[parts[0]]
        if name.endswith("num_batches_tracked"):
            v = np.zeros(shape, np.int64)
        elif name.endswith("running_mean") or name.endswith("bn.bn.bias"):
            v = rs.normal(0.0, 0.1, shape)
        elif name.endswith("running_var") or name.endswith("bn.bn.weight"):
            v = rs.uniform(0.75, 1.25, shape)
        elif name.endswith("conv.weight"):
            fan_in = int(np.prod(shape[1:]))
            std = math.sqrt(2.0 / fan_in)
            if is_last:
                std = 0.2 if parts[0] == "rpn_cls_layer" else 0.05
            v = rs.normal(0.0, std, shape)
        elif name.endswith("conv.bias"):
            v = rs.normal(0.0, 0.2 if parts[0] == "rpn_cls_layer" else 0.5, shape) if is_last else np.zeros(shape)
        else:
            raise KeyError(f"random_state: no rule for {name}")
        out[name] = v if v.dtype == np.int64 else v.astype(F)
    return out


# ---- seeded inputs, shaped like InstancePointCloud's output: centred, extent about 2 x 1.6 x 4.2 m
def make_cloud(kind, seed, n=768):
    """'surface': points on the two visible faces of a car-sized box, with depth noise; 'dup': 90 distinct surface points padded by
    repetition (back_project's draw with replacement); 'sparse': uniform in the volume, so that most radius-0.1 balls hold only their
    centre."""
    rs = np.random.RandomState(seed)
    if kind == "sparse":
        p = rs.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 0.8, 2.1])
    else:
        k = 90 if kind == "dup" else n
        side = rs.uniform(size=k) < 0.68
        u, v = rs.uniform(-1.0, 1.0, k), rs.uniform(-1.0, 1.0, k)
        x = np.where(side, -1.0, u)                       # the long side at x = -1, the rear at z = -2.1
        z = np.where(side, u * 2.1, -2.1)
        p = np.stack([x, v * 0.8, z], 1) + rs.normal(0.0, 0.03, (k, 3))
        if kind == "dup":
            p = p[np.concatenate([np.arange(k), rs.randint(0, k, n - k)])]
            p = p[rs.permutation(n)]
    p = p - p.mean(0, keepdims=True)
    return p.astype(F)


def make_batch(kinds, seed):
    return np.stack([make_cloud(k, seed + 17 * i) for i, k in enumerate(kinds)])


BATCHES = {"b2": (("surface", "dup"), 100), "b5": (("surface", "surface", "sparse", "dup", "surface"), 200)}


# ---- layers
def fold_bn(w, b, gamma, beta, mean, var, eps=1e-5):
    """W' = W g / sqrt(var + eps), b' = beta + (b - mean) g / sqrt(var + eps), in fp64."""
    w = np.asarray(w, np.float64).reshape(w.shape[0], -1)
    b = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return w * s[:, None], np.asarray(beta, np.float64) + (b - np.asarray(mean, np.float64)) * s


def folded_layer(sd, prefix, dtype=np.float64):
    """(W [Cout,Cin], b [Cout]) of the conv(+bn) unit at `prefix` (e.g. 'backbone_net.SA_modules.0.mlps.0.layer0'); dtype float32 rounds
    the fp64 fold once, as the product does."""
    w = sd[prefix + ".conv.weight"]
    b = sd.get(prefix + ".conv.bias")
    if prefix + ".bn.bn.weight" in sd:
        w, b = fold_bn(w, b, sd[prefix + ".bn.bn.weight"], sd[prefix + ".bn.bn.bias"], sd[prefix + ".bn.bn.running_mean"],
                       sd[prefix + ".bn.bn.running_var"])
    else:
        w = np.asarray(w, np.float64).reshape(w.shape[0], -1)
        b = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
    return w.astype(dtype), b.astype(dtype)


def mlp_prefixes(sd, prefix):
    n = 0
    while f"{prefix}.layer{n}.conv.weight" in sd:
        n += 1
    return [f"{prefix}.layer{i}" for i in range(n)]


def grouped_input(xyz, new_xyz, feats, idx, dtype=np.float64):
    """QueryAndGroup with use_xyz: (B, 3 + C, M, ns), the relative coordinates first, subtracted in `dtype`."""
    g = PO.group(np.ascontiguousarray(np.transpose(xyz, (0, 2, 1))), idx).astype(dtype) - np.transpose(new_xyz, (0, 2, 1))[..., None].astype(dtype)
    if feats is not None and feats.shape[1]:
        B, C = feats.shape[:2]
        gf = np.stack([feats[b][:, idx[b].reshape(-1)].reshape(C, *idx.shape[1:]) for b in range(B)])
        g = np.concatenate([g, gf.astype(dtype)], 1)
    return g


def sa_mlp_max(xyz, new_xyz, feats, idx, layers, dtype=np.float64):
    """max over the neighbourhood of the ReLU MLP of the grouped input -> (B, Cout, M)."""
    x = grouped_input(xyz, new_xyz, feats, idx, dtype)
    for w, b in layers:
        x = np.maximum(np.einsum("oc,bcms->boms", w.astype(dtype), x) + b.astype(dtype)[None, :, None, None], 0)
    return x.max(3)


def pointwise_mlp(in0, in1, w, b, relu, dtype=np.float64):
    x = in0.astype(dtype) if in1 is None else np.concatenate([in0.astype(dtype), in1.astype(dtype)], 1)
    y = np.einsum("oc,bcn->bon", w.astype(dtype), x) + b.astype(dtype)[None, :, None]
    return np.maximum(y, 0) if relu else y


def fp_interpolate(unknown, known, known_feats, dtype=np.float64):
    """PointnetFPModule's interpolation: fp32 three_nn, then weights and the weighted sum in `dtype`."""
    dist2, idx = PO.three_nn(unknown, known)
    dist = np.sqrt(dist2.astype(dtype))
    recip = 1.0 / (dist + dtype(1e-8))
    weight = recip / recip.sum(2, keepdims=True)
    out = []
    for b in range(known_feats.shape[0]):
        p = known_feats[b].astype(dtype)
        out.append(weight[b, :, 0] * p[:, idx[b, :, 0]] + weight[b, :, 1] * p[:, idx[b, :, 1]] + weight[b, :, 2] * p[:, idx[b, :, 2]])
    return np.stack(out)


def backbone(sd, cfg, pts, dtype=np.float64, prefix="backbone_net"):
    """Pointnet2MSG on (B,N,3) clouds -> xyz, features (B,C,N), levels {'sa': [...], 'fp': [...]} (fp[k] = FP_modules[k]'s output)."""
    sa_cfg = cfg.RPN.SA_CONFIG
    xyz = np.asarray(pts, F)[..., :3]
    l_xyz, l_feat, sa_out = [xyz], [None], []
    for k in range(len(sa_cfg.NPOINTS)):
        cur = l_xyz[-1]
        fidx = PO.fps(cur, sa_cfg.NPOINTS[k])
        new_xyz = np.stack([cur[b][fidx[b]] for b in range(cur.shape[0])])
        outs = []
        for s in range(len(sa_cfg.RADIUS[k])):
            idx = PO.ball_query(sa_cfg.RADIUS[k][s], sa_cfg.NSAMPLE[k][s], cur, new_xyz)
            layers = [folded_layer(sd, p) for p in mlp_prefixes(sd, f"{prefix}.SA_modules.{k}.mlps.{s}")]
            outs.append(sa_mlp_max(cur, new_xyz, l_feat[-1], idx, layers, dtype))
        l_xyz.append(new_xyz)
        l_feat.append(np.concatenate(outs, 1))
        sa_out.append(l_feat[-1])
    nfp = len(cfg.RPN.FP_MLPS)
    fp_out = [None] * nfp
    for i in range(-1, -(nfp + 1), -1):
        x = fp_interpolate(l_xyz[i - 1], l_xyz[i], l_feat[i], dtype)
        skip = l_feat[i - 1]
        for p in mlp_prefixes(sd, f"{prefix}.FP_modules.{nfp + i}.mlp"):
            w, b = folded_layer(sd, p)
            x = pointwise_mlp(x, skip, w, b, True, dtype)
            skip = None
        l_feat[i - 1] = x
        fp_out[nfp + i] = x
    return xyz, l_feat[0], {"sa": sa_out, "fp": fp_out}


def heads(sd, feats, dtype=np.float64):
    """-> rpn_cls (B,N,1), rpn_reg (B,N,R)"""
    out = []
    for head in ("rpn_cls_layer", "rpn_reg_layer"):
        ids = sorted({int(k.split(".")[1]) for k in sd if k.startswith(head + ".")})
        x = feats
        for j, i in enumerate(ids):
            w, b = folded_layer(sd, f"{head}.{i}")
            x = pointwise_mlp(x, None, w, b, j + 1 < len(ids), dtype)
        out.append(np.ascontiguousarray(np.transpose(x, (0, 2, 1))))
    return out


# ---- proposals (fp32, the reference's expression order)
def decode_constants(loc_scope, loc_bin_size, num_head_bin):
    apc = (2 * np.pi) / num_head_bin
    return dict(nb=int(loc_scope / loc_bin_size) * 2, bin=F(loc_bin_size), half_bin=F(loc_bin_size / 2), scope=F(loc_scope), apc=F(apc),
                half_apc=F(apc / 2), two_pi=F(2 * np.pi), pi=F(np.pi))


def torch_remainder(a, b):
    """torch.remainder for fp32: C fmod, then the divisor's sign."""
    m = np.fmod(a, b).astype(F)
    return np.where((m != 0) & ((b < 0) != (m < 0)), (m + b).astype(F), m).astype(F)


def decode(xyz, reg, mean_size, loc_scope, loc_bin_size, num_head_bin, xz_fine=False):
    """decode_bbox_target (get_y_by_bin False, get_ry_fine False) + `y += h / 2`: xyz (n,3), reg (n,R) -> boxes (n,7) fp32."""
    xyz, reg = np.asarray(xyz, F).reshape(-1, 3), np.asarray(reg, F)
    reg = reg.reshape(xyz.shape[0], -1)
    c = decode_constants(loc_scope, loc_bin_size, num_head_bin)
    nb, hb = c["nb"], int(num_head_bin)
    rows = np.arange(reg.shape[0])
    xb, zb = reg[:, :nb].argmax(1), reg[:, nb:2 * nb].argmax(1)          # numpy's argmax is the first maximum, as torch's
    pos_x = ((xb.astype(F) * c["bin"]).astype(F) + c["half_bin"]).astype(F) - c["scope"]
    pos_z = ((zb.astype(F) * c["bin"]).astype(F) + c["half_bin"]).astype(F) - c["scope"]
    off = 2 * nb
    if xz_fine:
        pos_x = pos_x + reg[rows, 2 * nb + xb] * c["bin"]
        pos_z = pos_z + reg[rows, 3 * nb + zb] * c["bin"]
        off = 4 * nb
    pos_y = xyz[:, 1] + reg[:, off]
    off += 1
    rbin = reg[:, off:off + hb].argmax(1)
    ry_res = reg[rows, off + hb + rbin] * c["half_apc"]
    ry = torch_remainder(((rbin.astype(F) * c["apc"]).astype(F) + ry_res).astype(F), c["two_pi"])
    ry = np.where(ry > c["pi"], (ry - c["two_pi"]).astype(F), ry)
    off += 2 * hb
    assert off + 3 == reg.shape[1]
    anchor = np.asarray(mean_size, np.float64).astype(F)
    hwl = (reg[:, off:off + 3] * anchor).astype(F) + anchor
    x, z = pos_x.astype(F) + xyz[:, 0], pos_z.astype(F) + xyz[:, 2]
    y = pos_y + hwl[:, 0] / F(2)
    return np.stack([x, y, z, hwl[:, 0], hwl[:, 1], hwl[:, 2], ry], 1).astype(F)


def argmax_margin(reg, loc_scope, loc_bin_size, num_head_bin):
    """The smallest gap between the best and the second-best bin of any of a row's three argmax groups."""
    reg = np.asarray(reg, F)
    nb, hb = int(loc_scope / loc_bin_size) * 2, int(num_head_bin)
    gaps = []
    for lo, hi in ((0, nb), (nb, 2 * nb), (2 * nb + 1, 2 * nb + 1 + hb)):
        s = np.sort(reg[:, lo:hi].astype(np.float64), 1)
        gaps.append((s[:, -1] - s[:, -2]).min())
    return float(min(gaps))


def nms_walk(boxes, thresh, max_keep=-1):
    """box3d_oracle.nms_sorted's walk that also reports the smallest |IoU - thresh| it compared -> (keep, margin)."""
    boxes = np.asarray(boxes, F).reshape(-1, 5)
    n = boxes.shape[0]
    g = BO._geom(boxes)
    removed = np.zeros(n, bool)
    keep, margin = [], np.inf
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if 0 < max_keep <= len(keep):
            break
        if i + 1 < n:
            j = np.arange(i + 1, n)
            iou = BO._iou_pairs(BO._take(g, np.full(j.size, i)), BO._take(g, j))
            margin = min(margin, float(np.abs(iou.astype(np.float64) - np.float64(F(thresh))).min()))
            removed[j] |= iou > F(thresh)
    return np.asarray(keep, np.int64), margin


def score_based_proposal(scores, boxes, pre, post, thresh):
    """One cloud: scores (N), boxes (N,7) -> rois (post,7), roi scores (post) zero padded, the walk's IoU margin."""
    scores, boxes = np.asarray(scores, F), np.asarray(boxes, F)
    order = np.argsort(-scores, kind="stable")[:pre]
    s, b = scores[order], boxes[order]
    keep, margin = nms_walk(BO.boxes3d_to_bev(b), thresh, post)
    keep = keep[:post]
    rois, rs = np.zeros((post, 7), F), np.zeros(post, F)
    rois[:len(keep)], rs[:len(keep)] = b[keep], s[keep]
    return rois, rs, margin


def proposal_layer(cfg, scores, reg, xyz):
    """ProposalLayer.forward: mode 'TRAIN' always, both top-N divided by the batch size -> rois (B,post,7), scores (B,post), margins (B)."""
    B = xyz.shape[0]
    rpn, mode = cfg.RPN, cfg["TRAIN"]
    pre, post = mode.RPN_PRE_NMS_TOP_N // B, mode.RPN_POST_NMS_TOP_N // B
    out = [score_based_proposal(scores[b], decode(xyz[b], reg[b], cfg.MEAN_SIZE[0], rpn.LOC_SCOPE, rpn.LOC_BIN_SIZE, rpn.NUM_HEAD_BIN,
                                                  rpn.LOC_XZ_FINE), pre, post, mode.RPN_NMS_THRESH) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.asarray([o[2] for o in out])

"""torch-CPU autograd restatement, generic in dtype, of what RCNNNet's training step computes: one pointwise layer, the SA chain (index
gather, subtract the centre, matmul, ReLU, max over the samples) and the whole step (xyz_up, merge_down, the SA levels, the heads, the
loss), plus the seeded inputs of the training fixtures.

FPS and ball query come from tests/pn2_oracle.py on the fp32 coordinates; the loss value and its gradients with respect to the
network's outputs come from tests/pointrcnn_loss_oracle.py (fp64, analytic) and are fed in with torch.autograd.backward.  Weights and
inputs are built from seeds as tests/rcnn_oracle.py does.  As in the product, the coordinates are constants of the graph: a gradient
reaches pts_input through the channels the shared MLPs read (all of them for xyz_up, the RPN features for merge_down), not through
the grouped coordinates of the SA levels.

Shared by tests/golden/make_golden_rcnn_train.py, tests/test_rcnn_train_host.py (which pins this file to the recording and to
tests/rcnn_oracle.py) and the GPU tests.
"""
import numpy as np
import torch

from . import pn2_oracle as PO
from . import pointrcnn_loss_oracle as LO
from . import rcnn_oracle as CO
from . import rpn_oracle as RO

F = np.float32
TRAIN_ROIS = (0, 15, 18, 21)            # of batch "b2": fewer than S points in 15 and 18 (10 points: its pooled cloud repeats them)
CLS_LABEL = (1.0, 0.0, -1.0, 1.0)
REG_VALID = (1, 0, 0, 1)


# ---- layers
def pointwise(in0, in1, w, b, relu):
    """in0 (B,C0,N), in1 (B,C1,N) or None, w [Cout,Cin], b [Cout] torch tensors of one dtype -> act(W . concat + b)"""
    x = in0 if in1 is None else torch.cat([in0, in1], 1)
    y = torch.einsum("oc,bcn->bon", w.reshape(w.shape[0], -1), x) + b[None, :, None]
    return torch.relu(y) if relu else y


def group(p, idx):
    """p (B,C,N) torch, idx (B,M,ns) integer array -> (B,C,M,ns); an index outside [0, N) reads 0, as pn2_oracle._take"""
    idx = torch.as_tensor(np.asarray(idx)).long()
    B, C, N = p.shape
    ok = (idx >= 0) & (idx < N)
    flat = torch.where(ok, idx, torch.zeros_like(idx)).reshape(B, 1, -1).expand(-1, C, -1)
    return torch.gather(p, 2, flat).reshape(B, C, *idx.shape[1:]) * ok[:, None].to(p.dtype)


def sa_chain(xyz, new_xyz, feats, idx, layers, dtype):
    """xyz (B,N,3), new_xyz (B,M,3) fp32 arrays (constants), feats (B,C,N) torch or None, idx (B,M,ns), layers [(w, b)] torch
    -> (B, Cout, M): max over the samples of the ReLU MLP of concat(xyz[idx] - new_xyz, feats[:, idx])"""
    np_dtype = F if dtype == torch.float32 else np.float64          # the subtraction in the run's own precision
    g = torch.from_numpy(RO.grouped_input(np.asarray(xyz, F), np.asarray(new_xyz, F), None, np.asarray(idx), np_dtype)).to(dtype)
    x = g if feats is None or feats.shape[1] == 0 else torch.cat([g, group(feats, idx)], 1)
    for w, b in layers:
        x = torch.relu(torch.einsum("oc,bcms->boms", w.reshape(w.shape[0], -1), x) + b[None, :, None, None])
    return x.max(3)[0]


# ---- the network
def params(sd, dtype):
    """state dict of arrays -> {name: leaf tensor requiring grad}"""
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_() for k, v in sd.items() if v.dtype != np.int64}


def _layers(P, prefix):
    out, n = [], 0
    while f"{prefix}.layer{n}.conv.weight" in P:
        out.append((P[f"{prefix}.layer{n}.conv.weight"], P[f"{prefix}.layer{n}.conv.bias"]))
        n += 1
    return out


def network(P, cfg, pts_input, dtype):
    """P: params(...), pts_input (R,S,3+E+C) torch (may require grad) -> levels dict, rcnn_cls (R,1), rcnn_reg (R,reg)"""
    rc = cfg.RCNN
    n_in = 3 + 1 + int(rc.USE_DEPTH)
    xyz0 = pts_input.detach()[..., :3].to(torch.float32).numpy().copy()
    levels = {}
    x = pts_input[..., :n_in].transpose(1, 2)
    for w, b in _layers(P, "xyz_up_layer"):
        x = pointwise(x, None, w, b, True)
    levels["xyz_up"] = x
    (w, b), = _layers(P, "merge_down_layer")
    f = pointwise(x, pts_input[..., n_in:].transpose(1, 2), w, b, True)
    levels["merge_down"] = f
    cur = xyz0
    for k, npoint in enumerate(rc.SA_CONFIG.NPOINTS):
        layers = _layers(P, f"SA_modules.{k}.mlps.0")
        nb = cur.shape[0]
        if npoint == -1:
            new_xyz = np.zeros((nb, 1, 3), F)
            idx = np.broadcast_to(np.arange(cur.shape[1], dtype=np.int32), (nb, 1, cur.shape[1])).copy()
        else:
            fidx = PO.fps(cur, npoint)
            new_xyz = np.stack([cur[i][fidx[i]] for i in range(nb)])
            idx = PO.ball_query(rc.SA_CONFIG.RADIUS[k], rc.SA_CONFIG.NSAMPLE[k], cur, new_xyz)
        f = sa_chain(cur, new_xyz, f, idx, layers, dtype)
        levels[f"sa{k}"] = f
        cur = new_xyz
    x0 = f[:, :, 0].t().unsqueeze(0)                     # (1,C,R)
    outs = []
    for head in ("cls_layer", "reg_layer"):
        ids = sorted({int(k.split(".")[1]) for k in P if k.startswith(head + ".")})
        x = x0
        for j, i in enumerate(ids):
            x = pointwise(x, None, P[f"{head}.{i}.conv.weight"], P[f"{head}.{i}.conv.bias"], j + 1 < len(ids))
        outs.append(x[0].t())
    return levels, outs[0], outs[1]


def loss_and_output_grads(cfg, cls, reg, prop):
    """-> loss (fp64 float), d loss / d rcnn_cls (R,1), d loss / d rcnn_reg (R,reg) in fp64, from tests/pointrcnn_loss_oracle.py"""
    inp = {"rcnn_cls": np.asarray(cls, np.float64), "rcnn_reg": np.asarray(reg, np.float64), "cls_label": np.asarray(prop["cls_label"]),
           "reg_valid_mask": np.asarray(prop["reg_valid_mask"]), "gt_of_rois": np.asarray(prop["gt_boxes3d_ct"], np.float64),
           "roi_boxes3d": np.asarray(prop["roi_boxes3d"], np.float64).reshape(-1, 7)}
    out, gc, gr = LO.rcnn_loss(cfg, inp)
    return float(out["rcnn_loss"]), gc.reshape(-1, 1), gr


def train_step(sd, cfg, prop, dtype=torch.float64):
    """One training step of RCNNNet on the sampled ROIs `prop` (arrays: pts_input, roi_boxes3d, cls_label, reg_valid_mask, gt_boxes3d_ct)
    -> loss, {parameter name: gradient (fp64 array)}, d loss / d pts_input (fp64 array), (rcnn_cls, rcnn_reg) arrays"""
    P = params(sd, dtype)
    pin = torch.from_numpy(np.asarray(prop["pts_input"])).to(dtype).requires_grad_()
    _, cls, reg = network(P, cfg, pin, dtype)
    loss, gc, gr = loss_and_output_grads(cfg, cls.detach().double().numpy(), reg.detach().double().numpy(), prop)
    torch.autograd.backward([cls, reg], [torch.from_numpy(gc).to(dtype), torch.from_numpy(gr).to(dtype)])
    grads = {k: (v.grad.double().numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items()}
    return loss, grads, pin.grad.double().numpy(), (cls.detach().numpy(), reg.detach().numpy())


# ---- seeded fixtures
def train_cfg(cfg_json):
    """the car config of the RCNN fixtures with ROI_SAMPLE_JIT off and the focal classification loss: the reference's BinaryCrossEntropy
    branch cannot take the ignore label -1 (F.binary_cross_entropy refuses a target outside [0, 1]), which the fixture must contain"""
    import copy
    c = copy.deepcopy(cfg_json)
    c["RCNN"]["ROI_SAMPLE_JIT"] = False
    c["RCNN"]["LOSS_CLS"] = "SigmoidFocalLoss"
    return RO.make_cfg(c)


def make_train_inputs(cfg, bump, gt_seed):
    """R = 4 sampled ROIs from seeds: pts_input (R,S,3+E+C) fp32 (rcnn_oracle's pooled, canonical tensor of four ROIs of batch "b2"),
    roi_boxes3d (R,7), cls_label (R) with 1, 0 and -1, reg_valid_mask (R) of both kinds, gt_boxes3d_ct (R,7) in the canonical frame."""
    rc = cfg.RCNN
    inp = CO.make_inputs("b2", bump)
    pool = CO.pool_canonical(inp, rc.POOL_EXTRA_WIDTH, rc.NUM_POINTS, rc.USE_DEPTH, F)
    sel = np.array(TRAIN_ROIS)
    assert (pool["empty"][sel] == 0).all()
    rs = np.random.RandomState(gt_seed)
    R = len(sel)
    gt = np.concatenate([rs.uniform(-1.4, 1.4, (R, 1)), rs.uniform(-0.4, 0.4, (R, 1)), rs.uniform(-1.4, 1.4, (R, 1)),
                         np.array(LO.MEAN_SIZE) * rs.uniform(0.85, 1.15, (R, 3)), rs.uniform(-np.pi, np.pi, (R, 1))], 1).astype(F)
    return {"pts_input": np.ascontiguousarray(CO.pts_input_of(pool)[sel]).astype(F), "roi_boxes3d": inp["roi_boxes3d"].reshape(-1, 7)[sel].copy(),
            "cls_label": np.array(CLS_LABEL, F), "reg_valid_mask": np.array(REG_VALID, np.int64), "gt_boxes3d_ct": gt}

"""Plain fp64 references (torch, CPU) of the train step's reductions: train-mode BatchNorm forward / backward on [N,C,D,H,W] tensors,
the disparity loss sums and their gradient, and a mirror of the launch arithmetic of the two fixed-order BatchNorm reductions.
Shared by tests/test_bn_oracle.py (pins this file to torch autograd and to oracle.psmnet_oracle) and tests/test_hip_train_reductions.py
(holds the HIP kernels to it)."""
import torch

F64 = torch.float64
_S = (1, -1, 1, 1, 1)
_RED = (0, 2, 3, 4)


# ------------------------------------------------------------------------------------------------ BatchNorm
def stats(x):
    """Per-channel mean and BIASED variance of x [N,C,D,H,W] over (N, D, H, W)."""
    x = x.to(F64)
    mean = x.mean(_RED)
    var = ((x - mean.view(_S)) ** 2).mean(_RED)
    return mean, var


def apply(x, mean, invstd, gamma, beta, res=None, relu=False):
    """y = act((x - mean) * invstd * gamma + beta (+ res)) with the statistics GIVEN (upcast as they are)."""
    y = (x.to(F64) - mean.to(F64).view(_S)) * invstd.to(F64).view(_S) * gamma.to(F64).view(_S) + beta.to(F64).view(_S)
    if res is not None:
        y = y + res.to(F64)
    return torch.relu(y) if relu else y


def finalize(mean, m2, M, eps, momentum, running_mean=None, running_var=None):
    """invstd = 1/sqrt(m2/M + eps) and nn.BatchNorm's running update (momentum, UNBIASED batch variance m2/(M-1); M >= 2, as
    nn.BatchNorm demands in train mode).  Returns (invstd, running_mean', running_var'); the last two None without running buffers."""
    mean, m2 = mean.to(F64), m2.to(F64)
    invstd = 1.0 / torch.sqrt(m2 / M + eps)
    if running_mean is None:
        return invstd, None, None
    rm = (1.0 - momentum) * running_mean.to(F64) + momentum * mean
    rv = (1.0 - momentum) * running_var.to(F64) + momentum * m2 / (M - 1)
    return invstd, rm, rv


def bwd(dy, y, raw, mean, invstd, gamma, relu, sums=None):
    """BatchNorm backward with the ReLU mask fused: dz = dy * [y > 0] (relu) else dy;  xhat = (raw - mean) * invstd with the fp32
    statistics handed in, upcast (the reduction is under test, not the statistics).  `sums` = (sum_dz, sum_dz_xhat) replaces the
    reference sums inside draw (to hold the apply kernel to ITS inputs).  dres is the gradient of a residual added before the ReLU."""
    dy, raw = dy.to(F64), raw.to(F64)
    dz = dy * (y.to(F64) > 0).to(F64) if relu else dy
    xhat = (raw - mean.to(F64).view(_S)) * invstd.to(F64).view(_S)
    t2 = dz * xhat
    out = dict(sum_dz=dz.sum(_RED), sum_dz_xhat=t2.sum(_RED), sum_abs_dz=dz.abs().sum(_RED), sum_abs_dz_xhat=t2.abs().sum(_RED))
    s1, s2 = (out["sum_dz"], out["sum_dz_xhat"]) if sums is None else (sums[0].to(F64), sums[1].to(F64))
    M = dy.shape[0] * dy.shape[2] * dy.shape[3] * dy.shape[4]
    out["draw"] = (gamma.to(F64) * invstd.to(F64)).view(_S) * (dz - s1.view(_S) / M - xhat * s2.view(_S) / M)
    out["dres"] = dz
    return out


# ------------------------------------------------------------------------------------------------ loss
def _smooth_l1(d):
    d = d.abs()
    return torch.where(d < 1.0, 0.5 * d * d, d - 0.5)


def loss_sums(p1, p2, p3, tgt, mask):
    """[sum m*sl1(p1-t), sum m*sl1(p2-t), sum m*sl1(p3-t), sum m, sum m*|p1-t|]; a head given as None contributes 0 (eval form)."""
    m, t = (mask != 0).to(F64), tgt.to(F64)
    out = torch.zeros(5, dtype=F64)
    for k, p in enumerate((p1, p2, p3)):
        if p is not None:
            out[k] = (m * _smooth_l1(p.to(F64) - t)).sum()
    out[3] = m.sum()
    out[4] = (m * (p1.to(F64) - t).abs()).sum()
    return out


def loss_grad(pred, tgt, mask, weight, gscale):
    """d(weight * sum m*sl1(pred - tgt) / sum m)/d pred * gscale; the sum is NOT divided when the mask is empty (and is zero anyway)."""
    m = (mask != 0).to(F64)
    msum = m.sum()
    k = weight * gscale / (msum if msum != 0 else 1.0)
    return k * m * (pred.to(F64) - tgt.to(F64)).clamp(-1.0, 1.0)


# ------------------------------------------------------------------------------------------------ launch arithmetic
THREADS = 256


def launch_plan(N, D, H, W, voxels_per_block=512, cap=512):
    """Grid of the two fixed-order reductions over a [N, *, D, H, W] tensor and the rows every block walks.  Mirrors
      train_ops.hip  drc_bn_stats_blocked: chunks = ceil(nvox / ((kThreads/4)*8)), >= 1, <= DRC_BN_MAX_CHUNKS, <= rows   (lines 221-225)
      bwd_ops.hip    drc_bn_bwd_reduce:    chunks = ceil(nvox / (64*8)), <= DRC_BN_MAX_CHUNKS, <= rows                  (lines 510-513)
      blocked_walk.h walk_rows / rows_of_block: tpr = 4W, rpb = 1 if tpr >= THREADS else THREADS // tpr, chunk = ceil(rows / grid)
                     rounded up to a multiple of rpb, block b walks rows [b*chunk, min((b+1)*chunk, rows))               (lines 20-26, 62-69)
    Returns dict(blocks, rpb, chunk, rows, ranges=[(r0, r1)] * blocks) with empty blocks as (rows, rows)."""
    rows = N * D * H
    nvox = rows * W
    blocks = max(1, -(-nvox // voxels_per_block))
    blocks = min(blocks, cap, max(rows, 1))
    tpr = 4 * W
    rpb = 1 if tpr >= THREADS else THREADS // tpr
    chunk = -(-rows // blocks)
    chunk = -(-chunk // rpb) * rpb
    ranges = [(min(b * chunk, rows), min((b + 1) * chunk, rows)) for b in range(blocks)]
    return dict(blocks=blocks, rpb=rpb, chunk=chunk, rows=rows, ranges=ranges)


# Geometry cases of tests/test_hip_train_reductions.py: name -> ((N, C, D, H, W), (pd, ph, pw), expected grid).  `grid` = (blocks,
# blocks without rows, rows of the last block that has any); "rpb" where the case is about it.  3D tensors carry halo 1, the 2D layout
# (D = 1, pd = 0) the halo 2 of the dilated 2D convs.
CASES = {
    "a": ((1, 16, 1, 3, 5), (1, 1, 1), dict(blocks=1, empty=0, last=3, rpb=12)),            # rpb 12 > 3 rows
    "b": ((4, 40, 5, 13, 3), (1, 1, 1), dict(blocks=2, empty=0, last=113, rpb=21)),         # ragged second block, 8 padded channels
    "c": ((2, 32, 4, 32, 32), (1, 1, 1), dict(blocks=16, empty=0, last=16)),                # one full ticket group
    "d": ((2, 32, 4, 32, 33), (1, 1, 1), dict(blocks=17, empty=1, last=16)),                # a second group of one, and that one empty
    "e": ((1, 16, 3, 50, 110), (1, 1, 1), dict(blocks=33, empty=3, last=5, rpb=1)),         # W > 64: two x per thread
    "f": ((2, 16, 1, 47, 64), (0, 2, 2), dict(blocks=12, empty=0, last=6, rpb=1)),          # 2D layout, W*4 == 256
    "g": ((2, 16, 1, 47, 65), (0, 2, 2), dict(blocks=12, empty=0, last=6, rpb=1)),          # 2D layout, W*4 == 260
    "h": ((2, 16, 4, 128, 128), (1, 1, 1), dict(blocks=256, empty=0, last=4)),
    "i": ((1, 16, 4, 128, 257), (1, 1, 1), dict(blocks=257, empty=1, last=2)),
    "j": ((4, 16, 4, 128, 128), (1, 1, 1), dict(blocks=512, empty=0, last=4)),              # the cap, 32 full groups
    "k": ((2, 32, 12, 112, 112), (1, 1, 1), dict(blocks=512, empty=64, last=6)),            # 588 capped to 512
    "l": ((1, 16, 1, 2, 700), (1, 1, 1), dict(blocks=2, empty=0, last=1)),                  # capped by the row count
    "m": ((1, 16, 1, 93, 311), (1, 1, 1), dict(blocks=57, empty=10, last=1)),               # the quarter-resolution KITTI row
    "n": ((2, 40, 3, 9, 20), (1, 1, 1), dict(blocks=3, empty=0, last=18, rpb=3)),           # run as channel blocks [2, 5) of 7
}


def grid_of(plan):
    """(blocks, blocks without rows, rows of the last block that has any) of a launch_plan."""
    full = [r for r in plan["ranges"] if r[1] > r[0]]
    return plan["blocks"], plan["blocks"] - len(full), full[-1][1] - full[-1][0]


def is_ragged(plan):
    """True where the Chan merge has chunks of different weight: an empty block, or a last block shorter than the others."""
    sizes = {r1 - r0 for r0, r1 in plan["ranges"]}
    return len(sizes) > 1


def chunk_stats(x, plan):
    """(count, mean, M2) per channel of every block's rows, fp64: [blocks] , [blocks, C], [blocks, C]; empty blocks are (0, 0, 0)."""
    N, C, D, H, W = x.shape
    rowsv = x.to(F64).permute(1, 0, 2, 3, 4).reshape(C, N * D * H, W)
    ns, means, m2s = [], [], []
    for r0, r1 in plan["ranges"]:
        if r1 > r0:
            blk = rowsv[:, r0:r1].reshape(C, -1)
            mu = blk.mean(1)
            ns.append(float(blk.shape[1])); means.append(mu); m2s.append(((blk - mu[:, None]) ** 2).sum(1))
        else:
            ns.append(0.0); means.append(torch.zeros(C, dtype=F64)); m2s.append(torch.zeros(C, dtype=F64))
    return torch.tensor(ns, dtype=F64), torch.stack(means), torch.stack(m2s)


def merge_chunks(ns, means, m2s):
    """Exact (fp64) combination of chunk statistics with the weights `ns`: (mean, M2) per channel."""
    tot = ns.sum()
    mean = (ns[:, None] * means).sum(0) / tot
    m2 = m2s.sum(0) + (ns[:, None] * (means - mean[None]) ** 2).sum(0)
    return mean, m2


# ------------------------------------------------------------------------------------------------ inputs
def channel_params(C):
    """(mu_c, sigma_c, A_c): offsets in [-2, 2], widths in [0.5, 1.7], a trend over the rows of +-4 sigma alternating by channel."""
    c = torch.arange(C, dtype=F64)
    mu = ((c * 7) % 11 - 5) * 0.4
    sigma = 0.5 + 0.1 * (c % 13)
    A = 4.0 * sigma * torch.where(c % 2 == 0, 1.0, -1.0).to(F64)
    return mu, sigma, A


def trend_input(key, shape, trend=True, mu=None, sigma=None):
    """fp32 x = mu_c + sigma_c*u + A_c*(r/(rows-1) - 0.5) + 0.5*sigma_c*(xcol/W): u = synth.hash_uniform in [-1, 1), r the flattened
    (n, d, y) row.  Every row block has its own mean, so a chunk merged with a wrong weight, dropped or counted twice moves the
    statistics by far more than rounding (iid data cannot show it).  trend=False with scalar mu, sigma: x = mu + sigma*u."""
    from disprcnn_amd.utils import synth
    N, C, D, H, W = shape
    u = synth.hash_uniform(key, (N, C, D, H, W)).to(F64)
    if not trend:
        return (mu + sigma * u).float()
    mu_c, sg, A = channel_params(C)
    rows = N * D * H
    r = torch.arange(rows, dtype=F64).view(N, 1, D, H, 1) / max(rows - 1, 1) - 0.5
    xcol = torch.arange(W, dtype=F64).view(1, 1, 1, 1, W) / W
    x = mu_c.view(_S) + sg.view(_S) * u
    x += A.view(_S) * r
    x += 0.5 * sg.view(_S) * xcol
    return x.float()


def stat_mutants(x, plan):
    """What two wrong merges would report for x, in fp64: {name: (mean, biased var)}.
      equal_weights: every block of the grid -- an empty one as (mean 0, M2 0) -- merged with the weight of a full chunk
      drop_last:     the last block that has rows left out
    A test of the statistics is only as strong as the distance of these from the truth."""
    ns, means, m2s = chunk_stats(x, plan)
    M = float(ns.sum())
    W = x.shape[4]
    out = {}
    mean, m2 = merge_chunks(torch.full_like(ns, float(plan["chunk"] * W)), means, m2s)
    out["equal_weights"] = (mean, m2 / M)
    keep = torch.ones_like(ns, dtype=torch.bool)
    keep[int(torch.nonzero(ns > 0)[-1])] = False
    mean, m2 = merge_chunks(ns[keep], means[keep], m2s[keep])
    out["drop_last"] = (mean, m2 / M)
    return out

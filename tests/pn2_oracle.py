"""NumPy restatement of the reference's PointNet++ ops (pointnet2_lib/pointnet2/src/*_gpu.cu), fp32 arithmetic in the kernels' order.
Shared by tests/test_points_host.py (hand-computed cases) and tests/test_hip_points.py (vs the HIP kernels)."""
import math

import numpy as np


def opt_n_threads(n):
    return max(min(1 << int(math.log(float(n)) / math.log(2.0)), 1024), 1)


def fps(xyz, m, return_temp=False):
    """sampling_gpu.cu: per-slot running best (strict >), then the shared-memory tree (ties keep the lower slot of each pair).
    return_temp: also return the final `temp` [B,N] the kernel leaves behind, the running minimum distance (1e10 where m <= 1)."""
    xyz = np.asarray(xyz, np.float32)
    B, N, _ = xyz.shape
    bs = opt_n_threads(N)
    rows = -(-N // bs)
    out = np.zeros((B, m), np.int32)
    temps = np.full((B, N), 1e10, np.float32)
    for b in range(B):
        p = xyz[b]
        temp = np.full(N, 1e10, np.float32)
        old = 0
        for j in range(1, m):
            dx, dy, dz = p[:, 0] - p[old, 0], p[:, 1] - p[old, 1], p[:, 2] - p[old, 2]
            d = dx * dx + dy * dy + dz * dz
            temp = np.minimum(d, temp)
            D = np.full(rows * bs, -1.0, np.float32)
            D[:N] = temp
            D = D.reshape(rows, bs)
            vals = D.max(0)
            idx = ((D == vals[None]).argmax(0) * bs + np.arange(bs)).astype(np.int64)
            s = bs // 2
            while s >= 1:
                take = vals[s:2 * s] > vals[:s]
                idx[:s] = np.where(take, idx[s:2 * s], idx[:s])
                vals[:s] = np.maximum(vals[:s], vals[s:2 * s])
                s //= 2
            old = int(idx[0])
            out[b, j] = old
        temps[b] = temp
    return (out, temps) if return_temp else out


def ball_query(radius, nsample, xyz, new_xyz):
    xyz, new_xyz = np.asarray(xyz, np.float32), np.asarray(new_xyz, np.float32)
    B, M = new_xyz.shape[:2]
    r2 = np.float32(radius) * np.float32(radius)
    out = np.zeros((B, M, nsample), np.int32)
    for b in range(B):
        for q0 in range(0, M, 256):
            c = new_xyz[b, q0:q0 + 256]
            dx = c[:, None, 0] - xyz[b][None, :, 0]
            dy = c[:, None, 1] - xyz[b][None, :, 1]
            dz = c[:, None, 2] - xyz[b][None, :, 2]
            hit = (dx * dx + dy * dy + dz * dz) < r2
            for qi in range(hit.shape[0]):
                k = np.flatnonzero(hit[qi])[:nsample]
                if len(k):
                    out[b, q0 + qi, :] = k[0]
                    out[b, q0 + qi, :len(k)] = k
    return out


def three_nn(unknown, known):
    unknown, known = np.asarray(unknown, np.float32), np.asarray(known, np.float32)
    B, N = unknown.shape[:2]
    m = known.shape[1]
    dist2 = np.full((B, N, 3), np.inf, np.float32)          # (float)1e40
    idx = np.zeros((B, N, 3), np.int32)
    for b in range(B):
        for n0 in range(0, N, 1024):
            u = unknown[b, n0:n0 + 1024]
            dx = u[:, None, 0] - known[b][None, :, 0]
            dy = u[:, None, 1] - known[b][None, :, 1]
            dz = u[:, None, 2] - known[b][None, :, 2]
            d = dx * dx + dy * dy + dz * dz
            order = np.argsort(d, axis=1, kind="stable")[:, :3]       # strict `<` insertion == stable order, first index first
            k = order.shape[1]
            idx[b, n0:n0 + len(u), :k] = order
            dist2[b, n0:n0 + len(u), :k] = np.take_along_axis(d, order, 1)
    return dist2, idx


def _take(p, idx):
    """p[:, idx] with the API's rule for an index outside [0, N): it reads 0 (pointnet2.hip; the reference has no check)."""
    ok = (idx >= 0) & (idx < p.shape[1])
    return np.where(ok, p[:, np.where(ok, idx, 0)], np.float32(0))


def gather(points, idx):
    points, idx = np.asarray(points, np.float32), np.asarray(idx)
    return np.stack([_take(points[b], idx[b]) for b in range(points.shape[0])])


def group(points, idx):
    return gather(points, np.asarray(idx).reshape(idx.shape[0], -1)).reshape(points.shape[0], points.shape[1], *idx.shape[1:])


def three_interpolate(points, idx, weight):
    points, idx, weight = np.asarray(points, np.float32), np.asarray(idx), np.asarray(weight, np.float32)
    out = []
    for b in range(points.shape[0]):
        p = points[b]
        out.append(weight[b, :, 0] * _take(p, idx[b, :, 0]) + weight[b, :, 1] * _take(p, idx[b, :, 1]) + weight[b, :, 2] * _take(p, idx[b, :, 2]))
    return np.stack(out)


def scatter_grad(grad_out, idx, n, weight=None):
    """float64 reference of the three backward ops: grad_out [B,C,K], idx [B,E] (E = K, or 3K with weight [B,E]).
    An index outside [0, n) contributes nothing."""
    grad_out, idx = np.asarray(grad_out, np.float64), np.asarray(idx).reshape(grad_out.shape[0], -1)
    B, C, K = grad_out.shape
    per = idx.shape[1] // K
    out = np.zeros((B, C, n), np.float64)
    for b in range(B):
        cols = np.arange(idx.shape[1]) // per
        v = grad_out[b][:, cols]
        if weight is not None:
            v = v * np.asarray(weight, np.float64).reshape(B, -1)[b][None]
        ok = (idx[b] >= 0) & (idx[b] < n)
        np.add.at(out[b].T, idx[b][ok], v.T[ok])
    return out

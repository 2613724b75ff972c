"""tests/det2d_loss_oracle.py, the comparator of the 2D stage's training kernels, held to torch's own functions and to statistics that
need no measured number; and the plain-torch pieces of the feature (BoxCoder.encode 6-from-6, layers.smooth_l1_loss).  No GPU.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import det2d_loss_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _labels(rng, n, n_pos, n_neg):
    lab = np.full(n, -1.0, np.float32)
    perm = rng.permutation(n)
    lab[perm[:n_pos]] = 1
    lab[perm[n_pos:n_pos + n_neg]] = 0
    return lab


def test_oracle_sampler_counts_and_classes():
    rng = np.random.default_rng(0)
    for n, n_pos, n_neg, batch, frac in ((300, 40, 200, 64, 0.5), (300, 10, 200, 64, 0.5), (300, 40, 12, 64, 0.25), (20, 5, 10, 256, 0.5),
                                         (50, 0, 0, 16, 0.5), (50, 0, 30, 16, 0.5)):
        lab = _labels(rng, n, n_pos, n_neg)
        pm, nm = O.sample(lab, rng.random(n, dtype=np.float32), batch, frac)
        num_pos = min(n_pos, int(batch * frac))
        assert pm.sum() == num_pos and nm.sum() == min(n_neg, batch - num_pos)
        assert (lab[pm == 1] >= 1).all() and (lab[nm == 1] == 0).all() and not (pm & nm).any()


def test_oracle_sampler_is_uniform():
    """Each candidate of a class is taken with probability k / n: over T draw tensors its count is binomial(T, k / n), held to 5 standard
    deviations."""
    rng = np.random.default_rng(1)
    n, n_pos, n_neg, batch, frac, T = 40, 12, 20, 16, 0.5, 2000
    lab = _labels(rng, n, n_pos, n_neg)
    hits_p, hits_n = np.zeros(n), np.zeros(n)
    for _ in range(T):
        pm, nm = O.sample(lab, rng.random(n, dtype=np.float32), batch, frac)
        hits_p += pm
        hits_n += nm
    for hits, members, k in ((hits_p, lab >= 1, 8), (hits_n, lab == 0, 8)):
        p = k / members.sum()
        sd = np.sqrt(p * (1 - p) / T)
        assert (np.abs(hits[members] / T - p) <= 5 * sd).all(), (hits[members] / T, p, sd)
        assert not hits[~members].any()


def test_oracle_sampler_breaks_equal_draws_by_index():
    lab = np.array([1, 1, 0, 1, 0, 1, 0, 0, 1], np.float32)
    pm, nm = O.sample(lab, np.zeros(9, np.float32), 4, 0.5)
    assert pm.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0] and nm.tolist() == [0, 0, 1, 0, 1, 0, 0, 0, 0]


def _srpn_case(rng, N, A, shapes):
    z = [rng.standard_normal((N, 2 * A, h, w)).astype(np.float32) * 3 for h, w in shapes]
    b = [rng.standard_normal((N, 6 * A, h, w)).astype(np.float32) * 0.3 for h, w in shapes]
    total = sum(h * w * A for h, w in shapes)
    lab = np.concatenate([_labels(rng, total, 30, total // 2) for _ in range(N)])
    reg = rng.standard_normal((N * total, 6)).astype(np.float32) * 0.3
    pm = np.concatenate([O.sample(lab[n * total:(n + 1) * total], rng.random(total, dtype=np.float32), 32, 0.5)[0] for n in range(N)])
    nm = ((lab == 0) & (rng.random(N * total) < 0.2)).astype(np.uint8)
    return z, b, lab, reg, pm, nm, total


def test_oracle_srpn_loss_is_the_pairing_spelled_out():
    """The literal view / softmax / permute composition against loops over anchors: raw channel c is paired with c + A, anchor a reads
    probabilities 2a and 2a + 1.  Then F.cross_entropy and smooth_l1_loss on the compacted rows, to 1e-12 in fp64."""
    from disprcnn_amd.layers import smooth_l1_loss
    rng = np.random.default_rng(2)
    for A, shapes in ((1, [(3, 4), (2, 2)]), (3, [(3, 5), (2, 3), (1, 1)])):
        N = 2
        z, b, lab, reg, pm, nm, total = _srpn_case(rng, N, A, shapes)
        lo, lb, gz, gb = O.srpn_loss(z, b, lab, reg, pm, nm)
        rows_obj, rows_lab, rows_box, rows_reg = [], [], [], []
        for n in range(N):
            off = 0
            for zl, bl in zip(z, b):
                H, W = zl.shape[2:]
                zz = torch.from_numpy(zl[n]).double()
                p = torch.empty_like(zz)
                for c in range(A):
                    e0, e1 = zz[c].exp(), zz[c + A].exp()
                    p[c], p[c + A] = e0 / (e0 + e1), e1 / (e0 + e1)
                for y in range(H):
                    for x in range(W):
                        for a in range(A):
                            i = n * total + off + (y * W + x) * A + a
                            if pm[i] or nm[i]:
                                rows_obj.append(torch.stack([p[2 * a, y, x], p[2 * a + 1, y, x]]))
                                rows_lab.append(int(lab[i]))
                            if pm[i]:
                                rows_box.append(torch.from_numpy(bl[n, 6 * a:6 * a + 6, y, x]).double())
                                rows_reg.append(torch.from_numpy(reg[i]).double())
                off += H * W * A
        want_obj = F.cross_entropy(torch.stack(rows_obj), torch.tensor(rows_lab))
        want_box = smooth_l1_loss(torch.stack(rows_box), torch.stack(rows_reg), beta=1.0 / 9, size_average=False) / len(rows_lab)
        assert abs(lo - float(want_obj)) <= 1e-12 and abs(lb - float(want_box)) <= 1e-12
        assert all(np.isfinite(g).all() for g in gz + gb)


def test_oracle_fastrcnn_loss_is_torchs():
    from disprcnn_amd.layers import smooth_l1_loss
    rng = np.random.default_rng(3)
    R, C = 37, 4
    x, b = rng.standard_normal((R, C)).astype(np.float32) * 2, rng.standard_normal((R, 6 * C)).astype(np.float32)
    lab, reg = rng.integers(0, C, R), rng.standard_normal((R, 6)).astype(np.float32)
    lc, lb, gx, gb = O.fastrcnn_loss(x, b, lab, reg)
    xt, bt = torch.from_numpy(x).double(), torch.from_numpy(b).double()
    assert abs(lc - float(F.cross_entropy(xt, torch.from_numpy(lab)))) <= 1e-12
    rows = [r for r in range(R) if lab[r] > 0]
    picked = torch.stack([bt[r, 6 * lab[r]:6 * lab[r] + 6] for r in rows])
    want = smooth_l1_loss(picked, torch.from_numpy(reg[rows]).double(), beta=1, size_average=False) / R
    assert abs(lb - float(want)) <= 1e-12
    assert not gb[lab == 0].any() and np.abs(gx.sum(axis=1)).max() <= 1e-15


def test_smooth_l1_loss_matches_torch_at_beta_one():
    from disprcnn_amd.layers import smooth_l1_loss
    a, b = torch.linspace(-3, 3, 41, dtype=torch.float64), torch.zeros(41, dtype=torch.float64)
    assert abs(float(smooth_l1_loss(a, b, beta=1.0)) - float(F.smooth_l1_loss(a, b))) <= 1e-15
    assert abs(float(smooth_l1_loss(a, b, beta=1.0, size_average=False)) - float(F.smooth_l1_loss(a, b, reduction="sum"))) <= 1e-13


def _decode6(codes, boxes6, weights):
    """decode_x1y1x2y2x1px2p_fromboxes6 for one class, fp64"""
    wx, wy, ww, wh = weights
    w, h, wp = boxes6[:, 2] - boxes6[:, 0] + 1, boxes6[:, 3] - boxes6[:, 1] + 1, boxes6[:, 5] - boxes6[:, 4] + 1
    cx, cy, cxp = boxes6[:, 0] + 0.5 * w, boxes6[:, 1] + 0.5 * h, boxes6[:, 4] + 0.5 * wp
    pcx, pcy, pcxp = codes[:, 0] / wx * w + cx, codes[:, 1] / wy * h + cy, codes[:, 4] / wx * wp + cxp
    pw, ph, pwp = np.exp(codes[:, 2] / ww) * w, np.exp(codes[:, 3] / wh) * h, np.exp(codes[:, 5] / ww) * wp
    return np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1, pcxp - 0.5 * pwp, pcxp + 0.5 * pwp - 1], axis=1)


def test_box_coder_encodes_six_from_six():
    from disprcnn_amd.modeling.box_coder import BoxCoder
    rng = np.random.default_rng(4)
    weights = (10.0, 10.0, 5.0, 5.0)
    R = 50
    xy, wh = rng.uniform(0, 200, (R, 3)), rng.uniform(4, 90, (R, 3))
    boxes6 = np.stack([xy[:, 0], xy[:, 1], xy[:, 0] + wh[:, 0], xy[:, 1] + wh[:, 1], xy[:, 2], xy[:, 2] + wh[:, 2]], axis=1)
    codes = rng.uniform(-1, 1, (R, 6))
    decoded = _decode6(codes, boxes6, weights)
    got = BoxCoder(weights).encode(torch.from_numpy(decoded), torch.from_numpy(boxes6)).numpy()
    assert got.shape == (R, 6) and np.abs(got - codes).max() <= 1e-9
    f32 = BoxCoder(weights).encode(torch.from_numpy(decoded).float(), torch.from_numpy(boxes6).float()).numpy()
    want = O.encode(decoded.astype(np.float32), boxes6.astype(np.float32), weights)
    assert np.abs(f32 - want).max() <= 4e-6 * np.abs(want).max()
    # the 4-coordinate proposal form is unchanged: the right view coded against the same box
    four = BoxCoder(weights).encode(torch.from_numpy(decoded), torch.from_numpy(boxes6[:, :4])).numpy()
    assert np.array_equal(four[:, :4], got[:, :4]) and not np.allclose(four[:, 4:], got[:, 4:])


def test_oracle_matcher_is_the_projects_matcher():
    from disprcnn_amd.modeling.matcher import Matcher
    rng = np.random.default_rng(5)
    for G, R in ((1, 30), (5, 200)):
        gt = np.concatenate([rng.uniform(0, 60, (G, 2)), rng.uniform(70, 120, (G, 2))], axis=1).astype(np.float32)
        c0 = rng.uniform(0, 100, (R, 2))
        cand = np.concatenate([c0, c0 + rng.uniform(1, 80, (R, 2))], axis=1).astype(np.float32)
        cand[0] = gt[0]
        iou = O.iou_matrix(gt, cand)
        assert iou[0, 0] == 1.0
        for lq in (False, True):
            want = Matcher(0.7, 0.3, lq)(torch.from_numpy(iou.copy())).numpy()
            assert np.array_equal(O.match(iou, 0.7, 0.3, lq), want)


def test_build_lists_the_source_and_binds_the_entries():
    from disprcnn_amd.pts import _lib, build
    assert "det_train.hip" in build.SOURCES
    for name in ("drc_det2d_match_fwd", "drc_det2d_sample_fwd", "drc_det2d_srpn_loss_fwd", "drc_det2d_fastrcnn_loss_fwd",
                 "drc_det2d_mask_loss_fwd"):
        assert name in _lib.EXPORTED_SYMBOLS
    from disprcnn_amd.layers import det2d_loss
    assert det2d_loss.MAX_GT == 128 and "#define DRC_DET2D_MAX_GT 128" in open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read()


def test_oracle_mask_targets_are_torchs_interpolate():
    """The crops of the GPU test's fixture (tests/test_hip_det2d_loss.py: both images, every instance, every ROI, M = 28 and 7): the oracle's
    resize equals F.interpolate(bilinear, align_corners=False) on the CPU value for value, hence the truncated targets pixel for pixel."""
    n = ones = 0
    for H, W in ((37, 53), (64, 48)):
        for M in (28, 7):
            for box in O.mask_rois(H, W, M):
                for mask in O.mask_instances(H, W):
                    x0, y0, w, h = O.crop_bounds(box, W, H)
                    assert 0 <= x0 < x0 + w <= W and 0 <= y0 < y0 + h <= H
                    crop = mask[y0:y0 + h, x0:x0 + w]
                    ref = F.interpolate(torch.from_numpy(crop.copy())[None, None].float(), size=(M, M), mode="bilinear", align_corners=False)[0, 0]
                    assert np.array_equal(O.mask_target(mask, box, M), ref.byte().numpy()), (H, W, M, box.tolist())
                    assert np.array_equal(O.resize_crop(crop, M), ref.numpy())
                    n += 1
                    ones += int(ref.byte().sum())
    assert n == 108 and ones > 1000
    # half-to-even both ways, the clamps, at least one pixel, the M x M crop
    assert O.crop_bounds([2.5, 3.5, 20.5, 21.5], 53, 37) == (2, 4, 18, 18)
    assert O.crop_bounds([113.0, 87.0, 133.0, 127.0], 53, 37) == (52, 36, 1, 1)
    assert O.crop_bounds([10.2, 10.3, 10.4, 10.45], 53, 37) == (10, 10, 1, 1)
    assert O.crop_bounds([5.0, 6.0, 33.0, 34.0], 53, 37)[2:] == (28, 28)


def test_oracle_mask_loss_is_torchs():
    rng = np.random.default_rng(6)
    x, t = rng.standard_normal((5, 3, 7, 7)).astype(np.float32) * 4, rng.integers(0, 2, (5, 7, 7)).astype(np.uint8)
    cls = np.array([1, 0, 2, 2, 0])
    loss, grad = O.mask_loss(x, cls, t)
    rows = [0, 2, 3]
    want = F.binary_cross_entropy_with_logits(torch.from_numpy(x).double()[rows, cls[rows]], torch.from_numpy(t[rows]).double())
    assert abs(loss - float(want)) <= 1e-12 and not grad[[1, 4]].any()
    assert O.mask_loss(x, np.zeros(5, np.int64), t)[0] == 0.0

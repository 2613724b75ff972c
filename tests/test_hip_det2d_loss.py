"""The 2D stage's training targets, balanced sampling and losses on the GPU (disprcnn_amd/pts/det_train.hip through layers/det2d_loss.py and the
reference-named evaluators) against tests/det2d_loss_oracle.py, which tests/test_det2d_loss_host.py holds to torch's own functions.

Matched indices, labels and sample masks must equal the oracle's exactly.  Regression targets, losses and gradients are held to the bound
tests/test_hip_pointrcnn_loss.py uses for kernels: |got - ref64| <= 2 e32 + 1e-6 |ref64| for a loss, max|got - ref64| <= 2 e32 + 1e-6 max|ref64|
for a tensor, e32 being the oracle's own fp32-vs-fp64 error, computed with the case.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from . import det2d_loss_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES, STRIDES, RATIOS = (32, 64, 128, 256, 512), (4, 8, 16, 32, 64), (0.5, 1.0, 2.0)
PYR1 = [(6, 10), (3, 5), (2, 3), (1, 2), (1, 1)]          # 252 anchors: less than one block, level ends off the wavefront
PYR2 = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]      # 3 843 anchors: the per-ground-truth maximum and the select cross blocks
IMAGES = [(160, 100), (120, 90), (100, 60)]               # (width, height): visibility differs per image
# candidates whose IoU with their own ground truth is exactly 7/10, 3/10 and 5/10, far from everything else
THRESH_CAND = np.array([[1000, 1000, 1009, 1000], [2000, 1000, 2009, 1000], [3000, 1000, 3009, 1000]], F32)
THRESH_GT = np.array([[1000, 1000, 1006, 1000], [2000, 1000, 2002, 1000], [3000, 1000, 3004, 1000]], F32)


def D():
    from disprcnn_amd.layers import det2d_loss
    return det2d_loss


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check_term(got, ref, e32, what):
    got, ref, e32 = float(got), float(ref), float(e32)
    print(f"{what}: got {got!r} ref {ref!r} err {abs(got - ref):.3g} bound {2 * e32 + 1e-6 * abs(ref):.3g}")
    assert np.isfinite(got) and abs(got - ref) <= 2 * e32 + 1e-6 * abs(ref), what


def check_tensor(got, ref, ref32, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e32 = np.abs(np.asarray(ref32, np.float64) - ref).max(initial=0.0)
    err = np.abs(got - ref).max(initial=0.0)
    bound = 2 * e32 + 1e-6 * np.abs(ref).max(initial=0.0)
    print(f"{what}: err {err:.3g} bound {bound:.3g} (|ref| <= {np.abs(ref).max(initial=0.0):.3g})")
    assert np.isfinite(got).all() and err <= bound, what


def anchors_of(pyr):
    from disprcnn_amd.modeling.rpn.anchor_generator import pyramid_level_anchors
    return np.concatenate([pyramid_level_anchors(z, RATIOS, shp, st) for z, shp, st in zip(SIZES, pyr, STRIDES)]).astype(F32)


def anchor_index(pyr, y, x, a):
    return (y * pyr[0][1] + x) * 3 + a


def random_gt(rng, n, size):
    w, h = size
    x1, y1 = rng.uniform(0, w / 2, n), rng.uniform(0, h / 2, n)
    left = np.stack([x1, y1, x1 + rng.uniform(8, 60, n), y1 + rng.uniform(8, 50, n)], axis=1)
    right = left + np.stack([-rng.uniform(0, 10, n), rng.uniform(-1, 1, n), -rng.uniform(0, 10, n), rng.uniform(-1, 1, n)], axis=1)
    return left.astype(F32), right.astype(F32)


def rpn_case(pyr, G, seed=0):
    """Three images; the candidates of each are the pyramid's anchors plus THRESH_CAND.  Image 0's ground truths are planted, in this order:
    0 an anchor itself (IoU exactly 1), 1 a 3 x 3 box (every IoU below the low threshold), 2 an anchor moved half a stride (two anchors tie
    for its maximum), 3 and 4 the same box twice (bit-equal IoUs: the lower row wins), 5 .. 7 THRESH_GT; then random boxes up to G."""
    rng = np.random.default_rng(seed)
    anc = anchors_of(pyr)
    cand = np.concatenate([anc, THRESH_CAND])
    k_same, k_tie = anchor_index(pyr, 3, 5, 1), anchor_index(pyr, 2, 4, 1)
    dup = np.array([[20.5, 10.25, 70.0, 48.5]], F32)
    planted = np.concatenate([anc[k_same][None], np.array([[50.2, 30.1, 52.2, 32.1]], F32), anc[k_tie][None] + F32([2, 0, 2, 0]), dup, dup,
                              THRESH_GT]).astype(F32)
    images = []
    for n, size in enumerate(IMAGES):
        gl, gr = random_gt(rng, G, size)
        if n == 0:
            k = min(G, len(planted))
            gl[:k], gr[:k] = planted[:k], planted[:k]
        vis = (anc[:, 0] >= 0) & (anc[:, 1] >= 0) & (anc[:, 2] < size[0]) & (anc[:, 3] < size[1])
        images.append(SimpleNamespace(cand=cand, vis=np.concatenate([vis, np.ones(3, bool)]), gl=gl, gr=gr))
    return images, k_same, k_tie, len(anc)


# ------------------------------------------------------------------------------------------------------------ matching / labels
@pytest.mark.parametrize("pyr", [PYR1, PYR2], ids=["252", "3843"])
@pytest.mark.parametrize("G", [1, 5, 8, 128])
def test_rpn_match_label_encode(pyr, G):
    images, k_same, k_tie, T = rpn_case(pyr, G)
    got = D().match_label_encode(dev(np.concatenate([i.cand for i in images])), [len(i.cand) for i in images],
                                 dev(np.concatenate([i.gl for i in images])), dev(np.concatenate([i.gr for i in images])), [G] * 3, 0.7, 0.3,
                                 allow_low_quality=True, visibility=dev(np.concatenate([i.vis for i in images])))
    matched, labels, reg = (host(t) for t in got)
    assert matched.dtype == np.int64 and labels.dtype == np.float32
    first = 0
    for n, im in enumerate(images):
        m, lab, enc = O.rpn_targets(im.cand, im.vis, im.gl, im.gr, 0.7, 0.3)
        enc64 = O.rpn_targets(im.cand, im.vis, im.gl, im.gr, 0.7, 0.3, dtype=np.float64)[2]
        sl = slice(first, first + len(im.cand))
        assert np.array_equal(matched[sl], m), f"image {n}: {np.count_nonzero(matched[sl] != m)} matched indices differ"
        assert np.array_equal(labels[sl], lab), f"image {n}: labels differ"
        check_tensor(reg[sl], enc64, enc, f"image {n} regression targets")
        first += len(im.cand)
    m0 = matched[:len(images[0].cand)]
    assert m0[k_same] == 0                                                     # IoU exactly 1
    if G >= 5:
        assert m0[k_tie] == 2 and m0[k_tie + 3] == 2, "both anchors tied for a ground truth's maximum keep it"
        assert not (m0 == 4).any(), "bit-equal IoUs go to the lowest row"
    if G >= 8:
        assert m0[T:T + 3].tolist() == [5, 6, 7]                               # at the high threshold; the other two rescued
        assert (labels == -1).any() and (labels == 1).any() and (labels == 0).any()


def box_case(P, G, seed=1):
    """Joint 6-boxes from the second pyramid's case: candidates THRESH_CAND first, then the anchors; the right view of a candidate is moved by
    0, 1 or 2 pixels (0 on the planted ones)."""
    images, k_same, k_tie, T = rpn_case(PYR2, G, seed)
    rng = np.random.default_rng(seed + 100)
    out = []
    for n, im in enumerate(images):
        pool = np.concatenate([im.cand[T:], im.cand[:T]])[:P + n]             # images of different lengths
        d = ((np.arange(len(pool)) + 2) % 3).astype(F32)
        d[:3] = 0
        prop6 = np.concatenate([pool, pool[:, [0]] - d[:, None], pool[:, [2]] - d[:, None]], axis=1).astype(F32)
        gt6 = np.concatenate([im.gl, im.gr[:, [0, 2]]], axis=1).astype(F32)
        out.append(SimpleNamespace(prop6=prop6, gt6=gt6, labels=rng.integers(1, 4, G).astype(np.int64)))
    return out


@pytest.mark.parametrize("thresholds", [(0.5, 0.5), (0.7, 0.3)], ids=["fg.5", "fg.7-bg.3"])
@pytest.mark.parametrize("P,G", [(1, 8), (63, 8), (65, 1), (65, 5), (700, 8), (700, 128)])
def test_box_match_label_encode(P, G, thresholds):
    high, low = thresholds
    weights = (10.0, 10.0, 5.0, 5.0)
    images = box_case(P, G)
    gt6 = np.concatenate([i.gt6 for i in images])
    got = D().match_label_encode(dev(np.concatenate([i.prop6 for i in images])), [len(i.prop6) for i in images], dev(gt6[:, :4]),
                                 dev(gt6[:, [4, 1, 5, 3]]), [G] * 3, high, low, weights=weights,
                                 gt_labels=dev(np.concatenate([i.labels for i in images])))
    matched, labels, reg = (host(t) for t in got)
    assert labels.dtype == np.int64
    first = 0
    for n, im in enumerate(images):
        m, lab, enc = O.box_targets(im.prop6, im.gt6, im.labels, high, low, weights)
        enc64 = O.box_targets(im.prop6, im.gt6, im.labels, high, low, weights, dtype=np.float64)[2]
        sl = slice(first, first + len(im.prop6))
        assert np.array_equal(matched[sl], m) and np.array_equal(labels[sl], lab), f"image {n}"
        check_tensor(reg[sl], enc64, enc, f"image {n} regression targets")
        first += len(im.prop6)
    if G >= 8:
        m0 = matched[:min(3, P)].tolist()
        assert m0 == ([5, -1, 7] if high == 0.5 else [5, -2, -2])[:len(m0)]   # IoU exactly 7/10, 3/10, 5/10 against the two thresholds
        if high == 0.7 and P >= 63:
            assert (labels == -1).any()


def test_match_raises_from_the_span_lengths():
    z4 = torch.zeros((4, 4), device="cuda")
    with pytest.raises(ValueError, match="ground-truth"):
        D().match_label_encode(z4, [2, 2], z4[:1], z4[:1], [1, 0], 0.7, 0.3)
    with pytest.raises(ValueError, match="proposal"):
        D().match_label_encode(z4, [4, 0], z4[:2], z4[:2], [1, 1], 0.7, 0.3)
    many = torch.zeros((D().MAX_GT + 1, 4), device="cuda")
    with pytest.raises(ValueError, match="at most"):
        D().match_label_encode(z4, [4], many, many, [D().MAX_GT + 1], 0.7, 0.3)


# ------------------------------------------------------------------------------------------------------------ sampling
def class_labels(rng, n, n_pos, n_neg, dtype=F32):
    lab = np.full(n, -1, dtype)
    perm = rng.permutation(n)
    lab[perm[:n_pos]] = 1 if dtype == F32 else rng.integers(1, 4, n_pos)
    lab[perm[n_pos:n_pos + n_neg]] = 0
    return lab


def run_sampler(labels, draws, batch, fraction, indices=False):
    counts = [len(v) for v in labels]
    pos, neg, cnt, idx = D().balanced_sample(dev(np.concatenate(labels)), counts, batch, fraction, dev(np.concatenate(draws)), want_indices=indices)
    pos, neg, cnt = host(pos), host(neg), host(cnt)
    first = 0
    for n, (lab, dr) in enumerate(zip(labels, draws)):
        pm, nm = O.sample(lab, dr, batch, fraction)
        sl = slice(first, first + len(lab))
        assert np.array_equal(pos[sl], pm), f"image {n}: positive masks differ at {np.nonzero(pos[sl] != pm)[0][:8]}"
        assert np.array_equal(neg[sl], nm), f"image {n}: negative masks differ at {np.nonzero(neg[sl] != nm)[0][:8]}"
        assert cnt[n].tolist() == [pm.sum(), nm.sum()]
        if indices:
            want = np.nonzero(pm | nm)[0]
            row = host(idx)[n]
            assert np.array_equal(row[:len(want)], want) and (row[len(want):] == -1).all()
        first += len(lab)
    return pos, neg


SPANS = (3000, 700, 50, 1)


def sampler_labels(rng, dtype=F32):
    # more positives than num_pos; fewer positives and enough negatives; fewer negatives than needed; a single candidate
    return [class_labels(rng, 3000, 400, 2000, dtype), class_labels(rng, 700, 20, 500, dtype), class_labels(rng, 50, 30, 10, dtype),
            class_labels(rng, 1, 0, 1, dtype)]


@pytest.mark.parametrize("kind", ["uniform", "ties", "low-bits", "high-bits", "zero"])
def test_balanced_sample_draws(kind):
    rng = np.random.default_rng(10)
    labels = sampler_labels(rng)
    if kind == "uniform":
        draws = [rng.random(n, dtype=F32) for n in SPANS]
    elif kind == "ties":            # eight distinct keys: equal keys straddle every k-th position
        draws = [(rng.integers(0, 8, n) / 8).astype(F32) for n in SPANS]
    elif kind == "low-bits":        # keys that differ in the lowest mantissa byte only: the first three passes see one bin
        draws = [(0.5 + rng.integers(0, 256, n) * 2.0 ** -24).astype(F32) for n in SPANS]
    elif kind == "high-bits":       # powers of two: keys that differ in the highest byte(s) only
        draws = [(2.0 ** -rng.integers(1, 60, n).astype(np.float64)).astype(F32) for n in SPANS]
    else:
        draws = [np.zeros(n, F32) for n in SPANS]
    run_sampler(labels, draws, 256, 0.5)


def test_balanced_sample_edges():
    rng = np.random.default_rng(11)
    # a batch larger than the candidates, an image whose labels are all -1, int64 labels, the compacted indices
    labels = [class_labels(rng, 300, 60, 200, np.int64), np.full(90, -1, np.int64), class_labels(rng, 1500, 3, 1400, np.int64)]
    draws = [rng.random(len(v), dtype=F32) for v in labels]
    pos, neg = run_sampler(labels, draws, 512, 0.25, indices=True)
    assert pos[:300].sum() == 60 and neg[:300].sum() == 200 and not pos[300:390].any() and not neg[300:390].any()
    run_sampler(labels, draws, 64, 0.25, indices=True)
    run_sampler(labels, draws, 0, 0.5)


def test_sampler_class_returns_the_reference_lists():
    from disprcnn_amd.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    rng = np.random.default_rng(12)
    labels = [class_labels(rng, 400, 50, 300), class_labels(rng, 130, 5, 100)]
    draws = [rng.random(len(v), dtype=F32) for v in labels]
    pos, neg = BalancedPositiveNegativeSampler(64, 0.5)([dev(v) for v in labels], dev(np.concatenate(draws)))
    for p, q, lab, dr in zip(pos, neg, labels, draws):
        pm, nm = O.sample(lab, dr, 64, 0.5)
        assert p.dtype == torch.uint8 and np.array_equal(host(p), pm) and np.array_equal(host(q), nm)
    pos2, _ = BalancedPositiveNegativeSampler(64, 0.5)([dev(v) for v in labels])          # its own torch.rand
    assert [int(p.sum()) for p in pos2] == [32, 5]


# ------------------------------------------------------------------------------------------------------------ RPN loss
def srpn_inputs(A, shapes, N=2, seed=20, batch=48, scale=3.0, sampled=True):
    rng = np.random.default_rng(seed + A)
    z = [(rng.standard_normal((N, 2 * A, h, w)) * scale).astype(F32) for h, w in shapes]
    b = [(rng.standard_normal((N, 6 * A, h, w)) * 0.3).astype(F32) for h, w in shapes]
    total = sum(h * w * A for h, w in shapes)
    labels = np.concatenate([class_labels(rng, total, total // 6, total // 2) for _ in range(N)])
    reg = (rng.standard_normal((N * total, 6)) * 0.3).astype(F32)
    if sampled:
        masks = [O.sample(labels[n * total:(n + 1) * total], rng.random(total, dtype=F32), batch, 0.5) for n in range(N)]
    else:
        masks = [(np.zeros(total, np.uint8), np.zeros(total, np.uint8))] * N
    pm, nm = np.concatenate([m[0] for m in masks]), np.concatenate([m[1] for m in masks])
    counts = np.array([[m[0].sum(), m[1].sum()] for m in masks], np.int32)
    return SimpleNamespace(z=z, b=b, labels=labels, reg=reg, pm=pm, nm=nm, counts=counts, total=total, A=A, N=N)


def run_srpn(c, w_obj=1.0, w_box=1.0):
    z, b = [dev(v).requires_grad_() for v in c.z], [dev(v).requires_grad_() for v in c.b]
    obj, box, terms = D().srpn_loss(z, b, dev(c.pm), dev(c.nm), dev(c.reg), dev(c.counts))
    assert obj.dim() == 0 and obj.dtype == torch.float32 and obj.is_cuda and not terms.requires_grad
    (w_obj * obj + w_box * box).backward()
    return host(terms).copy(), [host(v.grad).copy() for v in z], [host(v.grad).copy() for v in b]


@pytest.mark.parametrize("A", [1, 3])
def test_srpn_loss_and_gradient(A):
    """Against autograd on the CPU through the reference's literal composition (softmax over view(N, 2, -1, W), permute_and_flatten,
    cross_entropy): a slip in either pairing shows at A = 3; at A = 1 the two pairings coincide."""
    c = srpn_inputs(A, [(6, 10), (3, 5), (1, 2)])
    c.z[0][0, :, 2, 3] = 40.0 * np.where(np.arange(2 * A) % 2, 1, -1)       # saturated pairs
    c.z[1][1, :, 1, 1] = -40.0 * np.where(np.arange(2 * A) < A, 1, -1)
    terms, gz, gb = run_srpn(c, 0.7, 1.3)
    terms2, gz2, gb2 = run_srpn(c, 0.7, 1.3)
    assert np.array_equal(terms, terms2) and all(np.array_equal(a, b) for a, b in zip(gz + gb, gz2 + gb2)), "two runs differ"
    o64, b64, rz64, rb64 = O.srpn_loss(c.z, c.b, c.labels, c.reg, c.pm, c.nm, torch.float64)
    o32, b32, rz32, rb32 = O.srpn_loss(c.z, c.b, c.labels, c.reg, c.pm, c.nm, torch.float32)
    assert terms[2] == c.pm.sum() + c.nm.sum() > 0
    check_term(terms[0], o64, abs(o32 - o64), f"A={A} loss_objectness")
    check_term(terms[1], b64, abs(b32 - b64), f"A={A} loss_rpn_box_reg")
    for l in range(len(gz)):
        check_tensor(gz[l], 0.7 * rz64[l], 0.7 * rz32[l], f"A={A} level {l} d/d cls_logits")
        check_tensor(gb[l], 1.3 * rb64[l], 1.3 * rb32[l], f"A={A} level {l} d/d bbox_pred")
    # exactly zero wherever no sampled anchor reaches: box codes of unsampled-positive anchors, raw pairs whose two probabilities belong to
    # unsampled anchors
    off = 0
    for l, zl in enumerate(c.z):
        H, W = zl.shape[2:]
        for n in range(c.N):
            s = (c.pm | c.nm)[n * c.total + off:n * c.total + off + H * W * A].reshape(H, W, A).astype(bool)
            p = c.pm[n * c.total + off:n * c.total + off + H * W * A].reshape(H, W, A).astype(bool)
            for ch in range(A):
                touched = s[:, :, ch // 2] | s[:, :, (ch + A) // 2]
                assert not gz[l][n, ch][~touched].any() and not gz[l][n, ch + A][~touched].any()
                assert touched.sum() == 0 or np.abs(gz[l][n, ch][touched]).max() > 0
            for a in range(A):
                assert not gb[l][n, 6 * a:6 * a + 6][:, ~p[:, :, a]].any()
        off += H * W * A


def test_srpn_loss_saturated_logits_are_finite():
    c = srpn_inputs(3, [(4, 6), (2, 3)], scale=40.0)
    terms, gz, gb = run_srpn(c)
    o64, b64, _, _ = O.srpn_loss(c.z, c.b, c.labels, c.reg, c.pm, c.nm, torch.float64)
    o32, b32, _, _ = O.srpn_loss(c.z, c.b, c.labels, c.reg, c.pm, c.nm, torch.float32)
    assert np.isfinite(terms).all() and all(np.isfinite(g).all() for g in gz + gb)
    check_term(terms[0], o64, abs(o32 - o64), "loss_objectness at +-40")
    check_term(terms[1], b64, abs(b32 - b64), "loss_rpn_box_reg at +-40")


def test_srpn_loss_without_a_sampled_anchor_is_zero():
    c = srpn_inputs(3, [(4, 6), (2, 3)], sampled=False)
    terms, gz, gb = run_srpn(c)
    assert terms.tolist() == [0.0, 0.0, 0.0] and not any(g.any() for g in gz + gb)


# ------------------------------------------------------------------------------------------------------------ box-head loss
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("R,kind", [(1, "mixed"), (65, "mixed"), (513, "mixed"), (65, "none-positive"), (65, "all-positive")])
def test_fastrcnn_loss_and_gradient(C, R, kind):
    rng = np.random.default_rng(30 + R + C)
    x, b = (rng.standard_normal((R, C)) * 3).astype(F32), rng.standard_normal((R, 6 * C)).astype(F32) * 2
    reg = rng.standard_normal((R, 6)).astype(F32)
    labels = {"mixed": rng.integers(0, C, R), "none-positive": np.zeros(R, np.int64), "all-positive": rng.integers(1, C, R)}[kind].astype(np.int64)

    def run():
        xt, bt = dev(x).requires_grad_(), dev(b).requires_grad_()
        lc, lb, terms = D().fastrcnn_loss(xt, bt, dev(labels), dev(reg))
        (0.6 * lc + 1.7 * lb).backward()
        return host(terms).copy(), host(xt.grad).copy(), host(bt.grad).copy()
    terms, gx, gb = run()
    terms2, gx2, gb2 = run()
    assert np.array_equal(terms, terms2) and np.array_equal(gx, gx2) and np.array_equal(gb, gb2), "two runs differ"
    c64, b64, gx64, gb64 = O.fastrcnn_loss(x, b, labels, reg, torch.float64)
    c32, b32, gx32, gb32 = O.fastrcnn_loss(x, b, labels, reg, torch.float32)
    check_term(terms[0], c64, abs(c32 - c64), "loss_classifier")
    check_term(terms[1], b64, abs(b32 - b64), "loss_box_reg")
    check_tensor(gx, 0.6 * gx64, 0.6 * gx32, "d/d class_logits")
    check_tensor(gb, 1.7 * gb64, 1.7 * gb32, "d/d box_regression")
    if kind == "none-positive":
        assert terms[1] == 0 and not gb.any()
    assert not gb[labels == 0].any() and terms[2] == R


# ------------------------------------------------------------------------------------------------------------ evaluators
def cfg_2d():
    return SimpleNamespace(MODEL=SimpleNamespace(
        CLS_AGNOSTIC_BBOX_REG=False,
        RPN=SimpleNamespace(FG_IOU_THRESHOLD=0.7, BG_IOU_THRESHOLD=0.3, BATCH_SIZE_PER_IMAGE=256, POSITIVE_FRACTION=0.5),
        ROI_HEADS=SimpleNamespace(FG_IOU_THRESHOLD=0.5, BG_IOU_THRESHOLD=0.5, BBOX_REG_WEIGHTS=(10.0, 10.0, 5.0, 5.0), BATCH_SIZE_PER_IMAGE=128,
                                  POSITIVE_FRACTION=0.25),
        ROI_MASK_HEAD=SimpleNamespace(RESOLUTION=28)))


def boxlist(boxes, size, **fields):
    from disprcnn_amd.structures.bounding_box import BoxList
    out = BoxList(dev(np.asarray(boxes, F32)), size)
    for k, v in fields.items():
        out.add_field(k, dev(v))
    return out


def test_srpn_evaluator_end_to_end():
    from disprcnn_amd.modeling.box_coder import BoxCoder
    from disprcnn_amd.modeling.rpn.stereo_rpn_loss import make_srpn_loss_evaluator
    from disprcnn_amd.utils.synth import hash_uniform
    from disprcnn.modeling.rpn.stereo_rpn_loss import make_srpn_loss_evaluator as aliased
    assert aliased is make_srpn_loss_evaluator
    images, _, _, T = rpn_case(PYR2, 8)
    images, N, A = images[:2], 2, 3
    ends = np.cumsum([0] + [h * w * A for h, w in PYR2])
    anchors = [[boxlist(im.cand[s:e], size, visibility=im.vis[s:e]) for s, e in zip(ends[:-1], ends[1:])] for im, size in zip(images, IMAGES)]
    z = [hash_uniform(f"srpn_cls{l}", (N, 2 * A, h, w), -4, 4) for l, (h, w) in enumerate(PYR2)]
    b = [hash_uniform(f"srpn_box{l}", (N, 6 * A, h, w), -0.5, 0.5) for l, (h, w) in enumerate(PYR2)]
    draws = hash_uniform("srpn_draws", (N * T,), 0.0, 1.0)
    zt, bt = [v.cuda().requires_grad_() for v in z], [v.cuda().requires_grad_() for v in b]
    ev = make_srpn_loss_evaluator(cfg_2d(), BoxCoder(weights=(1.0, 1.0, 1.0, 1.0)))
    obj, box = ev(anchors, zt, bt, [boxlist(im.gl, s) for im, s in zip(images, IMAGES)], [boxlist(im.gr, s) for im, s in zip(images, IMAGES)],
                  draws=draws.cuda())
    (obj + box).backward()
    labels, regs, pms, nms = [], [], [], []
    for n, im in enumerate(images):
        _, lab, enc = O.rpn_targets(im.cand[:T], im.vis[:T], im.gl, im.gr, 0.7, 0.3)
        pm, nm = O.sample(lab, draws.numpy()[n * T:(n + 1) * T], 256, 0.5)
        labels.append(lab); regs.append(enc); pms.append(pm); nms.append(nm)
    args = ([v.numpy() for v in z], [v.numpy() for v in b], np.concatenate(labels), np.concatenate(regs), np.concatenate(pms), np.concatenate(nms))
    o64, b64, rz64, rb64 = O.srpn_loss(*args, torch.float64)
    o32, b32, rz32, rb32 = O.srpn_loss(*args, torch.float32)
    assert np.concatenate(pms).sum() > 0
    check_term(obj.detach().cpu(), o64, abs(o32 - o64), "evaluator loss_objectness")
    check_term(box.detach().cpu(), b64, abs(b32 - b64), "evaluator loss_rpn_box_reg")
    for l in range(len(z)):
        check_tensor(host(zt[l].grad), rz64[l], rz32[l], f"level {l} cls_logits.grad")
        check_tensor(host(bt[l].grad), rb64[l], rb32[l], f"level {l} bbox_pred.grad")


def test_box_evaluator_end_to_end():
    from disprcnn_amd.modeling.roi_heads.box_head_loss import make_roi_box_loss_evaluator
    from disprcnn_amd.utils.synth import hash_uniform
    cases = box_case(700, 8)[:2]
    sizes, C, batch = IMAGES[:2], 4, 128
    total = sum(len(c.prop6) for c in cases)
    draws = hash_uniform("box_draws", (total,), 0.0, 1.0)
    props = {"left": [boxlist(c.prop6[:, :4], s) for c, s in zip(cases, sizes)], "right": [boxlist(c.prop6[:, [4, 1, 5, 3]], s) for c, s in zip(cases, sizes)]}
    tgts = {"left": [boxlist(c.gt6[:, :4], s, labels=c.labels) for c, s in zip(cases, sizes)],
            "right": [boxlist(c.gt6[:, [4, 1, 5, 3]], s, labels=c.labels) for c, s in zip(cases, sizes)]}
    ev = make_roi_box_loss_evaluator(cfg_2d())
    left, right = ev.subsample(props, tgts, draws=draws.cuda())
    lab_all, reg_all, reg64_all, first, n_pos = [], [], [], 0, 0
    for n, c in enumerate(cases):
        _, lab, enc = O.box_targets(c.prop6, c.gt6, c.labels, 0.5, 0.5, (10.0, 10.0, 5.0, 5.0))
        enc64 = O.box_targets(c.prop6, c.gt6, c.labels, 0.5, 0.5, (10.0, 10.0, 5.0, 5.0), dtype=np.float64)[2]
        pm, nm = O.sample(lab, draws.numpy()[first:first + len(lab)], batch, 0.25)
        keep = np.nonzero(pm | nm)[0]
        assert len(left[n]) == len(keep) == len(right[n])
        n_pos += int(pm.sum())
        assert np.array_equal(host(left[n].bbox), c.prop6[keep][:, :4]) and np.array_equal(host(right[n].bbox), c.prop6[keep][:, [4, 1, 5, 3]])
        assert np.array_equal(host(left[n].get_field("labels")), lab[keep])
        check_tensor(host(left[n].get_field("regression_targets")), enc64[keep], enc[keep], f"image {n} sampled regression targets")
        lab_all.append(lab[keep]); reg_all.append(enc[keep]); reg64_all.append(enc64[keep])
        first += len(lab)
    R = sum(len(v) for v in lab_all)
    assert n_pos > 0
    x, b = hash_uniform("box_cls", (R, C), -3, 3), hash_uniform("box_reg", (R, 6 * C), -1, 1)
    xt, bt = x.cuda().requires_grad_(), b.cuda().requires_grad_()
    lc, lb = ev([xt], [bt])
    (lc + lb).backward()
    reg_dev = np.concatenate([host(v.get_field("regression_targets")) for v in left])
    c64, b64, gx64, gb64 = O.fastrcnn_loss(x.numpy(), b.numpy(), np.concatenate(lab_all), reg_dev, torch.float64)
    c32, b32, gx32, gb32 = O.fastrcnn_loss(x.numpy(), b.numpy(), np.concatenate(lab_all), reg_dev, torch.float32)
    check_term(lc.detach().cpu(), c64, abs(c32 - c64), "evaluator loss_classifier")
    check_term(lb.detach().cpu(), b64, abs(b32 - b64), "evaluator loss_box_reg")
    check_tensor(host(xt.grad), gx64, gx32, "class_logits.grad")
    check_tensor(host(bt.grad), gb64, gb32, "box_regression.grad")


# ------------------------------------------------------------------------------------------------------------ mask targets and loss
MASK_IMAGES = [(37, 53), (64, 48)]          # (height, width), three instances each


def mask_case(M, C=4, seed=40):
    """Every ROI of O.mask_rois on every instance of both images; every fifth ROI is made non-positive (its match is -1)."""
    rng = np.random.default_rng(seed + M)
    inst = [O.mask_instances(H, W) for H, W in MASK_IMAGES]
    boxes, matched, want = [], [], []
    for (H, W), masks in zip(MASK_IMAGES, inst):
        for g in range(3):
            for box in O.mask_rois(H, W, M):
                k = len(matched)
                boxes.append(box)
                matched.append(-1 if k % 5 == 4 else g)
                want.append(np.zeros((M, M), np.uint8) if k % 5 == 4 else O.mask_target(masks[g], box, M))
    P = len(boxes)
    inst_labels = np.array([1, 2, 3, 3, 1, 2], np.int64)
    cls = np.array([0 if m < 0 else inst_labels[(i // (P // 2)) * 3 + m] for i, m in enumerate(matched)], np.int64)
    logits = (rng.standard_normal((P, C, M, M)) * 3).astype(F32)
    logits[0, :, 0, :4] = [40.0, -40.0, 40.0, -40.0]
    return SimpleNamespace(inst=inst, boxes=np.array(boxes, F32), matched=np.array(matched, np.int64), targets=np.stack(want), cls=cls,
                           inst_labels=inst_labels, logits=logits, counts=[P // 2, P // 2])


def run_mask(c, matched, weight=1.0):
    flat, table, inst_counts = D().pack_masks([dev(m) for m in c.inst])
    x = dev(c.logits).requires_grad_()
    loss, terms, targets, count = D().mask_loss(x, dev(c.boxes), c.counts, dev(matched), dev(c.inst_labels), flat, table, inst_counts)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and targets.dtype == torch.uint8
    (weight * loss).backward()
    return host(terms).copy(), host(targets).copy(), host(x.grad).copy(), int(count)


@pytest.mark.parametrize("M", [28, 7])
def test_mask_targets_loss_and_gradient(M):
    c = mask_case(M)
    terms, targets, grad, count = run_mask(c, c.matched, 1.9)
    terms2, targets2, grad2, _ = run_mask(c, c.matched, 1.9)
    assert np.array_equal(terms, terms2) and np.array_equal(grad, grad2) and np.array_equal(targets, targets2), "two runs differ"
    wrong = np.count_nonzero(targets != c.targets)
    assert wrong == 0, f"{wrong} target pixels differ from the oracle's on ROIs {sorted(set(np.nonzero(targets != c.targets)[0]))}"
    assert 0 < c.targets.sum() < c.targets.size and count == np.count_nonzero(c.cls > 0) and terms[1] == count * M * M
    l64, g64 = O.mask_loss(c.logits, c.cls, c.targets, torch.float64)
    l32, g32 = O.mask_loss(c.logits, c.cls, c.targets, torch.float32)
    check_term(terms[0], l64, abs(l32 - l64), f"M={M} loss_mask")
    check_tensor(grad, 1.9 * g64, 1.9 * g32, f"M={M} d/d mask_logits")
    for p in range(len(c.cls)):
        others = [k for k in range(c.logits.shape[1]) if k != c.cls[p] or c.cls[p] == 0]
        assert not grad[p, others].any(), "gradient on a plane or a ROI that is not selected"


def test_mask_loss_without_a_positive_roi_is_zero():
    c = mask_case(7)
    terms, targets, grad, count = run_mask(c, np.full_like(c.matched, -1))
    assert terms.tolist() == [0.0, 0.0] and count == 0 and not targets.any() and not grad.any()


def test_mask_evaluator_end_to_end():
    from disprcnn_amd.modeling.roi_heads.mask_head_loss import keep_only_positive_boxes, make_roi_mask_loss_evaluator
    from disprcnn_amd.utils.synth import hash_uniform
    M, C = 28, 4
    gt_boxes = [np.array([[5, 6, 30, 28], [20, 2, 33, 35], [1, 1, 50, 35]], F32), np.array([[4, 8, 40, 50], [10, 30, 30, 60], [0, 0, 47, 63]], F32)]
    gt_labels = [np.array([1, 2, 3], np.int64), np.array([3, 1, 2], np.int64)]
    inst = [O.mask_instances(H, W) for H, W in MASK_IMAGES]
    shifts = np.array([[0, 0, 0, 0], [1.5, -0.5, 2.5, 1.5], [-2.2, 1.3, -0.6, 2.1]], F32)
    props, cls, want = [], [], []
    for boxes, labels, masks in zip(gt_boxes, gt_labels, inst):
        p = np.concatenate([boxes + s for s in shifts] + [np.array([[40, 30, 44, 33]], F32) + 100]).astype(F32)
        m = O.match(O.iou_matrix(boxes, p), 0.5, 0.5, False)
        props.append(p)
        cls.append(np.where(m == -1, 0, labels[np.maximum(m, 0)]))
        want += [np.zeros((M, M), np.uint8) if k < 0 else O.mask_target(masks[k], b, M) for k, b in zip(m, p)]
    cls, want = np.concatenate(cls), np.stack(want)
    assert (cls > 0).sum() >= 12 and (cls == 0).sum() >= 2
    sizes = [(W, H) for H, W in MASK_IMAGES]
    plists = [boxlist(p, s, labels=np.ones(len(p), np.int64)) for p, s in zip(props, sizes)]
    assert [len(b) for b in keep_only_positive_boxes(plists)[0]] == [len(p) for p in props]
    tlists = [boxlist(b, s, labels=l, masks=m) for b, l, m, s in zip(gt_boxes, gt_labels, inst, sizes)]
    logits = hash_uniform("mask_logits", (len(cls), C, M, M), -4, 4)
    x = logits.cuda().requires_grad_()
    ev = make_roi_mask_loss_evaluator(cfg_2d())
    loss = ev(plists, x, tlists)
    loss.backward()
    assert np.array_equal(host(ev.last_targets), want)
    l64, g64 = O.mask_loss(logits.numpy(), cls, want, torch.float64)
    l32, g32 = O.mask_loss(logits.numpy(), cls, want, torch.float32)
    check_term(loss.detach().cpu(), l64, abs(l32 - l64), "evaluator loss_mask")
    check_tensor(host(x.grad), g64, g32, "mask_logits.grad")

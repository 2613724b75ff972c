"""CPU tests of the inputs of tests/test_hip_nms_walks.py: the host model of the NMS walks (tests/nms_walk_model.py) equals the oracle on
the cases the GPU tests run, their closed-form keeps equal the oracle's, and every named mutant of the model is told from the oracle by
at least one of those cases in each walk width -- so the GPU comparison would notice that bug in that kernel.  `pytest -s` prints, per
mutant and width, the cases that catch it."""
import functools

import numpy as np
import pytest

from oracle import nms_oracle as N
from tests import nms_walk_model as M

# the random_clustered cases of the GPU list the model is built for (its n x n IoU costs about a second at 16,385)
MODEL_SIZES = [63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 16385]
NONSTRICT_SIZES = [4097, 8193, 16385]
EDGE_SIZES = [4160, 8256, 16448, 32832]            # pairs, chain and dense_chunk: one size per walk (65, 129, 257 and 513 column blocks)
JOINT_SIZES = {2: [65, 4097], 4: [8193], 8: [16385]}   # the joint register walks (32,769 is the Python fallback: no walk of its own)


@functools.lru_cache(maxsize=None)
def _case(kind, n, thr=0.7, strict=True):
    """-> (boxes, thr, strict, expected keep indices, mask words or None)."""
    if kind == "clustered":
        b, _, k = M.clustered_case(n, thr, strict)
    elif kind in ("pairs", "chain"):
        _, b, _, thr, k = [c for c in M.pairs_and_chain(n) if c[0] == kind][0]
    elif kind == "dense":
        b, _, k = M.dense_chunk(n)
        thr = 0.5
    elif kind == "exact":
        b, _, ks = M.exact_iou(n)
        thr, k = 0.5, ks[strict]
    else:
        b, s = M.degenerate(n)
        with np.errstate(invalid="ignore", divide="ignore"):
            k = N.nms(b, s, thr, strict=strict)
    return b, thr, strict, k, (M.mask_words(b, thr, strict) if M.k_max_words(n) else None)


def _gpu_cases(kmw):
    """The GPU list's cases that run nms_walk_kernel<kmw>."""
    if kmw == 2:
        return ([("clustered", n, 0.7, True) for n in MODEL_SIZES if n <= 8192] + [("clustered", 4097, 0.3, False)] +
                [(k, 4160, 0.7, True) for k in ("pairs", "chain", "dense")] +
                [(k, 4160, 0.5, st) for k in ("exact", "degenerate") for st in (True, False)])
    if kmw == 4:
        return [("clustered", 8193, 0.7, True), ("clustered", 8193, 0.3, False)] + [(k, 8256, 0.7, True) for k in ("pairs", "chain", "dense")]
    return [("clustered", 16385, 0.7, True)] + [(k, 16448, 0.7, True) for k in ("pairs", "chain", "dense")]


@pytest.mark.parametrize("kmw", [2, 4, 8])
def test_model_equals_oracle_on_the_gpu_cases(kmw):
    for key in _gpu_cases(kmw):
        n = key[1]
        _, _, _, k, mask = _case(*key)
        assert M.k_max_words(n) == kmw
        assert np.array_equal(np.nonzero(M.walk(mask, n, kmw))[0], k), key


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_closed_form_keeps_equal_the_oracle(n):
    """pairs at every size the GPU runs it, chain up to 16,448 and dense_chunk, which is `pairs` with another list, up to 8,256: the
    oracle walks n kept boxes here, 2 s per case at 16,448 and 9 s at 32,832.  (The model stands in for it above up to 16,448; the
    32,832-box chain differs from the 16,448-box one in its last block only.)"""
    cases = [(name, b, s, thr, k) for name, b, s, thr, k in M.pairs_and_chain(n) if name == "pairs" or n < 32832]
    if n <= 8256:
        cases.append(("dense",) + M.dense_chunk(n)[:2] + (0.5, M.dense_chunk(n)[2]))
    for name, b, s, thr, k in cases:
        for strict in (True, False):
            if strict or n == 4160:
                assert np.array_equal(N.nms(b, s, thr, strict=strict), k), (name, n, strict)
        assert 0 < n - len(k) <= 64


def test_exact_iou_is_exact_and_degenerate_is_finite():
    b, s, ks = M.exact_iou(4160)
    for strict in (True, False):
        assert np.array_equal(N.nms(b, s, 0.5, strict=strict), ks[strict])
    assert len(ks[True]) == 4160 and 0 < len(ks[True]) - len(ks[False]) == len(M.edge_pairs(4160))
    d, _ = M.degenerate(4160)
    w, h = d[:, 2] - d[:, 0] + 1, d[:, 3] - d[:, 1] + 1
    assert np.isfinite(d).all() and (w == 0).sum() > 100 and (w < 0).sum() > 100 and (h < 0).sum() > 100


def test_builders_sit_on_the_layout_edges():
    for n, last in zip(EDGE_SIZES, (64, 128, 256, 512)):
        bp = M.edge_block_pairs(n)
        want = [(0, 63), (0, 64), (63, 64), (64, 64), (0, last), (last, last)]
        want += [(0, 65), (64, 127), (64, 128), (127, 128)] if last >= 128 else []
        want += [(0, 255), (0, 256), (255, 256)] if last >= 256 else []
        want += [(0, 511)] if last >= 512 else []
        assert set(want) <= set(bp)
        st = M.edge_pairs(n)
        assert {(s // 64, t // 64) for s, t in st} == set(bp)                      # every block pair is there
        for bt in {t // 64 for _, t in st}:
            rows = {t % 64: s // 64 for s, t in st if t // 64 == bt}
            assert {31, 32, 63} <= set(rows) and rows[31] != bt                        # bit 31 arrives through a removed-word
        assert len({s for s, _ in st}) == len(st)
        for s, t, u in M.chain_triples(n):
            words = {s >> 12, t >> 12, u >> 12}
            assert len({s >> 6, t >> 6, u >> 6}) == 3 and len(words) == (3 if last >= 128 else 2)


@pytest.mark.parametrize("kmw", [2, 4, 8])
def test_every_walk_mutant_is_caught_in_this_width(kmw):
    caught = {m: [] for m in M.MUTANTS}
    for key in _gpu_cases(kmw):
        n = key[1]
        _, _, _, k, mask = _case(*key)
        want = M.flags_of(n, k)
        for m in M.MUTANTS:
            if not np.array_equal(M.walk(mask, n, kmw, m), want):
                caught[m].append(f"{key[0]}:{n}:{key[2]}{'' if key[3] else ':ge'}")
    for m in M.MUTANTS:
        print(f"walk<{kmw}> mutant {m}: caught by {len(caught[m])} case(s): {', '.join(caught[m])}")
    assert all(caught.values()), {m: c for m, c in caught.items() if not c}
    # closed-form cases alone (no oracle involved) already catch the layout mutants
    for m in ("word0", "smear", "one_round", "no_last_block"):
        assert any(c.split(":")[0] in ("pairs", "dense") for c in caught[m]), m


@functools.lru_cache(maxsize=None)
def _joint_case(n):
    a, _, ka = M.clustered_case(n, 0.7, True)
    b, _, kb = M.clustered_case(n, 0.7, True, 1)
    return ka, kb, M.mask_words(a, 0.7, True), M.mask_words(b, 0.7, True)


@pytest.mark.parametrize("kmw", [2, 4, 8])
def test_joint_model_and_its_mutants(kmw):
    """The joint walk's model writes joint_flags (the oracle intersection up to the end of the exit chunk) for every max_keep the GPU test
    uses, and both exit mutants are caught in every joint width (65 and 4,097: <2>, 8,193: <4>, 16,385: <8>)."""
    caught = {m: [] for m in M.JOINT_MUTANTS}
    for n in JOINT_SIZES[kmw]:
        assert M.k_max_words(n) == kmw
        ka, kb, ma, mb = _joint_case(n)
        mks = M.joint_max_keeps(n, ka, kb)
        assert {1, n, n + 1, 0, -1} <= set(mks)
        for mk in mks:
            want = M.joint_flags(n, ka, kb, mk)
            assert np.array_equal(M.walk_joint(ma, mb, n, kmw, mk), want), (n, mk)
            for m in M.JOINT_MUTANTS:
                if not np.array_equal(M.walk_joint(ma, mb, n, kmw, mk, m), want):
                    caught[m].append((n, mk))
    for m in M.JOINT_MUTANTS:
        print(f"joint walk<{kmw}> mutant {m}: caught at (n, max_keep) {caught[m]}")
    assert all(caught.values())
    # what the Python wrapper returns (the first max_keep set flags) shows exit_before_store; exit_gt shows only in the flags after the exit chunk
    n, mk = [c for c in caught["exit_before_store"] if c[1] > 0][0]
    ka, kb, ma, mb = _joint_case(n)
    got = np.nonzero(M.walk_joint(ma, mb, n, kmw, mk, "exit_before_store"))[0][:mk]
    assert not np.array_equal(got, np.intersect1d(ka, kb)[:mk])

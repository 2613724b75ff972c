"""GPU parity of every greedy-NMS walk of csrc/nms_ops.hip against oracle.nms_oracle (or a closed form), exact int64 indices.

drc_nms_sorted_batch_fwd picks the walk by col_blocks = ceil(n / 64), drc_nms_sorted_pair_joint_fwd the joint walk:

    n <= 8,192            nms_walk_kernel<2>     nms_walk_joint_kernel<2>       ids ...-walk2
    8,193 .. 16,384       nms_walk_kernel<4>     nms_walk_joint_kernel<4>       ids ...-walk4
    16,385 .. 32,768      nms_walk_kernel<8>     nms_walk_joint_kernel<8>       ids ...-walk8
    > 32,768              nms_walk_big_kernel    Python fallback, layers/nms.py ids ...-walkbig

SIZES are the smallest and largest n of every walk, the 64-row block edges next to them and the first n with column block 64 (the
second removed-word, lane 0 again).  The cases come from tests/nms_walk_model.py; tests/test_nms_walk_model.py shows on the CPU that
they tell every named wrong-value mutant of a walk from the oracle in every width.  The oracle's result of a case is computed once per
process (nms_walk_model.clustered_case) and never written to."""
import numpy as np
import pytest
import torch

from oracle import nms_oracle as N
from tests import nms_walk_model as M

pytestmark = pytest.mark.gpu

SIZES = [63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385, 32767, 32768, 32769]
NONSTRICT_SIZES = [4097, 8193, 16385]
EDGE_SIZES = [4160, 8256, 16448, 32832]            # 65, 129, 257 and 513 column blocks: one size per walk
PAIR_SIZES = [65, 4097, 8193, 16385, 32769]


def _id(n):
    return f"{n}-{M.walk_name(n)}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nms(dev, boxes, scores, thr, strict=True):
    from disprcnn_amd.layers import nms
    k = nms(torch.tensor(boxes).to(dev), torch.tensor(scores).to(dev), thr, strict=strict).cpu().numpy()
    assert k.dtype == np.int64
    return k


@pytest.mark.parametrize("n", SIZES, ids=_id)
def test_nms_walk_vs_oracle(dev, n):
    """random_clustered, IoU > 0.7, at both ends of every walk: <2> up to 8,192, <4> up to 16,384, <8> up to 32,768, the LDS walk at 32,769."""
    b, s, k = M.clustered_case(n, 0.7, True)
    assert 0 < len(k) < n and np.array_equal(_nms(dev, b, s, 0.7), k)


@pytest.mark.parametrize("n", NONSTRICT_SIZES, ids=_id)
def test_nms_walk_vs_oracle_nonstrict(dev, n):
    """IoU >= 0.3 (the reference's CPU test): far more suppression per kept row, first n of the second word and of the <4> and <8> walks."""
    b, s, k = M.clustered_case(n, 0.3, False)
    assert 0 < len(k) < n and np.array_equal(_nms(dev, b, s, 0.3, strict=False), k)


@pytest.mark.parametrize("n", EDGE_SIZES, ids=_id)
def test_pairs_and_chain_on_the_word_edges(dev, n):
    """Closed form: disjoint boxes, box t a copy of box s with (s, t) on the removed-word layout's edges (blocks 0/63/64/65, 127/128,
    255/256, 511, the last; rows 0, 31, 32, 63), and chains s -> t -/-> u over three words.  Walks <2>, <4>, <8> and the LDS walk."""
    for name, b, s, thr, keep in M.pairs_and_chain(n):
        got = _nms(dev, b, s, thr)
        assert np.array_equal(got, keep), (name, n, np.setxor1d(got, keep)[:16])


@pytest.mark.parametrize("n", EDGE_SIZES, ids=_id)
def test_dense_chunk_needs_several_rounds(dev, n):
    """40 kept rows of one chunk, each suppressing a box in a different later block: 3, 5 and 10 rounds of the 16, 8 and 4 rows that the
    <2>, <4> and <8> walks load together; once in the LDS walk."""
    b, s, keep = M.dense_chunk(n)
    got = _nms(dev, b, s, 0.5)
    assert np.array_equal(got, keep), np.setxor1d(got, keep)[:16]


@pytest.mark.parametrize("strict", [True, False])
def test_exact_iou_at_the_threshold(dev, strict):
    """IoU exactly 0.5 in fp32 across the word edges, threshold 0.5: > keeps both boxes, >= removes the later one (walk <2>, 65 blocks)."""
    b, s, ks = M.exact_iou(4160)
    assert np.array_equal(_nms(dev, b, s, 0.5, strict=strict), ks[strict])


@pytest.mark.parametrize("strict", [True, False])
def test_degenerate_boxes(dev, strict):
    """Zero-area and inverted boxes, finite coordinates: 0/0 and negative unions compare as in the oracle (walk <2>, 65 blocks)."""
    b, s = M.degenerate(4160)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = N.nms(b, s, 0.5, strict=strict)
    assert 0 < len(k) < 4160 and np.array_equal(_nms(dev, b, s, 0.5, strict=strict), k)


def _pair_case(n):
    a, s, ka = M.clustered_case(n, 0.7, True)
    b, _, kb = M.clustered_case(n, 0.7, True, 1)
    return a, b, s, ka, kb


@pytest.mark.parametrize("n", PAIR_SIZES, ids=_id)
def test_nms_pair_vs_oracle(dev, n):
    """Two views in one batched launch (sets = 2) through every walk: each view's keep is the oracle's on that view, joint=True their
    sorted intersection."""
    from disprcnn_amd.layers import nms_pair
    a, b, s, ka, kb = _pair_case(n)
    ta, tb, ts = (torch.tensor(x).to(dev) for x in (a, b, s))
    ga, gb = nms_pair(ta, tb, ts, 0.7)
    assert np.array_equal(ga.cpu().numpy(), ka) and np.array_equal(gb.cpu().numpy(), kb) and not np.array_equal(ka, kb)
    gj = nms_pair(ta, tb, ts, 0.7, joint=True).cpu().numpy()
    assert gj.dtype == np.int64 and np.array_equal(gj, np.intersect1d(ka, kb))


def _joint_flags_gpu(dev, a, b, thr, max_keep, strict=True):
    """drc_nms_sorted_pair_joint_fwd itself: the joint flags, which the Python wrapper reduces to indices."""
    from disprcnn_amd import _lib
    from disprcnn_amd import engine as E
    n = len(a)
    boxes = torch.from_numpy(np.stack((a, b))).to(dev).contiguous()
    mask = torch.empty(2 * n * ((n + 63) // 64), dtype=torch.int64, device=dev)
    keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)             # the entry zero-fills it
    st = _lib.lib().drc_nms_sorted_pair_joint_fwd(E._ptr(boxes), n, float(thr), int(strict), int(max_keep), E._ptr(mask), E._ptr(keep),
                                                  E._stream_ptr(dev))
    assert st == 0
    return keep.cpu().numpy()


@pytest.mark.parametrize("n", PAIR_SIZES, ids=_id)
def test_nms_pair_sorted_joint_early_exit(dev, n):
    """The joint walk (<2> at 65 and 4,097, <4> at 8,193, <8> at 16,385; the Python fallback of layers/nms.py at 32,769) with max_keep
    on the oracle's own joint count at chunk ends (first, middle, 63, 64, 65, last), that +- 1, and 1, n, n + 1, 0, -1: the first max_keep
    of the oracle intersection, and in the kernel's flags nothing after the chunk of the exit."""
    from disprcnn_amd.layers import nms_pair_sorted_joint
    a, b, _, ka, kb = _pair_case(n)
    full = np.intersect1d(ka, kb)
    ta, tb = torch.tensor(a).to(dev), torch.tensor(b).to(dev)
    for mk in M.joint_max_keeps(n, ka, kb):
        got = nms_pair_sorted_joint(ta, tb, 0.7, mk).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, full[:mk] if mk > 0 else full), (n, mk)
        if M.k_max_words(n):
            assert np.array_equal(_joint_flags_gpu(dev, a, b, 0.7, mk), M.joint_flags(n, ka, kb, mk)), (n, mk)


def _batch(dev, sets_boxes, thr, strict, fn="batch"):
    """drc_nms_sorted_batch_fwd on box sets of one length -> (status, keep [sets, n] u8, mask words [sets, n, col_blocks])."""
    from disprcnn_amd import _lib
    from disprcnn_amd import engine as E
    sets, n = len(sets_boxes), len(sets_boxes[0])
    cb = (n + 63) // 64
    boxes = torch.from_numpy(np.stack(sets_boxes)).to(dev).contiguous()
    mask = torch.full((sets, n, cb), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    keep = torch.full((sets, n), 7, dtype=torch.uint8, device=dev)
    if fn == "batch":
        st = _lib.lib().drc_nms_sorted_batch_fwd(E._ptr(boxes), sets, n, float(thr), int(strict), E._ptr(mask), E._ptr(keep), E._stream_ptr(dev))
    else:
        assert sets == 1
        st = _lib.lib().drc_nms_sorted_fwd(E._ptr(boxes), n, float(thr), int(strict), E._ptr(mask), E._ptr(keep), E._stream_ptr(dev))
    return st, keep.cpu().numpy(), mask.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("sets", [1, 3, 5])
@pytest.mark.parametrize("n", [65, 129, 4097])
def test_batch_abi_sets_equal_per_set_calls(dev, n, sets):
    """The `sets` dimension of the batched launch with DIFFERENT box sets: set i's flags and mask words are those of a call on set i alone,
    and the oracle's."""
    views = [M.clustered_case(n, 0.7, True, 0)[0], M.clustered_case(n, 0.7, True, 1)[0]]
    views += [np.ascontiguousarray(views[0][::-1]), M.clustered_case(n, 0.3, False)[0], views[1] + np.float32(3)]
    st, keep, mask = _batch(dev, views[:sets], 0.7, True)
    assert st == 0 and set(np.unique(keep)) <= {0, 1}
    for i in range(sets):
        st1, k1, m1 = _batch(dev, [views[i]], 0.7, True)
        assert st1 == 0 and np.array_equal(keep[i], k1[0]) and np.array_equal(mask[i], m1[0]), (n, sets, i)
    assert np.array_equal(np.nonzero(keep[0])[0], M.clustered_case(n, 0.7, True)[2])
    if sets > 1:
        assert np.array_equal(np.nonzero(keep[1])[0], M.clustered_case(n, 0.7, True, 1)[2])


def test_abi_argument_errors_return_before_any_launch(dev):
    from disprcnn_amd import _lib
    from disprcnn_amd import engine as E
    L = _lib.lib()
    boxes = torch.zeros(2, 64, 4, device=dev)
    mask = torch.zeros(2 * 64, dtype=torch.int64, device=dev)
    keep = torch.full((2 * 64,), 7, dtype=torch.uint8, device=dev)
    p, s = (E._ptr(boxes), E._ptr(mask), E._ptr(keep)), E._stream_ptr(dev)

    def batch(sets, n):
        return L.drc_nms_sorted_batch_fwd(p[0], sets, n, 0.5, 1, p[1], p[2], s)

    assert batch(0, 64) == 0 and batch(2, 0) == 0 and batch(0, 0) == 0
    assert batch(65536, 64) == -2 and batch(-1, 64) == -2 and batch(1, -1) == -2
    assert batch(1, 524289) == -5                                          # 8,193 column blocks: beyond the LDS walk's 64 KB
    assert L.drc_nms_sorted_pair_joint_fwd(p[0], 32769, 0.5, 1, -1, p[1], p[2], s) == -5      # 513 blocks: the caller's fallback
    assert L.drc_nms_sorted_pair_joint_fwd(p[0], 0, 0.5, 1, -1, p[1], p[2], s) == 0
    assert L.drc_nms_sorted_pair_joint_fwd(p[0], -1, 0.5, 1, -1, p[1], p[2], s) == -2
    torch.cuda.synchronize(dev)
    assert (keep.cpu() == 7).all() and (mask.cpu() == 0).all()            # nothing was launched


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("thr,strict", [(0.7, True), (0.3, False)])
def test_mask_words_vs_model(dev, n, thr, strict):
    """All n * col_blocks words of nms_mask_kernel over a sentinel-filled workspace: the zero words below the diagonal, row 63 of a
    diagonal block (no later box in it) and the bits of a last block past n."""
    b = M.clustered_case(n, thr, strict)[0]
    st, keep, mask = _batch(dev, [b], thr, strict, fn="single")
    want = M.mask_words(b, thr, strict)
    assert st == 0 and mask[0].shape == want.shape and np.array_equal(mask[0], want)
    assert np.array_equal(np.nonzero(keep[0])[0], M.clustered_case(n, thr, strict)[2])
    if n >= 64:
        assert want[63, 0] == 0 and (want[64:, 0] == 0).all() and want.any()


@pytest.mark.parametrize("n", [8193, 32769], ids=_id)
def test_walk_reproducible(dev, n):
    """Two calls on the same input give identical bytes (the <4> register walk and the LDS walk, whose ORs go through shared memory)."""
    b = M.clustered_case(n, 0.7, True)[0]
    _, k1, m1 = _batch(dev, [b], 0.7, True)
    _, k2, m2 = _batch(dev, [b], 0.7, True)
    assert k1.tobytes() == k2.tobytes() and m1.tobytes() == m2.tobytes()

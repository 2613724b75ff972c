"""Case builders and a host model of the greedy NMS walks of csrc/nms_ops.hip (plain numpy, no GPU).

The builders return (boxes [n,4] float32 ALREADY in descending-score order, scores [n] float32 strictly decreasing), so a result never
depends on a sort.  The model restates the kernels' DATA LAYOUT, not just their result: `mask_words` gives the 64x64-blocked suppression
words as nms_mask_kernel defines them, `walk` / `walk_joint` keep the removed-words as remv[w][lane] for column block w*64 + lane, take
the diagonal word prefetched one chunk ahead and OR kept rows into the later blocks kRows at a time.  That is what lets a NAMED MUTANT
-- one wrong value on one of those lines, never an out-of-range access -- be applied to the model: tests/test_nms_walk_model.py shows
on the CPU that the cases the GPU tests run tell every mutant from the oracle, i.e. that the GPU tests would notice that bug."""
import functools

import numpy as np

from oracle import nms_oracle

MUTANTS = ("word0", "smear", "one_round", "no_last_block", "stale_diag")
JOINT_MUTANTS = ("exit_gt", "exit_before_store")
EDGE_ROWS = (31, 0, 32, 63)            # target rows within a block (bit 31 of the low half first: every target block gets it)


def scores_for(n):
    """Strictly decreasing and exact in fp32 (n < 2**24)."""
    return np.arange(n, 0, -1, dtype=np.float32)


def k_max_words(n):
    """Removed-words per lane of the register walk the library picks for n boxes; 0 = beyond the register walks (LDS walk / Python fallback)."""
    cb = (n + 63) // 64
    return 2 if cb <= 128 else 4 if cb <= 256 else 8 if cb <= 512 else 0


def walk_name(n):
    k = k_max_words(n)
    return f"walk{k}" if k else "walkbig"


# ------------------------------------------------------------------------------------------------ case builders
def random_clustered(n, thr):
    """tests.golden.make_golden_nms.proposals re-ordered by its scores: the members of a cluster are scattered over all column blocks,
    so a kept row sets bits in every removed-word."""
    from tests.golden.make_golden_nms import proposals
    dets, s = proposals(f"walk{n}_{thr}", n)
    order = np.argsort(-s.numpy(), kind="stable")
    return np.ascontiguousarray(dets.numpy()[order], dtype=np.float32), scores_for(n)


def second_view(boxes):
    """The right view of a stereo list: the first view shifted left by 17..57 px, more for the better-scored boxes (the shift of
    tests/test_hip_nms.py::test_nms_pair_equals_two_calls with the rank as the score)."""
    n = len(boxes)
    b = boxes.copy()
    b[:, [0, 2]] -= (np.float32(17.0) + np.float32(40.0) * (scores_for(n) / np.float32(n)))[:, None]
    return b


def _grid(n, side, pitch, per_row=256):
    """n disjoint side x side boxes (legacy +1 widths) on a grid."""
    i = np.arange(n)
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return np.stack([x, y, x + side - 1, y + side - 1], 1).astype(np.float32)


def edge_block_pairs(n):
    """(source block, target block) on the edges of the removed-word layout that exist for n boxes."""
    last = (n + 63) // 64 - 1
    want = [(0, 63), (0, 64), (0, 65), (63, 64), (64, 64), (64, 127), (64, 128), (127, 128), (0, last), (last, last),
            (0, 255), (0, 256), (255, 256), (0, 511)]
    out = []
    for p in want:
        if p[1] <= last and p not in out:
            out.append(p)
    return out


def edge_pairs(n):
    """(s, t) box indices for `pairs`: every block pair of edge_block_pairs(n), the target rows EDGE_ROWS of a target block dealt out
    to its source blocks (a source in another block first: it gets row 31, which only matters on the removed-word path; the diagonal
    pair cannot take row 0).  Every t is distinct, no s is a t, and every pair has a source of its own (never a target row: a pair
    from another block counts them down from row 62, a diagonal pair up from row 1, so that s < t)."""
    by_target = {}
    for bs, bt in edge_block_pairs(n):
        by_target.setdefault(bt, []).append(bs)
    free = [r for r in range(1, 63) if r not in EDGE_ROWS]
    used_hi, used_lo = {}, {}
    out = []
    for bt, srcs in by_target.items():
        srcs = sorted(srcs, key=lambda b: b == bt)
        for i, trow in enumerate(EDGE_ROWS):
            bs = srcs[i % len(srcs)]
            if bs == bt and trow == 0:
                bs = srcs[(i + 1) % len(srcs)]
                if bs == bt:
                    continue
            t = bt * 64 + trow
            if t >= n:
                continue
            if bs == bt:
                k = used_lo[bs] = used_lo.get(bs, -1) + 1
                srow = free[k]
            else:
                k = used_hi[bs] = used_hi.get(bs, 0) + 1
                srow = free[-k]
            assert used_lo.get(bs, -1) + 1 + used_hi.get(bs, 0) <= len(free) and (bs != bt or srow < trow)
            out.append((bs * 64 + srow, t))
    return out


def _check_closed_form(n, sources, targets):
    assert len(set(targets)) == len(targets) and not set(sources) & set(targets) and all(0 <= s < t < n for s, t in zip(sources, targets))


def pairs(n, st):
    """n disjoint 5x5 boxes, box t overwritten by a copy of box s for every (s, t).  -> boxes, scores, the closed-form keep
    (everything except the ts), valid for any threshold < 1."""
    _check_closed_form(n, [s for s, _ in st], [t for _, t in st])
    b = _grid(n, 5, 8)
    for s, t in st:
        b[t] = b[s]
    return b, scores_for(n), np.setdiff1d(np.arange(n, dtype=np.int64), np.array([t for _, t in st], dtype=np.int64))


CHAIN_THR = 0.5


def chain_triples(n):
    """(s, t, u) with s, t and u in three different removed-words where n has three (else in different blocks of two words)."""
    last = (n + 63) // 64 - 1
    if last >= 128:
        blocks = [(0, 64, 128), (63, 127, last), (1, 65, last)]
    else:
        blocks = [(0, 63, 64), (1, 62, last), (2, 3, last)]
    return [(bs * 64 + 5 + i, bt * 64 + 31 + i, bu * 64 + 40 + i) for i, (bs, bt, bu) in enumerate(blocks)]


def chain(n, stu):
    """n disjoint 21x21 boxes; t = s shifted by 6 px (IoU 15/27 > 0.5) and u = s shifted by 12 px (IoU 15/27 with t, 9/33 with s):
    s suppresses t, and t would suppress u but must not, because t is already removed.  Threshold CHAIN_THR, either test.
    -> boxes, scores, the closed-form keep (everything except the ts)."""
    flat = [i for stu_ in stu for i in stu_]
    assert len(set(flat)) == len(flat) and all(0 <= s < t < u < n for s, t, u in stu)
    b = _grid(n, 21, 48)
    for s, t, u in stu:
        b[t] = b[s] + np.float32([6, 0, 6, 0])
        b[u] = b[s] + np.float32([12, 0, 12, 0])
    return b, scores_for(n), np.setdiff1d(np.arange(n, dtype=np.int64), np.array([t for _, t, _ in stu], dtype=np.int64))


def pairs_and_chain(n):
    """The `pairs` case on the layout's edges and the `chain` case of n boxes as the GPU tests run them: [(name, boxes, scores, thr, keep)]."""
    b, s, k = pairs(n, edge_pairs(n))
    cb, cs, ck = chain(n, chain_triples(n))
    return [("pairs", b, s, 0.5, k), ("chain", cb, cs, CHAIN_THR, ck)]


DENSE_ROWS = 40


def dense_chunk(n):
    """DENSE_ROWS (> 2 x 16) kept rows of chunk 1, each with a copy in a DIFFERENT later block (spread over all words): the chunk's kept
    rows need more than one round of the kRows batching for every kRows.  -> boxes, scores, closed-form keep."""
    last = (n + 63) // 64 - 1
    stride = (last - 2) // (DENSE_ROWS - 1)
    assert stride >= 1
    st = [(64 + r, (2 + r * stride) * 64 + (r * 7 + 3) % 64) for r in range(DENSE_ROWS)]
    st[-1] = (st[-1][0], last * 64 + 31)                   # the last one in the last block
    st = [(s, t) for s, t in st if t < n]
    return pairs(n, st)


def exact_iou(n):
    """Pairs whose IoU is EXACTLY 0.5 in fp32 ([x,y,x+9,y+9], area 100, and its upper half [x,y,x+9,y+4], area 50) on the layout's
    edges.  Threshold 0.5: the strict test keeps both, the other removes the later one.  -> boxes, scores, {strict: keep}."""
    st = edge_pairs(n)
    b = _grid(n, 10, 16)
    for s, t in st:
        b[t] = b[s] - np.float32([0, 0, 0, 5])
    every = np.arange(n, dtype=np.int64)
    return b, scores_for(n), {True: every, False: np.setdiff1d(every, np.array([t for _, t in st], dtype=np.int64))}


def degenerate(n):
    """Zero-area boxes (x2 = x1 - 1) and inverted boxes mixed into a clustered set, finite coordinates only, some of them twice
    (0/0 and negative unions; the expectation is the oracle)."""
    b, s = random_clustered(n, "degenerate")
    i = np.arange(n)
    z = i % 7 == 3
    b[z, 2] = b[z, 0] - 1
    inv = i % 11 == 5
    b[inv] = b[inv][:, [2, 1, 0, 3]]
    inv_y = i % 13 == 6
    b[inv_y] = b[inv_y][:, [0, 3, 2, 1]]
    for src, t in edge_pairs(n):
        b[t] = b[src - src % 7 + 3] if t % 2 else b[src - src % 11 + 5]      # copies of degenerate boxes across the word edges
    return b, s


# ------------------------------------------------------------------------------------------------ oracle, once per case
@functools.lru_cache(maxsize=None)
def clustered_case(n, thr, strict, view=0):
    """(boxes, scores, oracle keep) of the random_clustered case; computed once per process, treat as read-only."""
    b, s = random_clustered(n, thr)
    if view:
        b = second_view(b)
    k = nms_oracle.nms(b, s, thr, strict=strict)
    for a in (b, s, k):
        a.setflags(write=False)
    return b, s, k


def joint_flags(n, keep_a, keep_b, max_keep):
    """What drc_nms_sorted_pair_joint_fwd must write for score-sorted input: 1 where both views keep the box, up to the end of the
    64-row chunk in which the max_keep-th joint box falls, 0 after it (max_keep <= 0 or > n: all)."""
    f = np.zeros(n, dtype=np.uint8)
    f[np.intersect1d(keep_a, keep_b)] = 1
    if max_keep <= 0 or max_keep > n:
        max_keep = n
    cum = np.cumsum(f, dtype=np.int64)
    ends = cum[np.minimum(np.arange(63, n + 63, 64), n - 1)]            # joint count at the end of every chunk
    hit = np.nonzero(ends >= max_keep)[0]
    if hit.size:
        f[(hit[0] + 1) * 64:] = 0
    return f


def joint_max_keeps(n, keep_a, keep_b):
    """max_keep values at which the early exit can go wrong, from the oracle's own joint count per 64-row chunk: the count at the end
    of a chunk and that +- 1 (first chunk, one in the middle, chunks 62 .. 65 where they exist, the last two), 1, n, n + 1, 0, -1."""
    f = joint_flags(n, keep_a, keep_b, -1)
    cum = np.cumsum(f, dtype=np.int64)
    nchunks = (n + 63) // 64
    ends = cum[np.minimum(np.arange(63, n + 63, 64), n - 1)]
    out = []
    for c in (0, nchunks // 2, 62, 63, 64, 65, nchunks - 2, nchunks - 1):
        if 0 <= c < nchunks:
            out += [int(ends[c]) - 1, int(ends[c]), int(ends[c]) + 1]
    out += [1, n, n + 1, 0, -1]
    return list(dict.fromkeys(out))


# ------------------------------------------------------------------------------------------------ the model
def mask_words(boxes, thr, strict):
    """[n, col_blocks] uint64 as nms_mask_kernel writes them: bit i of word [r, C] = row r suppresses box 64C + i (fp32 IoU with the
    legacy +1, in the oracle's operation order); upper triangle only, the diagonal block limited to later rows, zero below the diagonal."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    n = b.shape[0]
    cb = (n + 63) // 64
    f = np.float32
    x1, y1, x2, y2 = (np.ascontiguousarray(b[:, i]) for i in range(4))
    area = (x2 - x1 + f(1)) * (y2 - y1 + f(1))
    out = np.zeros((n, cb), dtype=np.uint64)
    tri = np.arange(64)[None, :] > np.arange(64)[:, None]
    thr = f(thr)
    with np.errstate(invalid="ignore", divide="ignore"):
        for rb in range(cb):
            r0, r1 = rb * 64, min(n, rb * 64 + 64)
            rows, cols = slice(r0, r1), slice(r0, n)
            w = np.maximum(np.minimum(x2[rows, None], x2[None, cols]) - np.maximum(x1[rows, None], x1[None, cols]) + f(1), f(0))
            h = np.maximum(np.minimum(y2[rows, None], y2[None, cols]) - np.maximum(y1[rows, None], y1[None, cols]) + f(1), f(0))
            inter = w * h
            o = inter / ((area[rows, None] + area[None, cols]) - inter)
            hit = (o > thr) if strict else (o >= thr)
            hit[:, :64][:, :min(64, n - r0)] &= tri[:r1 - r0, :min(64, n - r0)]
            bits = np.zeros((r1 - r0, (cb - rb) * 64), dtype=bool)
            bits[:, :n - r0] = hit
            out[rows, rb:] = np.packbits(bits, axis=1, bitorder="little").view("<u8")
    return out


def _k_rows(kmw):
    return 16 if kmw <= 2 else 8 if kmw <= 4 else 4


class _Walker:
    """One wavefront's state of nms_walk_kernel<k_max_words> for one box set."""

    def __init__(self, mask, n, kmw, mutant):
        self.mask, self.n, self.kmw, self.mutant = mask, n, kmw, mutant
        self.col_blocks = mask.shape[1]
        assert self.col_blocks == (n + 63) // 64 and self.col_blocks <= 64 * kmw
        self.remv = np.zeros(kmw * 64, dtype=np.uint64)        # remv[w][lane] at w * 64 + lane: column block j = w * 64 + lane
        self.dnext = self._diag_of(0)
        self.dprev = self.dnext

    def _diag_of(self, c):
        d = [0] * 64
        if c < self.col_blocks:
            r0 = c * 64
            col = self.mask[r0:min(self.n, r0 + 64), c]
            d[:len(col)] = [int(v) for v in col]
        return d

    def resolve(self, c):
        """Rows of chunk c against the removed-word of block c and against each other -> (kept bits, number of rows)."""
        diag = self.dnext
        if self.mutant == "stale_diag" and c > 0:
            diag = self.dprev
        self.dprev = self.dnext
        self.dnext = self._diag_of(c + 1)
        nr = min(self.n - c * 64, 64)
        w = 0 if self.mutant == "word0" else c >> 6
        cur = int(self.remv[w * 64 + (c & 63)])
        if self.mutant == "smear" and cur & 0x80000000:
            cur |= 0xFFFFFFFF00000000
        kept = 0
        for r in range(nr):
            if not (cur >> r) & 1:
                kept |= 1 << r
                cur |= diag[r]
        return kept, nr

    def propagate(self, c, kept):
        rows = [r for r in range(64) if (kept >> r) & 1]
        k_rows = _k_rows(self.kmw)
        if self.mutant == "one_round":
            rows = rows[:k_rows]
        hi = self.col_blocks - 1 if self.mutant == "no_last_block" else self.col_blocks
        for i in range(0, len(rows), k_rows):
            if c + 1 < hi:
                v = self.mask[c * 64 + np.array(rows[i:i + k_rows]), c + 1:hi]
                self.remv[c + 1:hi] |= np.bitwise_or.reduce(v, axis=0)


def _store(keep, c, nr, bits):
    keep[c * 64:c * 64 + nr] = [(bits >> r) & 1 for r in range(nr)]


def walk(mask, n, kmw, mutant=None):
    """keep flags [n] u8 of nms_walk_kernel<kmw>."""
    assert mutant is None or mutant in MUTANTS
    wk = _Walker(mask, n, kmw, mutant)
    keep = np.zeros(n, dtype=np.uint8)
    for c in range(wk.col_blocks):
        kept, nr = wk.resolve(c)
        _store(keep, c, nr, kept)
        wk.propagate(c, kept)
    return keep


def walk_joint(mask_a, mask_b, n, kmw, max_keep, mutant=None):
    """joint keep flags [n] u8 of drc_nms_sorted_pair_joint_fwd's nms_walk_joint_kernel<kmw> (zero-filled first)."""
    assert mutant is None or mutant in JOINT_MUTANTS
    if max_keep <= 0 or max_keep > n:
        max_keep = n
    views = (_Walker(mask_a, n, kmw, None), _Walker(mask_b, n, kmw, None))
    keep = np.zeros(n, dtype=np.uint8)
    total = 0
    for c in range(views[0].col_blocks):
        (ka, nr), (kb, _) = views[0].resolve(c), views[1].resolve(c)
        both = ka & kb
        total += bin(both).count("1")
        leave = total > max_keep if mutant == "exit_gt" else total >= max_keep
        if leave and mutant == "exit_before_store":
            break
        _store(keep, c, nr, both)
        if leave:
            break
        views[0].propagate(c, ka)
        views[1].propagate(c, kb)
    return keep


def flags_of(n, keep_idx):
    f = np.zeros(n, dtype=np.uint8)
    f[keep_idx] = 1
    return f

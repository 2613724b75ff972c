"""Host-side checks behind tests/test_hip_head_train_edges.py and tests/test_hip_srpn_train_edges.py: the numpy restatements of
tests/head_kernels_oracle.py against independent witnesses (explicit index loops, torch's unfold and its fp64 autograd, a brute-force scan),
and every condition a GPU case relies on that is a property of its inputs -- so a case that stops reaching its branch fails here, on any
machine, before a GPU sees it.  No GPU.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_kernels_oracle as O

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ oracle witnesses
@pytest.mark.parametrize("R,K", O.PACK_SMALL + [(33, 49)])
def test_pack_layouts_are_the_documented_index_maps(R, K):
    a = O.pack_case(R, K) if (R, K) in O.PACK_SMALL else O.uniform("hk:w", (R, K))
    RB, KC = (R + 15) // 16, (K + 15) // 16
    rows, cols = np.zeros(RB * KC * 256, F32), np.zeros(RB * KC * 256, F32)
    at = lambda r, k: a[r, k] if r < R and k < K else F32(0)
    for rb in range(RB):
        for kc in range(KC):
            for g in range(4):
                for r in range(16):
                    for e in range(4):
                        rows[(rb * KC + kc) * 256 + (g * 16 + r) * 4 + e] = at(rb * 16 + r, kc * 16 + g * 4 + e)
    for cb in range(KC):
        for rc in range(RB):
            for g in range(4):
                for c in range(16):
                    for e in range(4):
                        cols[(cb * RB + rc) * 256 + (g * 16 + c) * 4 + e] = at(rc * 16 + g * 4 + e, cb * 16 + c)
    assert np.array_equal(O.pack_rows_np(a), rows) and np.array_equal(O.pack_cols_np(a), cols)
    assert O.pack_rows_np(a).size == O.packed_floats(R, K) and O.pack_cols_np(a).size == O.packed_floats(K, R)
    assert np.array_equal(O.pack_cols_np(a), O.pack_rows_np(np.ascontiguousarray(a.T)))
    assert np.count_nonzero(rows) == np.count_nonzero(a) == np.count_nonzero(cols)          # a permutation of a, plus zeros


def test_wrapped_pack_cases_pass_one_trip_of_the_grid():
    for R, K in O.PACK_WRAPPED:
        assert O.packed_floats(R, K) > O.PACK_GRID_FLOATS and O.packed_floats(K, R) > O.PACK_GRID_FLOATS
        assert R % 16 and K % 16
    assert [K % 4 for _, K in O.PACK_WRAPPED] == [0, 3]                                     # pack_rows' float4 path and its scalar path
    assert all(O.packed_floats(R, K) < O.PACK_GRID_FLOATS for R, K in O.PACK_SMALL)
    assert {K % 4 != 0 for _, K in O.PACK_SMALL} == {True, False}


def test_gather_xcol_is_unfold():
    for C in (3, 8):
        c = O.gather_case(C, 3)
        _, X, _ = O.gather_rows_np(c.row_pix, O.GATHER_N, 3, C, O.GATHER_CAP, O.GATHER_SHAPES, feats=(c.left, c.right))
        R = O.GATHER_N * O.GATHER_CAP
        un = [[F.unfold(torch.from_numpy(f), 3, padding=1).numpy() for f in side] for side in (c.left, c.right)]
        want, live = np.zeros_like(X), 0
        for r, img, l, y, x, pix in O.row_coords(c.row_pix, O.GATHER_SHAPES, O.GATHER_CAP):
            want[r], want[R + r] = un[0][l][img, :, pix], un[1][l][img, :, pix]
            live += 1
        assert live == 9 and np.array_equal(X, want) and (X[:R][c.row_pix >= 0] == 0).any()


def test_gather_t_and_g_are_plain_reads():
    c = O.gather_case(8, 3)
    T, _, G = O.gather_rows_np(c.row_pix, O.GATHER_N, 3, 8, O.GATHER_CAP, O.GATHER_SHAPES, hidden=c.hidden, grads=(c.gz, c.gb), s_obj=c.s_obj,
                               s_box=None)
    off = O.pix_offsets(O.GATHER_SHAPES)
    for r in range(O.GATHER_N * O.GATHER_CAP):
        q, img = int(c.row_pix[r]), r // O.GATHER_CAP
        if q < 0:
            assert not T[r].any() and not G[r].any()
            continue
        l = 0 if q < off[1] else 1
        assert np.array_equal(T[r], c.hidden[l].reshape(O.GATHER_N, 32, -1)[img, :, q - off[l]])
        assert np.array_equal(G[r, :6], c.gz[l].reshape(O.GATHER_N, 6, -1)[img, :, q - off[l]] * c.s_obj) and not G[r, 6:].any()


@pytest.mark.parametrize("C", [2, 8])
def test_col2im_is_the_autograd_gradient_of_unfold_on_the_active_rows(C):
    c = O.col2im_case(C)
    N, cap, shapes = O.COL2IM_N, O.COL2IM_CAP, O.COL2IM_SHAPES
    R = N * cap
    rows = list(O.row_coords(c.row_pix, shapes, cap))
    for view in range(2):
        maps = [torch.zeros(N, C, h, w, dtype=torch.float64, requires_grad=True) for h, w in shapes]
        cols = [F.unfold(m, 3, padding=1) for m in maps]
        loss = sum((cols[l][img, :, pix] * torch.from_numpy(c.dxcol[view * R + r].astype(F64))).sum() for r, img, l, y, x, pix in rows)
        loss.backward()
        for l in range(len(shapes)):
            assert np.abs(maps[l].grad.numpy() - c.ref64[view][l]).max() <= 1e-12
            e32 = np.abs(c.ref32[view][l].astype(F64) - c.ref64[view][l]).max()
            assert e32 <= 9 * 2.0 ** -24 * np.abs(c.ref64[view][l]).max()                   # at most nine addends


def brute_active(pos, neg, N, A, shapes, cap):
    off = O.pix_offsets(shapes)
    P = off[-1]
    row_pix, counts, index = [-1] * (N * cap), [0] * N, []
    per_image = []
    for i in range(N):
        idx, n = [-1] * P, 0
        for q in range(P):
            if any(pos[(i * P + q) * A + a] or neg[(i * P + q) * A + a] for a in range(A)):
                if n < cap:
                    row_pix[i * cap + n], idx[q] = q, i * cap + n
                    n += 1
        counts[i] = n
        per_image.append(idx)
    for l in range(len(shapes)):
        for i in range(N):
            index += per_image[i][off[l]: off[l + 1]]
    return np.array(row_pix, np.int32).reshape(-1), np.array(counts, np.int32), np.array(index, np.int32)


@pytest.mark.parametrize("cap", [0, 1, 3, 40])
def test_active_pixels_np_is_the_brute_force_scan(cap):
    shapes, A, N = [(3, 4), (2, 2), (1, 1)], 2, 2
    P = O.pix_offsets(shapes)[-1]
    pos = (O.uniform("hk:toy:p", (N * P * A,), 0, 1) < 0.2).astype(np.uint8)
    neg = (O.uniform("hk:toy:n", (N * P * A,), 0, 1) < 0.2).astype(np.uint8)
    pos[(P - 1) * A] = 1                                                                    # the single pixel of the last level, image 0
    got, want = O.active_pixels_np(pos, neg, N, A, shapes, cap), brute_active(pos, neg, N, A, shapes, cap)
    assert all(np.array_equal(g, w) and g.dtype == np.int32 for g, w in zip(got, want))
    assert min(O.active_counts(pos, neg, N, A, shapes)) > 3


def test_blocked_layout_helper():
    d = O.uniform("hk:blk", (2, 20, 3, 5))
    b = O.blocked_np(d, 1, 2, halo=O.SENTINEL)
    assert b.shape == (2, 2, 5, 9, 16)
    for c in (0, 15, 16, 19):
        assert np.array_equal(b[:, c // 16, 1:4, 2:7, c % 16], d[:, c])
    assert not b[:, 1, 1:4, 2:7, 4:].any()                                                  # padding channels
    m = O.interior_mask(b.shape, 1, 2)
    assert m.sum() == 2 * 2 * 3 * 5 * 16 and (b[~m] == O.SENTINEL).all()


def test_act_bwd_np_is_torch_where():
    for relu, p in O.ACT_MODES:
        dy, y, draws = O.act_inputs("hk:w", (37, 13), p)
        mask = torch.ones(37, 13, dtype=torch.bool)
        if relu:
            mask &= torch.from_numpy(y) > 0
        if p > 0:
            mask &= torch.from_numpy(draws) >= float(F32(p))
        scaled = torch.from_numpy((dy * O.scale_of(p)).astype(F32)) if p > 0 else torch.from_numpy(dy)
        want = torch.where(mask, scaled, torch.zeros(()))
        dz, db, sabs = O.act_bwd_np(dy, y, draws, p, relu)
        assert np.array_equal(dz, want.numpy()) and np.array_equal(db, want.double().sum(0).numpy()) and np.array_equal(sabs, want.double().abs().sum(0).numpy())
        x = O.uniform("hk:w:x", (37, 13))
        v = torch.relu(torch.from_numpy(x)) if relu else torch.from_numpy(x)
        fw = torch.where(torch.from_numpy(draws) >= float(F32(p)), torch.from_numpy((v.numpy() * O.scale_of(p)).astype(F32)), torch.zeros(())) if p > 0 else v
        assert np.array_equal(O.relu_dropout_np(x, draws, p, relu), fw.numpy())


# ------------------------------------------------------------------------------------------------ case conditions
@pytest.mark.parametrize("pyr,A,which", O.ACTIVE_CASES)
def test_active_pixel_cases_reach_their_branches(pyr, A, which):
    shapes, cap, calls = O.active_case(pyr, A, which)
    off, chunk = O.pix_offsets(shapes), O.chunk_of(shapes)
    P = off[-1]
    assert (P, chunk) == dict(five=(2777, 3), one=(4160, 5), small=(960, 1))[pyr]
    assert pyr != "one" or chunk >= 4
    if pyr == "five":                                        # level edges inside a thread's chunk
        assert [o % chunk for o in off[1:-1]] == [1, 2, 0, 2] and len(shapes) == 5
    (pos, neg), (pos2, neg2) = calls
    counts = O.active_counts(pos, neg, 2, A, shapes)
    assert not np.array_equal(pos[: P * A] | neg[: P * A], pos[P * A:] | neg[P * A:])        # the two images differ
    assert not (np.array_equal(pos, pos2) and np.array_equal(neg, neg2))                     # so do the two calls
    on = (pos.astype(bool) | neg.astype(bool)).reshape(2, P, A).any(2)
    q0 = np.nonzero(on[0])[0]
    if which in "acd":
        assert list(counts) == [11, 2] and list(q0) == O.pixels_a(shapes)
        assert q0[7] // chunk == q0[8] // chunk == O.STRADDLE_THREAD and q0[8] == q0[7] + 1  # the 8th and the 9th share a thread
        assert q0[-1] == P - 1
    if which == "a":
        assert cap == 8 and counts[0] > cap > counts[1] and P - 1 in q0[cap:]                # more than cap; the last pixel is dropped
    elif which == "b":
        assert cap == 8 and list(counts) == [P, P - 2]
    elif which == "c":
        assert cap == 1 and counts.min() > cap
    elif which == "d":
        assert cap == 0
    elif which == "e":
        assert cap == 1100 > O.SCAN_THREADS and list(counts) == [5, 0]                       # the -1 tail is longer than one pass of the block
        assert cap - counts.max() > O.SCAN_THREADS
    else:
        assert len(shapes) == 1 and P < O.SCAN_THREADS and counts.max() <= cap
    row_pix, cnt, index = O.active_pixels_np(pos, neg, 2, A, shapes, cap)
    assert list(cnt) == [min(c, cap) for c in counts] and (index >= 0).sum() == cnt.sum() == (row_pix >= 0).sum()


def test_gather_cases_wrap_their_loops():
    assert [(9 * C > 256, 4 * C > 256, (9 * C) % 256 != 0, (2 * C) % 16) for C in O.GATHER_C] == [(True, True, True, 0), (True, False, True, 0)]
    assert (4 * 72) % 256 != 0 and 8 * 3 < 256 < 8 * O.GATHER_A_WIDE and (8 * O.GATHER_A_WIDE) % 256 != 0
    for A in (3, O.GATHER_A_WIDE):
        row_pix, counts, _ = O.gather_row_pix(A)
        assert list(counts) == [7, 2] and (row_pix < 0).sum() == 2 * O.GATHER_CAP - 9        # zero rows past both counts
        got = {(l, y, x) for _, img, l, y, x, _ in O.row_coords(row_pix, O.GATHER_SHAPES, O.GATHER_CAP) if img == 0}
        assert {(0, 0, 0), (0, 0, 9), (0, 5, 0), (0, 5, 9), (1, 0, 0), (1, 0, 6)} <= got and O.GATHER_SHAPES[1][0] == 1
    c = O.gather_case(72, 3)
    for per_level in (c.hidden, c.left, c.right, c.gz, c.gb):
        assert all(np.abs(m).min() > 0 for m in per_level)                                   # a skipped element cannot pass for a zero
    assert max(2 * O.GATHER_N * O.GATHER_CAP * 9 * 72, O.GATHER_N * O.GATHER_CAP * 8 * O.GATHER_A_WIDE) * 4 < (1 << 20)


def test_col2im_case_sits_on_the_block_edges():
    hw = [h * w for h, w in O.COL2IM_SHAPES]
    assert hw == [256, 257, 5, 1] and [s for s in O.COL2IM_SHAPES if 1 in s] == [(1, 257), (5, 1), (1, 1)]
    c = O.col2im_case(8)
    assert list(c.counts) == [10, 2] and c.counts.max() < O.COL2IM_CAP
    rows = {(img, l, pix) for _, img, l, _, _, pix in O.row_coords(c.row_pix, O.COL2IM_SHAPES, O.COL2IM_CAP)}
    assert {(0, 0, 255), (0, 1, 255), (0, 1, 256), (0, 2, 0), (0, 2, 4), (0, 3, 0), (1, 3, 0)} <= rows
    for C in O.COL2IM_C:
        c = O.col2im_case(C)
        for view in range(2):
            r = c.ref64[view]
            assert r[1][0, :, 0, 254:257].all() and not r[1][0, :, 0, :254].any()            # taps on both sides of the 256-pixel block edge
            assert r[2][0].all() == False and r[2][0, :, :2, 0].all() and r[2][0, :, 3:, 0].all() and not r[2][0, :, 2, 0].any()
            assert r[3].all() and r[0][0, :, 15, 15].all() and r[0][0, :, 7:9, 7].all() and not r[0][1].any()
            assert max(np.abs(m).max() for m in r) > 0
        assert not np.array_equal(c.ref64[0][1], c.ref64[1][1])                              # the views differ: a wrong view shows


@pytest.mark.parametrize("M,N,folds,parts,last", O.ACT_ROWS_CASES)
def test_act_rows_cases_reach_their_splits(M, N, folds, parts, last):
    per, got_parts, got_last = O.rows_split(M, 4)
    assert (got_parts, got_last) == (parts, last) and got_parts <= O.K_MAX_PARTS
    if M >= 65536:
        assert per == {65536: 64, 65537: 68, 69633: 72}[M] and (M == 65536) == (parts == O.K_MAX_PARTS)
    else:
        assert N > 64 and N % 64 == 1 and parts > 1                                           # a second column tile with one live column
    for relu, p in O.ACT_MODES:
        c = O.act_rows_case(M, N, relu, p)
        live = c.dz != 0
        assert p == 0 or ((c.draws == F32(p)) & live).any()                                   # kept draws that equal p exist
        assert (relu == 0 and p == 0) or (~live).any()
        for fold in folds:
            ref, sabs = O.fold_cols(c.db, fold), O.fold_cols(c.sabs, fold)
            bound = O.db_bound(ref, sabs, M * fold)
            assert (bound < 1e-6 * np.abs(ref) + 1e-30).all()                                 # the bound is a few fp32 ulps, no more
            if not c.big:
                continue
            # every row block's partial is positive and outweighs the bound: a dropped or doubled block cannot pass
            part = O.block_partials(c.dz, per).reshape(parts, -1, fold).sum(2)
            assert part.shape == (parts, N // fold) and (part > bound[None, :]).all(), (relu, p, fold, float(part.min()), float(bound.max()))
            assert np.abs(part.sum(0) - ref).max() <= bound.min() * 1e-3


@pytest.mark.parametrize("units,C,H,W,ph,pw,parts", O.ACT_BLOCKED_CASES)
def test_act_blocked_cases_reach_their_splits(units, C, H, W, ph, pw, parts):
    per, got_parts, last = O.rows_split(units * H, 1)
    assert got_parts == parts
    if units * H > 16384:
        assert per == 17 and H % per != 0 and (units * H) % per != 0 and last < per         # the chunks cross unit edges; a ragged last chunk
        assert any((u * H) % per for u in range(1, units))
    else:
        assert per == 16
    for relu in (1, 0):
        c = O.act_blocked_case(units, C, H, W, ph, pw, relu)
        CB = (C + 15) // 16
        assert c.dz_b.shape == (units, CB, H + 2 * ph, W + 2 * pw, 16) and c.db.shape == (CB * 16,)
        assert not c.db[C:].any() and (units * H * W == 1 or np.abs(c.db[:C]).min() > 0)
        dense = np.where(c.y > 0, c.dy, F32(0)) if relu else c.dy
        assert np.array_equal(c.db[:C], dense.astype(F64).sum((0, 2, 3)))
        inside = O.interior_mask(c.dz_b.shape, ph, pw)
        assert not c.dz_b[~inside].any() and (c.dy_b[~inside] == O.SENTINEL).all()
        if units * H > 16384:
            bound = O.db_bound(c.db, c.sabs, units * H * W)[:C]
            rows = c.dz_b.astype(F64).transpose(0, 2, 1, 3, 4)[:, ph: ph + H].reshape(units * H, CB, W + 2 * pw, 16).sum(2).reshape(units * H, CB * 16)
            part = O.block_partials(rows, per)[:, :C]
            assert part.shape == (parts, C) and (part > bound[None, :]).all()


def test_special_values_case():
    c = O.act_special_case()
    dz, db, _ = O.act_bwd_np(c.dy, c.y, c.draws, c.p, 1)
    s = O.scale_of(c.p)
    assert dz[0, 0] == 0 and dz[1, 0] == 0 and dz[0, 1] == F32(c.dy[0, 1] * s) != 0 and dz[1, 1] == F32(c.dy[1, 1] * s) != 0
    assert not np.isfinite(c.dy[c.masked]).any() and not dz[c.masked].any() and not np.signbit(dz[c.masked]).any()
    assert np.isfinite(dz).all() and np.isfinite(db).all()


def test_relu_dropout_cases_wrap_the_grid():
    assert [t > O.RELU_DROPOUT_GRID for t in O.RELU_DROPOUT_TOTALS] == [False, False, False, True]
    assert O.RELU_DROPOUT_TOTALS[-1] % 256 == 1 and {1, 255, 257} <= set(O.RELU_DROPOUT_TOTALS)
    for relu, p in O.RELU_DROPOUT_MODES:
        total = O.RELU_DROPOUT_TOTALS[-1]
        x, draws = O.relu_dropout_case(total, p)
        want = O.relu_dropout_np(x, draws, p, relu)
        tail = slice(O.RELU_DROPOUT_GRID, total)                                              # the second trip of the grid
        assert not np.array_equal(want[0, tail], x[0, tail])                                  # in place: an element left alone shows
        if p > 0:
            kept_at_p = (draws == F32(p)) & (want != 0)
            assert kept_at_p[0, tail].any() and kept_at_p[0, : O.RELU_DROPOUT_GRID].any()
            assert ((draws < F32(p)) & (x > 0))[0, tail].any()

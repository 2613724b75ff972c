"""csrc/srpn_train.hip at the loops the Stereo RPN's real sizes need (C = 256, ~40 000 pyramid pixels) and the feature's own tests never run:
the rank >= cap branch, the wrapped -1 fill, cap = 0 and chunk 3 / 5 of active_pixels_kernel; the `+= 256` wraps of all three gathers of
gather_rows_kernel; the right view alone, one-pixel-wide levels and hw on a 256-pixel block edge in col2im_kernel.

The C entry points are called directly on outputs prefilled with a sentinel (the Python wrappers allocate with torch.empty: a freed buffer
that still holds an earlier correct result would hide a skipped element).  Gathers and the integer bookkeeping are compared exactly with
tests/head_kernels_oracle.py; col2im sums at most nine addends and is held to 2 e32 + 1e-6 max|ref64|, e32 the oracle's own fp32-vs-fp64
difference, with exact zeros wherever the oracle is zero.  No element is excluded.  The cases and the conditions that make them reach their
branches are held on the host by tests/test_head_kernels_oracle_host.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import head_kernels_oracle as O

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def ST():
    from disprcnn_amd.modeling.rpn import srpn_train
    return srpn_train


def LIB():
    from disprcnn_amd import _lib
    return _lib.lib()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cuda(a):
    return torch.tensor(np.asarray(a)).cuda()                # a copy: the cached cases are read-only


def host(t):
    return t.detach().cpu().numpy()


def sentinel(*shape, dtype=torch.float32):
    return torch.full(shape, float(O.SENTINEL) if dtype == torch.float32 else int(O.SENTINEL_I32), dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. active pixels
@pytest.mark.parametrize("pyr,A,which", O.ACTIVE_CASES)
def test_active_pixels_at_every_branch(pyr, A, which):
    shapes, cap, calls = O.active_case(pyr, A, which)
    N, P = 2, O.pix_offsets(shapes)[-1]
    before = O.active_counts(*calls[0], N, A, shapes)
    assert -(-P // O.SCAN_THREADS) == O.chunk_of(shapes) == dict(five=3, one=5, small=1)[pyr]
    assert dict(a=before[0] > cap > 0, b=before.min() > cap, c=before.min() > cap == 1, d=cap == 0, e=cap - before.max() > O.SCAN_THREADS,
                f=before.max() <= cap)[which]
    row_pix, counts, index = sentinel(N * cap, dtype=torch.int32), sentinel(N, dtype=torch.int32), sentinel(N * P, dtype=torch.int32)
    lv = ST().level_table(N, A, 1, cap, shapes)
    for pos, neg in calls:                                   # the second call, on other masks, rewrites the same buffers completely
        p, n = cuda(pos), cuda(neg)
        st = LIB().drc_srpn_active_pixels(C.byref(lv), ptr(p), ptr(n), ptr(row_pix), ptr(counts), ptr(index), stream())
        assert st == 0
        want = O.active_pixels_np(pos, neg, N, A, shapes, cap)
        assert np.array_equal(host(row_pix), want[0]), "row_pix"
        assert np.array_equal(host(counts), want[1]), "counts"
        assert np.array_equal(host(index), want[2]), "index"
        assert want[0].shape == (N * cap,) and list(want[1]) == [min(int(c), cap) for c in O.active_counts(pos, neg, N, A, shapes)]
    if which == "d":
        assert row_pix.numel() == 0 and not host(counts).any() and (host(index) == -1).all()


# ------------------------------------------------------------------------------------------------ 2. gather rows
def gather_levels(c, N, cap, shapes, hidden=False, feats=False, grads=False):
    lv = ST().level_table(N, c.A, c.C, cap, shapes)
    keep = []
    for l in range(len(shapes)):
        if hidden:
            h = cuda(O.blocked_np(c.hidden[l], 0, 0).reshape(-1))          # [N][4C / 16][H][W][16], no halo
            keep.append(h)
            lv.hidden[l], lv.hidden_n_stride[l] = h.data_ptr(), 4 * c.C * shapes[l][0] * shapes[l][1]
        if feats:
            fl, fr = cuda(c.left[l]), cuda(c.right[l])
            keep += [fl, fr]
            lv.left[l], lv.right[l] = fl.data_ptr(), fr.data_ptr()
        if grads:
            gz, gb = cuda(c.gz[l]), cuda(c.gb[l])
            keep += [gz, gb]
            lv.glogits[l], lv.gbbox[l] = gz.data_ptr(), gb.data_ptr()
    return lv, keep


@pytest.mark.parametrize("Cin", O.GATHER_C)
def test_gather_rows_wraps_past_256_columns(Cin):
    A, N, cap, shapes = 3, O.GATHER_N, O.GATHER_CAP, O.GATHER_SHAPES
    c = O.gather_case(Cin, A)
    R = N * cap
    assert 9 * Cin > 256 and (4 * Cin > 256) == (Cin == 72) and 8 * A < 256
    lv, keep = gather_levels(c, N, cap, shapes, hidden=True, feats=True, grads=True)
    rp = cuda(c.row_pix)
    T, X, G = sentinel(R, 4 * Cin), sentinel(2 * R, 9 * Cin), sentinel(R, 8 * A)
    so, sb = cuda(np.array([c.s_obj], F32)), cuda(np.array([c.s_box], F32))
    st = LIB().drc_srpn_gather_rows(C.byref(lv), ptr(rp), ptr(so), ptr(sb), ptr(T), ptr(X), ptr(G), stream())
    assert st == 0
    wT, wX, wG = O.gather_rows_np(c.row_pix, N, A, Cin, cap, shapes, hidden=c.hidden, feats=(c.left, c.right), grads=(c.gz, c.gb), s_obj=c.s_obj,
                                  s_box=c.s_box)
    assert np.array_equal(host(T), wT), "T"
    assert np.array_equal(host(X), wX), "Xcol"
    assert np.array_equal(host(G), wG), "G"
    dead = c.row_pix < 0
    assert dead.sum() == R - 9 and not host(T)[dead].any() and not host(X)[:R][dead].any() and not host(X)[R:][dead].any() and not host(G)[dead].any()
    assert wT[~dead].all() and wG[~dead].all() and (wX[:R][~dead] == 0).any()                # live rows: only Xcol's taps outside the map are zero
    for obj, box in ((so, None), (None, sb)):                # one of the two incoming gradients absent: its columns are zeros
        G1 = sentinel(R, 8 * A)
        st = LIB().drc_srpn_gather_rows(C.byref(lv), ptr(rp), ptr(obj), ptr(box), None, None, ptr(G1), stream())
        assert st == 0
        w1 = O.gather_rows_np(c.row_pix, N, A, Cin, cap, shapes, grads=(c.gz, c.gb), s_obj=None if obj is None else c.s_obj,
                              s_box=None if box is None else c.s_box)[2]
        assert np.array_equal(host(G1), w1) and (w1[:, : 2 * A].any() == (obj is not None)) and (w1[:, 2 * A:].any() == (box is not None))


def test_gather_rows_wide_anchor_axis():
    A, Cin, N, cap, shapes = O.GATHER_A_WIDE, 8, O.GATHER_N, O.GATHER_CAP, O.GATHER_SHAPES
    c = O.gather_case(Cin, A)
    R = N * cap
    assert 8 * A == 264 > 256
    lv, keep = gather_levels(c, N, cap, shapes, grads=True)
    rp = cuda(c.row_pix)
    so, sb = cuda(np.array([c.s_obj], F32)), cuda(np.array([c.s_box], F32))
    G = sentinel(R, 8 * A)
    st = LIB().drc_srpn_gather_rows(C.byref(lv), ptr(rp), ptr(so), ptr(sb), None, None, ptr(G), stream())
    assert st == 0
    wG = O.gather_rows_np(c.row_pix, N, A, Cin, cap, shapes, grads=(c.gz, c.gb), s_obj=c.s_obj, s_box=c.s_box)[2]
    assert np.array_equal(host(G), wG) and wG[c.row_pix >= 0].all() and not host(G)[c.row_pix < 0].any()
    got = ST().gather_rows(rp, N, A, Cin, cap, shapes, grads=([cuda(g) for g in c.gz], [cuda(g) for g in c.gb]), g_obj=so, g_box=sb)
    assert got[0] is None and got[1] is None and np.array_equal(host(got[2]), wG)            # the wrapper hands over the same call


# ------------------------------------------------------------------------------------------------ 3. col2im
def run_col2im(Cin, cap, index, dxcol, mask):
    """both views' maps are handed over whatever the mask: -> [view][level], a view not asked for as None after it is seen untouched"""
    N, shapes = O.COL2IM_N, O.COL2IM_SHAPES
    lv = ST().level_table(N, 1, Cin, cap, shapes)
    maps = [[sentinel(N, Cin, h, w) for h, w in shapes] for view in range(2)]
    for l in range(len(shapes)):
        lv.left[l], lv.right[l] = maps[0][l].data_ptr(), maps[1][l].data_ptr()
    st = LIB().drc_srpn_col2im(C.byref(lv), ptr(dxcol), ptr(index), mask, stream())
    assert st == 0
    for view in range(2):
        if not mask & (1 << view):
            assert all((m == float(O.SENTINEL)).all().item() for m in maps[view]), f"view {view} written under mask {mask}"
            maps[view] = None
    return maps


@pytest.mark.parametrize("Cin", O.COL2IM_C)
def test_col2im_views_and_block_edges(Cin):
    c = O.col2im_case(Cin)
    shapes, cap = O.COL2IM_SHAPES, O.COL2IM_CAP
    assert [h * w for h, w in shapes] == [256, 257, 5, 1]
    index, dx = cuda(c.index), cuda(c.dxcol)
    both, left, right = (run_col2im(Cin, cap, index, dx, m) for m in (3, 1, 2))
    assert left[1] is None and right[0] is None
    for view in range(2):
        for l in range(len(shapes)):
            g, r64, r32 = host(both[view][l]).astype(F64), c.ref64[view][l], c.ref32[view][l]
            e32, err = np.abs(r32 - r64).max(), np.abs(g - r64).max()
            print(f"C {Cin} view {view} level {l}: err {err:.3g} e32 {e32:.3g} max {np.abs(r64).max():.3g}")
            assert err <= 2 * e32 + 1e-6 * np.abs(r64).max()
            assert not g[r64 == 0].any() and np.abs(r64).max() > 0                           # written zeros, not leftovers; every level is active
    for l in range(len(shapes)):                             # a view alone: the bits of the two-view launch
        assert torch.equal(left[0][l], both[0][l]), f"left alone, level {l}"
        assert torch.equal(right[1][l], both[1][l]), f"right alone, level {l}"


def test_col2im_wrapper_single_views():
    """the wrapper's form of a single view: no buffer at all for the other one"""
    Cin = O.COL2IM_C[0]
    c = O.col2im_case(Cin)
    shapes, cap = O.COL2IM_SHAPES, O.COL2IM_CAP
    index, dx = cuda(c.index), cuda(c.dxcol)
    both = run_col2im(Cin, cap, index, dx, 3)
    for want_left in (True, False):
        dl, dr = ST().col2im(dx, index, O.COL2IM_N, 1, Cin, cap, shapes, want_left=want_left, want_right=not want_left)
        assert (dl is None) == (not want_left) and (dr is None) == want_left
        assert all(torch.equal(a, b) for a, b in zip(dl if want_left else dr, both[0 if want_left else 1]))


@pytest.mark.parametrize("mask", [3, 2, 1])
def test_col2im_without_rows_writes_zero_maps(mask):
    N, shapes = O.COL2IM_N, O.COL2IM_SHAPES
    P = O.pix_offsets(shapes)[-1]
    pos = np.ones(N * P, np.uint8)
    _, counts, index = O.active_pixels_np(pos, pos, N, 1, shapes, 0)
    assert not counts.any() and (index == -1).all()
    maps = run_col2im(8, 0, cuda(index), torch.empty(0, 72, device="cuda"), mask)
    for view in range(2):
        assert (maps[view] is not None) == bool(mask & (1 << view))
        for m in maps[view] or []:
            assert not m.any().item()

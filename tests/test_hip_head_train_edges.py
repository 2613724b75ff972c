"""csrc/head_train.hip and the two pack kernels of csrc/linear.hip at the splits and grid wraps the heads' real sizes need (M = ROIs x 196
rows, packed operands past 4 M floats) and the features' own tests never run: rows_per_block_for past its floor and at kMaxParts itself for
both activation-backward kernels, a second column tile with one live column, odd widths and halos of the blocked form, the grid-stride
wrap of relu_dropout_fwd_kernel, linear_pack_kernel and linear_pack_cols_kernel.

The C entry points are called directly on outputs prefilled with a sentinel.  Each case asks the library's own size query for the split it
is built for and asserts it, so a later change of kMaxParts or of a block cap fails the case's precondition instead of letting it miss its
branch.  Elementwise results (dz, y, the packed operands, padding lanes included) are compared exactly with
tests/head_kernels_oracle.py; the bias gradient by a derived bound, per column:

    |db - ref64| <= 2 (2^-24 |ref64| + n 2^-53 sum|dz|),    n = the column's addends (M rows x fold columns; units H W pixels)

The kernels round ONE fp64 sum to fp32 -- half an fp32 ulp of the result -- and an fp64 sum of n addends in any order lies within
(n - 1) 2^-53 sum|dz| of the exact one; the factor 2 is the margin.  For M > 65 536 dy is drawn from [0.5, 2] and
tests/test_head_kernels_oracle_host.py shows that every row block's partial exceeds this bound, so a partial left out or added twice cannot
pass.  No element is excluded.  Measured on an MI355X: db at most 0.47 of its bound (0.00192 against 0.00413 at 65 537 x 5), everything
elementwise bit-equal.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import head_kernels_oracle as O

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def H():
    from disprcnn_amd.modeling import head_ops
    return head_ops


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
    return torch.full(shape, float(O.SENTINEL), dtype=dtype, device="cuda")


def check_db(got, ref64, sabs, addends, what):
    got = np.asarray(got, F64)
    bound = O.db_bound(ref64, sabs, addends)
    err = np.abs(got - ref64)
    k = int(np.argmax(err - bound))
    print(f"{what}: worst err {err[k]:.3g} bound {bound[k]:.3g} (|ref| {abs(ref64[k]):.3g}, {addends} addends)")
    assert got.shape == ref64.shape and np.isfinite(got).all() and (err <= bound).all(), what


# ------------------------------------------------------------------------------------------------ 1. activation backward, row-major
def act_rows(dev, M, N, relu, p, fold, want_db=True):
    dy, y, draws = dev
    nd = LIB().drc_act_bwd_rows_scratch_doubles(M, N) if want_db else 0
    dz, db = sentinel(M, N), (sentinel(N // fold) if want_db else None)
    scr = sentinel(nd, dtype=torch.float64) if want_db else None
    st = LIB().drc_act_bwd_rows(ptr(dy), ptr(y) if relu else None, ptr(draws) if p > 0 else None, float(p), relu, M, N, fold, ptr(dz), ptr(db), ptr(scr), nd,
                                stream())
    assert st == 0
    return dz, db


@pytest.mark.parametrize("relu,p", O.ACT_MODES)
@pytest.mark.parametrize("M,N,folds,parts,last", O.ACT_ROWS_CASES)
def test_act_bwd_rows_at_the_partial_splits(M, N, folds, parts, last, relu, p):
    c = O.act_rows_case(M, N, relu, p)
    nd = LIB().drc_act_bwd_rows_scratch_doubles(M, N)
    assert nd % N == 0 and nd // N == parts == c.parts and M - (parts - 1) * c.per == last and parts <= O.K_MAX_PARTS
    assert (N > 64) == ((M, N) == (260, 65))
    dev = cuda(c.dy), cuda(c.y), cuda(c.draws)
    first = None
    for fold in folds:
        dz, db = act_rows(dev, M, N, relu, p, fold)
        assert np.array_equal(host(dz), c.dz), "dz differs from the fp32 formula"
        check_db(host(db), O.fold_cols(c.db, fold), O.fold_cols(c.sabs, fold), M * fold, f"db {M}x{N} relu {relu} p {p} fold {fold}")
        dz2, db2 = act_rows(dev, M, N, relu, p, fold)
        assert torch.equal(db, db2) and torch.equal(dz, dz2)                                 # the same bits run to run
        first = first if first is not None else dz
    dz3, none = act_rows(dev, M, N, relu, p, 1, want_db=False)
    assert none is None and torch.equal(dz3, first)
    got = H().act_bwd_rows(dev[0], dev[1], dev[2], p, relu, fold=folds[0])
    assert torch.equal(got[0], first)                                                         # the wrapper hands over the same call
    check_db(host(got[1]), O.fold_cols(c.db, folds[0]), O.fold_cols(c.sabs, folds[0]), M * folds[0], "db through the wrapper")


def test_act_bwd_rows_special_values():
    c = O.act_special_case()
    dz, db = act_rows((cuda(c.dy), cuda(c.y), cuda(c.draws)), c.M, c.N, 1, c.p, 1)
    want, ref, sabs = O.act_bwd_np(c.dy, c.y, c.draws, c.p, 1)
    got = host(dz)
    assert got[0, 0] == 0 and got[1, 0] == 0, "-0.0 and 0.0 pass no gradient"
    assert got[0, 1] == want[0, 1] != 0 and got[1, 1] == want[1, 1] != 0, "a positive denormal passes the gradient"
    assert not got[c.masked].any() and not np.signbit(got[c.masked]).any(), "a masked inf / NaN gives an exact 0"
    assert np.array_equal(got, want) and np.isfinite(got).all()
    check_db(host(db), ref, sabs, c.M, "db special values")


# ------------------------------------------------------------------------------------------------ 2. activation backward, blocked
def act_blocked(c, dy, y, dz, want_db=True):
    CB = (c.C + 15) // 16
    nd = LIB().drc_act_bwd_blocked_scratch_doubles(c.units, c.C, c.H) if want_db else 0
    db = sentinel(CB * 16) if want_db else None
    scr = sentinel(nd, dtype=torch.float64) if want_db else None
    st = LIB().drc_act_bwd_blocked(ptr(dy), ptr(y), c.relu, c.units, c.C, c.H, c.W, c.ph, c.pw, ptr(dz), ptr(db), ptr(scr), nd, stream())
    assert st == 0
    return db


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("units,Cn,Hh,W,ph,pw,parts", O.ACT_BLOCKED_CASES)
def test_act_bwd_blocked_at_the_partial_splits(units, Cn, Hh, W, ph, pw, parts, relu):
    c = O.act_blocked_case(units, Cn, Hh, W, ph, pw, relu)
    CB = (Cn + 15) // 16
    nd = LIB().drc_act_bwd_blocked_scratch_doubles(units, Cn, Hh)
    assert nd == parts * CB * 16 and parts == c.parts
    assert (units * Hh > 16384) == (c.per > 16) and (parts, c.per) in ((966, 17), (1, 16), (3, 16), (2, 16))
    dy, y = cuda(c.dy_b.reshape(-1)), cuda(c.y_b.reshape(-1))                                 # their halo holds values the kernel must not read
    dz = sentinel(c.dz_b.size)
    db = act_blocked(c, dy, y, dz)
    got = host(dz).reshape(c.dz_b.shape)
    inside = O.interior_mask(c.dz_b.shape, ph, pw)
    assert np.array_equal(got[inside], c.dz_b[inside]), "dz differs from the fp32 formula on the interior (padding channels: zeros)"
    assert (got[~inside] == O.SENTINEL).all(), "halo written"
    check_db(host(db), c.db, c.sabs, units * Hh * W, f"db blocked {units}x{Cn}x{Hh}x{W} relu {relu}")
    assert not host(db)[Cn:].any()                                                            # the padding channels sum zeros
    dz0 = torch.zeros(c.dz_b.size, device="cuda")                                             # the engine's tensors: a zero halo stays zero
    db2 = act_blocked(c, dy, y, dz0)
    assert np.array_equal(host(dz0).reshape(c.dz_b.shape), c.dz_b) and torch.equal(db, db2)
    dz1 = sentinel(c.dz_b.size)
    assert act_blocked(c, dy, y, dz1, want_db=False) is None and torch.equal(dz1, dz)


# ------------------------------------------------------------------------------------------------ 3. ReLU / dropout forward
@pytest.mark.parametrize("relu,p", O.RELU_DROPOUT_MODES)
@pytest.mark.parametrize("total", O.RELU_DROPOUT_TOTALS)
def test_relu_dropout_forward_past_the_grid(total, relu, p):
    x, draws = O.relu_dropout_case(total, p)
    want = O.relu_dropout_np(x, draws, p, relu)
    assert (total > O.RELU_DROPOUT_GRID) == (total == O.RELU_DROPOUT_TOTALS[-1]) and x.shape == (1, total)
    assert p == 0 or total < 5 or ((draws == F32(p)) & (x > 0) & (want != 0)).any()          # draws equal to p are present and kept
    xd, dd = cuda(x), cuda(draws)
    y = sentinel(1, total)
    st = LIB().drc_relu_dropout_fwd(ptr(xd), ptr(dd) if p > 0 else None, ptr(y), total, float(p), relu, stream())
    assert st == 0 and np.array_equal(host(y), want) and np.array_equal(host(xd), x)
    got = H().relu_dropout(xd, dd, p, relu)                                                   # in place, as the heads call it
    assert got is xd and np.array_equal(host(xd), want)


# ------------------------------------------------------------------------------------------------ 4. the packed GEMM operands
@pytest.mark.parametrize("R,K", O.PACK_SMALL + O.PACK_WRAPPED)
def test_pack_rows_and_pack_cols_are_the_documented_layouts(R, K):
    a = O.pack_case(R, K)
    ad = cuda(a)
    n_rows, n_cols = LIB().drc_linear_packed_floats(R, K), LIB().drc_linear_packed_floats(K, R)
    assert (n_rows, n_cols) == (O.packed_floats(R, K), O.packed_floats(K, R))
    assert (n_rows > O.PACK_GRID_FLOATS) == (n_cols > O.PACK_GRID_FLOATS) == ((R, K) in O.PACK_WRAPPED)
    rows, cols = sentinel(n_rows), sentinel(n_cols)
    assert LIB().drc_linear_pack_rows(ptr(ad), R, K, ptr(rows), stream()) == 0
    assert LIB().drc_linear_pack_cols(ptr(ad), R, K, ptr(cols), stream()) == 0
    want_rows, want_cols = O.pack_rows_np(a), O.pack_cols_np(a)
    assert np.array_equal(host(rows), want_rows), "pack_rows"                                 # padding lanes: exact zeros over the sentinel
    assert np.array_equal(host(cols), want_cols), "pack_cols"
    assert np.count_nonzero(want_rows) == np.count_nonzero(a) == np.count_nonzero(want_cols)
    assert torch.equal(H()._pack_rows(ad), rows) and torch.equal(H()._pack_cols(ad), cols)    # the wrappers hand over the same calls

"""The train step's adjoint kernels held to fp64 (tests/resample_oracle.py) at the edges of their grids, through the C entries:
drc_conv3d_cout1_bwd_data / _bwd_weight, drc_cost_volume_bwd, drc_bilinear_up_blocked_bwd (both branches), drc_avgpool2d_blocked_bwd.

Inputs live in NaN-filled storage wherever the kernel must not read (halos, slack, neighbouring channel blocks, guard bands around dense
arrays, stale scratch); the halo of the classifier's x is zero, which is the engine's contract (for N = 1 x is blocks [1, 3) of a 4-block
NaN tensor; the entry takes packed [N][cb_in] storage, so for N > 1 the NaN sits in the slack and the guard bands).  Outputs go into
sentinel-filled storage, and the sentinel must survive everywhere outside the interior.  tests/test_resample_oracle.py shows on the CPU
that every case's input moves by >= 10x its bound under a plausible kernel mistake.

Bounds (eps = 2^-24; none fitted to what the kernels give; "sum" is the sum of the absolute values of the terms the kernel adds, the value
it accumulates onto included -- it is the first term of the kernel's sum):
  cout1_bwd_data     32 eps sum|w||gy| + 1e-30 per element: 27 products and 27 additions in fp32 (+ 1 onto the old value), 32 taken
  cout1_bwd_weight   1e-5 sum|x||gy| per entry (bn_bwd_reduce's argument: <= ~100 dependent fp32 additions is <= 6e-6).  The depth here is
                     trips per thread + 4 shuffle levels + 4 waves + trips of the finish lane loop + 6 shuffle levels: 17 + 4 + 4 + 16 + 6
                     = 47 at the 1024-block cap (28 x 12x56x56), 47 eps = 2.8e-6 -- the factor stays 1e-5.  |gw| >= 0.2 sum|x||gy| is
                     asserted on the reference, two runs are bit-identical, N = 0 zeroes grad_w
  cost_volume_bwd    Dp eps sum_j|g_j| per element (Dp sequential additions)
  up_bwd, gather     (depth + 2) eps sum: depth = the 64 pixel slots' trip count over the cell's window + 4 shuffle levels + 3 additions
                     from LDS (resample_oracle.up_bwd_gather_depth mirrors the kernel's float32 window); + 2 for the weight product and
                     the addition onto grad_x
  up_bwd, scatter    (contributors + 2) eps sum; atomic order is free: fp64 only, no bit-reproducibility
  avgpool_bwd        4 eps (|old| + |g|/k^2): 1/k^2, the product, the addition

Largest measured error / bound per kernel on an MI355X: cout1_bwd_data 0.20, cout1_bwd_weight 0.013 (of 1e-5 sum|x||gy|), cost_volume_bwd
0.25, up_bwd scatter 0.40, up_bwd gather 0.083, avgpool_bwd 0.25.  Every test prints its figure next to the bound (-s)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resample_oracle as R

pytestmark = pytest.mark.gpu

SENT, NAN, EPS = R.SENT, R.NAN, R.EPS32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release():
    """free the references and hand the freed blocks back to the driver: later modules count allocated bytes"""
    yield
    R.data_case.cache_clear()
    R.weight_case.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _env(dev):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    return E, _lib, _lib.lib(), E._stream_ptr(dev)


def _filled(E, dev, fill, *geom):
    t = E.Blocked(*geom, dev)
    t.storage.fill_(fill)
    return t


def _dense(a, dev, fill=NAN):
    """a flat copy of `a` on the device between two guard bands of `fill`"""
    a = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).flatten()
    whole, view = R.guarded(a.numel(), fill, dev)
    view.copy_(a.to(dev))
    return whole, view


def _say(name, err, bound):
    """largest error / bound over the elements"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    i = int(np.argmax(r)) if r.size else 0
    worst = float(r.flat[i]) if r.size else 0.0
    print(f"[{name}] err {float(err.flat[i]) if r.size else 0.0:.3e}  bound {float(np.broadcast_to(bound, err.shape).flat[i]) if r.size else 0.0:.3e}"
          f"  ({worst:.3g} of it; max err {float(err.max()) if r.size else 0.0:.3e})")
    return worst


# ------------------------------------------------------------------------------------------------ classifier conv, data gradient
@pytest.mark.parametrize("name,n,dims,cb", R.DATA_CASES)
def test_cout1_bwd_data(dev, name, n, dims, cb):
    E, _lib, lib, sp = _env(dev)
    c = R.data_case(name, cb)
    Cn, (D, H, W) = c["C"], dims
    blocks, wraps = R.cout1_data_grid(n, cb, D, H, W)
    assert wraps == (name == "24x56x56") and blocks == min(-(-n * cb * D * H * W * 4 // 256), 8192)
    wp = R.pack_cout1(c["w"], cb)
    if cb == 2:                                                                       # the hand packing is the engine's
        conv_w = torch.from_numpy(c["w"].T.copy()).reshape(1, 32, 3, 3, 3)
        assert torch.equal(torch.from_numpy(wp).view(27, 32), E.pack_weight_cout1(conv_w))
    _, w_dev = _dense(wp, dev)
    _, g_dev = _dense(c["gy"], dev)
    for acc in (0, 1):
        gx = _filled(E, dev, SENT, n, cb * 16, D, H, W, 1, 1, 1)
        old = R.data_old(name, cb, c["dx"].shape) if acc else None
        if acc:
            R.put(gx, old)
        else:
            R.interior(gx).fill_(NAN)
        st = lib.drc_conv3d_cout1_bwd_data(E._ptr(g_dev), E._ptr(w_dev), E._ptr(gx.storage), n, cb, D, H, W, acc, sp)
        _lib.check(st, "drc_conv3d_cout1_bwd_data")
        got = R.get(gx, cb * 16)
        ref = c["dx"] + (old.astype(np.float64) if acc else 0.0)
        bound = 32 * EPS * (c["mag"] + (np.abs(old) if acc else 0.0)) + 1e-30
        assert np.isfinite(got).all() and not got[:, Cn:].any()                       # padded channels: w is zero there
        worst = _say(f"cout1_bwd_data {name} cb={cb} acc={acc} ({blocks} blocks)", np.abs(got[:, :Cn] - ref), bound)
        assert worst <= 1.0
        assert R.outside_keeps(gx, SENT)
        del gx
    # N = 0 touches nothing
    gx = _filled(E, dev, SENT, 1, cb * 16, D, H, W, 1, 1, 1)
    assert lib.drc_conv3d_cout1_bwd_data(E._ptr(g_dev), E._ptr(w_dev), E._ptr(gx.storage), 0, cb, D, H, W, 0, sp) == 0
    assert bool((gx.storage == SENT).all())


# ------------------------------------------------------------------------------------------------ classifier conv, weight gradient
def _x_for_wgrad(E, dev, x):
    """x [N, C, D, H, W] -> (keep-alive, device pointer) of the zero-haloed blocked tensor the kernel reads; NaN everywhere else"""
    N, Cn, D, H, W = x.shape
    cb = (Cn + 15) // 16
    if N == 1:                                                                        # blocks [1, 1 + cb) of a (cb + 2)-block NaN tensor
        base = _filled(E, dev, NAN, 1, (cb + 2) * 16, D, H, W, 1, 1, 1)
        base.view6()[:, 1:1 + cb].zero_()
        R.put(base, x, off=1)
        return base, C.c_void_p(base.storage.data_ptr() + 4 * base.cb_stride)
    t = _filled(E, dev, 0.0, N, Cn, D, H, W, 1, 1, 1)
    t.storage[t.numel:].fill_(NAN)
    R.put(t, x)
    return t, E._ptr(t.storage)


@pytest.mark.parametrize("name,n,dims,want,Cn", [c + (32,) for c in R.WEIGHT_CASES] + [R.WEIGHT_CASES[2] + (Cn,) for Cn in (16, 40)])
def test_cout1_bwd_weight(dev, name, n, dims, want, Cn):
    E, _lib, lib, sp = _env(dev)
    c = R.weight_case(name, Cn)
    D, H, W = dims
    cb = (Cn + 15) // 16
    nvox = n * D * H * W
    blocks, trips, finish, depth = R.cout1_weight_grid(n, D, H, W)
    assert blocks == want == min(-(-nvox // 1024), 1024) and depth * EPS < 1e-5
    assert (np.abs(c["gw"]) >= 0.2 * c["mag"]).all()
    keep, xptr = _x_for_wgrad(E, dev, c["x"])
    _, g_dev = _dense(c["gy"], dev)
    scratch = torch.full((_lib.cout1_wgrad_scratch_floats(cb),), NAN, device=dev)     # stale partials are never read
    runs = []
    for _ in range(2):
        whole, gw = R.guarded(27 * cb * 16, SENT, dev)
        st = lib.drc_conv3d_cout1_bwd_weight(xptr, E._ptr(g_dev), E._ptr(gw), n, cb, D, H, W, E._ptr(scratch), sp)
        _lib.check(st, "drc_conv3d_cout1_bwd_weight")
        assert R.guards_keep(whole, SENT)
        runs.append(gw.cpu().view(27, cb * 16))
    assert torch.equal(runs[0], runs[1]), "not reproducible run to run"
    got = runs[0].double().numpy()
    assert not got[:, Cn:].any()
    worst = _say(f"cout1_bwd_weight nvox={nvox} C={Cn} ({blocks} blocks, {trips} trips, finish {finish}, depth {depth})",
                 np.abs(got[:, :Cn] - c["gw"]), 1e-5 * c["mag"] + 1e-300)
    assert worst <= 1.0
    if name != "cap":                                                                 # the mapping of modeling/psmnet/train.py
        wt = torch.zeros(1, Cn, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv3d(torch.from_numpy(c["x"]).double(), wt, None, 1, 1).backward(torch.from_numpy(c["gy"]).double()[:, None])
        mapped = runs[0][:, :Cn].t().reshape(wt.shape).double()
        bar = 1e-5 * torch.from_numpy(c["mag"])[:, :Cn].t().reshape(wt.shape)
        assert bool(((mapped - wt.grad).abs() <= bar).all()), "gw[:, :C].t().reshape(conv.weight.shape) is not conv.weight.grad"
    # N = 0 zeroes grad_w
    whole, gw = R.guarded(27 * cb * 16, SENT, dev)
    assert lib.drc_conv3d_cout1_bwd_weight(xptr, E._ptr(g_dev), E._ptr(gw), 0, cb, D, H, W, E._ptr(scratch), sp) == 0
    assert not gw.cpu().any() and R.guards_keep(whole, SENT)
    del keep


# ------------------------------------------------------------------------------------------------ cost volume
@pytest.mark.parametrize("shape", R.CV_SHAPES)
@pytest.mark.parametrize("mx,mn", R.CV_RANGES)
def test_cost_volume_bwd(dev, mx, mn, shape):
    E, _lib, lib, sp = _env(dev)
    N, Cn, Hp, Wp = shape
    lo4, hi4, Dp0 = R.cv_args(mx, mn)
    assert Dp0 == hi4 - lo4
    per = N * Cn * Hp * Wp
    for Dp in (Dp0, Dp0 + 2):                                                         # the second call: two surplus slices, to be ignored
        g = R.cv_grad(mx, mn, shape, Dp, positive=Dp > Dp0)
        _, g_dev = _dense(g, dev)
        wl, gl = R.guarded(per, SENT, dev)
        wr, gr = R.guarded(per, SENT, dev)
        st = lib.drc_cost_volume_bwd(E._ptr(g_dev), E._ptr(gl), E._ptr(gr), N, Cn, Dp, Hp, Wp, lo4, hi4, sp)
        _lib.check(st, "drc_cost_volume_bwd")
        rl, rr, ml, mr = R.cost_volume_bwd(g, lo4, hi4, Dp)
        got = np.stack([gl.cpu().double().numpy().reshape(shape), gr.cpu().double().numpy().reshape(shape)])
        worst = _say(f"cost_volume_bwd ({mx},{mn}) {shape} Dp={Dp}", np.abs(got - np.stack([rl, rr])), Dp * EPS * np.stack([ml, mr]) + 1e-300)
        assert worst <= 1.0 and R.guards_keep(wl, SENT) and R.guards_keep(wr, SENT)
        if Dp > Dp0:                                                                  # the forward on the same arguments: zeros there, and adjoint
            L, Rt = R.uniform(f"cvL{shape}", shape, 0.5, 1.5), R.uniform(f"cvR{shape}", shape, 0.5, 1.5)
            _, l_dev = _dense(L, dev)
            _, r_dev = _dense(Rt, dev)
            wc, cost = R.guarded(N * 2 * Cn * Dp * Hp * Wp, SENT, dev)
            _lib.check(lib.drc_cost_volume_fwd(E._ptr(l_dev), E._ptr(r_dev), E._ptr(cost), N, Cn, Dp, Hp, Wp, lo4, hi4, sp), "drc_cost_volume_fwd")
            cost = cost.cpu().numpy().reshape(N, 2 * Cn, Dp, Hp, Wp)
            assert np.array_equal(cost, R.cost_volume_fwd(L, Rt, lo4, hi4, Dp)) and not cost[:, :, Dp0:].any() and R.guards_keep(wc, SENT)
            lhs = float((cost.astype(np.float64) * g).sum())
            rhs = float((L.astype(np.float64) * got[0]).sum() + (Rt.astype(np.float64) * got[1]).sum())
            print(f"[cost_volume adjoint ({mx},{mn}) {shape}] <fwd, g> {lhs:.9e}  <L, gL> + <R, gR> {rhs:.9e}  rel {abs(lhs - rhs) / lhs:.2e}")
            assert lhs > 0 and abs(lhs - rhs) <= 1e-6 * lhs
    # N = 0 touches nothing
    wl, gl = R.guarded(16, SENT, dev)
    assert lib.drc_cost_volume_bwd(E._ptr(g_dev), E._ptr(gl), E._ptr(gl), 0, Cn, Dp0, Hp, Wp, lo4, hi4, sp) == 0
    assert bool((wl == SENT).all())


# ------------------------------------------------------------------------------------------------ SPP adjoints
@pytest.mark.parametrize("ihw,ohw", R.UP_BWD_SCATTER + R.UP_BWD_GATHER)
def test_bilinear_up_bwd(dev, ihw, ohw):
    """g is channel blocks [2, 4) of a 5-block tensor (halo 1), grad_x blocks [1, 3) of a 4-block one, holding nonzero values"""
    E, _lib, lib, sp = _env(dev)
    (IH, IW), (OH, OW) = ihw, ohw
    g, old = R.up_bwd_inputs(ihw, ohw)
    gather = R.up_bwd_takes_gather(IH, IW, OH, OW, 2 * 2 * IH * IW)
    assert gather == ((ihw, ohw) in R.UP_BWD_GATHER) == (OH * OW >= 4 * IH * IW)
    gcat = _filled(E, dev, NAN, 2, 80, 1, OH, OW, 0, 1, 1)
    R.put(gcat, g[:, :, None], off=2)
    gsl = E.BlockedSlice(gcat, 2, 32)
    gbase = _filled(E, dev, SENT, 2, 64, 1, IH, IW, 0, 1, 1)
    R.put(gbase, old[:, :, None], off=1)
    gx = E.BlockedSlice(gbase, 1, 32)
    st = lib.drc_bilinear_up_blocked_bwd(E._ptr(gsl.storage), E._geom8(gsl), E._ptr(gx.storage), E._geom8(gx), sp)
    _lib.check(st, "drc_bilinear_up_blocked_bwd")
    ref, mag, cnt = R.bilinear_bwd(g, IH, IW, True)
    terms = R.up_bwd_gather_depth(IH, IW, OH, OW) if gather else cnt
    bound = (terms + 2) * EPS * (mag + np.abs(old))
    got = R.get(gbase, 32, off=1)[:, :, 0]
    worst = _say(f"up_bwd {ihw}->{ohw} {'gather' if gather else 'scatter'} (terms <= {int(terms.max())})", np.abs(got - (ref + old)), bound)
    assert np.isfinite(got).all() and worst <= 1.0
    assert R.outside_keeps(gbase, SENT, off=1, cb=2)


@pytest.mark.parametrize("hw,k", R.AVG_BWD_CASES)
def test_avgpool_bwd(dev, hw, k):
    """grad_x is channel blocks [1, 3) of a 4-block tensor with halo 2; the remainder rows and columns keep their values exactly"""
    E, _lib, lib, sp = _env(dev)
    H, W = hw
    g, old = R.avg_bwd_inputs(hw, k)
    gp = _filled(E, dev, NAN, 2, 32, 1, H // k, W // k, 0, 0, 0)
    R.put(gp, g[:, :, None])
    gbase = _filled(E, dev, SENT, 2, 64, 1, H, W, 0, 2, 2)
    R.put(gbase, old[:, :, None], off=1)
    gs = E.BlockedSlice(gbase, 1, 32)
    st = lib.drc_avgpool2d_blocked_bwd(E._ptr(gp.storage), E._geom8(gp), E._ptr(gs.storage), E._geom8(gs), k, sp)
    _lib.check(st, "drc_avgpool2d_blocked_bwd")
    ref = R.avgpool_bwd(g, k, H, W)
    got = R.get(gbase, 32, off=1)[:, :, 0]
    worst = _say(f"avgpool_bwd {hw} k={k}", np.abs(got - (ref + old)), 4 * EPS * (np.abs(old) + np.abs(ref)))
    assert worst <= 1.0
    assert np.array_equal(got[:, :, H // k * k:], old[:, :, H // k * k:].astype(np.float64))
    assert np.array_equal(got[:, :, :, W // k * k:], old[:, :, :, W // k * k:].astype(np.float64))
    assert R.outside_keeps(gbase, SENT, off=1, cb=2)

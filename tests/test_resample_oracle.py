"""tests/resample_oracle.py pinned to torch-CPU in float64 (1e-12; the bilinear references to what their float32 source coordinates
allow), its launch mirrors pinned to the grids the GPU cases are named for, and -- for every case of tests/test_hip_train_adjoints.py and
tests/test_hip_resample.py -- the proof that the case's input is strong enough: plausible kernel mistakes (taps not flipped, a shift by one
column, the last row or column dropped, remainder rows pooled, 1/k^2 missing, align_corners swapped, the two halves of the cost volume
swapped, dead slices summed, a zero start value of the maximum) move the reference by >= 10x the case's bound.  A mistake a geometry cannot
show (an identity resize, a 1-voxel map) must leave the reference exactly unchanged; every case needs at least one that clears 10x."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psmnet_oracle as O
from tests import resample_oracle as R

T64 = torch.float64


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _strong(name, ref, bound, mutants):
    """every mistake is invisible (exactly 0) or >= 10x the bound somewhere; at least one clears"""
    best = 0.0
    for mname, mut in mutants.items():
        m = R.margin(ref, mut, bound)
        print(f"[{name}] {mname}: {m:.3g}x the bound")
        assert m == 0.0 or m >= 10.0, f"{name}: input too weak for mistake {mname!r} ({m:.3g}x)"
        best = max(best, m)
    assert best >= 10.0, f"{name}: no mistake clears 10x the bound"


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("n,dims,C", [(2, (5, 9, 13), 40), (1, (1, 1, 1), 16), (2, (3, 4, 2), 32)])
def test_cout1_adjoints_vs_autograd(n, dims, C):
    w = R.uniform(f"pin:w{dims}", (27, C))
    x = R.uniform(f"pin:x{dims}", (n, C) + dims)
    gy = R.uniform(f"pin:g{dims}", (n,) + dims)
    xt = torch.from_numpy(x).to(T64).requires_grad_()
    wt = torch.from_numpy(w.T.copy()).to(T64).reshape(1, C, 3, 3, 3).requires_grad_()          # conv.weight[0, c, kd, kh, kw] = w[t, c]
    F.conv3d(xt, wt, None, 1, 1).backward(torch.from_numpy(gy).to(T64)[:, None])
    dx, mag = R.cout1_bwd_data(w, gy)
    gw, magw = R.cout1_bwd_weight(x, gy)
    assert _rel(dx, xt.grad.numpy()) <= 1e-12
    assert (mag >= np.abs(dx) - 1e-12).all() and (magw >= np.abs(gw) - 1e-12).all()
    # the mapping of modeling/psmnet/train.py: gw[:, :C].t().reshape(conv.weight.shape)
    mapped = torch.from_numpy(gw)[:, :C].t().reshape(wt.shape)
    assert _rel(mapped.numpy(), wt.grad.numpy()) <= 1e-12
    # the magnitude sums are the same sums of absolute values
    assert _rel(mag, R.cout1_bwd_data(np.abs(w), np.abs(gy))[0]) <= 1e-12
    assert _rel(magw, R.cout1_bwd_weight(np.abs(x), np.abs(gy))[0]) <= 1e-12


def test_pack_cout1_matches_the_engine():
    from disprcnn_amd import engine as E
    w = R.uniform("pin:pack", (27, 32))
    conv_w = torch.from_numpy(w.T.copy()).reshape(1, 32, 3, 3, 3)
    assert np.array_equal(R.pack_cout1(w, 2).reshape(27, 32), E.pack_weight_cout1(conv_w).numpy())
    p3 = R.pack_cout1(R.uniform("pin:pack3", (27, 40)), 3)
    assert p3.shape == (27, 3, 16) and not p3[:, 2, 8:].any()


@pytest.mark.parametrize("shape", R.CV_SHAPES)
@pytest.mark.parametrize("mx,mn", R.CV_RANGES)
def test_cost_volume_vs_oracle_autograd(mx, mn, shape):
    lo4, hi4, Dp = R.cv_args(mx, mn)
    L, Rt = R.uniform(f"pin:cvL{shape}", shape), R.uniform(f"pin:cvR{shape}", shape)
    assert np.array_equal(R.cost_volume_fwd(L, Rt, lo4, hi4, Dp), O.cost_volume(torch.from_numpy(L), torch.from_numpy(Rt), mx, mn).numpy())
    g = R.cv_grad(mx, mn, shape, Dp)
    lt, rt = torch.from_numpy(L).to(T64).requires_grad_(), torch.from_numpy(Rt).to(T64).requires_grad_()
    (O.cost_volume(lt * 1.0, rt * 1.0, mx, mn) * torch.from_numpy(g).to(T64)).sum().backward()
    gl, gr, ml, mr = R.cost_volume_bwd(g, lo4, hi4, Dp)
    assert _rel(gl, lt.grad.numpy()) <= 1e-12 and _rel(gr, rt.grad.numpy()) <= 1e-12
    al, ar, _, _ = R.cost_volume_bwd(np.abs(g), lo4, hi4, Dp)
    assert _rel(ml, al) <= 1e-12 and _rel(mr, ar) <= 1e-12
    # surplus slices (Dp = hi4 - lo4 + 2) are ignored by the adjoint and zero in the forward
    g2 = R.cv_grad(mx, mn, shape, hi4 - lo4 + 2)
    g2[:, :, :Dp] = g[:, :, :hi4 - lo4]
    assert all(np.array_equal(a, b) for a, b in zip(R.cost_volume_bwd(g2, lo4, hi4, hi4 - lo4 + 2), R.cost_volume_bwd(g, lo4, hi4, Dp)))
    assert not R.cost_volume_fwd(L, Rt, lo4, hi4, hi4 - lo4 + 2)[:, :, hi4 - lo4:].any()


@pytest.mark.parametrize("hw,k", [((9, 7), 2), ((9, 7), 4), ((8, 8), 8), ((66, 130), 64), ((56, 72), 1)])
def test_avgpool_vs_torch(hw, k):
    x = R.pool_input(f"pin:ap{hw}{k}", (2, 3) + hw)
    xt = torch.from_numpy(x).to(T64).requires_grad_()
    y = F.avg_pool2d(xt, k, k)
    g = R.uniform(f"pin:apg{hw}{k}", tuple(y.shape))
    y.backward(torch.from_numpy(g).to(T64))
    ref, mag = R.avgpool(x, k)
    assert ref.shape == tuple(y.shape) and _rel(ref, y.detach().numpy()) <= 1e-12 and _rel(mag, ref) <= 1e-12      # positive input
    assert _rel(R.avgpool_bwd(g, k, *hw), xt.grad.numpy()) <= 1e-12


def _coord_err(I):
    """|float32 source coordinate - exact| <= 4 * 2^-24 * I: the scale's rounding, the product's, and for align_corners = 0 the two
    additions of 0.5, each relative to a coordinate <= I"""
    return 4 * R.EPS32 * I


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("ihw,ohw", sorted(set(R.UP_FWD + R.RESIZE_FWD + R.UP_BWD_SCATTER + R.UP_BWD_GATHER)))
def test_bilinear_vs_torch(ihw, ohw, align):
    """Limit from the coordinates: the interpolant moves by at most (max - min of the input) per unit of either coordinate, a float32
    coordinate is within _coord_err of the exact one, 1 - t adds one float32 rounding per axis.  The adjoint: the same per weight, times
    the fine pixels under one coarse cell's hat (2 / scale + 1 per axis), times max |g|."""
    x = R.uniform(f"pin:bl{ihw}{ohw}", (2, 3) + ihw)
    xt = torch.from_numpy(x).to(T64).requires_grad_()
    y = F.interpolate(xt, ohw, mode="bilinear", align_corners=align)
    g = R.uniform(f"pin:blg{ihw}{ohw}", tuple(y.shape))
    y.backward(torch.from_numpy(g).to(T64))
    dw = _coord_err(ihw[0]) + _coord_err(ihw[1]) + 2 * R.EPS32
    ref, mag = R.bilinear(x, *ohw, align)
    lim = dw * float(x.max() - x.min() + np.abs(x).max()) + 1e-12
    err = float(np.abs(ref - y.detach().numpy()).max())
    print(f"[bilinear {ihw}->{ohw} align={align}] fwd off by {err:.3e}, coordinates allow {lim:.3e}")
    assert err <= lim and (mag >= np.abs(ref) - 1e-12).all()
    cnt = [min(o, int(2 * o / max(i - 1, 1)) + 2) for i, o in zip(ihw, ohw)]
    gref, gmag, n = R.bilinear_bwd(g, *ihw, align)
    glim = cnt[0] * cnt[1] * dw * float(np.abs(g).max()) + 1e-12
    gerr = float(np.abs(gref - xt.grad.numpy()).max())
    print(f"[bilinear {ihw}->{ohw} align={align}] adjoint off by {gerr:.3e}, coordinates allow {glim:.3e}")
    assert gerr <= glim and n.max() <= cnt[0] * cnt[1]
    # <fwd(x), g> == <x, bwd(g)> in fp64
    assert abs((ref * g).sum() - (x * gref).sum()) <= 1e-12 * max(1.0, abs((ref * g).sum()))


@pytest.mark.parametrize("k,s,hw", R.MAXPOOL_CASES + [(3, 2, (7, 8)), (2, 2, (5, 6))])
def test_maxpool_vs_torch(k, s, hw):
    x = R.uniform(f"pin:mp{hw}", (2, 3) + hw, -2.0, -0.5)
    ref = F.max_pool2d(torch.from_numpy(x), k, s, 0, ceil_mode=True).numpy()
    got = R.maxpool(x, k, s)
    assert got.shape == ref.shape == (2, 3, R.maxpool_out(hw[0], k, s), R.maxpool_out(hw[1], k, s)) and np.array_equal(got, ref)


def test_launch_mirrors():
    for name, n, dims, cb in R.DATA_CASES:
        blocks, wraps = R.cout1_data_grid(n, cb, *dims)
        assert wraps == (name == "24x56x56") and (blocks == 8192) == wraps
    assert R.cout1_data_grid(1, 1, 1, 1, 1)[0] == 1
    depth = {}
    for name, n, dims, want in R.WEIGHT_CASES:
        blocks, trips, finish, depth[name] = R.cout1_weight_grid(n, *dims)
        assert blocks == want and n * dims[0] * dims[1] * dims[2] == {"5": 5, "1024": 1024, "1025": 1025, "65k+3": 65 * 1024 + 3}.get(name, 1053696)
        assert finish == (2 if name == "65k+3" else 16 if name == "cap" else 1)
    # capped case: 17 trips per thread, 16 of the finish lane loop: 47 dependent additions, 47 * 2^-24 = 2.8e-6 < 1e-5
    assert R.cout1_weight_grid(28, 12, 56, 56)[1] == 17 and max(depth.values()) == 47 and 47 * R.EPS32 < 1e-5
    for (i, o) in R.UP_BWD_SCATTER:
        assert not R.up_bwd_takes_gather(*i, *o, 100)
    for (i, o) in R.UP_BWD_GATHER:
        assert R.up_bwd_takes_gather(*i, *o, 100)
        d = R.up_bwd_gather_depth(*i, *o)
        assert d.shape == i and d.min() >= 8 and d.max() <= -(-o[0] * o[1] // 64) + 7
    assert int(R.up_bwd_gather_depth(1, 1, 56, 72)[0, 0]) == 63 + 7


# ------------------------------------------------------------------------------------------------ every GPU case: is its input strong enough?
@pytest.mark.parametrize("name,n,dims,cb", R.DATA_CASES)
def test_strong_cout1_bwd_data(name, n, dims, cb):
    c = R.data_case(name, cb)
    for acc in (0, 1):
        old = R.data_old(name, cb, c["dx"].shape) if acc else 0.0
        ref = c["dx"] + old
        bound = 32 * R.EPS32 * (c["mag"] + np.abs(old)) + 1e-30
        mut = {"shift by one column": R.shift_col(c["dx"]) + old, "last column dropped": R.drop_last_col(c["dx"]) + old}
        if acc == 0 and n * dims[0] * dims[1] * dims[2] < 50000:
            mut["taps not flipped"] = R.cout1_bwd_data(c["w"], c["gy"], flip=False)[0]
        if acc:
            mut["not accumulated"] = c["dx"]
        _strong(f"bwd_data {name} cb={cb} acc={acc}", ref, bound, mut)


def _weight_tail(n, dims):
    """the voxels behind the last full grid stride (or the last trip of 64, or the last voxel) as a gy mask of the LAST sample"""
    nvox, per = n * dims[0] * dims[1] * dims[2], dims[0] * dims[1] * dims[2]
    stride = R.cout1_weight_grid(n, *dims)[0] * 64
    full = nvox // stride * stride
    start = full if 0 < full < nvox else max(nvox - 64, nvox // 2)
    assert nvox - start <= per
    mask = np.zeros(per, bool)
    mask[per - (nvox - start):] = True
    return mask.reshape(dims)


@pytest.mark.parametrize("name,n,dims,blocks,C", [c + (32,) for c in R.WEIGHT_CASES] + [R.WEIGHT_CASES[2] + (C,) for C in (16, 40)])
def test_strong_cout1_bwd_weight(name, n, dims, blocks, C):
    c = R.weight_case(name, C)
    assert (np.abs(c["gw"]) >= 0.2 * c["mag"]).all()
    tail = R.cout1_bwd_weight(c["x"][-1:], (c["gy"][-1] * _weight_tail(n, dims))[None])[0]
    kw_swapped = c["gw"].reshape(3, 3, 3, -1)[:, :, ::-1].reshape(27, -1)
    _strong(f"bwd_weight {name}", c["gw"], 1e-5 * c["mag"] + 1e-300,
            {"taps not flipped": c["gw"][::-1], "kw not flipped": kw_swapped, "remainder dropped": c["gw"] - tail})


@pytest.mark.parametrize("shape", R.CV_SHAPES)
@pytest.mark.parametrize("mx,mn", R.CV_RANGES)
@pytest.mark.parametrize("surplus", [0, 2])
def test_strong_cost_volume_bwd(mx, mn, shape, surplus):
    lo4, hi4, _ = R.cv_args(mx, mn)
    Dp = hi4 - lo4 + surplus
    g = R.cv_grad(mx, mn, shape, Dp, positive=bool(surplus))
    gl, gr, ml, mr = R.cost_volume_bwd(g, lo4, hi4, Dp)
    ref, bound = np.stack([gl, gr]), Dp * R.EPS32 * np.stack([ml, mr]) + 1e-300
    mut = {"shift by one column": np.stack(R.cost_volume_bwd(g, lo4, hi4, Dp, shift=1)[:2]),
           "halves swapped": np.stack(R.cost_volume_bwd(g, lo4, hi4, Dp, swap=True)[:2]),
           "dead slices summed": np.stack(R.cost_volume_bwd(g, lo4, hi4, Dp, dead=True)[:2]),
           "last column dropped": R.drop_last_col(ref)}
    _strong(f"cost_volume_bwd ({mx},{mn}) {shape} Dp={Dp}", ref, bound, mut)
    if surplus and max(abs(hi4), abs(hi4 + 1)) < shape[3]:                           # a dead slice's shift still lands inside the row
        assert R.margin(ref, mut["dead slices summed"], bound) >= 10.0


@pytest.mark.parametrize("ihw,ohw", R.UP_BWD_SCATTER + R.UP_BWD_GATHER)
def test_strong_bilinear_up_bwd(ihw, ohw):
    g, old = R.up_bwd_inputs(ihw, ohw)
    ref, mag, cnt = R.bilinear_bwd(g, *ihw, True)
    terms = R.up_bwd_gather_depth(*ihw, *ohw) if (ihw, ohw) in R.UP_BWD_GATHER else cnt
    bound = (terms + 2) * R.EPS32 * (mag + np.abs(old))
    _strong(f"up_bwd {ihw}->{ohw}", ref + old, bound,
            {"align_corners swapped": R.bilinear_bwd(g, *ihw, False)[0] + old, "shift by one column": R.shift_col(ref) + old,
             "last column dropped": R.drop_last_col(ref) + old, "last row dropped": R.drop_last_row(ref) + old, "not accumulated": ref})


@pytest.mark.parametrize("hw,k", R.AVG_BWD_CASES)
def test_strong_avgpool_bwd(hw, k):
    g, old = R.avg_bwd_inputs(hw, k)
    ref = R.avgpool_bwd(g, k, *hw)
    bound = 4 * R.EPS32 * (np.abs(old) + np.abs(ref))
    _strong(f"avgpool_bwd {hw} k={k}", ref + old, bound,
            {"remainder rows pooled": R.avgpool_bwd(g, k, *hw, remainder=True) + old, "1/k^2 missing": R.avgpool_bwd(g, k, *hw, scale=False) + old,
             "shift by one column": R.shift_col(ref) + old, "last row dropped": R.drop_last_row(ref) + old})


@pytest.mark.parametrize("k,hw", R.AVG_CASES)
@pytest.mark.parametrize("half", [False, True])
def test_strong_avgpool(k, hw, half):
    x = R.pool_input(f"ap:{hw}", (2, 32) + hw)
    x = R.half(x) if half else x
    ref, mag = R.avgpool(x, k)
    bound = R.avgpool_bound(k, mag)
    bound = R.f16_bound(ref, bound) if half else bound
    moved = np.zeros_like(x)
    moved[..., :-1] = x[..., 1:]
    mut = {"window moved by one column": R.avgpool(moved, k)[0], "1/k^2 missing": R.avgpool(x, k, scale=False)[0],
           "remainder rows pooled": R.avgpool(x, k, remainder=True)[0], "shift by one column": R.shift_col(ref)}
    _strong(f"avgpool k={k} {hw} half={half}", ref, bound, mut)

@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("align,ihw,ohw", [(True, i, o) for i, o in R.UP_FWD] + [(False, i, o) for i, o in R.RESIZE_FWD]
                         + [(True, i, o) for i, o in R.RESIZE_FWD])
def test_strong_bilinear(align, ihw, ohw, half):
    if half and (not align or (ihw, ohw) not in R.UP_FWD):
        return                                                                      # the fp16 kernel has align_corners = 1 only
    x = R.uniform(f"bl:{ihw}{ohw}", (2, 32) + ihw)
    x = R.half(x) if half else x
    ref, mag = R.bilinear(x, *ohw, align)
    bound = R.bilinear_bound(mag) + 1e-300
    bound = R.f16_bound(ref, bound) if half else bound
    _strong(f"bilinear {ihw}->{ohw} align={align} half={half}", ref, bound,
            {"align_corners swapped": R.bilinear(x, *ohw, not align)[0], "shift by one column": R.shift_col(ref),
             "last column dropped": R.drop_last_col(ref), "last row dropped": R.drop_last_row(ref)})


@pytest.mark.parametrize("k,s,hw", R.MAXPOOL_CASES)
def test_strong_maxpool(k, s, hw):
    x = R.uniform(f"mp:{hw}", (2, 32) + hw, -2.0, -0.5)
    ref = R.maxpool(x, k, s)
    assert (ref < 0).all()
    _strong(f"maxpool k={k} s={s} {hw}", ref, 0.0, {"zero start value": R.maxpool(x, k, s, start=0.0), "ragged windows dropped": R.maxpool(x, k, s, clip=False),
                                                   "shift by one column": R.shift_col(ref)})

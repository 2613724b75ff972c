"""The weight-gradient kernels behind drc_tapconv_wgrad -- wgrad_slide_kernel<13 / 14 / 16 / 0>, wgrad_kernel<1 / 2 / 4 / 9 / 49>,
wgrad_reduce_kernel and the atomicAdd flush -- held to the fp64 reference of tests/wgrad_oracle.py at every tile and flush edge.  The
cases, and what each is there for, are in tests/wgrad_oracle.py; tests/test_wgrad_host.py shows on the CPU that each case reaches its
branch and that a plausible kernel mistake cannot hide in it.

Storage.  `a` is an engine.Blocked with a zero halo (the engine's contract: the taps read it) whose slack -- and, where `a` is a prefix
view of a larger pool tensor, the units behind it -- hold the finite integer 4096: the generic kernel stages a ragged last tile without
clamping and multiplies what it over-read by b = 0, so the poison must contribute exactly nothing.  (Finite on purpose: 0 * NaN is NaN,
the kernels' contract is a finite slack.)  b's halo and slack and the whole partial-sum scratch are NaN before every call: ragged b slots
are removed by a select, and the reduce must read only what this launch wrote.  gw lies between two guard bands that must survive; it
starts as NaN (overwrite = 1) or as known integers (overwrite = 0).

Integer cases: a and b are integers in -3..3, so every product and every partial sum is an integer below 2^24, which fp32, the MFMA
accumulator, the fixed-order reduce and atomicAdd in any order all carry exactly.  The result must EQUAL the reference on every element,
the padded channel rows (zero) included.  No tolerance.

Real-valued cases: the same shapes with uniform(-1, 1).  Per element |got - ref| <= depth * 2^-24 * sum|a||b| + 1e-30, where depth is the
number of dependent fp32 roundings behind one element, taken from wgrad_oracle.launch_model and never fitted:
    1                                   the product
  + 4 * k-steps * work items per wave   one accumulator tile of a wave: an MFMA 16x16x4 step adds four products onto it; k-steps = ceil(R *
                                        WT / 4) per group (generic kernel) or per depth slice of a (column, segment) unit (slide kernel: x
                                        seglen); work items per wave = ceil(groups or units / waves), masked slots counted
  + ceil(waves / 4) + 3                 wgrad_reduce_kernel: a thread's run over its quarter of the waves, then three additions across the
                                        quarters
  or + waves                            the atomicAdd flush: one addition per wave, in any order -- there the number of terms of the sum
                                        (N * OD * OH * OW) is used if it is smaller
  + 1                                   overwrite = 0: the addition onto the old value (|old| joins the magnitude sum)
A ratio above 1 is a failure to investigate, not a reason to widen the factor.  Two partial-sum runs are bit-identical.

Largest measured error / bound per kernel form on an MI355X (every test prints its own with -s; the module prints this table at its end):
  wgrad_slide_kernel<0>   + reduce 0.10    + atomicAdd 0.65 (S1: two terms per element, so the bound is 2 * 2^-24 * sum)
  wgrad_slide_kernel<13>  + reduce 0.013   + atomicAdd 0.013
  wgrad_slide_kernel<14>  + reduce 0.0041  + atomicAdd 0.0039
  wgrad_slide_kernel<16>  + reduce 0.0064  + atomicAdd 0.0063
  wgrad_kernel<1>         + reduce 0.043   + atomicAdd 0.046
  wgrad_kernel<2>         + reduce 0.067   + atomicAdd 0.052
  wgrad_kernel<4>         + reduce 0.026   + atomicAdd 0.022
  wgrad_kernel<9>         + reduce 0.096   + atomicAdd 0.14
  wgrad_kernel<49>        + reduce 0.032   + atomicAdd 0.032
(the atomicAdd figures are the larger of two runs: the order of the additions is free and the figure moves with it)
Every integer case was exact on every flush; no bound had to be corrected and no kernel was found wrong.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from tests import resample_oracle as R
from tests import wgrad_oracle as O

pytestmark = pytest.mark.gpu

SENT, NAN = O.SENT, O.NAN
WORST = {}                                # kernel form -> largest error / bound seen by this module


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release():
    """free the references and hand the freed blocks back to the driver: later modules count allocated bytes"""
    yield
    for form in sorted(WORST):
        print(f"[wgrad edges] largest error / bound, {form}: {WORST[form]:.3g}")
    O.data.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _env(dev):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    from disprcnn_amd.modeling.psmnet import train as T
    return E, _lib, T


def _form(model):
    return (f"wgrad_slide_kernel<{model['NK']}>" if model["path"] == "slide" else f"wgrad_kernel<{model['NT']}>") + \
        (" + reduce" if model["partial"] else " + atomicAdd")


def _say(name, model, err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    i = int(np.argmax(r))
    worst = float(r.flat[i])
    print(f"[{name}: {_form(model)}, depth {model['depth']}] err {float(err.flat[i]):.3e}  bound {float(bound.flat[i]):.3e}  ({worst:.3g} of it)")
    WORST[_form(model)] = max(WORST.get(_form(model), 0.0), worst)
    return worst


def _tensors(E, dev, case, d):
    """(keep-alive, a, b): `a` zero-haloed with poisoned slack (and poisoned pool units behind a prefix view), b in NaN storage"""
    N, units = case["N"], case.get("units", case["N"])
    big = E.Blocked(units, case["Ca"], *case["a_dims"], *case["a_halo"], dev)
    a = big if units == N else E.Blocked(N, case["Ca"], *case["a_dims"], *case["a_halo"], dev, storage=big.storage)
    assert not bool(big.storage.any())
    big.storage[a.numel:].fill_(O.POISON)
    R.put(a, d["a"].copy())                                                       # (the shared reference data is read-only)
    b = E.Blocked(N, case["Cb"], *case["b_dims"], *case["b_halo"], dev)
    b.storage.fill_(NAN)
    R.put(b, d["b"].copy())
    return big, a, b


def _gw(case, dev, prior):
    T_ = int(np.prod(case["cls"]["n"]))
    shape = (O._ceil(case["Ca"], 16) * 16, O._ceil(case["Cb"], 16) * 16, T_)
    whole, view = R.guarded(shape[0] * shape[1] * T_, SENT, dev)
    if prior is None:
        view.fill_(NAN)
    else:
        view.copy_(torch.from_numpy(prior).float().flatten().to(dev))
    return whole, view.view(shape)


def _run(E, T, dev, case, a, b, partials=True, scratch_floats=None, prior=None):
    """one wgrad() call on NaN scratch -> [cbA*16][cbB*16][T] as fp64 numpy"""
    E.wgrad_scratch(dev).fill_(NAN)
    whole, gw = _gw(case, dev, prior)
    T.WGRAD_PARTIALS["enabled"] = partials
    try:
        out = T.wgrad(a, b, case["cls"], case["in_mul"], R=case.get("R"), WT=case.get("WT"), overwrite=int(prior is None), gw=gw,
                      scratch_floats=scratch_floats)
    finally:
        T.WGRAD_PARTIALS["enabled"] = True
    assert out is gw
    got = gw.cpu().double().numpy()
    assert R.guards_keep(whole, SENT), "a guard band of gw was written"
    return got


def _check(label, case, model, d, got, kind, prior=None):
    want = O.pad_gw(case, d["gw"]) + (0.0 if prior is None else prior)
    assert np.isfinite(got).all(), f"{label}: NaN / Inf (poison, stale scratch or b's halo reached the sum)"
    if kind == "int":
        bad = np.argwhere(got != want)
        assert not len(bad), f"{label} {_form(model)}: {len(bad)} elements differ, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        return
    pad = np.ones(got.shape, bool)
    pad[: case["Ca"], : case["Cb"]] = False
    assert np.array_equal(got[pad], want[pad]), f"{label}: padded channel rows moved"
    extra = 0 if prior is None else 1
    mag = O.pad_gw(case, d["mag"]) + (0.0 if prior is None else np.abs(prior))
    bound = O.bound(case, model, mag, O.pad_gw(case, d["terms"]), extra)
    assert _say(label, model, np.abs(got - want), bound) <= 1.0


NAMES = [c["name"] for c in O.SLIDE_CASES + O.GENERIC_CASES + O.FORCED_CASES]


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("name", NAMES)
def test_wgrad_vs_fp64(dev, name, kind):
    """partial sums (twice, bit-identical), the atomicAdd flush without a scratch pointer, and with one that is too small"""
    E, _lib, T = _env(dev)
    case, d = O.BY_NAME[name], O.data(name, kind)
    keep, a, b = _tensors(E, dev, case, d)
    mp, ma = O.model_of(case), O.model_of(case, scratch_floats=0)
    assert mp["partial"] and not ma["partial"]
    runs = [_run(E, T, dev, case, a, b) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]), "the partial-sum reduction is not reproducible run to run"
    _check(name, case, mp, d, runs[0], kind)
    _check(name, case, ma, d, _run(E, T, dev, case, a, b, partials=False), kind)
    _check(name, case, ma, d, _run(E, T, dev, case, a, b, scratch_floats=mp["need"][-1] - 1), kind)
    assert bool((keep.storage[a.numel:] == O.POISON).all())


@pytest.mark.parametrize("kind", ["int", "real"])
def test_g8_scratch_step_down(dev, kind):
    """128 -> 128 stride 2, 192 jobs: three, two and one wave per SIMD as the scratch shrinks, then the atomicAdd flush with a scratch present"""
    E, _lib, T = _env(dev)
    case, d = O.G8, O.data("G8", kind)
    keep, a, b = _tensors(E, dev, case, d)
    need = O.model_of(case)["need"]
    seen = []
    for floats in (O.SCRATCH_FLOATS, need[0] - 1, need[1] - 1, need[2] - 1):
        m = O.model_of(case, scratch_floats=floats)
        seen.append((m["per_simd"], m["partial"]))
        runs = [_run(E, T, dev, case, a, b, scratch_floats=floats) for _ in range(2 if m["partial"] else 1)]
        assert np.array_equal(runs[0], runs[-1])
        _check(f"G8 scratch {floats}, {m['per_simd']} per SIMD, {m['waves']} waves", case, m, d, runs[0], kind)
    assert seen == [(3, True), (2, True), (1, True), (1, False)]


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("name", ["G9", "G9S"])
def test_g9_overwrite_0_adds(dev, name, kind):
    """overwrite = 0: the prior integers plus the gradient, through the reduce and through the atomicAdd flush"""
    E, _lib, T = _env(dev)
    case, d = O.BY_NAME[name], O.data(name, kind)
    keep, a, b = _tensors(E, dev, case, d)
    shape = (O._ceil(case["Ca"], 16) * 16, O._ceil(case["Cb"], 16) * 16, 27)
    prior = np.round(O.hash_uniform(f"wg:{name}:prior", shape, -5.49, 5.49).numpy()).astype(np.float64)
    for floats in (None, 0):
        m = O.model_of(case, scratch_floats=O.SCRATCH_FLOATS if floats is None else 0)
        assert m["partial"] == (floats is None)
        _check(f"{name} overwrite=0", case, m, d, _run(E, T, dev, case, a, b, scratch_floats=floats, prior=prior), kind, prior=prior)
    with pytest.raises(ValueError):
        T.wgrad(a, b, case["cls"], case["in_mul"], overwrite=0)


# ------------------------------------------------------------------------------------------------ parameters built here
def _params(E, _lib, dev, case, a, b, gw, R_, WT, scratch=None, scratch_floats=0, overwrite=1):
    p = _lib.DrcWgradParams()
    (nd, nh, nw), cls, in_mul = case["cls"]["n"], case["cls"], case["in_mul"]
    p.a, p.b, p.gw = a.storage.data_ptr(), b.storage.data_ptr(), gw.data_ptr()
    p.a_n_stride, p.a_cb_stride, p.a_d_stride, p.a_h_stride = a.n_stride, a.cb_stride, a.d_stride, a.h_stride
    p.b_n_stride, p.b_cb_stride, p.b_d_stride, p.b_h_stride, p.b_off0 = b.n_stride, b.cb_stride, b.d_stride, b.h_stride, b.interior_off
    p.N, p.OD, p.OH, p.OW = b.N, b.D, b.H, b.W
    p.in_mul, p.cb_a, p.cb_b = in_mul, a.cb, b.cb
    p.nd, p.nh, p.nw = nd, nh, nw
    p.dd0, p.dh0, p.dw0 = cls["first"]
    p.sd, p.sh, p.sw = cls["step"]
    p.R, p.WT = R_, WT
    rows_in, seg_vox = in_mul * (R_ - 1) + (nh - 1) * cls["step"][1] + 1, in_mul * (WT - 1) + (nw - 1) * cls["step"][2] + 1
    p.lds_bytes_per_wave = (rows_in * seg_vox + R_ * WT) * 64                     # exactly what the entry asks for, not rounded up
    p.overwrite = overwrite
    if scratch is not None:
        p.scratch, p.scratch_floats = scratch.data_ptr(), scratch_floats
    return p


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("name", [c["name"] for c in O.RAW_CASES])
def test_instantiations_no_caller_reaches(dev, name, kind):
    """wgrad_kernel<2>, <4> and <49> (the only form without counted waits): partial sums twice, then the atomicAdd flush"""
    E, _lib, T = _env(dev)
    case, d = O.BY_NAME[name], O.data(name, kind)
    keep, a, b = _tensors(E, dev, case, d)
    mp, ma = O.model_of(case), O.model_of(case, scratch_floats=0)
    assert mp["NT"] == int(name[2:]) and mp["partial"] and not ma["partial"]
    scratch = E.wgrad_scratch(dev)
    runs = []
    for floats in (scratch.numel(), scratch.numel(), 0):
        scratch.fill_(NAN)
        whole, gw = _gw(case, dev, None)
        p = _params(E, _lib, dev, case, a, b, gw, mp["R"], mp["WT"], scratch, floats)
        _lib.check(_lib.lib().drc_tapconv_wgrad(C.byref(p), E._stream_ptr(dev)), "drc_tapconv_wgrad")
        runs.append(gw.cpu().double().numpy())
        assert R.guards_keep(whole, SENT)
    assert np.array_equal(runs[0], runs[1])
    _check(name, case, mp, d, runs[0], kind)
    _check(name, case, ma, d, runs[2], kind)


def test_argument_checks(dev):
    """what the entry rejects on the host before any launch, with valid pointers throughout; N = 0 stores nothing"""
    E, _lib, T = _env(dev)
    lib, sp = _lib.lib(), E._stream_ptr(dev)
    case = O.BY_NAME["G9"]                                                            # stride 2: never the slide kernel
    d = O.data("G9", "int")
    keep, a, b = _tensors(E, dev, case, d)
    whole, gw = _gw(case, dev, None)
    gw.fill_(SENT)
    scratch = E.wgrad_scratch(dev)

    def call(R_=2, WT=3, **over):
        p = _params(E, _lib, dev, case, a, b, gw, R_, WT, scratch, scratch.numel())
        for k, v in over.items():
            setattr(p, k, v)
        return lib.drc_tapconv_wgrad(C.byref(p), sp)

    assert lib.drc_tapconv_wgrad(None, sp) == -1
    assert call(in_mul=3) == -2 and call(dw0=-1) == -2 and call(dd0=-1) == -2
    assert call(R_=8, WT=15) == -3 and call(R_=113, WT=1) == -3
    assert call(nh=1, nw=3) == -4 and call(nh=3, nw=1) == -4
    ok = _params(E, _lib, dev, case, a, b, gw, 2, 3).lds_bytes_per_wave
    assert ok % 16 == 0 and call(lds_bytes_per_wave=ok - 16) == -5 and call(lds_bytes_per_wave=ok + 8) == -5
    assert call(N=0) == 0
    torch.cuda.synchronize()
    assert bool((whole == SENT).all()), "a rejected call or N = 0 wrote to gw"
    # wgrad() on an empty batch: zeros, not the uninitialised memory of its torch.empty
    a0 = E.Blocked(0, case["Ca"], *case["a_dims"], *case["a_halo"], dev)
    b0 = E.Blocked(0, case["Cb"], *case["b_dims"], *case["b_halo"], dev)
    for _ in range(2):
        junk = torch.full((32 * 32 * 27,), NAN, device=dev)                               # what a fresh torch.empty is likely to be handed
        del junk
        out = T.wgrad(a0, b0, case["cls"], case["in_mul"])
        assert out.shape == (32, 32, 27) and not bool(out.any())
    gw.fill_(NAN)
    assert not bool(T.wgrad(a0, b0, case["cls"], case["in_mul"], gw=gw).any())
    gw.fill_(3.0)
    assert bool((T.wgrad(a0, b0, case["cls"], case["in_mul"], overwrite=0, gw=gw) == 3.0).all())
    # the entry accepts the same struct once it is valid again
    p = _params(E, _lib, dev, case, a, b, gw, 2, 3, scratch, scratch.numel())
    _lib.check(lib.drc_tapconv_wgrad(C.byref(p), sp), "drc_tapconv_wgrad")
    assert np.array_equal(gw.cpu().double().numpy(), O.pad_gw(case, d["gw"])) and R.guards_keep(whole, SENT)

"""The ROI stage's kernels held to fp64 (tests/roi_stage_oracle.py) at their edges and past their grid caps, through the C entries:
drc_roi_align_bwd, drc_roi_align_fwd (every channel grouping, the fused normalisation), drc_roi_align_fpn_fwd, drc_align_roi_pairs,
drc_roi_train_targets_fwd, and -- through ops.disparity_paste / ops.roi_depth_maps -- drc_disparity_paste_fwd and drc_roi_depth_maps_fwd.

Inputs sit between NaN guard bands (integer inputs between bands of a large value), outputs in sentinel-filled storage; the sentinel must
survive outside the output, and inside it wherever the kernel must not write.  tests/test_roi_stage_oracle.py shows on the CPU that every
case's input moves by >= 10x its bound under each plausible kernel mistake that applies to it, and that every wrap case has more than
4096 x 256 work items, so the kernels' grid-stride step runs.

Bounds (eps = 2^-24; none fitted to what the kernels give; "mag" is the sum of the absolute values of the terms):
  roi_align_bwd      (contributors + 4) eps mag per pixel, the prior content of grad_in being the first term; where nothing contributes the
                     pixel keeps its prior value bit for bit.  The atomic order is free: fp64 only, no run-to-run identity
  roi_align_fwd      bit for bit against oracle/roi_oracle.py (pinned to the reference's kernel; the build is -ffp-contract=off); with the
                     normalisation fused, 2 ulp of the oracle's value normalised in float32
  roi_align_fpn_fwd  each roi bit for bit against the oracle on its own level's map and scale
  align_roi_pairs    exact
  train targets      12 eps mag (mag includes res / mw); masks by the five rules of roi_stage_oracle.mask_expect, rule-5 mismatches <= 2e-3
                     of the case's pixels
  paste              10 eps (mag wd / S + |x1 - x1p|) per pixel, exact zeros where no roi covers it
  depth              that bound carried through k / (d + 1e-6): k delta_d / d^2 + 2 eps |k / d|, where |d + 1e-6| >= 0.05

Rule 5's comparator, float32 F.interpolate on the CPU, is itself not exact: on an all-ones neighbourhood (exact answer 1, which the kernel
gives) it returns 0.99999994 -> 0 on about 1 % of the pixels at most slice sizes -- by itself more than the 2e-3 the rule allows.  The
`general` and `M14` cases therefore use slice sizes on which it is exact; the CPU test asserts that it eats at most half the allowance.

Largest measured error / bound per kernel on an MI355X: roi_align_bwd 0.40 (wrap; adaptive 0.37, scaled 0.36, outside 0.32, malformed
0.23, pileup 0.0015 with 6400 contributors), its autograd form 0.18 of twice the bound; roi_align_fwd, the wrap launch, every channel
grouping and roi_align_fpn_fwd: 0 elements differ; fused normalisation 0 ulp; align_roi_pairs exact; train targets 0.31 (wrap; general
0.23, M14 0.20, integer 0.073, degenerate 0.028), masks: no rule-2 / rule-3 break and 0 rule-5 mismatches in every case; disparity_paste 0.45
(wrap; gap 0.26, degenerate 0.21); roi_depth_maps 0.37 (wrap; gap 0.27, degenerate 0.20).  Every test prints its figure (-s)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from oracle import roi_oracle as RO
from tests import resample_oracle as R
from tests import roi_stage_oracle as S
from tests.test_hip_train_adjoints import _say

pytestmark = pytest.mark.gpu

SENT, NAN = R.SENT, R.NAN
ISENT, BSENT, IGUARD = 777777, 77, 1 << 30


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    S.bwd_case.cache_clear()
    S.tgt_case.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _env(dev):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    return E, _lib, _lib.lib(), E._stream_ptr(dev)


def _in(a, dev, dtype=torch.float32):
    """a flat copy of `a` on the device between two guard bands (NaN; for integer types a value no index may take) -> (whole, view)"""
    a = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).flatten()
    fill = NAN if dtype == torch.float32 else 255 if dtype == torch.uint8 else IGUARD
    whole, view = R.guarded(a.numel(), fill, dev, dtype)
    view.copy_(a.to(dev))
    return whole, view


def _small_rois():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_golden.npz"), allow_pickle=False)
    return z["small_rois"]


# ------------------------------------------------------------------------------------------------ ROIAlign backward
@pytest.mark.parametrize("name", [c[0] for c in S.BWD_CASES])
def test_roi_align_bwd(dev, name):
    E, _lib, lib, sp = _env(dev)
    c = S.bwd_case(name)
    (B, Cn, H, W), K = c["shape"], len(c["rois"])
    _, g_dev = _in(c["gout"], dev)
    _, r_dev = _in(c["rois"], dev)
    whole, gin = R.guarded(B * Cn * H * W, SENT, dev)
    gin.copy_(torch.from_numpy(c["init"]).flatten().to(dev))
    st = lib.drc_roi_align_bwd(E._ptr(g_dev), E._ptr(r_dev), E._ptr(gin), K, Cn, H, W, c["ph"], c["pw"], c["scale"], c["sr"], sp)
    _lib.check(st, "drc_roi_align_bwd")
    got32 = gin.cpu().numpy().reshape(c["shape"])
    assert R.guards_keep(whole, SENT) and np.isfinite(got32).all()
    untouched = c["cnt"] == 0
    assert np.array_equal(got32[untouched], c["init"][untouched]), "a pixel nothing contributes to lost its prior value"
    worst = _say(f"roi_align_bwd {name} (K={K}, {S.grid_for(K * Cn * c['ph'] * c['pw'])[0]} blocks, contributors <= {int(c['cnt'].max()) if K else 0})",
                 np.abs(got32.astype(np.float64) - c["gin"]), S.bwd_bound(c["mag"], c["cnt"]))
    assert worst <= 1.0
    if name == "empty":
        assert st == 0 and np.array_equal(got32, c["init"])
        for bad in ((K, 0, H, W, 3, 3, 1.0, 2), (K, Cn, H, W, 0, 3, 1.0, 2), (K, Cn, H, W, 3, 3, 1.0, -1), (-1, Cn, H, W, 3, 3, 1.0, 2),
                    (K, Cn, 0, W, 3, 3, 1.0, 2)):
            assert lib.drc_roi_align_bwd(E._ptr(g_dev), E._ptr(r_dev), E._ptr(gin), *bad, sp) == -2
        assert R.guards_keep(whole, SENT) and np.array_equal(gin.cpu().numpy().reshape(c["shape"]), c["init"])


def test_roi_align_autograd_backward(dev):
    """the package's autograd function on `adaptive`: the same tensor (no prior content) within twice the bound"""
    from disprcnn_amd.layers.roi_align import roi_align
    c = S.bwd_case("adaptive")
    x = torch.zeros(c["shape"], device=dev, requires_grad=True)
    y = roi_align(x, torch.from_numpy(c["rois"]).to(dev), (c["ph"], c["pw"]), c["scale"], c["sr"])
    y.backward(torch.from_numpy(c["gout"]).to(dev))
    ref, mag = c["gin"] - c["init"], c["mag"] - np.abs(c["init"])
    worst = _say("roi_align autograd backward (adaptive)", np.abs(x.grad.cpu().double().numpy() - ref), 2 * S.bwd_bound(mag, c["cnt"]) + 1e-300)
    assert worst <= 1.0 and not x.grad.cpu().numpy()[c["cnt"] == 0].any()


# ------------------------------------------------------------------------------------------------ ROIAlign forward, channel groupings
def _fwd(E, lib, sp, dev, x, rois, ph, pw, sr, scale, mean=None, std=None):
    B, Cn, H, W = x.shape
    K = len(rois)
    _, x_dev = _in(x, dev)
    _, r_dev = _in(rois, dev)
    whole, out = R.guarded(K * Cn * ph * pw, SENT, dev)
    st = lib.drc_roi_align_fwd(E._ptr(x_dev), E._ptr(r_dev), E._ptr(out), K, Cn, H, W, ph, pw, scale, sr, E._ptr(mean), E._ptr(std), sp)
    return st, whole, out.cpu().numpy().reshape(K, Cn, ph, pw)


@pytest.mark.parametrize("Cn", S.FWD_CHANNELS)
def test_roi_align_fwd_channel_groups(dev, Cn):
    E, _lib, lib, sp = _env(dev)
    x, rois = S.fwd_input(Cn), _small_rois()
    for ph, pw, sr, scale in S.FWD_SETTINGS:
        st, whole, got = _fwd(E, lib, sp, dev, x, rois, ph, pw, sr, scale)
        _lib.check(st, "drc_roi_align_fwd")
        ref = RO.roi_align(x, rois, scale, ph, pw, sr)
        diff = int((got != ref).sum())
        print(f"[roi_align_fwd C={Cn} ({Cn // S.fwd_cc(Cn)} groups of {S.fwd_cc(Cn)}) {ph}x{pw} sr={sr} scale={scale}] {diff} of {ref.size} differ from the pinned oracle")
        assert diff == 0 and R.guards_keep(whole, SENT)


@pytest.mark.parametrize("Cn", S.FWD_NORM_CHANNELS)
def test_roi_align_fwd_fused_normalisation(dev, Cn):
    E, _lib, lib, sp = _env(dev)
    x, rois = S.fwd_input(Cn), _small_rois()
    mean, std = S.norm_consts(Cn)
    _, m_dev = _in(mean, dev)
    _, s_dev = _in(std, dev)
    for ph, pw, sr, scale in S.FWD_SETTINGS:
        st, whole, got = _fwd(E, lib, sp, dev, x, rois, ph, pw, sr, scale, m_dev, s_dev)
        _lib.check(st, "drc_roi_align_fwd")
        ref = ((RO.roi_align(x, rois, scale, ph, pw, sr) - mean[None, :, None, None]) / std[None, :, None, None]).astype(np.float32)
        assert ref.dtype == np.float32
        worst = _say(f"roi_align_fwd + normalisation C={Cn} {ph}x{pw} sr={sr} (in ulp / 2)", np.abs(got.astype(np.float64) - ref), 2.0 * np.spacing(np.abs(ref)).astype(np.float64))
        assert worst <= 1.0 and R.guards_keep(whole, SENT)
    ph, pw, sr, scale = S.FWD_SETTINGS[0]
    for m, s in ((m_dev, None), (None, s_dev)):
        st, whole, got = _fwd(E, lib, sp, dev, x, rois, ph, pw, sr, scale, m, s)
        assert st == -2 and bool((whole == SENT).all())


def test_roi_align_fwd_wrap(dev):
    E, _lib, lib, sp = _env(dev)
    w = S.FWD_WRAP
    x, rois = S.fwd_input(w["shape"][1], w["shape"][2:]), S.rois_of(w["rois"])
    work = len(rois) * (x.shape[1] // S.fwd_cc(x.shape[1])) * w["ph"] * w["pw"]
    assert S.grid_for(work) == (4096, True)
    st, whole, got = _fwd(E, lib, sp, dev, x, rois, w["ph"], w["pw"], w["sr"], w["scale"])
    _lib.check(st, "drc_roi_align_fwd")
    ref = RO.roi_align(x, rois, w["scale"], w["ph"], w["pw"], w["sr"])
    diff = int((got != ref).sum())
    print(f"[roi_align_fwd wrap: {work} work items on 4096 blocks] {diff} of {ref.size} differ from the pinned oracle")
    assert diff == 0 and R.guards_keep(whole, SENT)


# ------------------------------------------------------------------------------------------------ FPN pooler
def _pyramid(_lib, feats_dev, n=None):
    pyr = _lib.DrcFpnPyramid()
    pyr.n_levels = len(feats_dev) if n is None else n
    for i, (f, (hw, s)) in enumerate(zip(feats_dev, S.FPN_LEVELS)):
        pyr.feat[i], pyr.H[i], pyr.W[i], pyr.scale[i] = f.data_ptr(), hw[0], hw[1], s
    return pyr


@pytest.mark.parametrize("Cn", S.FPN_CHANNELS)
def test_roi_align_fpn(dev, Cn):
    E, _lib, lib, sp = _env(dev)
    feats, rois, levels, big = S.fpn_case(Cn)
    K = len(rois)
    keep = [_in(f, dev) for f in feats]
    pyr = _pyramid(_lib, [v for _, v in keep])
    _, r_dev = _in(rois, dev)
    _, l_dev = _in(levels, dev, torch.int32)
    for ph, pw, sr in S.FPN_SETTINGS:
        whole, out = R.guarded(K * Cn * ph * pw, SENT, dev)
        st = lib.drc_roi_align_fpn_fwd(C.byref(pyr), E._ptr(r_dev), E._ptr(l_dev), E._ptr(out), K, Cn, ph, pw, sr, sp)
        _lib.check(st, "drc_roi_align_fpn_fwd")
        got = out.cpu().numpy().reshape(K, Cn, ph, pw)
        bad = [k for k in range(K) if not np.array_equal(got[k], RO.roi_align(feats[levels[k]], rois[k:k + 1], S.FPN_LEVELS[levels[k]][1], ph, pw, sr)[0])]
        print(f"[roi_align_fpn C={Cn} ({S.fpn_cc(Cn)} per thread) {ph}x{pw} sr={sr}] rois that differ from the oracle on their own level: {bad}")
        assert not bad and R.guards_keep(whole, SENT)
    # entry checks: nothing is written
    whole, out = R.guarded(64, SENT, dev)
    assert lib.drc_roi_align_fpn_fwd(C.byref(pyr), E._ptr(r_dev), E._ptr(l_dev), E._ptr(out), 0, Cn, 7, 7, 2, sp) == 0
    for n in (0, 9):
        assert lib.drc_roi_align_fpn_fwd(C.byref(_pyramid(_lib, [v for _, v in keep], n)), E._ptr(r_dev), E._ptr(l_dev), E._ptr(out), K, Cn, 1, 1, 2, sp) == -2
    holed = _pyramid(_lib, [v for _, v in keep])
    holed.feat[2] = None
    assert lib.drc_roi_align_fpn_fwd(C.byref(holed), E._ptr(r_dev), E._ptr(l_dev), E._ptr(out), K, Cn, 1, 1, 2, sp) == -2
    torch.cuda.synchronize()
    assert bool((whole == SENT).all())


# ------------------------------------------------------------------------------------------------ ROI pairing
@pytest.mark.parametrize("Rn", S.PAIR_R)
def test_align_roi_pairs(dev, Rn):
    E, _lib, lib, sp = _env(dev)
    for t, (lb, rb, idx) in enumerate(S.pair_tables(Rn)):
        _, l_dev = _in(lb, dev)
        _, r_dev = _in(rb, dev)
        _, i_dev = _in(idx, dev, torch.int32)
        wl, rl = R.guarded(Rn * 5, SENT, dev)
        wr, rr = R.guarded(Rn * 5, SENT, dev)
        wg, geom = R.guarded(Rn * 4, ISENT, dev, torch.int32)
        st = lib.drc_align_roi_pairs(E._ptr(l_dev), E._ptr(r_dev), E._ptr(i_dev), Rn, S.PAIR_W, S.PAIR_H, E._ptr(rl), E._ptr(rr), E._ptr(geom), sp)
        _lib.check(st, "drc_align_roi_pairs")
        el, er, eg = S.align_pairs(lb, rb, idx, S.PAIR_W, S.PAIR_H)
        ok = (np.array_equal(rl.cpu().numpy().reshape(Rn, 5), el), np.array_equal(rr.cpu().numpy().reshape(Rn, 5), er),
              np.array_equal(geom.cpu().numpy().reshape(Rn, 4), eg))
        print(f"[align_roi_pairs R={Rn} table {t} ({(Rn + 63) // 64} blocks of 64)] rois_l, rois_r, geom equal the oracle: {ok}")
        assert all(ok) and R.guards_keep(wl, SENT) and R.guards_keep(wr, SENT) and R.guards_keep(wg, ISENT)
    wl, rl = R.guarded(16, SENT, dev)
    assert lib.drc_align_roi_pairs(E._ptr(l_dev), E._ptr(r_dev), E._ptr(i_dev), 0, S.PAIR_W, S.PAIR_H, E._ptr(rl), E._ptr(rl), E._ptr(rl), sp) == 0
    assert lib.drc_align_roi_pairs(E._ptr(l_dev), E._ptr(r_dev), E._ptr(i_dev), Rn, 0, S.PAIR_H, E._ptr(rl), E._ptr(rl), E._ptr(rl), sp) == -2
    assert bool((wl == SENT).all())


# ------------------------------------------------------------------------------------------------ training targets
@pytest.mark.parametrize("name", list(S.TGT_CASES))
def test_roi_train_targets(dev, name):
    """rois_l and geom come from the oracle, so this does not depend on the pairing kernel"""
    E, _lib, lib, sp = _env(dev)
    c = S.tgt_case(name)
    Rn, res, H, W, M = len(c["idx"]), c["res"], c["H"], c["W"], c["M"]
    ins = [_in(c["disp"], dev), _in(c["gt"], dev, torch.uint8), _in(c["probs"], dev), _in(c["lbox"], dev), _in(c["rois_l"], dev),
           _in(c["geom"], dev, torch.int32)]
    d_dev, g_dev, p_dev, b_dev, r_dev, q_dev = (v for _, v in ins)
    wt, tgt = R.guarded(Rn * res * res, SENT, dev)
    wm, msk = R.guarded(Rn * res * res, BSENT, dev, torch.uint8)
    args = (E._ptr(d_dev), E._ptr(g_dev), E._ptr(p_dev), M, c["pad"], S.TGT_THRESH, E._ptr(b_dev), E._ptr(r_dev), E._ptr(q_dev))
    st = lib.drc_roi_train_targets_fwd(*args, Rn, H, W, res, E._ptr(tgt), E._ptr(msk), sp)
    _lib.check(st, "drc_roi_train_targets_fwd")
    got_t = tgt.cpu().double().numpy().reshape(Rn, res, res)
    got_m = msk.cpu().numpy().reshape(Rn, res, res)
    assert R.guards_keep(wt, SENT) and R.guards_keep(wm, BSENT) and np.isfinite(got_t).all() and set(np.unique(got_m).tolist()) <= {0, 1}
    worst = _say(f"roi_train_targets {name} (R={Rn}, res={res}, {S.grid_for(Rn * res * res)[0]} blocks)", np.abs(got_t - c["ref"]["target"]),
                 S.target_bound(c["ref"]["mag"]) + 1e-300)
    hard, soft = S.mask_mismatch(c["code"], c["interp"], got_m)
    n5 = int((c["code"] == S.INTERP).sum())
    print(f"[roi_train_targets {name} masks] {hard} pixels break rule 2 / 3; {soft} of {n5} rule-5 pixels differ from the CPU interpolation "
          f"({soft / got_m.size:.2e} of the case's {got_m.size} pixels, 2e-3 allowed); {int((c['code'] == S.SKIP).sum())} left out")
    assert worst <= 1.0 and hard == 0 and soft <= 2e-3 * got_m.size
    if name == "integer":                                                             # the entry checks: nothing is written
        wt, tgt = R.guarded(64, SENT, dev)
        wm, msk = R.guarded(64, BSENT, dev, torch.uint8)
        assert lib.drc_roi_train_targets_fwd(*args, 0, H, W, res, E._ptr(tgt), E._ptr(msk), sp) == 0
        assert lib.drc_roi_train_targets_fwd(*args, Rn, H, W, 0, E._ptr(tgt), E._ptr(msk), sp) == -2
        torch.cuda.synchronize()
        assert bool((wt == SENT).all()) and bool((wm == BSENT).all())


# ------------------------------------------------------------------------------------------------ paste and depth maps
@pytest.mark.parametrize("name", list(S.PASTE_CASES))
def test_disparity_paste(dev, name):
    from disprcnn_amd import ops
    c = S.PASTE_CASES[name]
    (H, W), counts = c["hw"], c["counts"]
    disp, boxes, masks = S.paste_inputs(name)
    _, d_dev = _in(disp, dev)
    _, m_dev = _in(masks, dev) if masks is not None else (None, None)
    got = ops.disparity_paste(d_dev.view(disp.shape), torch.from_numpy(boxes).to(dev), counts, H, W, c["clamp0"],
                              None if masks is None else m_dev.view(masks.shape)).cpu().double().numpy()
    ref, bound, covered = S.paste64(disp, boxes, counts, H, W, c["clamp0"], masks)
    assert got.shape == ref.shape and np.isfinite(got).all() and not got[~covered].any()
    worst = _say(f"disparity_paste {name} ({S.blocks_for(H * W)[0]} blocks per image, rois per image {counts})", np.abs(got - ref), bound + 1e-300)
    assert worst <= 1.0
    if c["clamp0"]:                                                                   # exactly max(., 0) of the largest covered value
        below = S.paste_surely_clamped(disp, boxes, counts, H, W)
        assert (got >= 0).all() and below.any() and not got[below].any()


@pytest.mark.parametrize("name", list(S.DEPTH_CASES))
def test_roi_depth_maps(dev, name):
    from disprcnn_amd import ops
    c = S.DEPTH_CASES[name]
    H, W = c["hw"]
    disp, boxes, _ = S.paste_inputs(name, depth=True)
    k = np.full(len(boxes), np.float32(S.FUXB))
    _, d_dev = _in(disp, dev)
    got = ops.roi_depth_maps(d_dev.view(disp.shape), torch.from_numpy(boxes).to(dev), torch.from_numpy(k).to(dev), H, W).cpu().double().numpy()
    ref, bound, ok, inside = S.depth64(disp, boxes, k, H, W)
    assert got.shape == ref.shape and not got[~inside].any() and np.isfinite(got[ok]).all()
    worst = _say(f"roi_depth_maps {name} ({S.blocks_for(H * W)[0]} blocks per roi, R={len(boxes)}, {int(ok.sum())} of {int(inside.sum())} box pixels compared)",
                 np.where(ok, np.abs(got - ref), 0.0), np.where(ok, bound, 1.0))
    assert worst <= 1.0 and ok.any()

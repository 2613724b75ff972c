"""The pool / resample kernels of the 2D stage held to fp64 (tests/resample_oracle.py), each on its own, through the C entries:
drc_avgpool2d_blocked / _slice (and the nested k // fine form), drc_bilinear_up_blocked, drc_bilinear_resize_blocked (both align_corners
settings), drc_maxpool2d_blocked, drc_copy_blocks, and the fp16-storage twins drc_avgpool2d_blocked16_slice / drc_bilinear_up_blocked16.

Inputs live in NaN-filled storage (halo, slack, the other channel blocks of the 20-block concat tensor), outputs in sentinel-filled storage
whose sentinel must survive outside the interior.  tests/test_resample_oracle.py shows on the CPU that every case's input moves by >= 10x
its bound under a plausible kernel mistake.

Bounds (eps = 2^-24; none fitted to what the kernels give):
  avgpool            (k^2/16 + 8) eps sum|x|/k^2: a lane adds k^2/16 window positions in sequence, four shuffle levels, 1/k^2 and the
                     product with it
  bilinear           8 eps sum w_i|v_i| with the oracle's float32 source coordinates (the build has no fp contraction, so they are the
                     kernel's): 1 - t, the products and the additions are <= 7 roundings on any path; bit-equality with torch-CPU float32
                     F.interpolate is printed, not asserted
  maxpool            exact, all-negative input (a zero start value or a halo read shows), F.max_pool2d(ceil_mode=True)
  fp16 twins         2^-11 |ref| + 2^-25 + the fp32 term, against fp64 of the fp16-rounded input
  copy_blocks        bit-exact (the entry is exported but has no caller in the package: the concat is written in place)

Largest measured error / bound per kernel on an MI355X: avgpool 0.22 (nested 0.21), bilinear_up 0.42, bilinear_resize 0.41 (align_corners
= 0) / 0.35 (= 1), the fp16 twins 0.999 / 0.995 (the rounding of the result to fp16 IS the bound: half an ulp is reached), maxpool and
copy_blocks exact.  bilinear is bit-equal to torch-CPU float32 only on the identity and one-cell cases (the CPU kernel rounds in another
order).  Every test prints its figure next to the bound (-s)."""
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
    """hand the freed blocks back to the driver: later modules count allocated bytes"""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _env(dev):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    return E, _lib, _lib.lib(), E._stream_ptr(dev)


def _filled(cls, dev, fill, *geom):
    t = cls(*geom, dev)
    t.storage.fill_(fill)
    return t


def _say(name, got, ref, bound):
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    i = int(np.argmax(r))
    print(f"[{name}] err {float(err.flat[i]):.3e}  bound {float(np.broadcast_to(bound, err.shape).flat[i]):.3e}  ({float(r.flat[i]):.3g} of it)")
    return float(r.flat[i])


# ------------------------------------------------------------------------------------------------ AvgPool2d
def _avgpool_variants(E, dev, x, k, half):
    """(label, x tensor, cb_total, cb_off, px, py) over input halo 0 / 2, output halo 0 / 1, the plain tensor and blocks [0, cb) and
    [4, 4 + cb) of a 20-block tensor"""
    cls, lanes = (E.Blocked16, 32) if half else (E.Blocked, 16)
    N, Cn, H, W = x.shape
    cb = Cn // lanes
    for px in (0, 2):
        for total, off in ((cb, 0), (20, 0), (20, 4)):
            xb = _filled(cls, dev, NAN, N, total * lanes, 1, H, W, 0, px, px)
            R.put(xb, x[:, :, None], off=off)
            for py in (0, 1):
                yield f"px={px} py={py} blocks [{off},{off + cb}) of {total}", xb, total, off, px, py


@pytest.mark.parametrize("k,hw", R.AVG_CASES)
@pytest.mark.parametrize("half", [False, True])
def test_avgpool(dev, k, hw, half):
    E, _lib, lib, sp = _env(dev)
    H, W = hw
    OH, OW = H // k, W // k
    lanes = 32 if half else 16
    x = R.pool_input(f"ap:{hw}", (2, 32) + hw)
    if half:
        x = np.concatenate([R.half(x), R.half(x[:, ::-1] * np.float32(0.75))], 1)    # 64 channels = two fp16 blocks
    ref, mag = R.avgpool(x, k)
    bound = R.avgpool_bound(k, mag)
    bound = R.f16_bound(ref, bound) if half else bound
    cb = x.shape[1] // lanes
    worst = 0.0
    for label, xb, total, off, px, py in _avgpool_variants(E, dev, x, k, half):
        y = _filled(E.Blocked16 if half else E.Blocked, dev, SENT, 2, x.shape[1], 1, OH, OW, 0, py, py)
        if half:
            sl = E.Blocked16Slice(xb, off, x.shape[1])
            st = lib.drc_avgpool2d_blocked16_slice(E._ptr(sl.base.storage), E._ptr(y.storage), 2, sl.cb, H, W, px, k, OH, OW, py, sl.base.cb, sl.cb_off, sp)
        elif total == cb:
            st = lib.drc_avgpool2d_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, cb, H, W, px, k, OH, OW, py, sp)
        else:
            st = lib.drc_avgpool2d_blocked_slice(E._ptr(xb.storage), E._ptr(y.storage), 2, cb, H, W, px, k, OH, OW, py, total, off, sp)
        _lib.check(st, "drc_avgpool2d_blocked")
        got = R.get(y, x.shape[1])[:, :, 0]
        assert np.isfinite(got).all() and R.outside_keeps(y, SENT), label
        r = R.margin(ref, got, bound)
        assert r <= 1.0, (label, r)
        worst = max(worst, r)
    print(f"[avgpool{'16' if half else ''} k={k} {hw}] largest error {worst:.3f} of the bound over 12 layouts")
    # refusals: a window past the input
    y = _filled(E.Blocked, dev, SENT, 2, 32, 1, OH + 1, OW, 0, 0, 0)
    assert lib.drc_avgpool2d_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, 2, H, W, 2, k, OH + 1, OW, 0, sp) == -2


@pytest.mark.parametrize("hw,fine,k", [((56, 72), 8, 16), ((64, 64), 8, 64), ((66, 130), 8, 64), ((56, 72), 8, 32)])
def test_avgpool_nested(dev, hw, fine, k):
    """the pooled map of the finest branch pooled again with k // fine (psmnet/runtime.py): (56, 72) -> (7, 9) -> 2x2 windows leave a
    remainder row and column of the POOLED map out"""
    E, _lib, lib, sp = _env(dev)
    H, W = hw
    x = R.pool_input(f"ap:{hw}", (2, 32) + hw)
    xb = _filled(E.Blocked, dev, NAN, 2, 20 * 16, 1, H, W, 0, 2, 2)
    R.put(xb, x[:, :, None], off=4)
    src = _filled(E.Blocked, dev, NAN, 2, 32, 1, H // fine, W // fine, 0, 0, 0)
    _lib.check(lib.drc_avgpool2d_blocked_slice(E._ptr(xb.storage), E._ptr(src.storage), 2, 2, H, W, 2, fine, src.H, src.W, 0, 20, 4, sp), "fine")
    mid = R.get(src, 32)[:, :, 0]
    assert np.isfinite(mid).all()
    kk = k // fine
    oh, ow = H // k, W // k
    assert oh * kk <= src.H and ow * kk <= src.W
    y = _filled(E.Blocked, dev, SENT, 2, 32, 1, oh, ow, 0, 0, 0)
    _lib.check(lib.drc_avgpool2d_blocked_slice(E._ptr(src.storage), E._ptr(y.storage), src.N, src.cb, src.H, src.W, src.ph, kk, oh, ow, 0, src.cb, 0, sp),
               "nested")
    ref, mag = R.avgpool(mid, kk)
    assert _say(f"avgpool nested {hw} {fine} then {kk}", R.get(y, 32)[:, :, 0], ref[:, :, :oh, :ow], R.avgpool_bound(kk, mag[:, :, :oh, :ow])) <= 1.0
    assert R.outside_keeps(y, SENT)
    # and it is AvgPool2d(k) of the input up to both kernels' bounds
    full, fmag = R.avgpool(x, k)
    first = R.avgpool_bound(fine, fmag)                                                # positive input: the windows' bounds average
    assert R.margin(full, R.get(y, 32)[:, :, 0], first + R.avgpool_bound(kk, fmag + first)) <= 1.0


# ------------------------------------------------------------------------------------------------ bilinear
def _bilinear_case(dev, ihw, ohw, align, half, entry):
    E, _lib, lib, sp = _env(dev)
    (IH, IW), (OH, OW) = ihw, ohw
    cls, lanes = (E.Blocked16, 32) if half else (E.Blocked, 16)
    Cn = 2 * lanes
    x = R.uniform(f"bl:{ihw}{ohw}", (2, 32) + ihw)
    if half:
        x = np.concatenate([R.half(x), R.half(x[:, ::-1] * np.float32(0.75))], 1)
    ref, mag = R.bilinear(x, OH, OW, align)
    bound = R.bilinear_bound(mag) + 1e-300
    bound = R.f16_bound(ref, bound) if half else bound
    worst = 0.0
    for px in (0, 1):
        for py in (0, 1):
            xb = _filled(cls, dev, NAN, 2, Cn, 1, IH, IW, 0, px, px)
            R.put(xb, x[:, :, None])
            y = _filled(cls, dev, SENT, 2, 5 * lanes, 1, OH, OW, 0, py, py)               # channel blocks [2, 4) of 5
            if entry == "up16":
                sl = E.Blocked16Slice(y, 2, Cn)
                st = lib.drc_bilinear_up_blocked16(E._ptr(xb.storage), E._ptr(sl.base.storage), 2, sl.cb, IH, IW, px, OH, OW, py, sl.base.cb, sl.cb_off, sp)
            elif entry == "up":
                st = lib.drc_bilinear_up_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, 2, IH, IW, px, OH, OW, py, 5, 2, sp)
            else:
                st = lib.drc_bilinear_resize_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, 2, IH, IW, px, OH, OW, py, 5, 2, int(align), sp)
            _lib.check(st, entry)
            got = R.get(y, Cn, off=2)[:, :, 0]
            assert np.isfinite(got).all() and R.outside_keeps(y, SENT, off=2, cb=2), (px, py)
            r = R.margin(ref, got, bound)
            assert r <= 1.0, (px, py, r)
            worst = max(worst, r)
    msg = f"[{entry} {ihw}->{ohw} align={int(align)}] largest error {worst:.3f} of the bound over 4 layouts"
    if not half:
        cpu = F.interpolate(torch.from_numpy(x), ohw, mode="bilinear", align_corners=bool(align)).numpy()
        msg += f"; bit-equal to torch-CPU float32: {np.array_equal(cpu.astype(np.float64), got)}"
    print(msg)


@pytest.mark.parametrize("ihw,ohw", R.UP_FWD)
@pytest.mark.parametrize("half", [False, True])
def test_bilinear_up(dev, ihw, ohw, half):
    _bilinear_case(dev, ihw, ohw, True, half, "up16" if half else "up")


@pytest.mark.parametrize("ihw,ohw", R.RESIZE_FWD)
@pytest.mark.parametrize("align", [False, True])
def test_bilinear_resize(dev, ihw, ohw, align):
    _bilinear_case(dev, ihw, ohw, align, False, "resize")


# ------------------------------------------------------------------------------------------------ max_pool2d
@pytest.mark.parametrize("k,s,hw", R.MAXPOOL_CASES)
def test_maxpool(dev, k, s, hw):
    E, _lib, lib, sp = _env(dev)
    H, W = hw
    x = R.uniform(f"mp:{hw}", (2, 32) + hw, -2.0, -0.5)
    OH, OW = R.maxpool_out(H, k, s), R.maxpool_out(W, k, s)
    ref = F.max_pool2d(torch.from_numpy(x), k, s, 0, ceil_mode=True).numpy()
    assert ref.shape[-2:] == (OH, OW) and np.array_equal(ref, R.maxpool(x, k, s)) and (ref < 0).all()
    for px in (0, 1):
        xb = _filled(E.Blocked, dev, NAN, 2, 32, 1, H, W, 0, px, px)
        R.put(xb, x[:, :, None])
        for py in (0, 1):
            y = _filled(E.Blocked, dev, SENT, 2, 32, 1, OH, OW, 0, py, py)
            _lib.check(lib.drc_maxpool2d_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, 2, H, W, px, k, s, OH, OW, py, sp), "drc_maxpool2d_blocked")
            got = R.get(y, 32)[:, :, 0]
            assert np.array_equal(got, ref.astype(np.float64)), (px, py, float(np.abs(got - ref).max()))
            assert R.outside_keeps(y, SENT)
    print(f"[maxpool k={k} s={s} {hw} -> {(OH, OW)}] exact on 4 layouts")
    # a window that would start outside the input is refused
    bh, bw = -(-H // s) + 1, -(-W // s) + 1                                           # the first sizes whose last window starts at >= H / W
    y = _filled(E.Blocked, dev, SENT, 2, 32, 1, bh, bw, 0, 0, 0)
    assert lib.drc_maxpool2d_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, 2, H, W, 1, k, s, bh, OW, 0, sp) == -2
    assert lib.drc_maxpool2d_blocked(E._ptr(xb.storage), E._ptr(y.storage), 2, 2, H, W, 1, k, s, OH, bw, 0, sp) == -2
    assert bool((y.storage == SENT).all())


# ------------------------------------------------------------------------------------------------ copy_blocks
def test_copy_blocks(dev):
    """a 3-block source (halo included: whole blocks travel) into blocks [2, 5) of a 7-block target"""
    E, _lib, lib, sp = _env(dev)
    src = E.Blocked(2, 48, 1, 5, 7, 0, 1, 1, dev)
    src.storage[: src.numel].copy_(torch.from_numpy(R.uniform("copy", (src.numel,))).to(dev))
    dst = _filled(E.Blocked, dev, SENT, 2, 7 * 16, 1, 5, 7, 0, 1, 1)
    _lib.check(lib.drc_copy_blocks(E._ptr(src.storage), E._ptr(dst.storage), 2, 3, src.Dp * src.Hp * src.Wp, 7, 2, sp), "drc_copy_blocks")
    v = dst.view6()
    assert torch.equal(v[:, 2:5], src.view6())
    assert bool((v[:, :2] == SENT).all()) and bool((v[:, 5:] == SENT).all()) and bool((dst.storage[dst.numel:] == SENT).all())
    assert lib.drc_copy_blocks(E._ptr(src.storage), E._ptr(dst.storage), 2, 3, src.Dp * src.Hp * src.Wp, 4, 2, sp) == -2

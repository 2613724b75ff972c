"""The last two steps of the disparity path on the MI355X against fp64 (tests/disp_tail_oracle.py): the soft-argmin head
(drc_upsample_softargmin_fwd: the generic kernel and the three register-column instantiations, at every edge of the host predicate that
chooses between them) and the post-processing (drc_disparity_paste_fwd, drc_roi_depth_maps_fwd, drc_disparity_resize_fwd) at 1-pixel
boxes, crops, image edges, every map size and above the grid cap of 4096 x 256 pixels, where the grid-stride loops run.

Tolerance: err <= 2 * e32 + 1e-6 * max|ref|, e32 being the error of the reference's own fp32 chain on the CPU (oracle/psmnet_oracle.py,
oracle/post_oracle.py, the fp32 evaluation of the resize) against fp64 on the same inputs.  The signed max pooling selects values and
rounds twice (the division by IW and the multiplication by OW): |got - ref| <= 2^-23 |ref|.  Its mixed-sign map holds multiples of 2^-8, so
that the difference of the two pooled parts -- a third fp32 operation the reference has too -- is exact and the two roundings are all there is.
The identity resize is exact where IW is a power of two (x / IW * IW in fp32 is x only then); the 40 x 40 one is held to the rule.

The soft-argmin template evaluates exp(v - m) as one hardware exp2 of (v - m) * log2 e (1 ulp, and a relative 2^-24 |v - m| log 2 from the
rounded product, which matters only where exp(v - m) itself is negligible).  No term was added for it: the measured errors below stay inside
the rule that torch's expf chain sets.

Measured on the MI355X, worst err / (2 * e32 + 1e-6 * max|ref|) per kernel and form (1.0 is the bound):
    soft-argmin generic        0.370 at amplitude 3 (g_dp96)    0.543 at amplitude 2000 (g_w85)
    soft-argmin <6,24>         0.350 (t6_grid104)               0.494 (t6_tail_grid62)
    soft-argmin <12,48>        0.350 (t12_hp1)                  0.506 (t12_wp33)
    soft-argmin <24,96>        0.344 (t24_wp64)                 0.499 (t24_wp64)
    disparity_paste            0.485 (S = 224); 0.319 above the grid cap
    roi_depth_maps             0.494 (S = 224); 0.337 above the grid cap
    disparity_resize bilinear  0.490 (120 x 200 -> 48 x 64); 0.467 above the grid cap
    disparity_resize max pool  0.771 x 2^-23 relative (37 x 53 -> 40 x 60, mixed signs)
Many worst cases equal e32 to the last digit: the kernels round where torch's fp32 chain rounds.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

from disprcnn_amd.utils import synth
from oracle import post_oracle as P
from tests import disp_tail_oracle as T

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _check(name, got, ref64, ref32):
    """the e32 rule; prints the figures before it asserts"""
    bound, e32 = T.e32_bound(ref64, ref32)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    assert torch.isfinite(got).all(), name
    err = (got.double() - ref64).abs().max().item() if got.numel() else 0.0
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"RATIO {name}: err {err:.3e} e32 {e32:.3e} max|ref| {ref64.abs().max().item() if got.numel() else 0:.4g} ratio {ratio:.3f}")
    assert err <= bound, (name, err, e32, bound)
    return bound


# ------------------------------------------------------------------------------------------------ soft-argmin forward
SA = collections.namedtuple("SA", "name N Dp Hp Wp D H W form amps")


def _sa(name, N, Dp, Hp, Wp, H, W, form, D=None, sharp=False):
    return SA(name, N, Dp, Hp, Wp, 4 * Dp if D is None else D, H, W, form, (3.0, 2000.0) if sharp else (3.0,))


SA_CASES = [
    _sa("t6_tail_grid62", 2, 6, 22, 22, 88, 88, 6, sharp=True),           # 31 blocks per ROI, the last one 64 pixels; 62 blocks: no renumbering
    _sa("t6_grid104", 8, 6, 9, 25, 33, 100, 6),                           # 104 blocks: the XCD renumbering
    _sa("t12_w86", 1, 12, 7, 22, 27, 86, 12),                             # the narrowest W of the template
    _sa("t12_wp32", 1, 12, 4, 32, 13, 128, 12),                           # 32 lanes per staged row, all busy
    _sa("t12_wp33", 2, 12, 3, 33, 10, 130, 12, sharp=True),               # 64 lanes per staged row, 31 idle
    _sa("t12_hp1", 1, 12, 1, 30, 2, 120, 12),                             # one coarse row staged
    _sa("t24_wp64", 2, 24, 5, 64, 19, 255, 24, sharp=True),               # the widest Wp
    _sa("t24_net", 1, 24, 14, 14, 56, 96, 24),                            # 21 full blocks, three coarse rows staged
    _sa("g_w85", 1, 12, 7, 22, 27, 85, 0, sharp=True),
    _sa("g_wp65", 1, 24, 5, 65, 19, 257, 0),
    _sa("g_sy", 1, 12, 12, 30, 14, 120, 0),                               # D = 4 Dp, W >= 86, but 256 pixels span too many coarse rows
    _sa("g_small", 2, 5, 4, 6, 9, 11, 0, D=7),
    _sa("g_d1", 1, 4, 3, 5, 6, 7, 0, D=1),
    _sa("g_d_eq_dp", 1, 8, 5, 5, 10, 12, 0, D=8),
    _sa("g_dp96", 1, 96, 3, 3, 5, 5, 0),
    _sa("g_down", 1, 6, 9, 9, 4, 4, 0),
    _sa("g_h1", 2, 6, 3, 7, 1, 20, 0),
    _sa("g_w1", 2, 6, 7, 3, 20, 1, 0),
    _sa("g_3x7x13", 3, 6, 3, 5, 7, 13, 0),                                # 273 pixels: three blocks of 128, the last one 17 wide
]


def _sa_cost(c, amp):
    shape = (c.N, c.Dp, c.Hp, c.Wp)
    if amp <= 3.0:
        return synth.hash_uniform(f"tail:sa:{c.name}", shape, -amp, amp)
    # sharp columns: |c| in [amp/4, amp], every neighbour (along D', H', W') of the opposite sign
    mag = synth.hash_uniform(f"tail:sharp:{c.name}", shape, amp / 4, amp)
    k, y, x = torch.meshgrid(torch.arange(c.Dp), torch.arange(c.Hp), torch.arange(c.Wp), indexing="ij")
    return mag * (1 - 2 * ((k + y + x) % 2)).float()


def _sa_mindisp(i, D):
    return (5, 0, -(D // 2))[i % 3]


@pytest.mark.parametrize("i", range(len(SA_CASES)), ids=[c.name for c in SA_CASES])
def test_softargmin_fwd_vs_fp64(dev, i):
    from disprcnn_amd import _lib, ops
    c = SA_CASES[i]
    assert _lib.lib().drc_upsample_softargmin_form(c.Dp, c.Hp, c.Wp, c.D, c.H, c.W) == c.form
    mn = _sa_mindisp(i, c.D)
    for amp in c.amps:
        cost = _sa_cost(c, amp)
        ref = T.upsample_softargmin(cost, mn + c.D, mn, c.H, c.W)
        ref32 = T.upsample_softargmin(cost, mn + c.D, mn, c.H, c.W, dtype=F32)
        got = ops.upsample_softargmin(cost.to(dev), mn + c.D, mn, c.H, c.W)
        bound = _check(f"softargmin form={c.form} amp={amp:g} {c.name}", got, ref, ref32)
        g = got.cpu().double()
        assert g.min().item() >= mn - bound and g.max().item() <= mn + c.D - 1 + bound, (c.name, g.min().item(), g.max().item())
        if c.D == 1:
            assert torch.equal(got.cpu(), torch.full((c.N, c.H, c.W), float(mn)))
        assert torch.equal(ops.upsample_softargmin(cost.to(dev), mn + c.D, mn, c.H, c.W), got), f"{c.name}: second call differs"


def test_softargmin_form_table_covers_every_kernel_twice():
    forms = collections.Counter(c.form for c in SA_CASES)
    sharp = {c.form for c in SA_CASES if 2000.0 in c.amps}
    assert all(forms[f] >= 2 for f in (0, 6, 12, 24)) and sharp == {0, 6, 12, 24}


def test_softargmin_statuses(dev):
    """Dp = 97 -> -3 before anything is launched; N = 0 -> 0 and the output is left alone."""
    from disprcnn_amd import _lib, engine as E
    L = _lib.lib()
    cost = torch.zeros(1, 97, 2, 2, device=dev)
    out = torch.full((1, 5, 5), -7.5, device=dev)
    assert L.drc_upsample_softargmin_fwd(E._ptr(cost), E._ptr(out), 1, 97, 2, 2, 388, 5, 5, 0, E._stream_ptr(dev)) == -3
    assert L.drc_upsample_softargmin_form(97, 2, 2, 388, 5, 5) == -3
    assert L.drc_upsample_softargmin_fwd(E._ptr(cost), E._ptr(out), 0, 12, 2, 2, 48, 5, 5, 0, E._stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert (out == -7.5).all()


# ------------------------------------------------------------------------------------------------ paste / depth: explicit boxes
IMG_H, IMG_W = 187, 413
# (left xyxy, right x1 / x2, tag); the right box takes the left one's rows
_BOXES = [
    # image 0
    [((20.0, 10.0, 120.0, 11.0), (5.0, 100.0), "one pixel high, right narrower"),
     ((200.0, 30.0, 201.0, 150.0), (190.0, 191.0), "one pixel wide"),
     ((300.0, 100.0, 301.0, 101.0), (290.0, 291.0), "1 x 1"),
     ((50.3, 40.2, 130.7, 120.9), (10.5, 140.2), "right wider: the crop")],
    # image 1
    [((330.5, 100.5, 413.0, 187.0), (300.2, 380.0), "flush with the right and bottom edges, right narrower"),
     ((100.0, 50.0, 180.0, 110.0), (90.0, 170.0), "integer-valued floats"),
     ((100.0, 50.0, 180.0, 110.0), (100.0, 180.0), "the same pixels, all-negative map, no shift")],
    # image 2: no ROI (equal consecutive offsets)
    [],
    # image 3
    [((10.9, 5.1, 60.2, 90.8), (0.0, 45.5), "fractional"),
     ((40.0, 60.0, 100.0, 140.0), (35.0, 95.0), "overlaps the fractional one"),
     ((250.0, 20.0, 251.0, 60.0), (200.0, 230.0), "one pixel wide, right 30 wide: crop to one column"),
     ((412.0, 0.0, 413.0, 187.0), (400.0, 401.0), "last column, full height")],
]
_NEGATIVE_ROI = 6                                                          # index into the concatenated list
_BIG_H, _BIG_W = 1100, 960                                                 # 1,056,000 pixels > 4096 * 256: the grid-stride loop
_BIG_BOXES = [[((0.0, 0.0, 960.0, 1100.0), (0.0, 940.0), "the whole image"),
               ((100.5, 200.5, 900.2, 1000.7), (60.0, 880.0), "interior, right wider"),
               ((500.0, 600.0, 960.0, 1100.0), (470.0, 900.0), "flush with the far corner")]]


def _box_tensors(images):
    lbs = [torch.tensor([b[0] for b in im], dtype=F32).reshape(-1, 4) for im in images]
    rbs = [torch.tensor([(b[1][0], b[0][1], b[1][1], b[0][3]) for b in im], dtype=F32).reshape(-1, 4) for im in images]
    return lbs, rbs, [len(im) for im in images]


def _union(lb, h, w):
    u = torch.zeros(h, w, dtype=torch.bool)
    for b in lb.tolist():
        x1, y1, x2, y2 = T.expand_box_to_integer(b)
        u[y1:y2, x1:x2] = True
    return u


def test_integer_valued_boxes_do_not_grow(dev):
    from disprcnn_amd import ops
    lbs, rbs, _ = _box_tensors(_BOXES)
    got = ops.integer_roi_boxes(torch.cat(lbs).to(dev), torch.cat(rbs).to(dev)).cpu()
    ref = [list(T.expand_box_to_integer(l)) + [T.expand_box_to_integer(r)[0], T.expand_box_to_integer(r)[2]]
           for l, r in zip(torch.cat(lbs).tolist(), torch.cat(rbs).tolist())]
    assert got.tolist() == ref
    assert got[0].tolist() == [20, 10, 120, 11, 5, 100] and got[2].tolist() == [300, 100, 301, 101, 290, 291]


def _run_paste(dev, images, h, w, S, clamp0, with_masks, tag):
    from disprcnn_amd import ops
    lbs, rbs, counts = _box_tensors(images)
    R = sum(counts)
    disp = synth.hash_uniform(f"tail:paste:{tag}:{S}", (R, S, S), -48.0, 48.0)
    if R > _NEGATIVE_ROI and len(images) > 1:
        disp[_NEGATIVE_ROI] = -disp[_NEGATIVE_ROI].abs() - 1.0
    masks = None
    if with_masks:
        masks = (synth.hash_uniform(f"tail:mask:{tag}", (R, h, w), 0.0, 1.0) > 0.3).float()
        masks[1 if R > 1 else 0] = 0                                      # one ROI masked out altogether
    boxes6 = ops.integer_roi_boxes(torch.cat(lbs).to(dev), torch.cat(rbs).to(dev))
    got = ops.disparity_paste(disp.to(dev), boxes6, counts, h, w, clamp0, masks.to(dev) if with_masks else None).cpu()
    assert tuple(got.shape) == (len(images), h, w)
    o = 0
    for b, c in enumerate(counts):
        m = masks[o:o + c] if with_masks else None
        ref = T.disparity_map(lbs[b], rbs[b], disp[o:o + c], h, w, clamp0, m)
        ref32 = P.disparity_map(lbs[b], rbs[b], disp[o:o + c], h, w, clamp0, m) if c else torch.zeros(h, w)
        _check(f"paste {tag} S={S} clamp0={int(clamp0)} masks={int(with_masks)} image {b}", got[b], ref, ref32)
        assert (got[b][~_union(lbs[b], h, w)] == 0).all(), f"image {b}: a pixel outside every box is not 0"
        if clamp0:
            assert (got[b] >= 0).all()
        if c == 0:
            assert (got[b] == 0).all()
        o += c
    return got


@pytest.mark.parametrize("S,clamp0,with_masks", [(1, False, False), (2, True, False), (28, False, True), (56, True, True), (224, False, False),
                                                 (224, True, True), (56, False, False)])
def test_disparity_paste_explicit_boxes_vs_fp64(dev, S, clamp0, with_masks):
    got = _run_paste(dev, _BOXES, IMG_H, IMG_W, S, clamp0, with_masks, "boxes")
    assert (got >= 0).all()                          # every image here has 0 or >= 2 ROIs: a negative value never survives the max


def test_disparity_paste_above_the_grid_cap_vs_fp64(dev):
    assert _BIG_H * _BIG_W > 4096 * 256
    _run_paste(dev, _BIG_BOXES, _BIG_H, _BIG_W, 8, False, False, "big")
    _run_paste(dev, _BIG_BOXES, _BIG_H, _BIG_W, 8, True, True, "big")


def _run_depth(dev, images, h, w, S, fuxb, tag):
    from disprcnn_amd import ops
    lbs, rbs, _ = _box_tensors(images)
    lb, rb = torch.cat(lbs), torch.cat(rbs)
    assert (rb[:, 0] <= lb[:, 0]).all()
    R = len(lb)
    disp = synth.hash_uniform(f"tail:depth:{tag}:{S}", (R, S, S), 8.0, 48.0)
    k = torch.as_tensor(fuxb, dtype=F32).expand(R)
    ref = torch.zeros(R, h, w, dtype=torch.float64)
    ref32 = torch.zeros(R, h, w)
    for r in range(R):
        d64, dd = T.roi_depth_maps(lb[r:r + 1], rb[r:r + 1], disp[r:r + 1], h, w, float(k[r]), return_disparity=True)
        inside = ~dd.isnan()
        assert inside.any() and dd[inside].min().item() >= 1.0, (tag, S, r, dd[inside].min().item())
        ref[r], ref32[r] = d64[0], P.roi_depth_maps(lb[r:r + 1], rb[r:r + 1], disp[r:r + 1], h, w, float(k[r]))[0]
    got = ops.roi_depth_maps(disp.to(dev), ops.integer_roi_boxes(lb.to(dev), rb.to(dev)), fuxb if isinstance(fuxb, float) else k.to(dev), h, w).cpu()
    _check(f"depth {tag} S={S}", got, ref, ref32)
    assert (got == 0).eq(ref == 0).all()
    for r in range(R):
        assert (got[r] != 0).eq(_union(lb[r:r + 1], h, w)).all()


@pytest.mark.parametrize("S", [1, 2, 28, 56, 224])
def test_roi_depth_maps_explicit_boxes_vs_fp64(dev, S):
    R = sum(len(im) for im in _BOXES)
    fuxb = 389.34 if S != 28 else synth.hash_uniform("tail:fuxb", (R,), 200.0, 400.0)
    _run_depth(dev, _BOXES, IMG_H, IMG_W, S, fuxb, "boxes")


def test_roi_depth_maps_above_the_grid_cap_vs_fp64(dev):
    _run_depth(dev, [_BIG_BOXES[0][:2]], _BIG_H, _BIG_W, 8, 389.34, "big")


# ------------------------------------------------------------------------------------------------ DisparityMap.resize
def _resize(dev, d, oh, ow, pool=False):
    from disprcnn_amd.structures import DisparityMap
    return DisparityMap(d.to(dev)).resize((ow, oh), use_max_pooling=pool).data.cpu()


@pytest.mark.parametrize("name,ihw,ohw", [("up", (37, 53), (80, 96)), ("down", (120, 200), (48, 64)), ("oh1", (20, 30), (1, 45)),
                                          ("ow1", (20, 30), (25, 1)), ("ih1", (1, 17), (5, 9)), ("one", (8, 8), (1, 1)),
                                          ("same40", (40, 40), (40, 40)), ("big", (37, 53), (_BIG_H, _BIG_W))])
def test_disparity_resize_bilinear_vs_fp64(dev, name, ihw, ohw):
    d = synth.hash_uniform(f"tail:resize:{name}", ihw, -48.0, 48.0)
    got = _resize(dev, d, *ohw)
    _check(f"resize bilinear {name}", got, T.disparity_resize(d, ohw[1], ohw[0]), T.disparity_resize(d, ohw[1], ohw[0], dtype=F32))


@pytest.mark.parametrize("pool", [False, True])
def test_disparity_resize_identity_is_exact(dev, pool):
    """IW = OW = 32: the division and the multiplication are exact, so is a blend with weights 1 and 0 and a 1 x 1 window."""
    d = synth.hash_uniform("tail:resize:identity", (24, 32), -48.0, 48.0)
    assert torch.equal(_resize(dev, d, 24, 32, pool), d)


def _pool_maps(ihw):
    u = synth.hash_uniform("tail:pool", ihw, -48.0, 48.0)
    return {"negative": -u.abs() - 0.5, "mixed": (u * 256).round() / 256, "zero": torch.zeros(ihw)}


@pytest.mark.parametrize("ohw", [(10, 7), (40, 60), (1, 1), (_BIG_H // 10, 53)])
@pytest.mark.parametrize("kind", ["negative", "mixed", "zero"])
def test_disparity_resize_max_pooling_vs_fp64(dev, kind, ohw):
    ihw = (37, 53)
    d = _pool_maps(ihw)[kind]
    ref = T.disparity_resize(d, ohw[1], ohw[0], True)
    if kind == "mixed" and ohw == (10, 7):          # windows that hold both signs: the two pooled parts are subtracted
        x = d[None, None]
        assert ((F.adaptive_max_pool2d(x.clamp_min(0), ohw) > 0) & (F.adaptive_max_pool2d((-x).clamp_min(0), ohw) > 0)).any()
    got = _resize(dev, d, *ohw, pool=True)
    assert tuple(got.shape) == ohw and torch.isfinite(got).all()
    excess = ((got.double() - ref).abs() - 2.0 ** -23 * ref.abs()).max().item()
    rel = ((got.double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item() if kind != "zero" else 0.0
    print(f"RATIO resize maxpool {kind} {ohw}: worst relative error {rel:.3e} = {rel * 2 ** 23:.3f} x 2^-23")
    assert excess <= 0.0, (kind, ohw, rel)
    if kind == "zero":
        assert (got == 0).all()
    if kind == "negative":
        assert (got < 0).all()

"""GPU parity tests: HIP path (through the C ABI) vs the CPU oracle and the committed golden fixtures.

Tolerances (stated): cost volume bit-exact; single conv layers |err| <= 2e-5*max|ref| + 1e-5
(fp32 FMA chains in a different summation order); disparities mean <= 1e-3 px, max <= 2e-2 px vs the
reference fp32 outputs (measured fp32-vs-fp64 floor of the reference itself: mean 9.4e-5 / max 2.0e-3).
"""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psmnet_oracle as O
from disprcnn_amd.utils import synth
from tests.helpers import golden_npz, state_for
from tests.test_oracle_golden import CV_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _close(got, ref, rel=2e-5, abs_=1e-5):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    tol = rel * ref.abs().max().item() + abs_
    err = (got - ref).abs().max().item()
    assert err <= tol, f"max err {err:.3e} > tol {tol:.3e}"


# ------------------------------------------------------------------------------------------------ a1
@pytest.mark.parametrize("mx,mn,shp", CV_CASES)
def test_cost_volume_bit_exact(dev, mx, mn, shp):
    from disprcnn_amd import ops
    z = golden_npz("cost_volume.npz")
    fl, fr = synth.synth_features(*shp, tag=f"cv{mx}_{mn}")
    c = ops.cost_volume(fl.to(dev), fr.to(dev), mx, mn)
    assert _sha(c) == str(z[f"cv_{mx}_{mn}_{'x'.join(map(str, shp))}_sha"])
    assert torch.equal(c.cpu(), O.cost_volume(fl, fr, mx, mn))


def test_cost_volume_odd_width_and_empty(dev):
    from disprcnn_amd import ops
    fl, fr = synth.synth_features(2, 3, 5, 13, tag="odd")
    c = ops.cost_volume(fl.to(dev), fr.to(dev), 8, -8)
    assert torch.equal(c.cpu(), O.cost_volume(fl, fr, 8, -8))
    e = ops.cost_volume(torch.zeros(0, 32, 28, 28, device=dev), torch.zeros(0, 32, 28, 28, device=dev), 48, 0)
    assert tuple(e.shape) == (0, 64, 12, 28, 28)


def test_cost_volume_blocked_matches_dense(dev):
    from disprcnn_amd import engine as E
    fl, fr = synth.synth_features(2, 32, 28, 28, tag="blk")
    out = E.Blocked(2, 64, 12, 28, 28, 1, 1, 1, dev)
    E.cost_volume_blocked(fl.to(dev), fr.to(dev), out, -24 // 4, 24 // 4, 0)
    assert torch.equal(out.to_dense().cpu(), O.cost_volume(fl, fr, 24, -24))
    v = out.view6()
    assert v[:, :, 0].abs().sum() == 0 and v[:, :, :, 0].abs().sum() == 0 and v[:, :, :, :, -1].abs().sum() == 0   # halo intact


def test_cost_volume_backward_is_adjoint(dev):
    """drc_cost_volume_bwd against the oracle's autograd (one shape; edge shapes in `test_hip_train_adjoints.py`)."""
    from disprcnn_amd import ops
    fl, fr = synth.synth_features(2, 4, 6, 20, tag="adj")
    g = synth.hash_uniform("adj:g", (2, 8, 6, 6, 20))
    fl.requires_grad_(True); fr.requires_grad_(True)
    c = O.cost_volume(fl * 1.0, fr * 1.0, 12, -12)
    # the oracle's slice assignment is differentiable in torch: autograd gives the reference adjoint
    (c * g).sum().backward()
    gl, gr = ops.cost_volume_backward(g.to(dev), 12, -12)
    _close(gl, fl.grad, 1e-6, 1e-6); _close(gr, fr.grad, 1e-6, 1e-6)


def test_layout_roundtrip_full_size(dev):
    """Size-independent property at BASELINE config-B size: dense -> blocked -> dense is the identity, halo stays 0."""
    from disprcnn_amd import engine as E
    x = synth.hash_uniform("rt", (2, 64, 24, 56, 56)).to(dev)
    b = E.Blocked(2, 64, 24, 56, 56, 1, 1, 1, dev).from_dense(x)
    assert torch.equal(b.to_dense(), x)
    assert abs(b.storage.double().sum().item() - x.double().sum().item()) < 1e-6 * x.numel()


@pytest.mark.parametrize("shape,pads", [((3, 3, 1, 20, 37), (0, 1, 1)), ((2, 24, 3, 9, 30), (1, 1, 1)), ((2, 32, 1, 28, 28), (0, 2, 2)),
                                        ((1, 40, 2, 5, 5), (1, 1, 1)), ((4, 32, 1, 7, 130), (0, 1, 1))])
def test_layout_roundtrip_shapes(dev, shape, pads):
    """Both dense -> blocked kernels (line-per-block with the LDS transpose; thread-per-float4 for narrow rows): identity
    round trip, zero halo and zero channel padding, against a torch restatement of the layout."""
    from disprcnn_amd import engine as E
    x = synth.hash_uniform(f"rt{shape}", shape).to(dev)
    n, c, d, h, w = shape
    b = E.Blocked(n, c, d, h, w, *pads, dev).from_dense(x)
    assert torch.equal(b.to_dense(), x)
    cb = (c + 15) // 16
    ref = torch.zeros(n, cb * 16, d + 2 * pads[0], h + 2 * pads[1], w + 2 * pads[2], device=dev)
    ref[:, :c, pads[0]:pads[0] + d, pads[1]:pads[1] + h, pads[2]:pads[2] + w] = x
    ref = ref.view(n, cb, 16, *ref.shape[2:]).permute(0, 1, 3, 4, 5, 2).contiguous()
    assert torch.equal(b.view6(), ref)


# ------------------------------------------------------------------------------------------------ a2-a6 layers
LAYERS = [  # cin, cout, stride, transposed, dims
    (64, 32, 1, False, (4, 12, 28)), (32, 32, 1, False, (3, 28, 28)), (32, 64, 2, False, (12, 28, 28)),
    (64, 64, 2, False, (6, 14, 14)), (64, 64, 1, False, (3, 7, 7)), (64, 64, 1, True, (3, 7, 7)),
    (64, 32, 1, True, (6, 14, 14)), (32, 32, 1, False, (2, 56, 56)), (16, 48, 1, False, (2, 5, 9)),
    (16, 48, 1, True, (2, 5, 9)), (32, 32, 1, True, (3, 12, 28)), (64, 64, 1, True, (1, 4, 4)), (24, 16, 1, True, (3, 9, 30)),
    (16, 48, 2, False, (6, 10, 18)), (32, 32, 2, False, (4, 8, 60)), (64, 64, 2, False, (2, 2, 2)), (24, 16, 2, False, (4, 24, 56)),
    (32, 32, 1, False, (12, 28, 28)),       # two units, default switches: the small-batch branch of plan_conv3d (tapdirect_kernel<7,1>)
]


@pytest.mark.parametrize("cin,cout,stride,transposed,dims", LAYERS)
def test_conv3d_layer_vs_oracle(dev, cin, cout, stride, transposed, dims):
    from disprcnn_amd import ops
    n = 2
    x = synth.hash_uniform(f"L{cin}{cout}{stride}{transposed}:x", (n, cin) + dims)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    w = synth.hash_uniform(f"L{cin}{cout}:w", wshape, -0.1, 0.1)
    scale = synth.hash_uniform("L:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("L:b", (cout,), -0.5, 0.5)
    if transposed:
        ref = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)
    else:
        ref = F.conv3d(x, w, None, stride, 1)
    res = synth.hash_uniform("L:r", tuple(ref.shape))
    ref = F.relu(ref * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1) + res)
    got = ops.conv3d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), stride, True, res.to(dev), transposed)
    assert got.shape == ref.shape
    _close(got, ref)


@pytest.mark.parametrize("cin,cout,dims", [(64, 32, (4, 12, 28)), (32, 32, (3, 28, 28)), (32, 32, (2, 56, 56)), (16, 48, (5, 5, 9)),
                                           (64, 64, (6, 14, 14)), (40, 24, (7, 9, 30))])
def test_conv3d_direct_kernel_vs_oracle(dev, cin, cout, dims):
    """The LDS-free sliding kernel (tapdirect.hip: operands straight from global memory, weights in the [tap][cb][cout][16]
    packing) on the stride-1 3x3x3 layers, incl. ragged tiles and channel counts that are not multiples of 16."""
    from disprcnn_amd import ops, engine as E
    n = 2
    x = synth.hash_uniform(f"D{cin}{cout}{dims}:x", (n, cin) + dims)
    w = synth.hash_uniform(f"D{cin}{cout}:w", (cout, cin, 3, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("D:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("D:b", (cout,), -0.5, 0.5)
    res = synth.hash_uniform(f"D{cout}{dims}:r", (n, cout) + dims)
    ref = F.relu(F.conv3d(x, w, None, 1, 1) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1) + res)
    saved = (E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"])
    E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"] = True, 2, 1      # force the sliding path at test sizes
    E.WINO["enabled"] = False
    try:
        xb = E.Blocked(n, cin, *dims, 1, 1, 1, dev)
        plan = E.plan_conv3d(xb, E.Blocked(n, cout, *dims, 1, 1, 1, dev), 1, cout, True)
        got = ops.conv3d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, True, res.to(dev))
    finally:
        E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"] = saved
    assert plan.direct and plan.slide and not plan.wino, "shape was expected to take the direct kernel"
    _close(got, ref)


@pytest.mark.parametrize("n,cin,cout,dims,with_res", [(2, 64, 32, (4, 12, 28), True), (3, 32, 32, (12, 28, 28), False), (1, 32, 32, (2, 56, 56), True),
                                                      (2, 16, 48, (6, 4, 10), True), (2, 64, 64, (6, 14, 14), False), (5, 40, 24, (8, 10, 30), True),
                                                      (1, 7, 33, (2, 2, 2), True), (9, 32, 32, (2, 2, 6), False)])
def test_conv3d_winograd_kernel_vs_oracle(dev, n, cin, cout, dims, with_res):
    """wino3d.hip (Winograd F(2x2x2,3x3x3), the default for stride-1 3x3x3 layers with even output dims) against the direct
    convolution: partial tile groups, blocks with fewer than four groups, one and two cout groups, channel counts that are
    not multiples of 16, with and without the residual.  Same tolerance as the direct kernels."""
    from disprcnn_amd import ops, engine as E
    x = synth.hash_uniform(f"W{cin}{cout}{dims}:x", (n, cin) + dims)
    w = synth.hash_uniform(f"W{cin}{cout}:w", (cout, cin, 3, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("W:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("W:b", (cout,), -0.5, 0.5)
    res = synth.hash_uniform(f"W{cout}{dims}:r", (n, cout) + dims) if with_res else None
    ref = F.conv3d(x, w, None, 1, 1) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    ref = F.relu(ref + res) if with_res else ref
    saved = (E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"])
    E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"] = True, 2, 1, True
    try:
        xb = E.Blocked(n, cin, *dims, 1, 1, 1, dev)
        plan = E.plan_conv3d(xb, E.Blocked(n, cout, *dims, 1, 1, 1, dev), 1, cout, True)
        got = ops.conv3d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, with_res, res.to(dev) if with_res else None)
    finally:
        E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"] = saved
    assert plan.wino, "shape was expected to take the Winograd kernel"
    _close(got, ref)


@pytest.mark.parametrize("n,cin,cout,dims,with_res,expect_rb", [
    (3, 32, 32, (12, 28, 28), True, True),       # the 32 -> 32 layers of Config A (TW = 14): chunks that straddle tile rows, slabs and ROIs
    (2, 64, 32, (4, 12, 28), False, True),       # TH = 6 != TW
    (5, 64, 64, (6, 14, 14), True, True),        # hourglass conv2 at half resolution (TW = 7, two cout groups, four channel blocks)
    (1, 32, 32, (2, 28, 28), False, True),       # fewer chunks than blocks, a partial last chunk
    (4, 40, 64, (4, 6, 14), True, True),         # three channel blocks (one partial), TH = 3 on a 14-wide map: a chunk spans four slabs
    (4, 40, 64, (4, 6, 28), True, False),        # the same on a 28-wide map: 18 row slots of the conflict-free layout exceed the LDS -> wino3d.hip
    (2, 32, 32, (4, 16, 56), True, True),        # a 56-wide map (Config B's volume): two strips of 14 tile columns
    (1, 16, 64, (2, 56, 84), False, True),       # three strips, TH = 28, one (partial) channel block, two cout groups
    (7, 48, 32, (2, 2, 14), True, False),        # TH = 1: more row slots than the LDS holds -> the engine keeps wino3d.hip
    (2, 32, 32, (4, 20, 20), True, False)])      # a width the row-brick kernel is not built for
def test_conv3d_winograd_rowbrick_kernel(dev, n, cin, cout, dims, with_res, expect_rb):
    """wino3d_rb.hip (round 3: two waves per SIMD, the input staged per block as depth- and w-transformed rows in LDS) against the direct
    convolution (same tolerance as the other kernels) AND against wino3d.hip, whose arithmetic it repeats operation for operation:
    bit-identical."""
    from disprcnn_amd import ops, engine as E
    x = synth.hash_uniform(f"RB{cin}{cout}{dims}:x", (n, cin) + dims)
    w = synth.hash_uniform(f"RB{cin}{cout}:w", (cout, cin, 3, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("RB:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("RB:b", (cout,), -0.5, 0.5)
    res = synth.hash_uniform(f"RB{cout}{dims}:r", (n, cout) + dims) if with_res else None
    ref = F.conv3d(x, w, None, 1, 1) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    ref = F.relu(ref + res) if with_res else ref
    saved = (E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"], E.WINO["rb"], E.WINO["rb_min_chunks"])
    E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"] = True, 2, 1, True
    got = {}
    try:
        for rb in (True, False):
            E.WINO["rb"], E.WINO["rb_min_chunks"] = rb, 0
            xb = E.Blocked(n, cin, *dims, 1, 1, 1, dev)
            plan = E.plan_conv3d(xb, E.Blocked(n, cout, *dims, 1, 1, 1, dev), 1, cout, True)
            assert plan.wino and plan.rb == (rb and expect_rb), (plan.kname, rb)
            got[rb] = ops.conv3d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, with_res, res.to(dev) if with_res else None)
    finally:
        E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"], E.WINO["rb"], E.WINO["rb_min_chunks"] = saved
    _close(got[True], ref)
    assert torch.equal(got[True], got[False]), (got[True] - got[False]).abs().max().item()


def test_winograd_rowbrick_weight_packing(dev):
    """drc_pack_weights_wino_rb = drc_pack_weights_wino re-ordered to [xi][cb][cout tile][ch / 4][cout % 16][ch % 4] (cout padded to 32)."""
    from disprcnn_amd import engine as E
    for cout, cin, transposed, flip in [(32, 32, False, False), (20, 40, False, False), (64, 16, True, True)]:
        w = synth.hash_uniform(f"RBW{cout}{cin}", (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), -1, 1).to(dev)
        a = E.pack_weight_wino(w, transposed, flip).cpu()                # [64][cb][cout_pad16][16]
        b = E.pack_weight_wino_rb(w, transposed, flip).cpu()             # [64][cb][cout_pad32][16] in rb order
        cb, cp16, cp32 = a.shape[1], a.shape[2], b.shape[2]
        a32 = torch.zeros(64, cb, cp32, 16)
        a32[:, :, :cp16] = a
        want = a32.view(64, cb, cp32 // 16, 16, 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(64, cb, cp32, 16)   # [ct][j][g][s] -> [ct][g][j][s]
        assert torch.equal(b, want)


@pytest.mark.parametrize("n,C,cout,D,H,W,lo4,pad", [(3, 32, 32, 12, 28, 28, 0, 1), (2, 32, 32, 6, 28, 28, -6, 1), (5, 16, 48, 8, 10, 30, 3, 2),
                                                     (1, 32, 32, 24, 56, 56, 0, 1), (2, 32, 32, 4, 6, 2, -1, 1), (19, 32, 32, 12, 28, 28, 0, 1),
                                                     (8, 32, 32, 8, 56, 56, -2, 1)])
def test_conv3d_winograd_fused_cost_volume(dev, n, C, cout, D, H, W, lo4, pad):
    """wino3d_cv_kernel (dres0[0] reading the 2D feature maps, cost volume never materialised; stackhourglass.py:115-130):
    bit-identical to drc_cost_volume_blocked_fwd + drc_conv3d_k3_wino_fwd, and within the layer tolerance of the oracle's
    volume convolved directly.  Covers negative / positive mindisp, widths below the disparity range, feature halos > 1,
    a right side named as a later range of the same tensor, and partial tile groups.  The two largest cases take the round-3 row-brick
    kernel and its fused form (wino3d_rb.hip: 28-wide maps, and a 56-wide map walked as two strips)."""
    from disprcnn_amd import engine as E
    fl = synth.hash_uniform(f"CV{n}{C}{H}{W}:l", (n, C, H, W))
    fr = synth.hash_uniform(f"CV{n}{C}{H}{W}:r", (n, C, H, W))
    w = synth.hash_uniform(f"CV{C}{cout}:w", (cout, 2 * C, 3, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("CV:s", (cout,), 0.5, 1.5).to(dev)
    shift = synth.hash_uniform("CV:b", (cout,), -0.5, 0.5).to(dev)
    mn, mx = 4 * lo4, 4 * (lo4 + D)
    cost = O.cost_volume(fl, fr, mx, mn)
    ref = F.relu(F.conv3d(cost, w, None, 1, 1) * scale.cpu().view(1, -1, 1, 1, 1) + shift.cpu().view(1, -1, 1, 1, 1))
    saved = (E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"])
    E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"] = True, 2, 1, True
    try:
        xb = E.Blocked(n, 2 * C, D, H, W, 1, 1, 1, dev)
        y0, y1 = E.Blocked(n, cout, D, H, W, 1, 1, 1, dev), E.Blocked(n, cout, D, H, W, 1, 1, 1, dev)
        plan = E.plan_conv3d(xb, y0, 1, cout, True)
    finally:
        E.DIRECT["enabled"], E.SLIDE["min_od"], E.SLIDE["min_units"], E.WINO["enabled"] = saved
    assert plan.wino
    w16p = w16 = plan.pack16(w.to(dev))                # the plan's own packing (wino3d.hip; at n = 19 wino3d_rb.hip -- both have a fused form)
    both = E.Blocked(2 * n, C, 1, H, W, 0, pad, pad, dev).from_dense(torch.cat((fl, fr), 0).to(dev))      # left maps, then right maps
    E.cost_volume_blocked(fl.to(dev), fr.to(dev), xb, lo4, lo4 + D, 0)
    plan.run(xb, w16p, scale, shift, y0, w16=w16p)
    plan.run_costvol(both, (both, n), lo4, w16, scale, shift, y1)
    torch.cuda.synchronize()
    a, b = y0.to_dense(), y1.to_dense()
    assert torch.equal(a, b), f"fused differs from materialised: max {(a - b).abs().max().item():.3e}"
    _close(b, ref)
    # separate left / right tensors
    fL = E.Blocked(n, C, 1, H, W, 0, pad, pad, dev).from_dense(fl.to(dev))
    fR = E.Blocked(n, C, 1, H, W, 0, pad, pad, dev).from_dense(fr.to(dev))
    y2 = E.Blocked(n, cout, D, H, W, 1, 1, 1, dev)
    plan.run_costvol(fL, fR, lo4, w16, scale, shift, y2)
    assert torch.equal(y2.to_dense(), a)


@pytest.mark.parametrize("n,cin,cout,hw,with_res", [(4, 32, 32, (112, 112), True), (3, 64, 64, (56, 56), False), (2, 128, 128, (28, 28), True),
                                                     (5, 7, 33, (2, 30), True), (9, 64, 32, (4, 4), False), (2, 20, 40, (8, 4), True),
                                                     (1, 16, 16, (2, 2), False),
                                                     # odd maps (round 3): half-used last tile row / column
                                                     (2, 64, 64, (47, 155), True), (3, 32, 48, (13, 20), False), (2, 20, 40, (8, 5), True),
                                                     (4, 16, 16, (1, 1), False), (2, 48, 32, (7, 7), True)])
def test_conv2d_winograd_kernel_vs_oracle(dev, n, cin, cout, hw, with_res):
    """wino2d.hip (Winograd F(2x2,3x3), the default for stride-1 undilated 3x3 Conv2d layers on even maps with enough work)
    against the direct convolution: partial tile groups, 1..4 cout groups, channel counts that are not multiples of 16, with
    and without the residual.  Same tolerance as the direct kernels."""
    from disprcnn_amd import ops, engine as E
    x = synth.hash_uniform(f"W2{cin}{cout}{hw}:x", (n, cin) + hw)
    w = synth.hash_uniform(f"W2{cin}{cout}:w", (cout, cin, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("W2:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("W2:b", (cout,), -0.5, 0.5)
    res = synth.hash_uniform(f"W2{cout}{hw}:r", (n, cout) + hw) if with_res else None
    ref = F.conv2d(x, w, None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.relu(ref + res) if with_res else ref
    saved = (E.WINO2D["enabled"], E.WINO2D["min_chunks"])
    E.WINO2D["enabled"], E.WINO2D["min_chunks"] = True, 0
    try:
        xb = E.Blocked(n, cin, 1, *hw, 0, 1, 1, dev)
        plan = E.plan_conv2d(xb, E.Blocked(n, cout, 1, *hw, 0, 1, 1, dev), 3, 1, 1, 1, cout, True)
        got = ops.conv2d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, 1, 1, with_res, res.to(dev) if with_res else None)
    finally:
        E.WINO2D["enabled"], E.WINO2D["min_chunks"] = saved
    assert plan.wino and plan.c2d, "shape was expected to take the 2D Winograd kernel"
    _close(got, ref)


@pytest.mark.parametrize("n,cin,cout,hw,dil,with_res", [(3, 128, 128, (56, 56), 2, True), (2, 32, 48, (16, 24), 2, False), (2, 20, 16, (16, 8), 4, True),
                                                         (5, 64, 32, (4, 12), 2, True)])
def test_conv2d_winograd_dilated_vs_oracle(dev, n, cin, cout, hw, dil, with_res):
    """Round 3: dilated 3x3 layers (pad = dilation; feature CNN layer4, submodule.py:71) on the 2D Winograd kernel as d*d interleaved
    sub-grids, against the direct dilated convolution; maps that 2d does not divide stay on the direct kernel."""
    from disprcnn_amd import ops, engine as E
    x = synth.hash_uniform(f"W2d{cin}{cout}{hw}:x", (n, cin) + hw)
    w = synth.hash_uniform(f"W2d{cin}{cout}:w", (cout, cin, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("W2d:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("W2d:b", (cout,), -0.5, 0.5)
    res = synth.hash_uniform(f"W2d{cout}{hw}:r", (n, cout) + hw) if with_res else None
    ref = F.conv2d(x, w, None, 1, dil, dil) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.relu(ref + res) if with_res else ref
    saved = (E.WINO2D["enabled"], E.WINO2D["min_chunks"])
    E.WINO2D["enabled"], E.WINO2D["min_chunks"] = True, 0
    try:
        xb = E.Blocked(n, cin, 1, *hw, 0, dil, dil, dev)
        plan = E.plan_conv2d(xb, E.Blocked(n, cout, 1, *hw, 0, 1, 1, dev), 3, 1, dil, dil, cout, True)
        odd = E.plan_conv2d(E.Blocked(n, cin, 1, hw[0] + 2, hw[1], 0, dil, dil, dev), E.Blocked(n, cout, 1, hw[0] + 2, hw[1], 0, 1, 1, dev), 3, 1, dil, dil, cout, True)
        got = ops.conv2d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, dil, dil, with_res, res.to(dev) if with_res else None)
    finally:
        E.WINO2D["enabled"], E.WINO2D["min_chunks"] = saved
    assert plan.wino and plan.c2d and not odd.wino
    _close(got, ref)


@pytest.mark.parametrize("n,cin,cout,hw,with_res,expect_rb", [
    (3, 32, 32, (112, 112), True, True),         # firstconv / layer1 of the PSMNet feature CNN: four strips of 14 tile columns
    (2, 64, 64, (56, 56), False, True),          # layer2: two strips, two cout groups
    (2, 320, 128, (56, 56), True, True),         # lastconv[0]: 20 channel blocks, four cout groups
    (5, 20, 40, (6, 28), True, False),           # cout padded to 48: not a multiple of 32 -> wino2d.hip
    (3, 48, 64, (10, 14), False, True),          # a 14-wide map (TW = 7), TH = 5
    (2, 32, 32, (30, 60), True, False)])         # a width the row-brick kernel is not built for
def test_conv2d_winograd_rowbrick_kernel(dev, n, cin, cout, hw, with_res, expect_rb):
    """The 2D form of wino3d_rb.hip (round 3; Conv2d 3x3 of submodule.py:13-17 on the 112- / 56-wide maps of the feature CNN) against the
    direct convolution and, bit for bit, against wino2d.hip."""
    from disprcnn_amd import ops, engine as E
    x = synth.hash_uniform(f"RB2{cin}{cout}{hw}:x", (n, cin) + hw)
    w = synth.hash_uniform(f"RB2{cin}{cout}:w", (cout, cin, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("RB2:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("RB2:b", (cout,), -0.5, 0.5)
    res = synth.hash_uniform(f"RB2{cout}{hw}:r", (n, cout) + hw) if with_res else None
    ref = F.conv2d(x, w, None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.relu(ref + res) if with_res else ref
    saved = (E.WINO2D["enabled"], E.WINO2D["min_chunks"], E.WINO2D["rb"], E.WINO2D["rb_min_chunks"], E.WINO2D["rb_max_cb"])
    got = {}
    try:
        for rb in (True, False):
            E.WINO2D["enabled"], E.WINO2D["min_chunks"], E.WINO2D["rb"], E.WINO2D["rb_min_chunks"], E.WINO2D["rb_max_cb"] = True, 0, rb, 0, 1 << 20
            xb = E.Blocked(n, cin, 1, *hw, 0, 1, 1, dev)
            plan = E.plan_conv2d(xb, E.Blocked(n, cout, 1, *hw, 0, 1, 1, dev), 3, 1, 1, 1, cout, True)
            assert plan.wino and plan.c2d and plan.rb == (rb and expect_rb), (plan.kname, rb)
            got[rb] = ops.conv2d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, 1, 1, with_res, res.to(dev) if with_res else None)
    finally:
        E.WINO2D["enabled"], E.WINO2D["min_chunks"], E.WINO2D["rb"], E.WINO2D["rb_min_chunks"], E.WINO2D["rb_max_cb"] = saved
    _close(got[True], ref)
    assert torch.equal(got[True], got[False]), (got[True] - got[False]).abs().max().item()


def test_winograd2d_weight_transform_vs_oracle(dev):
    """drc_pack_weights_wino2d against U = (G x G) g in float64, incl. the in/out swap and tap flip of the data gradient."""
    from disprcnn_amd import engine as E
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    for cout, cin, transposed, flip in [(32, 32, False, False), (20, 40, False, False), (24, 16, True, True)]:
        w = synth.hash_uniform(f"WT2{cout}{cin}", (cin, cout, 3, 3) if transposed else (cout, cin, 3, 3), -1, 1)
        got = E.pack_weight_wino2d(w.to(dev), transposed, flip).cpu()
        wc = w.transpose(0, 1) if transposed else w
        wc = wc.flip(2, 3) if flip else wc
        U = torch.einsum("ai,bj,ocij->aboc", G, G, wc.double())                   # [xh][xw][cout][cin]
        cb, cp = (cin + 15) // 16, (cout + 15) // 16 * 16
        ref = torch.zeros(16, cb * 16, cp, dtype=torch.float64)
        ref[:, :cin, :cout] = U.reshape(16, cout, cin).transpose(1, 2)
        ref = ref.view(16, cb, 16, cp).permute(0, 1, 3, 2)
        assert got.shape == ref.shape
        assert (got.double() - ref).abs().max().item() < 1e-6


def test_winograd_weight_transform_vs_oracle(dev):
    """drc_pack_weights_wino against U = (G x G x G) g in float64, incl. the in/out swap and tap flip of the data gradient."""
    from disprcnn_amd import engine as E
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    for cout, cin, transposed, flip in [(32, 32, False, False), (20, 40, False, False), (24, 16, True, True)]:
        w = synth.hash_uniform(f"WT{cout}{cin}", (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), -1, 1)
        got = E.pack_weight_wino(w.to(dev), transposed, flip).cpu()
        wc = w.transpose(0, 1) if transposed else w
        wc = wc.flip(2, 3, 4) if flip else wc
        U = torch.einsum("ai,bj,ek,ocijk->abeoc", G, G, G, wc.double())          # [xd][xh][xw][cout][cin]
        cb, cp = (cin + 15) // 16, (cout + 15) // 16 * 16
        ref = torch.zeros(64, cb * 16, cp, dtype=torch.float64)
        ref[:, :cin, :cout] = U.reshape(64, cout, cin).transpose(1, 2)
        ref = ref.view(64, cb, 16, cp).permute(0, 1, 3, 2)
        assert got.shape == ref.shape
        assert (got.double() - ref).abs().max().item() < 1e-6


@pytest.mark.parametrize("n,cout,hw", [(3, 32, (224, 224)), (2, 32, (30, 52)), (2, 20, (17, 35)), (1, 16, (6, 4)), (2, 32, (375, 1242))])
def test_stem_conv_from_dense_image_vs_oracle(dev, n, cout, hw):
    """stemconv.hip: Conv2d(3 -> cout, 3x3, stride 2, pad 1) + folded BN + ReLU read straight from the dense NCHW image, contraction over
    (channel, tap) = 27 (reference: feature_extraction.firstconv[0], submodule.py:65-66) -- against the oracle convolution; even and odd
    sizes, ragged 16-pixel tiles, cout 16 / 20 (padded) / 32; the halo of the blocked output stays zero."""
    from disprcnn_amd import engine as E
    x = synth.hash_uniform(f"ST{n}{hw}:x", (n, 3) + hw, -1.0, 1.0)
    w = synth.hash_uniform(f"ST{cout}:w", (cout, 3, 3, 3), -0.5, 0.5)
    scale = synth.hash_uniform("ST:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("ST:b", (cout,), -0.5, 0.5)
    ref = F.relu(F.conv2d(x, w, None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    oh, ow = ref.shape[2:]
    cp = E.cout_pad_of(cout)
    sc = torch.ones(cp, device=dev); sh = torch.zeros(cp, device=dev)
    sc[:cout] = scale.to(dev); sh[:cout] = shift.to(dev)
    yb = E.Blocked(n, cout, 1, oh, ow, 0, 1, 1, dev)
    wp = E.pack_weight_stem(w.to(dev))
    assert tuple(wp.shape) == (7, cp, 4) and wp[6, :, 3].abs().sum().item() == 0          # k = 27 is padding
    E.stem_conv(x.to(dev), wp, sc, sh, yb, True)
    got = yb.to_dense().cpu()[:, :, 0]
    assert got.shape == ref.shape
    _close(got, ref)
    v = yb.view6()
    assert v[:, :, :, 0].abs().sum() == 0 and v[:, :, :, -1].abs().sum() == 0 and v[:, :, :, :, 0].abs().sum() == 0 and v[:, :, :, :, -1].abs().sum() == 0
    # the generic path (layout conversion + stride-2 direct kernel) agrees to summation order
    xb = E.Blocked(n, 3, 1, hw[0], hw[1], 0, 1, 1, dev).from_dense(x.to(dev).unsqueeze(2))
    y2 = E.Blocked(n, cout, 1, oh, ow, 0, 1, 1, dev)
    if hw[0] % 2 == 0 and hw[1] % 2 == 0:
        plan = E.plan_conv2d(xb, y2, 3, 2, 1, 1, cout, True)
        plan.run(xb, E.pack_weight(w.to(dev)), sc, sh, y2, None, w16=plan.pack16(w.to(dev), False))
        assert (y2.to_dense().cpu()[:, :, 0] - got).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-6


@pytest.mark.parametrize("cin,cout,dims", [(64, 64, (3, 7, 7)), (64, 32, (6, 14, 14)), (16, 48, (2, 5, 9)), (24, 16, (3, 9, 30)), (64, 64, (1, 4, 4))])
def test_deconv_lds_staged_variant_vs_oracle(dev, cin, cout, dims):
    """tapdeconv.hip (LDS-staged fused transposed conv, the round-1 default) stays selectable with engine.DECONV_DIRECT off; the
    default LDS-free deconvdirect.hip is what test_conv3d_layer_vs_oracle's transposed cases run."""
    from disprcnn_amd import ops, engine as E
    x = synth.hash_uniform(f"TD{cin}{cout}:x", (2, cin) + dims)
    w = synth.hash_uniform(f"TD{cin}{cout}:w", (cin, cout, 3, 3, 3), -0.1, 0.1)
    scale = synth.hash_uniform("TD:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("TD:b", (cout,), -0.5, 0.5)
    ref = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    res = synth.hash_uniform("TD:r", tuple(ref.shape))
    ref = F.relu(ref + res)
    saved = E.DECONV_DIRECT["enabled"]
    try:
        E.DECONV_DIRECT["enabled"] = True
        xb = E.Blocked(2, cin, *dims, 1, 1, 1, dev)
        yb = E.Blocked(2, cout, *(2 * d for d in dims), 1, 1, 1, dev)
        assert E.plan_deconv3d(xb, yb, cout, True).deconv_direct
        E.DECONV_DIRECT["enabled"] = False
        plan = E.plan_deconv3d(xb, yb, cout, True)
        assert plan.fused_deconv and not plan.deconv_direct
        got = ops.conv3d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), 1, True, res.to(dev), True)
    finally:
        E.DECONV_DIRECT["enabled"] = saved
    _close(got, ref)


@pytest.mark.parametrize("kind,cin,cout,stride,dims", [("3d", 32, 32, 1, (6, 28, 28)), ("3d", 64, 32, 1, (4, 12, 28)), ("3d", 32, 64, 2, (12, 28, 28)),
                                                       ("3d", 16, 48, 2, (6, 10, 18)), ("2d", 32, 32, 1, (40, 56)), ("2d", 128, 128, 1, (28, 28))])
def test_generic_kernel_variants_vs_oracle(dev, kind, cin, cout, stride, dims):
    """engine.DIRECT['enabled'] = False sends every layer to the generic kernel (tapconv.hip: any tap grid, LDS-staged tiles) -- the fallback
    the planners keep for shapes the specialised kernels do not take; same layers, same tolerance as the default kernels.  (The LDS-staged
    specialisations of rounds 1-2 -- tapslide / tapdown / tap2d -- left the library in round 6: attic/.)"""
    from disprcnn_amd import ops, engine as E
    n = 2
    x = synth.hash_uniform(f"V{kind}{cin}{cout}{stride}:x", (n, cin) + dims)
    w = synth.hash_uniform(f"V{kind}{cin}{cout}:w", (cout, cin) + (3,) * len(dims), -0.1, 0.1)
    scale = synth.hash_uniform("V:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("V:b", (cout,), -0.5, 0.5)
    bc = (1, -1) + (1,) * len(dims)
    saved = (E.DIRECT["enabled"], E.SLIDE["min_units"])
    E.DIRECT["enabled"], E.SLIDE["min_units"] = False, 1
    try:
        xb = E.Blocked(n, cin, *((dims if kind == "3d" else (1,) + dims)), 1 if kind == "3d" else 0, 1, 1, dev)
        od = tuple(-(-d // stride) for d in dims)
        yb = E.Blocked(n, cout, *((od if kind == "3d" else (1,) + od)), 1 if kind == "3d" else 0, 1, 1, dev)
        pl = E.plan_conv3d(xb, yb, stride, cout, True) if kind == "3d" else E.plan_conv2d(xb, yb, 3, stride, 1, 1, cout, True)
        assert pl.kname.startswith("tapconv_kernel") and not (pl.direct or pl.wino or pl.down or pl.slide), pl.kname
        if kind == "3d":
            ref = F.relu(F.conv3d(x, w, None, stride, 1) * scale.view(bc) + shift.view(bc))
            got = ops.conv3d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), stride, True, None)
        else:
            ref = F.relu(F.conv2d(x, w, None, stride, 1) * scale.view(bc) + shift.view(bc))
            got = ops.conv2d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), stride, 1, 1, True, None)
    finally:
        E.DIRECT["enabled"], E.SLIDE["min_units"] = saved
    _close(got, ref)


@pytest.mark.parametrize("cin,cout,k,stride,pad,dil,hw", [(3, 32, 3, 2, 1, 1, (64, 80)), (32, 32, 3, 1, 1, 1, (40, 56)),
                                                         (32, 64, 1, 2, 0, 1, (40, 56)), (128, 128, 3, 1, 2, 2, (28, 28)),
                                                         (320, 128, 3, 1, 1, 1, (12, 20)), (128, 32, 1, 1, 0, 1, (3, 3)),
                                                         (256, 64, 1, 1, 0, 1, (47, 80)), (24, 40, 1, 1, 0, 1, (5, 7)),
                                                         (64, 256, 1, 2, 0, 1, (31, 45)), (512, 128, 1, 1, 0, 1, (24, 78))])
def test_conv2d_layer_vs_oracle(dev, cin, cout, k, stride, pad, dil, hw):
    from disprcnn_amd import ops
    x = synth.hash_uniform(f"C{cin}{cout}{k}:x", (2, cin) + hw)
    w = synth.hash_uniform(f"C{cin}{cout}{k}:w", (cout, cin, k, k), -0.1, 0.1)
    scale = synth.hash_uniform("C:s", (cout,), 0.5, 1.5)
    shift = synth.hash_uniform("C:b", (cout,), -0.5, 0.5)
    ref = F.conv2d(x, w, None, stride, pad, dil) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    got = ops.conv2d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), stride, pad, dil, False, None, in_halo=max(pad, 1))
    assert got.shape == ref.shape
    _close(got, ref)
    res = synth.hash_uniform(f"C{cin}{cout}{k}:r", tuple(ref.shape))                      # + residual + ReLU (Bottleneck conv3)
    got = ops.conv2d_bn(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), stride, pad, dil, True, res.to(dev), in_halo=max(pad, 1))
    _close(got, F.relu(ref + res))


@pytest.mark.parametrize("n,dims", [(3, (12, 28, 28)), (2, (6, 56, 56)), (2, (5, 9, 13)), (1, (1, 3, 112)), (2, (3, 30, 7)),
                                    (2, (24, 56, 56)), (1, (13, 28, 28)), (1, (9, 16, 20))])      # few columns: depth segments (round 3)
def test_classifier_conv_cout1_vs_oracle(dev, n, dims):
    """Conv3d(32->1, k3, p1, bias=False) + cumulative head add (stackhourglass.py:78-88,142-144): the MFMA 1x1x1-GEMM +
    shifted-sum kernel (and its scalar fallback shapes) vs F.conv3d; 2e-5 * max|ref| + 1e-5."""
    from disprcnn_amd import engine as E
    x = synth.hash_uniform(f"c1{dims}:x", (n, 32) + dims)
    w = synth.hash_uniform("c1:w", (1, 32, 3, 3, 3), -0.1, 0.1)
    res = synth.hash_uniform(f"c1{dims}:r", (n,) + dims)
    ref = F.conv3d(x, w, None, 1, 1)[:, 0] + res
    xb = E.Blocked(n, 32, *dims, 1, 1, 1, dev)
    xb.from_dense(x.to(dev))
    out = torch.empty(n, *dims, device=dev)
    E.conv3d_cout1(xb, E.pack_weight_cout1(w.to(dev)), res.to(dev), out)
    _close(out, ref)
    out2 = torch.empty(n, *dims, device=dev)
    E.conv3d_cout1(xb, E.pack_weight_cout1(w.to(dev)), None, out2)           # no head add
    _close(out2, ref - res)


def test_upsample_softargmin_vs_oracle(dev):
    from disprcnn_amd import ops
    for (dp, hp, wp, mx, mn) in [(12, 28, 28, 48, 0), (24, 56, 56, 48, -48), (12, 28, 28, 24, -24)]:
        cost = synth.hash_uniform(f"sa{dp}{mn}", (2, 1, dp, hp, wp), -3.0, 3.0)
        ref = O.upsample_softargmin(cost, mx, mn, 4 * hp, 4 * wp)
        got = ops.upsample_softargmin(cost.to(dev), mx, mn, 4 * hp, 4 * wp).cpu()
        err = (got - ref).abs()
        assert err.mean().item() < 1e-4 and err.max().item() < 2e-3, (err.mean().item(), err.max().item())


def test_upsample_softargmin_sharp_costs(dev):
    """Cost columns with |c| ~ 2000 and neighbours of opposite sign (an untrained regressor on out-of-range crops produces them):
    every exp underflows unless the softmax shift is the maximum of the UPSAMPLED column -- the kernel used the maximum of the coarse
    slices and returned 0/0 there.  Forward vs the oracle, backward finite and equal to the oracle's autograd."""
    from disprcnn_amd import ops
    dp, hp, wp, mx, mn = 24, 14, 14, 48, -48
    cost = synth.hash_uniform("sharp", (2, 1, dp, hp, wp), -2000.0, 2000.0)
    ref = O.upsample_softargmin(cost, mx, mn, 4 * hp, 4 * wp)
    got = ops.upsample_softargmin(cost.to(dev), mx, mn, 4 * hp, 4 * wp).cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert err.mean().item() < 1e-3 and err.max().item() < 5e-2, (err.mean().item(), err.max().item())
    from disprcnn_amd import _lib, engine as E
    c = cost[:, 0].contiguous().to(dev)
    gd = synth.hash_uniform("sharp:g", (2, 4 * hp, 4 * wp), -1.0, 1.0).to(dev)
    g = torch.full_like(c, float("nan"))                       # overwritten by the gather launch
    foot = E.scratch(dev, "softargmin_bwd", _lib.lib().drc_upsample_softargmin_bwd_scratch_floats(2, dp, hp, wp, 4 * hp, 4 * wp))
    st = _lib.lib().drc_upsample_softargmin_bwd(E._ptr(c), E._ptr(gd), E._ptr(g), 2, dp, hp, wp, mx - mn, 4 * hp, 4 * wp, mn, E._ptr(foot),
                                                foot.numel(), E._stream_ptr(dev))
    _lib.check(st, "drc_upsample_softargmin_bwd")
    assert torch.isfinite(g).all()
    cr = cost.double().requires_grad_()
    O.upsample_softargmin(cr, mx, mn, 4 * hp, 4 * wp).backward(gd.cpu().double())
    gref = cr.grad[:, 0]
    assert (g.cpu().double() - gref).abs().max().item() <= 1e-3 * max(gref.abs().max().item(), 1e-3) + 1e-6


# ------------------------------------------------------------------------------------------------ whole path
def _model(dev, case, mx, mn, math="auto"):
    """math: PSMNet.regressor_math -- "auto" (round-5 default: the full-resolution stride-1 3D layers in split-f16 arithmetic where the shape
    allows) or "f32" (every 3D layer on the fp32 MFMA kernels)."""
    from disprcnn_amd.modeling.psmnet.stackhourglass import PSMNet
    m = PSMNet(mx, mn)
    m.load_state_dict(state_for(case), strict=True)
    m.regressor_math = math
    m.feature_math = math           # the same switch for the 2D CNN's stride-1 3x3 layers (convs16r.hip)
    return m.to(dev).eval()


@pytest.mark.parametrize("math", ["f32", "auto"])
@pytest.mark.parametrize("case,mx,mn", [("A", 48, 0), ("At", 48, 0), ("A2", 24, -24)])
def test_config_a_vs_golden(dev, case, mx, mn, math):
    z = golden_npz()
    m = _model(dev, "At" if case == "At" else "A", mx, mn, math)
    fl, fr = synth.synth_features(2, 32, 28, 28, tag="caseA")
    with torch.no_grad():
        pred = m.forward_from_features(fl.to(dev), fr.to(dev), (112, 112)).cpu()
    ref = torch.from_numpy(z[f"{case}_pred"])
    err = (pred - ref).abs()
    print(case, "mean/max err px", err.mean().item(), err.max().item())
    assert err.mean().item() < 1e-3 and err.max().item() < 2e-2, (err.mean().item(), err.max().item())
    # intermediates: cost3 of the HIP path vs the oracle (sampled by the golden file too)
    rt = m._rt
    ws = rt._ws[("3d" if math == "f32" else "3ds16", 2, (mx - mn) // 4, 28, 28)]
    cost3 = ws["t"]["costk3"].cpu().reshape(-1)
    idx = torch.from_numpy(z[f"{case}_cost3_idx"]); val = torch.from_numpy(z[f"{case}_cost3_val"])
    assert (cost3[idx] - val).abs().max().item() < 1e-3 * max(1.0, val.abs().max().item())
    out3 = ws["t"]["out3"].to_dense().cpu().reshape(-1)
    idx = torch.from_numpy(z[f"{case}_out3_idx"]); val = torch.from_numpy(z[f"{case}_out3_val"])
    assert (out3[idx] - val).abs().max().item() < 1e-4 * max(1.0, val.abs().max().item()) + 1e-4


@pytest.mark.parametrize("math", ["f32", "auto"])
def test_config_b_vs_golden(dev, math):
    z = golden_npz()
    m = _model(dev, "B", 48, -48, math)
    left, right = synth.synth_images(2, 224, 224, tag="caseB")
    with torch.no_grad():
        pred = m((left.to(dev), right.to(dev))).cpu()
        pred2 = m({"left": left.to(dev), "right": right.to(dev)}).cpu()
    assert torch.equal(pred, pred2)                    # dict and tuple inputs, deterministic
    ref = torch.from_numpy(z["B_pred"])
    err = (pred - ref).abs()
    print("B mean/max err px", err.mean().item(), err.max().item())
    assert err.mean().item() < 1e-3 and err.max().item() < 2e-2, (err.mean().item(), err.max().item())
    feat = m._rt._ws[("2d" if math == "f32" else "2ds16", 4, 224, 224)]["t"]["feat"].to_dense().cpu()[:, :, 0]
    flat = feat[:2].reshape(-1)
    idx = torch.from_numpy(z["B_featL_idx"]); val = torch.from_numpy(z["B_featL_val"])
    assert (flat[idx] - val).abs().max().item() < 1e-4 * max(1.0, val.abs().max().item()) + 1e-4


def test_empty_roi_batch(dev):
    m = _model(dev, "A", 48, 0)
    out = m.forward_from_features(torch.zeros(0, 32, 28, 28, device=dev), torch.zeros(0, 32, 28, 28, device=dev), (112, 112))
    assert tuple(out.shape) == (0, 112, 112)


def test_batch_independence_large(dev):
    """Size-independent properties at a bench-like batch size.  (1) Waves never mix ROIs and the FMA order does not depend on
    where a ROI sits in the batch: permuting the batch permutes the output BITWISE.  (2) The same ROI run alone takes other
    kernels (the launch heuristics pick per batch size; their k-step groupings differ), so it matches to fp32 rounding."""
    m = _model(dev, "A", 48, 0)
    fl, fr = synth.synth_features(16, 32, 28, 28, tag="big")
    perm = torch.tensor([5, 0, 15, 3, 9, 1, 12, 7, 2, 14, 4, 11, 6, 13, 8, 10])
    with torch.no_grad():
        full = m.forward_from_features(fl.to(dev), fr.to(dev), (112, 112)).cpu()
        shuf = m.forward_from_features(fl[perm].to(dev), fr[perm].to(dev), (112, 112)).cpu()
        one = m.forward_from_features(fl[5:6].to(dev), fr[5:6].to(dev), (112, 112)).cpu()
    assert torch.equal(full[perm], shuf)
    assert (full[5:6] - one).abs().max().item() < 1e-3
    assert torch.isfinite(full).all() and full.min() >= 0 and full.max() <= 47

"""GPU: the flat-tile form of the plain and the residual 32 -> 32 split-f16 layer on 28-column maps (csrc/convs16.hip) against the
row-tile form of the same build, both forced through the library's switch bits (what engine.FLAT_TILES sets): an MFMA tile of 32 consecutive
voxels of the flattened (unit, row, x) order of a group of G units computes the sums of the row tiles in the same order, so the whole RS16
storage -- interior, zero halo and the slack behind the last unit -- and the guard word must be torch.equal.

  * units N in {1, 3, 4, 5, 9} (ragged half tile, short last group, exact group, seam plus ragged end), groups G in {1, 4}, depths D in
    {1, 2, 3, 6, 12} (phantom planes, the three-plane walk), heights H in {1, 2, 3, 28} (H <= 3: a unit seam in almost every column; H <= 2:
    up to four units in one column), with and without residual, ReLU on and off: the full product, random post-ReLU-like inputs;
  * values on the +-65504 clamp in the voxel before a unit seam and in the one after it, the seam in the middle of a tile (H = 28), between
    the two tiles of a column (H = 8) and between two columns (H = 16): the guard word trips in both forms;
  * 1024 one-plane units in one launch against the same units launched one by one (every column boundary of the batch is a change of
    group; a single unit never crosses one), as tests/test_hip_s16_columns.py does for the stride-2 and transposed kernels;
  * the switch: engine.FLAT_TILES through ConvPlanS16.run, and the library's choice (drc_conv3d_k3_s16_flat) at the bench's batches.
"""
import ctypes as C

import pytest
import torch

from disprcnn_amd import _lib
from disprcnn_amd import engine as E
from disprcnn_amd import s16
from disprcnn_amd._lib import DrcS16ConvParams

pytestmark = pytest.mark.gpu

ROWS, FLAT, G1 = 0x1000, 0x2000, 0x4000         # the switch bits of drc_s16conv_params.dil


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(dev):
    g = torch.Generator(device=dev).manual_seed(1216)
    w = torch.randn(32, 32, 3, 3, 3, generator=g, device=dev) * (2.0 / (27 * 32)) ** 0.5
    wp, wexp = s16.pack_weight_s16(w)
    sc = ((torch.rand(32, generator=g, device=dev) + 0.5) * (2.0 ** -wexp)).contiguous()
    sh = torch.randn(32, generator=g, device=dev) * 0.1
    return wp, sc, sh, w, wexp


def launch(dev, weights, x16, r16, y16, n, relu, bits, first=0):
    """Units [first, first + n) of x16 (+ r16) -> the same units of y16; returns the launch's guard word."""
    wp, sc, sh = weights[:3]
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    prm = DrcS16ConvParams(P(x16.storage, 2 * first * x16.unit), P(wp), P(sc), P(sh), P(r16.storage, 2 * first * r16.unit) if r16 is not None else None,
                           P(y16.storage, 2 * first * y16.unit), None, None, None, n, x16.D, x16.H, x16.W, 32, 32, int(relu), 0, 1 | bits, None, None, P(word))
    want = 0 if bits & ROWS else (1 if bits & G1 else 4)
    assert _lib.lib().drc_conv3d_k3_s16_flat(C.byref(prm)) == want
    _lib.check(_lib.lib().drc_conv3d_k3_s16_fwd(C.byref(prm), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s16 launch")
    return word


def inputs(dev, N, D, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.relu(torch.randn(N, 32, D, H, 28, generator=g, device=dev)) * 1.5
    r = torch.randn(N, 32, D, H, 28, generator=g, device=dev)
    return x, r


@pytest.mark.parametrize("H", [1, 2, 3, 28])
def test_flat_tiles_equal_row_tiles(dev, weights, H):
    n_cases = 0
    for D in (1, 2, 3, 6, 12):
        x, r = inputs(dev, 9, D, H, seed=100 * H + D)
        x16 = E.RS16(9, 32, D, H, 28, 1, dev).from_dense(x)
        r16 = E.RS16(9, 32, D, H, 28, 1, dev).from_dense(r)
        for N in (1, 3, 4, 5, 9):
            for with_res in (False, True):
                for relu in (False, True):
                    yr = E.RS16(N, 32, D, H, 28, 1, dev)
                    wr = launch(dev, weights, x16, r16 if with_res else None, yr, N, relu, ROWS)
                    assert yr.view7()[N - 1, :, D, 1:H + 1, :, 1:29].float().abs().max().item() > 0.01        # the last plane of the last unit was written
                    for gbit in (0, G1):
                        yf = E.RS16(N, 32, D, H, 28, 1, dev)
                        wf = launch(dev, weights, x16, r16 if with_res else None, yf, N, relu, FLAT | gbit)
                        assert torch.equal(yf.storage, yr.storage), f"N={N} D={D} H={H} res={with_res} relu={relu} G={1 if gbit else 4}: flat tiles differ from row tiles"
                        assert int(wf.item()) == int(wr.item()) == 0
                        n_cases += 1
    assert n_cases == 5 * 5 * 2 * 2 * 2


@pytest.mark.parametrize("H", [28, 8, 16])
@pytest.mark.parametrize("with_res", [False, True])
def test_clamp_on_both_sides_of_a_unit_seam(dev, weights, H, with_res):
    """The last voxel of unit 1 and the first voxel of unit 2 of a group of four carry 60000 sign(w[0, c, centre tap]) in input plane 0 and the
    negative of it in plane 2 (BN scale 2, no ReLU): cout 0 of both voxels is about +-150000 before the clamp in output planes 0 and 2.
    H = 28: the seam lies inside a tile (784 = 24.5 tiles); H = 8 (224 = 7 tiles): between the last lane of a column's first tile and the first
    lane of its second; H = 16 (448 = 14 tiles): between two columns."""
    N, D = 5, 3
    wp, _, sh, w, wexp = weights
    weights = (wp, torch.full((32,), 2.0 * 2.0 ** -wexp, device=dev), sh)
    x, r = inputs(dev, N, D, H, seed=7 + H)
    hot = torch.sign(w[0, :, 1, 1, 1]) * 60000.0
    for u, y_, x_ in ((1, H - 1, 27), (2, 0, 0)):
        x[u, :, 0, y_, x_] = hot
        x[u, :, 2, y_, x_] = -hot
    x16 = E.RS16(N, 32, D, H, 28, 1, dev).from_dense(x)
    r16 = E.RS16(N, 32, D, H, 28, 1, dev).from_dense(r) if with_res else None
    yr = E.RS16(N, 32, D, H, 28, 1, dev)
    wr = launch(dev, weights, x16, r16, yr, N, False, ROWS)
    dense = yr.to_dense()
    for v in (dense[1, 0, :, H - 1, 27], dense[2, 0, :, 0, 0]):
        assert v[0].item() == 65504.0 and v[2].item() == -65504.0, "the case must sit on both clamps next to the seam"
    assert int(wr.item()) == 1
    for gbit in (0, G1):
        yf = E.RS16(N, 32, D, H, 28, 1, dev)
        wf = launch(dev, weights, x16, r16, yf, N, False, FLAT | gbit)
        assert torch.equal(yf.storage, yr.storage)
        assert int(wf.item()) == 1


@pytest.mark.parametrize("H,with_res", [(28, True), (3, False)])
def test_1024_one_plane_units_equal_unit_by_unit(dev, weights, H, with_res):
    N = 1024
    x, r = inputs(dev, N, 1, H, seed=31 + H)
    x16 = E.RS16(N, 32, 1, H, 28, 1, dev).from_dense(x)
    r16 = E.RS16(N, 32, 1, H, 28, 1, dev).from_dense(r) if with_res else None
    yb, yu, yr = (E.RS16(N, 32, 1, H, 28, 1, dev) for _ in range(3))
    assert int(launch(dev, weights, x16, r16, yb, N, True, FLAT).item()) == 0
    assert int(launch(dev, weights, x16, r16, yr, N, True, ROWS).item()) == 0
    assert torch.equal(yb.storage, yr.storage)
    units = sorted(set([0, N - 1] + list(range(17, N - 1, 33))))
    for u in units:
        launch(dev, weights, x16, r16, yu, 1, True, FLAT, first=u)
    for u in units:
        assert torch.equal(yb.storage[u * yb.unit:(u + 1) * yb.unit], yu.storage[u * yu.unit:(u + 1) * yu.unit]), f"unit {u} of the batch differs from the unit launched alone"
    assert not yu.storage[yu.numel:].any()


def test_engine_switch_and_library_choice(dev, weights):
    wp, sc, sh = weights[:3]
    N, D, H = 6, 3, 28
    x, r = inputs(dev, N, D, H, seed=5)
    x16 = E.RS16(N, 32, D, H, 28, 1, dev).from_dense(x)
    r16 = E.RS16(N, 32, D, H, 28, 1, dev).from_dense(r)
    plan = E.ConvPlanS16(N, 32, 32, D, H, 28, True, device=dev)
    saved = dict(E.FLAT_TILES)
    outs = {}
    try:
        for tag, sw in (("rows", {"enabled": False, "group": 4}), ("flat4", {"enabled": True, "group": 4, "force": True}),
                        ("flat1", {"enabled": True, "group": 1, "force": True}), ("default", saved)):
            E.FLAT_TILES.clear()
            E.FLAT_TILES.update(sw)
            outs[tag] = E.RS16(N, 32, D, H, 28, 1, dev)
            plan.run(x16, wp, sc, sh, y16=outs[tag], res=r16)
    finally:
        E.FLAT_TILES.clear()
        E.FLAT_TILES.update(saved)
    for tag in ("flat4", "flat1", "default"):
        assert torch.equal(outs[tag].storage, outs["rows"].storage), tag
    assert E.FLAT_TILES == {"enabled": True, "group": 4}
    # the library's own choice: flat tiles at the bench's batches, row tiles for small launches, the fused head and other widths
    one = C.c_void_p(1)

    def choice(n, W=28, dil=1, head=None):
        prm = DrcS16ConvParams(one, one, one, one, None, None if head else one, None, None, None, n, 12, 28, W, 32, 32, 1, 0, dil, head, head, None)
        return _lib.lib().drc_conv3d_k3_s16_flat(C.byref(prm))
    assert choice(1024) == 4 and choice(256) == 4 and choice(1024, dil=1 | G1) == 1
    assert choice(16) == 0 and choice(16, dil=1 | FLAT) == 4 and choice(1024, dil=1 | ROWS) == 0
    assert choice(1024, W=56) == 0 and choice(1024, W=56, dil=1 | FLAT) == -4 and choice(1024, head=one) == 0

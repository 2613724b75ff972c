"""GPU: the flat-tile form of the half-resolution 64 -> 64 split-f16 layer on 14-column maps (csrc/convs16.hip; hg{1,2,3}.conv2)
against the row-tile form (2 x 14 tiles) of the same build, both forced through the library's switch bits (what engine.FLAT_TILES_HALF sets).
All four waves of a workgroup split K here, so a column is ONE tile of 32 consecutive voxels of the flattened (unit, row, x) order of a group of
G units, G in {1, 4, 8}; the sums and their order are the row form's, so the whole RS16 storage -- interior, zero halo, the slack behind the
last unit -- and the guard word must be torch.equal.

  * units N in {1, 3, 4, 5, 8, 9, 17} (17: a ragged last group at G = 4 and G = 8), G in {1, 4, 8}, depths D in {1, 2, 3, 6}, heights H in
    {1, 2, 3, 8, 14}, with and without residual, ReLU on and off: the full product.  The library proves on the host that every column's slab
    fits the chunk plane (8 stacked rows, at most 3 units behind the column's first); where it refuses an (N, G, H) the forced form returns -4,
    the unforced choice is 0 and nothing is launched;
  * values on the +-65504 clamp in the voxel before a unit seam and in the one after it, the seam inside a tile (H = 14: 196 voxels per unit,
    lane 4 of tile 6) and between two columns (H = 16: 7 tiles per unit), for a cout of each of the two cout tiles;
  * 1024 one-plane units in one launch against the row form and against units launched alone;
  * the switch engine.FLAT_TILES_HALF through ConvPlanS16.run, and the library's choice (drc_conv3d_k3_s16_flat) at the bench's batches.
"""
import ctypes as C

import pytest
import torch

from disprcnn_amd import _lib
from disprcnn_amd import engine as E
from disprcnn_amd import s16
from disprcnn_amd._lib import DrcS16ConvParams

pytestmark = pytest.mark.gpu

ROWS, FLAT = 0x1000, 0x2000                     # the switch bits of drc_s16conv_params.dil
GBIT = {1: 0x4000, 8: 0x8000, 4: 0x10000}       # ... and the group sizes of the 64 -> 64 form
G_DEFAULT = 8                                   # the library's group where the caller names none
W = 14


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(dev):
    g = torch.Generator(device=dev).manual_seed(1317)
    w = torch.randn(64, 64, 3, 3, 3, generator=g, device=dev) * (2.0 / (27 * 64)) ** 0.5
    wp, wexp = s16.pack_weight_s16(w)
    sc = ((torch.rand(64, generator=g, device=dev) + 0.5) * (2.0 ** -wexp)).contiguous()
    sh = torch.randn(64, generator=g, device=dev) * 0.1
    return wp, sc, sh, w, wexp


def params(dev, weights, x16, r16, y16, n, relu, bits, word, first=0):
    wp, sc, sh = weights[:3]
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    return DrcS16ConvParams(P(x16.storage, 2 * first * x16.unit), P(wp), P(sc), P(sh), P(r16.storage, 2 * first * r16.unit) if r16 is not None else None,
                            P(y16.storage, 2 * first * y16.unit), None, None, None, n, x16.D, x16.H, x16.W, 64, 64, int(relu), 0, 1 | bits, None, None, P(word))


def launch(dev, weights, x16, r16, y16, n, relu, bits, first=0, want=None):
    """Units [first, first + n) of x16 (+ r16) -> the same units of y16; returns the launch's guard word."""
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    prm = params(dev, weights, x16, r16, y16, n, relu, bits, word, first)
    if want is not None:
        assert _lib.lib().drc_conv3d_k3_s16_flat(C.byref(prm)) == want
    _lib.check(_lib.lib().drc_conv3d_k3_s16_fwd(C.byref(prm), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s16 launch")
    return word


def inputs(dev, N, D, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.relu(torch.randn(N, 64, D, H, W, generator=g, device=dev)) * 1.5
    r = torch.randn(N, 64, D, H, W, generator=g, device=dev)
    return x, r


@pytest.mark.parametrize("H", [1, 2, 3, 8, 14])
def test_flat_tiles_equal_row_tiles(dev, weights, H):
    n_run = n_refused = 0
    for D in (1, 2, 3, 6):
        x, r = inputs(dev, 17, D, H, seed=100 * H + D)
        x16 = E.RS16(17, 64, D, H, W, 1, dev).from_dense(x)
        r16 = E.RS16(17, 64, D, H, W, 1, dev).from_dense(r)
        for N in (1, 3, 4, 5, 8, 9, 17):
            for with_res in (False, True):
                for relu in (False, True):
                    yr = E.RS16(N, 64, D, H, W, 1, dev)
                    wr = launch(dev, weights, x16, r16 if with_res else None, yr, N, relu, ROWS, want=0)
                    assert yr.view7()[N - 1, :, D, 1:H + 1, :, 1:W + 1].float().abs().max().item() > 0.01        # the last plane of the last unit was written
                    for G in (1, 4, 8):
                        yf = E.RS16(N, 64, D, H, W, 1, dev)
                        word = torch.zeros(1, dtype=torch.int32, device=dev)
                        forced = _lib.lib().drc_conv3d_k3_s16_flat(C.byref(params(dev, weights, x16, None, yf, N, relu, FLAT | GBIT[G], word)))
                        if forced == -4:        # a column of this (N, G, H) would leave the chunk plane: the form refuses, nothing is launched
                            assert _lib.lib().drc_conv3d_k3_s16_flat(C.byref(params(dev, weights, x16, None, yf, N, relu, GBIT[G], word))) == 0
                            n_refused += 1
                            continue
                        wf = launch(dev, weights, x16, r16 if with_res else None, yf, N, relu, FLAT | GBIT[G], want=G)
                        assert torch.equal(yf.storage, yr.storage), f"N={N} D={D} H={H} res={with_res} relu={relu} G={G}: flat tiles differ from row tiles"
                        assert int(wf.item()) == int(wr.item()) == 0
                        n_run += 1
    print(f"H={H}: {n_run} cases run, {n_refused} refused")
    # no (N, H) is refused for G in {1, 4, 8} (columns start at multiples of 32 voxels of a group; H = 2 reaches the eighth stacked
    # row, H = 1 the third unit behind the first, neither the ninth row nor the fourth unit): every case of the product is launched
    assert n_refused == 0 and n_run == 4 * 7 * 2 * 2 * 3


@pytest.mark.parametrize("H", [14, 16])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("co", [0, 32])
def test_clamp_on_both_sides_of_a_unit_seam(dev, weights, H, with_res, co):
    """The last voxel of unit 0 and the first voxel of unit 1 carry 60000 sign(w[co, c, centre tap]) in input plane 0 and the negative of it in
    plane 2 (BN scale 2, no ReLU): cout `co` of both voxels is far outside +-65504 before the clamp in output planes 0 and 2.  H = 14: a unit
    is 196 voxels = 6 tiles + 4, the seam lies inside tile 6 between lanes 3 and 4; H = 16 (224 = 7 tiles): between two columns."""
    N, D = 5, 3
    wp, _, sh, w, wexp = weights
    weights = (wp, torch.full((64,), 2.0 * 2.0 ** -wexp, device=dev), sh)
    x, r = inputs(dev, N, D, H, seed=7 + H)
    hot = torch.sign(w[co, :, 1, 1, 1]) * 60000.0
    for u, y_, x_ in ((0, H - 1, W - 1), (1, 0, 0)):
        x[u, :, 0, y_, x_] = hot
        x[u, :, 2, y_, x_] = -hot
    x16 = E.RS16(N, 64, D, H, W, 1, dev).from_dense(x)
    r16 = E.RS16(N, 64, D, H, W, 1, dev).from_dense(r) if with_res else None
    yr = E.RS16(N, 64, D, H, W, 1, dev)
    wr = launch(dev, weights, x16, r16, yr, N, False, ROWS, want=0)
    dense = yr.to_dense()
    for v in (dense[0, co, :, H - 1, W - 1], dense[1, co, :, 0, 0]):
        assert v[0].item() == 65504.0 and v[2].item() == -65504.0, "the case must sit on both clamps next to the seam"
    assert int(wr.item()) == 1
    for G in (1, 4, 8):
        yf = E.RS16(N, 64, D, H, W, 1, dev)
        wf = launch(dev, weights, x16, r16, yf, N, False, FLAT | GBIT[G], want=G)
        assert torch.equal(yf.storage, yr.storage), G
        assert int(wf.item()) == 1


@pytest.mark.parametrize("H,with_res", [(14, True), (3, False)])
def test_1024_one_plane_units_equal_unit_by_unit(dev, weights, H, with_res):
    N = 1024
    x, r = inputs(dev, N, 1, H, seed=31 + H)
    x16 = E.RS16(N, 64, 1, H, W, 1, dev).from_dense(x)
    r16 = E.RS16(N, 64, 1, H, W, 1, dev).from_dense(r) if with_res else None
    yb, yu, yr = (E.RS16(N, 64, 1, H, W, 1, dev) for _ in range(3))
    assert int(launch(dev, weights, x16, r16, yb, N, True, FLAT, want=G_DEFAULT).item()) == 0
    assert int(launch(dev, weights, x16, r16, yr, N, True, ROWS, want=0).item()) == 0
    assert torch.equal(yb.storage, yr.storage)
    units = sorted(set([0, N - 1] + list(range(0, N, 33))))
    for u in units:
        launch(dev, weights, x16, r16, yu, 1, True, FLAT, first=u, want=G_DEFAULT)
    for u in units:
        assert torch.equal(yb.storage[u * yb.unit:(u + 1) * yb.unit], yu.storage[u * yu.unit:(u + 1) * yu.unit]), f"unit {u} of the batch differs from the unit launched alone"
    assert not yu.storage[yu.numel:].any()


def test_engine_switch_and_library_choice(dev, weights):
    wp, sc, sh = weights[:3]
    N, D, H = 9, 6, 14
    x, r = inputs(dev, N, D, H, seed=5)
    x16 = E.RS16(N, 64, D, H, W, 1, dev).from_dense(x)
    r16 = E.RS16(N, 64, D, H, W, 1, dev).from_dense(r)
    plan = E.ConvPlanS16(N, 64, 64, D, H, W, True, device=dev)
    saved, saved_full = dict(E.FLAT_TILES_HALF), dict(E.FLAT_TILES)
    assert saved == {"enabled": True, "group": G_DEFAULT}
    outs = {}
    try:
        for tag, sw in (("rows", {"enabled": False, "group": G_DEFAULT}), ("flat4", {"enabled": True, "group": 4, "force": True}),
                        ("flat8", {"enabled": True, "group": 8, "force": True}), ("default", saved)):
            E.FLAT_TILES_HALF.clear()
            E.FLAT_TILES_HALF.update(sw)
            outs[tag] = E.RS16(N, 64, D, H, W, 1, dev)
            plan.run(x16, wp, sc, sh, y16=outs[tag], res=r16)
    finally:
        E.FLAT_TILES_HALF.clear()
        E.FLAT_TILES_HALF.update(saved)
    assert outs["rows"].to_dense().abs().max().item() > 0.01
    for tag in ("flat4", "flat8", "default"):
        assert torch.equal(outs[tag].storage, outs["rows"].storage), tag
    assert E.FLAT_TILES_HALF == saved and E.FLAT_TILES == saved_full == {"enabled": True, "group": 4}
    # the library's own choice: flat tiles at the bench's batches, row tiles for small launches and for shapes without the form
    one = C.c_void_p(1)

    def choice(n, cin=64, w_=W, dil=1):
        prm = DrcS16ConvParams(one, one, one, one, None, one, None, None, None, n, 6, 14, w_, cin, cin, 1, 0, dil, None, None, None)
        return _lib.lib().drc_conv3d_k3_s16_flat(C.byref(prm))
    assert choice(1024) == G_DEFAULT and choice(256) == G_DEFAULT
    assert choice(1024, dil=1 | GBIT[4]) == 4 and choice(1024, dil=1 | GBIT[1]) == 1 and choice(1024, dil=1 | GBIT[8]) == 8
    assert choice(192) == G_DEFAULT                                                         # 1176 columns: the smallest batch measured faster
    assert choice(184) == 0 and choice(128) == 0 and choice(64) == 0 and choice(16) == 0 and choice(16, dil=1 | FLAT) == G_DEFAULT and choice(1024, dil=1 | ROWS) == 0
    assert choice(1024, cin=32) == 0 and choice(1024, cin=32, dil=1 | FLAT) == -4          # 32 -> 32 on 14-column maps: no flat form
    assert choice(1024, w_=28) == 0 and choice(1024, w_=28, dil=1 | FLAT) == -4            # 64 channels at W = 28 (the slab would not fit the LDS)

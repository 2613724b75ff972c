"""GPU: the stride-2 and transposed split-f16 kernels (csrc/convs16d.hip, convs16u.hip) run their pipeline THROUGH the ends of a workgroup's
columns -- the first step of a column closes the last output plane of the previous one, the slabs of the next column are staged meanwhile.
What a unit gets must not depend on the columns that ran before and after its own, bit for bit (torch.equal on the unit's whole RS16
storage, halo included, and on the guard word):

  * boundary-free reference: shapes where a unit is exactly ONE column.  A batch of 1024 units gives every workgroup at least four columns
    and makes every column boundary a change of unit; the same units launched one by one (N = 1: one column per workgroup) never run the
    boundary code.  A launch of N = 1 with SEVERAL columns per unit puts all of them on one workgroup, so only one-column units give such
    a reference.
  * neighbour independence: the hourglass' conv1 / conv3 / conv5 / conv6 at the Config A and Config B shapes and ragged last tiles; units at
    positions 0, 7, N - 1 of a batch of 128 different units against the same unit launched alone (other column sequences: 32 column
    workers per XCD against 1).

One case of each kind carries a value beyond 65504 in the last output plane of one unit: the clamp report crosses a column boundary.
tools/experiments/exp_nodrain.py runs the same cases against another build of the library.
"""
import ctypes as C

import pytest
import torch

from disprcnn_amd import _lib
from disprcnn_amd import engine as E
from disprcnn_amd import s16
from disprcnn_amd._lib import DrcS16ConvParams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Layer:
    """Inputs of one launch of kind "s2" (drc_conv3d_k3s2_s16_fwd) or "up" (drc_deconv3d_k3s2_s16_fwd) on N different units; D, H, W = the
    INPUT dims.  hot = (unit, magnitude): that unit's last input plane is +-magnitude, which drives its last output plane over the range."""

    def __init__(self, dev, kind, N, cin, cout, D, H, W, relu, with_res, seed, hot=None):
        self.kind, self.N, self.cin, self.cout, self.D, self.H, self.W, self.relu, self.dev = kind, N, cin, cout, D, H, W, relu, dev
        g = torch.Generator(device=dev).manual_seed(seed)
        x = torch.randn(N, cin, D, H, W, generator=g, device=dev)
        if hot is not None:
            u, mag = hot
            x[u, :, D - 1] = (torch.randint(0, 2, (cin, H, W), generator=g, device=dev).float() * 2 - 1) * mag
        if kind == "up":
            w = torch.randn(cin, cout, 3, 3, 3, generator=g, device=dev) * (2.0 / (27 * cin / 8)) ** 0.5
            self.od = (2 * D, 2 * H, 2 * W)
            wp, wexp = s16.pack_weight_s16(w.transpose(0, 1).contiguous())
        else:
            w = torch.randn(cout, cin, 3, 3, 3, generator=g, device=dev) * (2.0 / (27 * cin)) ** 0.5
            self.od = (D // 2, H // 2, W // 2)
            wp, wexp = s16.pack_weight_s16(w)
        self.wp = wp
        self.sc = ((torch.rand(cout, generator=g, device=dev) + 0.5) * (2.0 ** -wexp)).contiguous()
        self.sh = torch.randn(cout, generator=g, device=dev) * 0.1
        self.x16 = E.RS16(N, cin, D, H, W, 1, dev).from_dense(x)
        self.r16 = E.RS16(N, cout, *self.od, 1, dev).from_dense(torch.randn(N, cout, *self.od, generator=g, device=dev)) if with_res else None

    def out(self, n=None):
        return E.RS16(self.N if n is None else n, self.cout, *self.od, 1, self.dev)

    def launch(self, lib, y16, first=0, n=None, y_first=None, lo4=0):
        """Units [first, first + n) -> units [y_first, y_first + n) of y16 (default: the same positions).  Returns the launch's guard word."""
        n = self.N - first if n is None else n
        y_first = first if y_first is None else y_first
        word = torch.zeros(1, dtype=torch.int32, device=self.dev)
        P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        prm = DrcS16ConvParams(P(self.x16.storage, 2 * first * self.x16.unit), P(self.wp), P(self.sc), P(self.sh),
                               P(self.r16.storage, 2 * first * self.r16.unit) if self.r16 is not None else None,
                               P(y16.storage, 2 * y_first * y16.unit), None, None, None, n, self.D, self.H, self.W, self.cin, self.cout,
                               int(self.relu), lo4, 1, None, None, P(word))
        fn = lib.drc_deconv3d_k3s2_s16_fwd if self.kind == "up" else lib.drc_conv3d_k3s2_s16_fwd
        _lib.check(fn(C.byref(prm), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)), "s16 launch")
        return word


def sample_units(N):
    """The first, the last and about thirty units in between."""
    return sorted(set([0, N - 1] + list(range(17, N - 1, 33))))


def unit_slice(y16, u):
    return y16.storage[u * y16.unit:(u + 1) * y16.unit]


def last_plane_clamped(y16, u):
    v = y16.view7()[u, :, y16.D].float()               # padded plane index D = the last output plane; hi halfs and lo halfs alike
    return bool((v.abs() >= 65504).any())


# ---- boundary-free reference: (kind, cin, cout, D, H, W, relu, with_res).  One column per unit:
#   "up": input H x W within one tile -- W <= 7: 4 x 7, W <= 14: 2 x 14, else 1 x 28;
#   "s2": OUTPUT H/2 x W/2 within one workgroup's tile -- cin 64: RT rows, cin 32 -> 32: 2 RT rows (two spatial tiles), 32 -> 64 (cout
#         split): RT rows.  The depth walk is D input planes ("up") or D / 2 plane pairs ("s2"): 1, 2, 3 and 6 of each.
ONE_COLUMN = []
for _d in (1, 2, 3, 6):
    for _res in (False, True):
        ONE_COLUMN += [("up", 64, 64, _d, 4, 7, True, _res), ("up", 64, 32, _d, 2, 14, False, _res), ("up", 64, 32, _d, 1, 28, True, _res)]
    ONE_COLUMN += [("s2", 64, 64, 2 * _d, 8, 14, True, False), ("s2", 64, 64, 2 * _d, 4, 28, False, False), ("s2", 64, 32, 2 * _d, 2, 56, True, False),
                   ("s2", 32, 32, 2 * _d, 16, 14, True, False), ("s2", 32, 32, 2 * _d, 8, 28, True, False), ("s2", 32, 32, 2 * _d, 4, 56, False, False),
                   ("s2", 32, 64, 2 * _d, 8, 14, True, False), ("s2", 32, 64, 2 * _d, 4, 28, True, False), ("s2", 32, 64, 2 * _d, 2, 56, False, False)]
# ragged one-column units (masked lanes at the boundary)
ONE_COLUMN += [("up", 64, 64, 3, 3, 5, True, True), ("up", 64, 32, 2, 1, 20, False, True), ("s2", 32, 64, 6, 6, 10, True, False), ("s2", 64, 64, 2, 4, 24, True, False)]
# the unit that overflows (None: none), its position chosen among sample_units(1024)
HOT_ONE_COLUMN = {("up", 64, 64, 3, 4, 7, True, True): 512, ("s2", 32, 64, 6, 8, 14, True, False): 512, ("s2", 64, 64, 4, 8, 14, True, False): 1023,
                  ("up", 64, 32, 6, 2, 14, False, False): 0}


def check_one_column(dev, lib, case, N=1024, ref_lib=None):
    """The batch launch of `lib` against unit-by-unit launches of `ref_lib` (default: the same library)."""
    kind, cin, cout, D, H, W, relu, with_res = case
    hot_u = HOT_ONE_COLUMN.get(case)
    units = sample_units(N)
    assert hot_u is None or hot_u in units
    L = Layer(dev, kind, N, cin, cout, D, H, W, relu, with_res, seed=sum(int(v) * (i + 3) for i, v in enumerate(case[1:])) + len(kind),
              hot=(hot_u, 60000.0) if hot_u is not None else None)
    yb, yu = L.out(), L.out()
    wb = L.launch(lib, yb)
    words = {u: L.launch(ref_lib or lib, yu, first=u, n=1) for u in units}
    torch.cuda.synchronize()
    for u in units:
        assert torch.equal(unit_slice(yb, u), unit_slice(yu, u)), f"{case}: unit {u} of the batch differs from the unit launched alone"
        assert int(words[u].item()) == int(u == hot_u), f"{case}: guard word of unit {u} launched alone"
    assert not yb.storage[yb.numel:].any()                      # nothing behind the last unit
    if hot_u is not None:
        assert last_plane_clamped(yb, hot_u), "the case must clamp in the last output plane of its hot unit"
    assert int(wb.item()) == int(hot_u is not None), f"{case}: guard word of the batch"
    return yb, wb


@pytest.mark.parametrize("case", ONE_COLUMN, ids=lambda c: "-".join(str(int(v)) if not isinstance(v, str) else v for v in c))
def test_one_column_units_batch_equals_unit_by_unit(dev, case):
    check_one_column(dev, _lib.lib(), case)


# ---- neighbour independence: (kind, cin, cout, D, H, W, relu, with_res)
NEIGHBOUR = [
    ("s2", 32, 64, 12, 28, 28, True, False),     # conv1, Config A: convs16d_kernel<2,2,14,3,true,true>
    ("s2", 64, 64, 6, 14, 14, True, False),      # conv3, Config A: convs16d_kernel<4,4,7,2,true,false> (ragged row tile)
    ("up", 64, 64, 3, 7, 7, True, True),         # conv5, Config A: convs16u_kernel<4,7>
    ("up", 64, 32, 6, 14, 14, False, True),      # conv6, Config A: convs16u_kernel<2,14>
    ("s2", 32, 64, 24, 56, 56, True, False),     # conv1, Config B: 1 x 28 tiles, cout split
    ("s2", 64, 64, 12, 28, 28, True, False),     # conv3, Config B
    ("up", 64, 64, 6, 14, 14, True, True),       # conv5, Config B
    ("up", 64, 32, 12, 28, 28, False, True),     # conv6, Config B: convs16u_kernel<1,28>
    ("up", 64, 64, 3, 5, 36, True, False),       # ragged last tile: 28 + 8 columns
    ("s2", 32, 32, 4, 10, 72, False, False),     # ragged last tile: 36 wide = 28 + 8, two spatial tiles per workgroup with 5 rows
    ("s2", 64, 64, 2, 6, 8, True, False),        # one plane pair per column, 4 x 7 tile masked
    ("up", 64, 32, 1, 9, 14, True, True),        # one plane per column: every step crosses a boundary
]
HOT_NEIGHBOUR = {("up", 64, 32, 6, 14, 14, False, True): 7, ("s2", 64, 64, 6, 14, 14, True, False): 127}


def check_neighbours(dev, lib, case, N=128, ref_lib=None):
    kind, cin, cout, D, H, W, relu, with_res = case
    hot_u = HOT_NEIGHBOUR.get(case)
    L = Layer(dev, kind, N, cin, cout, D, H, W, relu, with_res, seed=sum(int(v) * (i + 5) for i, v in enumerate(case[1:])) + len(kind),
              hot=(hot_u, 60000.0) if hot_u is not None else None)
    yb = L.out()
    wb = L.launch(lib, yb)
    for u in (0, 7, N - 1):
        y1 = L.out(1)
        w1 = L.launch(ref_lib or lib, y1, first=u, n=1, y_first=0)
        torch.cuda.synchronize()
        assert torch.equal(unit_slice(yb, u), unit_slice(y1, 0)), f"{case}: unit {u} of the batch differs from the unit launched alone"
        assert not y1.storage[y1.numel:].any()
        assert int(w1.item()) == int(u == hot_u), f"{case}: guard word of unit {u} launched alone"
    assert not yb.storage[yb.numel:].any()
    if hot_u is not None:
        assert last_plane_clamped(yb, hot_u), "the case must clamp in the last output plane of its hot unit"
    assert int(wb.item()) == int(hot_u is not None), f"{case}: guard word of the batch"
    return yb, wb


@pytest.mark.parametrize("case", NEIGHBOUR, ids=lambda c: "-".join(str(int(v)) if not isinstance(v, str) else v for v in c))
def test_a_unit_does_not_depend_on_its_neighbour_columns(dev, case):
    check_neighbours(dev, _lib.lib(), case)

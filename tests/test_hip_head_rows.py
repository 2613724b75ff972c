"""GPU: the rows layout of the fused cout-1 heads (csrc/convs16.hip HEAD form with `head_rows`, drc_head_gather_rows_fwd in s16_ops.hip).

The head launch sums the three width taps across neighbouring lanes and stores (T0, T1a, T1b, T2) per source row and output column, 16 B per
voxel; one gather adds three rows of a column for up to three cumulative heads.  Held here: fp32-class results against the two
convolutions in fp64 at the bounds of tests/test_hip_s16.py::test_fused_cout1_head_vs_fp64, at the shapes where the walk changes (two columns
per worker, more units than XCDs, a masked last row tile, H = 1); the gather alone against torch; results independent of the batch position;
and the shapes the layout does not cover are refused.  Reference arithmetic: stackhourglass.py:78-88, 142-144."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from disprcnn_amd import _lib
from disprcnn_amd import engine as E
from disprcnn_amd import s16
from disprcnn_amd._lib import DrcS16ConvParams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _layer(g):
    w0 = torch.randn(32, 32, 3, 3, 3, generator=g) * (2.0 / (27 * 32)) ** 0.5
    w1 = torch.randn(1, 32, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    scale = torch.rand(32, generator=g) + 0.5
    shift = torch.randn(32, generator=g) * 0.1
    return w0, w1, scale, shift


def _head_rows(dev, x, w0, scale, shift, w1):
    """One head launch in the rows layout: (T buffer pre-filled with NaN [N, D, H, W, 4], 2^-wexp of the packed 32 -> 1 weights)."""
    N, _, D, H, W = x.shape
    wp, wexp = s16.pack_weight_s16(w0.to(dev))
    sc = (scale * (2.0 ** -wexp)).to(dev).contiguous()
    hp, hexp = s16.pack_head_weight_s16(w1)
    T = torch.full((N, D, H, W, 4), float("nan"), device=dev)
    plan = E.ConvPlanS16(N, 32, 32, D, H, W, True, device=dev, kind="s1")
    plan.run(E.RS16(N, 32, D, H, W, 1, dev).from_dense(x.to(dev)), wp, sc, shift.to(dev), head=(hp.to(dev), T), head_rows=True)
    return T, 2.0 ** -hexp


@pytest.mark.parametrize("N,D,H,W,with_prev", [
    (3, 12, 28, 28, True),          # Config A volume
    (18, 6, 28, 28, False),         # some workgroups walk two columns: the depth sums and the drain store cross column boundaries
    (9, 9, 4, 28, True),            # more units than XCDs
    (2, 6, 5, 28, True),            # masked last row tile: its lanes must neither write into the next plane nor be read
    (1, 6, 1, 28, False),           # H = 1: no row above or below
])
def test_head_rows_vs_fp64(dev, N, D, H, W, with_prev):
    g = torch.Generator().manual_seed(N * 1000 + D + H + W)
    x = torch.randn(N, 32, D, H, W, generator=g)
    w0, w1, scale, shift = _layer(g)
    prev = torch.randn(N, D, H, W, generator=g) if with_prev else None

    def chain(dt):
        a = F.conv3d(x.to(dt), w0.to(dt), padding=1) * scale.to(dt).view(1, -1, 1, 1, 1) + shift.to(dt).view(1, -1, 1, 1, 1)
        y = F.conv3d(a.clamp_min(0), w1.to(dt), padding=1)[:, 0]
        return y + prev.to(dt) if with_prev else y
    ref = chain(torch.float64)
    e32 = (chain(torch.float32).double() - ref).abs().max().item()
    T, hs = _head_rows(dev, x, w0, scale, shift, w1)
    assert torch.isfinite(T).all()                                      # every slot written
    out = torch.full((N, D, H, W), float("nan"), device=dev)
    E.head_gather_rows([T], [hs], prev.to(dev) if with_prev else None, out)
    got = out.cpu()
    m = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"head rows N={N} {D}x{H}x{W}: max|err| {err:.3e} (fp32 chain {e32:.3e}), max|ref| {m:.3f}")
    assert torch.isfinite(got).all()
    assert err <= 2e-5 * m + 1e-5
    assert err <= 2.0 * e32 + 1e-6 * m, (err, e32)


@pytest.mark.parametrize("N,D,H,W", [(2, 3, 5, 28), (1, 1, 1, 28), (3, 2, 28, 28)])
def test_head_gather_rows_vs_torch(dev, N, D, H, W):
    """drc_head_gather_rows_fwd alone, 1 to 3 heads, with and without res: c = res; c = scale_k * (T0[y-1] + (T1a[y] + T1b[y]) + T2[y+1]) + c."""
    g = torch.Generator().manual_seed(N + D + H + W)
    Ts = [torch.randn(N, D, H, W, 4, generator=g) for _ in range(3)]
    scales = [0.375, -1.5, 0.0625]
    res = torch.randn(N, D, H, W, generator=g)
    Td = [t.to(dev) for t in Ts]
    for nh in (1, 2, 3):
        for with_res in (True, False):
            ref = res.double().clone() if with_res else torch.zeros(N, D, H, W, dtype=torch.float64)
            for k in range(nh):
                t = F.pad(Ts[k].double(), (0, 0, 0, 0, 1, 1))          # zero rows above and below
                ref = scales[k] * (t[:, :, 0:H, :, 0] + (t[:, :, 1:H + 1, :, 1] + t[:, :, 1:H + 1, :, 2]) + t[:, :, 2:H + 2, :, 3]) + ref
            out = torch.full((N, D, H, W), float("nan"), device=dev)
            E.head_gather_rows(Td[:nh], scales[:nh], res.to(dev) if with_res else None, out)
            # fp32: 3 additions + a product + a sum per head on O(1) values -> a few ulp of the largest intermediate
            assert (out.cpu().double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item()), (nh, with_res)


def test_head_rows_do_not_depend_on_the_batch_position(dev):
    """One unit replicated at batch positions 0, 7 and 17 (another XCD, a worker's second column): the same bits in slots and costs."""
    N, D, H, W = 18, 6, 28, 28
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 32, D, H, W, generator=g)
    x[7] = x[0]
    x[17] = x[0]
    w0, w1, scale, shift = _layer(g)
    T, hs = _head_rows(dev, x, w0, scale, shift, w1)
    out = torch.empty(N, D, H, W, device=dev)
    E.head_gather_rows([T], [hs], None, out)
    assert torch.isfinite(T).all()
    assert torch.equal(T[0], T[7]) and torch.equal(T[0], T[17]) and not torch.equal(T[0], T[1])
    assert torch.equal(out[0], out[7]) and torch.equal(out[0], out[17])


def test_head_rows_rejected_where_a_row_is_not_one_tile(dev):
    lib = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    wp, _ = s16.pack_weight_s16(torch.randn(32, 32, 3, 3, 3, device=dev))
    hp = s16.pack_head_weight_s16(torch.randn(1, 32, 3, 3, 3))[0].to(dev)
    one, zero = torch.ones(32, device=dev), torch.zeros(32, device=dev)
    for D, W in ((6, 56), (3, 28)):
        x = E.RS16(1, 32, D, 4, W, 1, dev)
        T = torch.zeros(1, D, 4, W, 12, device=dev)
        prm = DrcS16ConvParams(P(x.storage), P(wp), P(one), P(zero), None, None, None, None, None, 1, D, 4, W, 32, 32, 1, 0, 0, P(T), P(hp), None, 1)
        assert lib.drc_conv3d_k3_s16_fwd(C.byref(prm), st) == -4
    plan = E.ConvPlanS16(1, 32, 32, 6, 4, 28, True, device=dev, kind="s1")
    with pytest.raises(ValueError):
        plan.run(E.RS16(1, 32, 6, 4, 28, 1, dev), wp, one, zero, head=(hp, torch.empty(6 * 4 * 28 * 4 - 1, device=dev)), head_rows=True)      # T too small
    with pytest.raises(ValueError):
        plan.run(E.RS16(1, 32, 6, 4, 28, 1, dev), wp, one, zero, y16=E.RS16(1, 32, 6, 4, 28, 1, dev), head_rows=True)                            # no head
    with pytest.raises(ValueError):
        E.head_gather_rows([], [], None, torch.empty(1, 6, 4, 28, device=dev))
    torch.cuda.synchronize()

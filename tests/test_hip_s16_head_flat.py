"""GPU: the fused cout-1 head on flat 32-voxel tiles (csrc/convs16.hip, HEAD form with RT == 0, convs16_headflat_kernel: planar partial sums
float [N][D][9][H W]) + drc_head_gather_planar_fwd against the ROWS path of the same build (row tiles, width taps summed in the conv kernel,
drc_head_gather_rows_fwd), which tests/test_hip_head_rows.py and tests/test_head_rows_identity.py hold to the oracle.  The planar gather
forms the rows path's sums in the rows path's order, so the only criterion is torch.equal: no tolerance anywhere in this file.

  * cost of one, two and three cumulative heads over N in {1, 3, 4, 5, 9} x G in {1, 4} x D in {1, 2, 3, 6, 12} x H in {1, 2, 3, 28}, W = 28,
    ReLU on: a tile that wraps a row once and twice, a tile in two units (H <= 2), a short last group (N = 5, 9 at G = 4), masked lanes past
    a group's end, D = 12 (the workload's depth).  The fused head exists from six planes on in multiples of three (the depth sums close
    over real planes only: -4 from the library, ValueError from the engine, in EVERY layout); at D in {1, 2, 3} the case therefore holds
    that the planar form is refused exactly as the rows path is, and writes nothing;
  * the planar buffers inside a larger NaN-filled tensor: NaN outside [N][D][9][H W], finite inside;
  * the guard word: equal to the rows path's, clean and with one activation driven to the fp16 clamp;
  * units 0, 7 and 127 of a 128-unit launch against the same units launched alone;
  * the library's choice at the bench's batches (ConvPlanS16.head_kname), and the whole forward_from_features at 8 ROIs with
    engine.HEAD_FLAT forced on against off.
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
PAD = 1031                                      # floats of NaN in front of and behind a planar buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def layers(dev):
    """Three heads: (packed 32 -> 32 weights, folded scale, shift, packed 32 -> 1 weights, its 2^-wexp, the dense 32 -> 32 weight)."""
    g = torch.Generator(device=dev).manual_seed(1218)
    out = []
    for _ in range(3):
        w0 = torch.randn(32, 32, 3, 3, 3, generator=g, device=dev) * (2.0 / (27 * 32)) ** 0.5
        w1 = torch.randn(1, 32, 3, 3, 3, generator=g, device=dev) * (2.0 / 27) ** 0.5
        wp, wexp = s16.pack_weight_s16(w0)
        sc = ((torch.rand(32, generator=g, device=dev) + 0.5) * (2.0 ** -wexp)).contiguous()
        sh = torch.randn(32, generator=g, device=dev) * 0.1
        hp, hexp = s16.pack_head_weight_s16(w1.cpu())
        out.append((wp, sc, sh, hp.to(dev), 2.0 ** -hexp, w0, wexp))
    return out


def head_launch(dev, layer, x16, n, buf, layout, bits=0, first=0):
    """Units [first, first + n) of x16 through one fused-head launch into buf (the layout's floats of unit 0 first); returns (status, guard word)."""
    wp, sc, sh, hp = layer[:4]
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    prm = DrcS16ConvParams(P(x16.storage, 2 * first * x16.unit), P(wp), P(sc), P(sh), None, None, None, None, None, n, x16.D, x16.H, x16.W, 32, 32, 1, 0,
                           1 | bits, P(buf), P(hp), P(word), layout)
    st = _lib.lib().drc_conv3d_k3_s16_fwd(C.byref(prm), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return st, word


def padded(dev, n):
    """A NaN-filled tensor and the view of n floats inside it."""
    whole = torch.full((n + 2 * PAD,), float("nan"), device=dev)
    return whole, whole[PAD:PAD + n]


def inputs(dev, N, D, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.relu(torch.randn(N, 32, D, H, 28, generator=g, device=dev)) * 1.5


@pytest.mark.parametrize("H", [1, 2, 3, 28])
@pytest.mark.parametrize("D", [1, 2, 3, 6, 12])
def test_flat_heads_equal_row_heads(dev, layers, D, H):
    W = 28
    x16 = E.RS16(9, 32, D, H, W, 1, dev).from_dense(inputs(dev, 9, D, H, seed=100 * H + D))
    n_cases = 0
    for N in (1, 3, 4, 5, 9):
        vox = N * D * H * W
        if D < 6:
            # no fused head at this depth, in any layout: refused alike, nothing written
            whole, S = padded(dev, vox * 9)
            T = torch.full((vox * 4,), float("nan"), device=dev)
            for gbit in (0, G1):
                assert head_launch(dev, layers[0], x16, N, T, E.HEAD_ROWS_LAYOUT, ROWS)[0] == -4
                assert head_launch(dev, layers[0], x16, N, S, E.HEAD_PLANAR, gbit)[0] == -4
                assert head_launch(dev, layers[0], x16, N, S, E.HEAD_PLANAR, FLAT | gbit)[0] == -4
                n_cases += 1
            assert torch.isnan(whole).all() and torch.isnan(T).all()
            continue
        rows = [torch.full((vox * 4,), float("nan"), device=dev) for _ in range(3)]
        words_r = []
        for k in range(3):
            st, w = head_launch(dev, layers[k], x16, N, rows[k], E.HEAD_ROWS_LAYOUT, ROWS)
            assert st == 0
            words_r.append(int(w.item()))
        ref = []
        for nh in (1, 2, 3):
            out = torch.full((N, D, H, W), float("nan"), device=dev)
            E.head_gather_rows(rows[:nh], [layers[k][4] for k in range(nh)], None, out)
            assert torch.isfinite(out).all() and out.abs().max().item() > 0.01
            ref.append(out)
        for gbit in (0, G1):
            bufs = [padded(dev, vox * 9) for _ in range(3)]
            for k in range(3):
                st, w = head_launch(dev, layers[k], x16, N, bufs[k][1], E.HEAD_PLANAR, gbit)
                assert st == 0
                assert int(w.item()) == words_r[k] == 0
                whole, S = bufs[k]
                assert torch.isfinite(S).all(), f"N={N} D={D} H={H} G={1 if gbit else 4} head {k}: a planar element was not written"
                assert torch.isnan(whole[:PAD]).all() and torch.isnan(whole[PAD + vox * 9:]).all(), "a store outside the planar buffer"
            for nh in (1, 2, 3):
                out = torch.full((N, D, H, W), float("nan"), device=dev)
                E.head_gather_planar([b[1] for b in bufs[:nh]], [layers[k][4] for k in range(nh)], None, out)
                assert torch.equal(out, ref[nh - 1]), f"N={N} D={D} H={H} G={1 if gbit else 4} heads={nh}: flat + planar gather differs from rows + rows gather"
            n_cases += 1
    assert n_cases == 5 * 2


def test_planar_gather_adds_res_like_the_rows_gather(dev, layers):
    """The optional `res` operand (the cost the chain starts from) through both gathers."""
    N, D, H, W = 3, 6, 3, 28
    x16 = E.RS16(N, 32, D, H, W, 1, dev).from_dense(inputs(dev, N, D, H, seed=77))
    T, S = torch.empty(N * D * H * W * 4, device=dev), torch.empty(N * D * H * W * 9, device=dev)
    assert head_launch(dev, layers[0], x16, N, T, E.HEAD_ROWS_LAYOUT, ROWS)[0] == 0
    assert head_launch(dev, layers[0], x16, N, S, E.HEAD_PLANAR)[0] == 0
    res = torch.randn(N, D, H, W, device=dev)
    a, b = torch.empty(N, D, H, W, device=dev), torch.empty(N, D, H, W, device=dev)
    E.head_gather_rows([T], [layers[0][4]], res, a)
    E.head_gather_planar([S], [layers[0][4]], res, b)
    assert torch.equal(a, b)


@pytest.mark.parametrize("H", [28, 8])
def test_guard_word_with_an_activation_on_the_clamp(dev, layers, H):
    """The last voxel of unit 1 and the first voxel of unit 2 carry 60000 sign(w[0, c, centre tap]) in input plane 0 (BN scale 2): cout 0 of
    both voxels passes 65504 before the clamp.  H = 28: the unit seam lies inside a tile; H = 8: between the two tiles of a column."""
    N, D, W = 5, 6, 28
    wp, _, sh, hp, hs, w0, wexp = layers[0]
    layer = (wp, torch.full((32,), 2.0 * 2.0 ** -wexp, device=dev), sh, hp, hs)
    x = inputs(dev, N, D, H, seed=7 + H)
    hot = torch.sign(w0[0, :, 1, 1, 1]) * 60000.0
    x[1, :, 0, H - 1, 27] = hot
    x[2, :, 0, 0, 0] = hot
    x16 = E.RS16(N, 32, D, H, W, 1, dev).from_dense(x)
    vox = N * D * H * W
    T = torch.empty(vox * 4, device=dev)
    st, wr = head_launch(dev, layer, x16, N, T, E.HEAD_ROWS_LAYOUT, ROWS)
    assert st == 0 and int(wr.item()) == 1, "the case must sit on the clamp"
    ref = torch.empty(N, D, H, W, device=dev)
    E.head_gather_rows([T], [hs], None, ref)
    for gbit in (0, G1):
        S = torch.empty(vox * 9, device=dev)
        st, wf = head_launch(dev, layer, x16, N, S, E.HEAD_PLANAR, gbit)
        assert st == 0 and int(wf.item()) == int(wr.item())
        out = torch.empty(N, D, H, W, device=dev)
        E.head_gather_planar([S], [hs], None, out)
        assert torch.equal(out, ref)


def test_units_of_a_128_unit_launch_equal_the_units_launched_alone(dev, layers):
    N, D, H, W = 128, 6, 28, 28
    x16 = E.RS16(N, 32, D, H, W, 1, dev).from_dense(inputs(dev, N, D, H, seed=128))
    per = D * 9 * H * W
    S = torch.empty(N * per, device=dev)
    assert head_launch(dev, layers[0], x16, N, S, E.HEAD_PLANAR)[0] == 0
    T = torch.empty(N * D * H * W * 4, device=dev)
    assert head_launch(dev, layers[0], x16, N, T, E.HEAD_ROWS_LAYOUT, ROWS)[0] == 0
    a, b = torch.empty(N, D, H, W, device=dev), torch.empty(N, D, H, W, device=dev)
    E.head_gather_planar([S], [layers[0][4]], None, a)
    E.head_gather_rows([T], [layers[0][4]], None, b)
    assert torch.equal(a, b)
    for u in (0, 7, 127):
        one = torch.full((per,), float("nan"), device=dev)
        assert head_launch(dev, layers[0], x16, 1, one, E.HEAD_PLANAR, first=u)[0] == 0
        assert torch.equal(one, S[u * per:(u + 1) * per]), f"unit {u} of the batch differs from the unit launched alone"


def test_library_choice_at_the_bench_batches(dev):
    flat, rows = "convs16_headflat_kernel<2,false,0,28,false,false,true>", "convs16_kernel<2,false,1,28,false,false,true>"
    assert E.HEAD_FLAT == {"enabled": True, "group": 4}
    for N, want in ((1024, flat), (192, flat), (64, rows), (16, rows)):
        plan = E.ConvPlanS16(N, 32, 32, 12, 28, 28, True, device=dev)
        assert plan.head_kname == want, (N, plan.head_kname)
        assert plan.kname == "convs16_kernel<2,false,1,28,false,false,false>"          # (the plain call's name: tests/test_hip_default_kernels.py)
    b = E.ConvPlanS16(16, 32, 32, 24, 56, 56, True, device=dev)                         # Config B: no flat head at W = 56
    assert b.head_kname == "convs16_kernel<2,false,1,28,false,false,true>" and b.head_flat() == 0
    saved = dict(E.HEAD_FLAT)
    try:
        plan = E.ConvPlanS16(16, 32, 32, 12, 28, 28, True, device=dev)
        E.HEAD_FLAT.update(force=True)
        assert plan.head_flat() == 4 and b.head_flat() == 0
        E.HEAD_FLAT.update(group=1)
        assert plan.head_flat() == 1
        E.HEAD_FLAT.update(enabled=False)
        assert plan.head_flat() == 0 and E.ConvPlanS16(1024, 32, 32, 12, 28, 28, True, device=dev).head_kname == rows
    finally:
        E.HEAD_FLAT.clear()
        E.HEAD_FLAT.update(saved)
    # the library itself: the planar layout on a map that has no flat form, and the untouched answers for the other head layouts
    one = C.c_void_p(1)

    def choice(n, W=28, dil=1, layout=E.HEAD_PLANAR, D=12):
        prm = DrcS16ConvParams(one, one, one, one, None, None, None, None, None, n, D, 28, W, 32, 32, 1, 0, dil, one, one, None, layout)
        return _lib.lib().drc_conv3d_k3_s16_flat(C.byref(prm))
    assert choice(1024) == 4 and choice(192) == 4 and choice(1024, dil=1 | G1) == 1 and choice(64) == 0 and choice(64, dil=1 | FLAT) == 4
    assert choice(1024, dil=1 | ROWS) == 0 and choice(1024, W=56) == 0 and choice(1024, W=56, dil=1 | FLAT) == -4 and choice(1024, D=4, dil=1 | FLAT) == -4
    assert choice(1024, layout=E.HEAD_ROWS_LAYOUT) == 0 and choice(1024, layout=E.HEAD_SLOTS) == 0


def test_small_workload_with_the_flat_head_forced_on_equals_off(dev):
    from disprcnn_amd.modeling.psmnet.stackhourglass import PSMNet
    from disprcnn_amd.utils import synth
    from tests.helpers import state_for
    m = PSMNet(48, 0)
    m.load_state_dict(state_for("A"), strict=True)
    m = m.to(dev).eval()
    m.graph_eval = False
    fl, fr = synth.synth_features(8, 32, 28, 28, tag="headflat")
    fl, fr = fl.to(dev), fr.to(dev)
    saved = dict(E.HEAD_FLAT)
    outs = {}
    try:
        for tag, sw in (("off", {"enabled": False, "group": 4}), ("on", {"enabled": True, "group": 4, "force": True}), ("on1", {"enabled": True, "group": 1, "force": True})):
            E.HEAD_FLAT.clear()
            E.HEAD_FLAT.update(sw)
            with torch.no_grad():
                outs[tag] = m.forward_from_features(fl, fr, (112, 112)).clone()
            ws = next(w for w in m._rt._ws.values() if getattr(w.get("ad"), "tag", None) == "3ds16")
            assert ws["fused_heads"] and ws["p"]["classif1.0"].head_flat() == {"off": 0, "on": 4, "on1": 1}[tag]       # (what _SplitF16.heads asked)
    finally:
        E.HEAD_FLAT.clear()
        E.HEAD_FLAT.update(saved)
    assert torch.isfinite(outs["off"]).all()
    assert torch.equal(outs["on"], outs["off"]) and torch.equal(outs["on1"], outs["off"])

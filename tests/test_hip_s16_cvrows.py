"""GPU checks of the cost-volume layer computed from per-row 2D tap maps (round 8: csrc/s16_cvrows.h, run by convs16w_kernel<4,true> with two
rows per work item and by convs16_kernel<4,true,1,28,...> with one).  Reference arithmetic: the concat loop of
stackhourglass.py:115-128 + dres0[0] (:63-66,130), fp32.

The bounds are the family's (tests/test_hip_s16.py): against the fp64 convolution of the materialised volume, err <= 2e-5 * max|ref| + 1e-5 and
err <= 2 x the fp32 chain's own error + 1e-6 * max|ref|.  One arithmetic: the three C entry points give the same bits, and so does a unit
launched alone or inside a batch.
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from disprcnn_amd import engine as E
from disprcnn_amd import s16
from tests.test_hip_s16 import _ref_costvol

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Layer:
    def __init__(self, dev, N, D, H, W, lo4, seed):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.N, self.D, self.H, self.W, self.lo4 = dev, N, D, H, W, lo4
        self.w = torch.randn(32, 64, 3, 3, 3, generator=g) * (2.0 / (27 * 64)) ** 0.5
        self.scale = torch.rand(32, generator=g) + 0.5
        self.shift = torch.randn(32, generator=g) * 0.1
        self.L, self.R = torch.randn(N, 32, H, W, generator=g), torch.randn(N, 32, H, W, generator=g)
        self.wp, wexp = s16.pack_weight_s16(self.w.to(dev))
        self.sc = (self.scale * (2.0 ** -wexp)).to(dev).contiguous()
        self.sh = self.shift.to(dev)

    def chain(self, dt):
        x = _ref_costvol(self.L, self.R, self.lo4, self.D)
        return (F.conv3d(x.to(dt), self.w.to(dt), padding=1) * self.scale.to(dt).view(1, -1, 1, 1, 1) + self.shift.to(dt).view(1, -1, 1, 1, 1)).clamp_min(0)

    def launch(self, entry, units=None):
        """entry: "wide" (drc_conv3d_k3_s16_wide_fwd), "dispatch" (drc_conv3d_k3_s16_fwd), "one row" (the same with dil = 0x800); units: a
        slice of the batch launched on its own.  Returns (RS16 output, guard word)."""
        from disprcnn_amd import _lib
        from disprcnn_amd._lib import DrcS16ConvParams
        lib = _lib.lib()
        dev, D, H, W = self.dev, self.D, self.H, self.W
        L, R = (self.L, self.R) if units is None else (self.L[units], self.R[units])
        N = L.shape[0]
        l16, r16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(L.to(dev)), E.RS16(N, 32, 1, H, W, 0, dev).from_dense(R.to(dev))
        y = E.RS16(N, 32, D, H, W, 1, dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        P = lambda t: C.c_void_p(t.data_ptr())
        fn, dil = {"wide": (lib.drc_conv3d_k3_s16_wide_fwd, 1), "dispatch": (lib.drc_conv3d_k3_s16_fwd, 1), "one row": (lib.drc_conv3d_k3_s16_fwd, 0x800)}[entry]
        prm = DrcS16ConvParams(None, P(self.wp), P(self.sc), P(self.sh), None, P(y.storage), None, P(l16.storage), P(r16.storage), N, D, H, W, 64, 32, 1,
                               self.lo4, dil, None, None, P(ovf))
        _lib.check(fn(C.byref(prm), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), entry)
        torch.cuda.synchronize()
        return y, int(ovf.item())


SHAPES = [
    # N, D, H, W, lo4
    (3, 12, 28, 28, 0),         # Config A
    (1, 24, 56, 56, -12),       # Config B: two x tiles, two 32-column tiles of the right map
    (2, 12, 28, 28, -6),
    (2, 6, 5, 28, 9),           # positive lo4, odd H
    (2, 6, 5, 16, -18),         # |s_j| >= W - 2 on planes 0..4, >= W (fully masked: relu(shift)) on planes 0..2; masked x tile
    (2, 8, 12, 40, 2),          # masked last x tile
    (3, 4, 7, 64, -1),          # three x tiles, odd H
    (2, 1, 3, 16, 0),           # D = 1
    (2, 2, 4, 40, -1),          # D = 2
    (9, 3, 9, 28, 1),           # D = 3, more units than XCDs
    (1, 40, 4, 28, -20),        # more planes than one work item takes (32)
]


@pytest.mark.parametrize("N,D,H,W,lo4", SHAPES)
def test_three_entry_points_bit_identical_and_vs_fp64(dev, N, D, H, W, lo4):
    lay = Layer(dev, N, D, H, W, lo4, seed=N * 100 + D + W + lo4)
    ref = lay.chain(torch.float64)
    e32 = (lay.chain(torch.float32).double() - ref).abs().max().item()
    outs = {k: lay.launch(k) for k in ("wide", "dispatch", "one row")}
    for k in ("dispatch", "one row"):
        assert torch.equal(outs["wide"][0].storage, outs[k][0].storage), k          # whole RS16 storage, halo included
        assert outs[k][1] == outs["wide"][1] == 0
    m = ref.abs().max().item()
    for k, (y, _) in outs.items():
        err = (y.to_dense().cpu().double() - ref).abs().max().item()
        print(f"cvrows {k} N={N} {D}x{H}x{W} lo4={lo4}: max|err| {err:.3e} (fp32 chain {e32:.3e}), max|ref| {m:.3f}")
        assert err <= 2e-5 * m + 1e-5 and err <= 2.0 * e32 + 1e-6 * m
    v = outs["wide"][0].view7().clone()
    v[:, :, 1:D + 1, 1:H + 1, :, 1:W + 1] = 0
    assert not v.any()                   # the halo stays zero


def test_unit_in_a_large_batch_equals_the_unit_alone(dev):
    """80 units x 14 two-row items = 1120 >= 1024: the library's dispatch picks the two-row kernel, every workgroup walks several items; a
    unit's bits do not depend on the batch around it, nor on the kernel (alone it runs the one-row form)."""
    from disprcnn_amd import _lib
    from disprcnn_amd._lib import DrcS16ConvParams
    N, D, H, W = 80, 6, 28, 28
    lay = Layer(dev, N, D, H, W, -2, seed=11)
    probe = DrcS16ConvParams(None, 1, 1, 1, None, 1, None, 1, 1, N, D, H, W, 64, 32, 1, -2, 1)
    assert _lib.lib().drc_conv3d_k3_s16_wide(C.byref(probe)) == 1
    yb, wb = lay.launch("dispatch")
    vb = yb.view7()
    for u in (0, 41, 79):
        for entry in ("dispatch", "wide"):
            y1, w1 = lay.launch(entry, units=slice(u, u + 1))
            assert torch.equal(y1.view7()[0], vb[u]), (u, entry)
            assert w1 == wb == 0


def test_guard_word_equal_between_entry_points_when_a_value_clamps(dev):
    lay = Layer(dev, 2, 4, 6, 28, 0, seed=3)
    lay.sh = lay.sh.clone()
    lay.sh[5] = 7.0e4                      # cout 5 leaves the split-f16 range everywhere: clamped to 65504 and reported
    outs = {k: lay.launch(k) for k in ("wide", "dispatch", "one row")}
    assert [w for _, w in outs.values()] == [1, 1, 1]
    assert torch.equal(outs["wide"][0].storage, outs["one row"][0].storage) and torch.equal(outs["dispatch"][0].storage, outs["one row"][0].storage)
    assert outs["wide"][0].to_dense()[:, 5].min().item() == 65504.0


def test_cost_volume_kernels_report_no_scratch():
    import re
    import subprocess
    import tempfile
    from disprcnn_amd.csrc.build import FLAGS, HIPCC
    for name, pat in (("convs16w.hip", "convs16w_kernelILi4ELb1E"), ("convs16.hip", "convs16_kernelILi4ELb1ELi1ELi28E")):
        src = os.path.join(os.path.dirname(HERE), "disprcnn_amd", "csrc", name)
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "k.o")],
                               capture_output=True, text=True, check=True)
        names = re.findall(r"Function Name: (\S+)", r.stderr)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
        assert len(names) == len(scratch)
        mine = [s_ for n_, s_ in zip(names, scratch) if pat in n_]
        print(name, mine)
        assert mine == [0]

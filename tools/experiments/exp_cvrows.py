"""The cost-volume layer dres0[0] (csrc/s16_cvrows.h: per-row 2D tap maps) of this tree against ANOTHER build of the library
-- the parent commit's depth-walking kernels, built from a checkout of it -- in one process:

    python tools/experiments/exp_cvrows.py --base-lib <other tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--rounds 5] [--log FILE]

  1. results: the layer at Config A / Config B shapes through both libraries; the two builds use different summation orders, so the outputs
     are compared as values (max |new - base| next to max |value|), and both against the fp64 convolution of the materialised volume.
  2. time: the layer at 1024 and 256 Config-A ROIs and 64 Config-B ROIs, through the library's dispatch (two rows per work item where the
     batch is large enough) and with the one-row form forced (dil = 0x800); both libraries in interleaved rounds, us per launch of each
     round; "faster" = the new library's slowest round is below the other's fastest.
"""
import argparse
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from disprcnn_amd import _lib  # noqa: E402
from disprcnn_amd import engine as E  # noqa: E402
from disprcnn_amd import s16  # noqa: E402
from disprcnn_amd._lib import DrcS16ConvParams  # noqa: E402

TIMED = [("Config A", 1024, 12, 28, 28, 0), ("Config A", 256, 12, 28, 28, 0), ("Config B", 64, 24, 56, 56, -12)]


def load(path):
    h = C.CDLL(os.path.abspath(path))
    h.drc_conv3d_k3_s16_fwd.restype, h.drc_conv3d_k3_s16_fwd.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return h


class Layer:
    def __init__(self, dev, N, D, H, W, lo4, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.N, self.D, self.H, self.W, self.lo4 = dev, N, D, H, W, lo4
        self.w = torch.randn(32, 64, 3, 3, 3, generator=g) * (2.0 / (27 * 64)) ** 0.5
        self.scale, self.shift = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1
        self.L, self.R = torch.randn(N, 32, H, W, generator=g), torch.randn(N, 32, H, W, generator=g)
        self.wp, wexp = s16.pack_weight_s16(self.w.to(dev))
        self.sc, self.sh = (self.scale * (2.0 ** -wexp)).to(dev).contiguous(), self.shift.to(dev)
        self.l16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(self.L.to(dev))
        self.r16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(self.R.to(dev))
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def out(self):
        return E.RS16(self.N, 32, self.D, self.H, self.W, 1, self.dev)

    def launch(self, lib, y, dil=1):
        P = lambda t: C.c_void_p(t.data_ptr())
        prm = DrcS16ConvParams(None, P(self.wp), P(self.sc), P(self.sh), None, P(y.storage), None, P(self.l16.storage), P(self.r16.storage),
                               self.N, self.D, self.H, self.W, 64, 32, 1, self.lo4, dil)
        _lib.check(lib.drc_conv3d_k3_s16_fwd(C.byref(prm), self.st), "drc_conv3d_k3_s16_fwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per round and library")
    ap.add_argument("--log", help="also write the report to this file")
    a = ap.parse_args()
    if os.path.samefile(a.base_lib, _lib.LIB_PATH):
        raise SystemExit("--base-lib is this tree's own library")
    dev = torch.device("cuda:0")
    new, base = _lib.lib(), load(a.base_lib)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"exp_cvrows: new {os.path.relpath(_lib.LIB_PATH, ROOT)}  base {a.base_lib}")
    for name, N, D, H, W, lo4 in (("Config A", 4, 12, 28, 28, 0), ("Config B", 1, 24, 56, 56, -12)):
        from tests.test_hip_s16 import _ref_costvol
        L = Layer(dev, N, D, H, W, lo4)
        x = _ref_costvol(L.L, L.R, lo4, D).double()
        ref = (F.conv3d(x, L.w.double(), padding=1) * L.scale.double().view(1, -1, 1, 1, 1) + L.shift.double().view(1, -1, 1, 1, 1)).clamp_min(0)
        yn, yb = L.out(), L.out()
        L.launch(new, yn)
        L.launch(base, yb)
        torch.cuda.synchronize()
        dn, db = yn.to_dense().cpu().double(), yb.to_dense().cpu().double()
        say(f"results {name} N={N}: max|new - base| {(dn - db).abs().max().item():.3e}  max|new - fp64| {(dn - ref).abs().max().item():.3e}  "
            f"max|base - fp64| {(db - ref).abs().max().item():.3e}  max|value| {ref.abs().max().item():.3f}")
    say(f"time: us per launch, {a.launches} launches per round, rounds interleaved base / new")
    for name, N, D, H, W, lo4 in TIMED:
        L = Layer(dev, N, D, H, W, lo4)
        y = L.out()
        for form, dil in (("dispatch", 1), ("one row", 0x800)):
            res = {"base": [], "new": []}
            for lib in (base, new):                      # clocks, caches, the libraries' one-time attribute calls
                for _w in range(10):
                    L.launch(lib, y, dil)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for tag, lib in (("base", base), ("new", new)):
                    for _w in range(3):
                        L.launch(lib, y, dil)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _k in range(a.launches):
                        L.launch(lib, y, dil)
                    e1.record()
                    torch.cuda.synchronize()
                    res[tag].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
            faster = max(res["new"]) < min(res["base"])
            fmt = lambda v: " ".join(f"{t:7.1f}" for t in v)
            say(f"{name} N={N:4d} {form:8s}  base [{fmt(res['base'])}]  new [{fmt(res['new'])}]  "
                f"median {sorted(res['base'])[len(res['base']) // 2]:.1f} -> {sorted(res['new'])[len(res['new']) // 2]:.1f}  "
                f"{'FASTER (slowest new < fastest base)' if faster else 'not outside the spread'}")
        del L, y
    return 0


if __name__ == "__main__":
    sys.exit(main())

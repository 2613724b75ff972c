"""The half-resolution 64 -> 64 layers of the hourglasses (conv2: 6 x 14 x 14 maps; csrc/convs16.hip; DESIGN 3.17: flat 32-voxel tiles) of this
tree against the PARENT commit's library, built from a checkout of it, in one process:

    python tools/experiments/exp_flat_tiles_half.py --base-lib <parent tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--rounds 5] [--rois 1024 256 192 128 64] [--log FILE]

  1. bits: hg1.conv2- (plain) and hg2.conv2-like (+ residual) launches on 37 units through the parent's 2 x 14 row tiles and this library's row
     tiles, flat tiles in groups of one, four and eight, and its own choice: torch.equal of the whole RS16 storage and of the guard word.
  2. time: hg1.conv2, hg2.conv2 and hg3.conv2 at 1024, 256, 192, 128 and 64 Config-A ROIs, per launch: the parent's library, then this one's
     row tiles (dil bit 0x1000), flat tiles G = 1 / 4 / 8 (0x2000 | 0x4000 / 0x10000 / 0x8000) and its own choice; all in interleaved rounds.
     Rule of DESIGN 3.11: a form is faster when its slowest round is below the parent's fastest.
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from disprcnn_amd import _lib  # noqa: E402
from disprcnn_amd import engine as E  # noqa: E402
from disprcnn_amd import s16  # noqa: E402
from disprcnn_amd._lib import DrcS16ConvParams  # noqa: E402

LAYERS = [("hg1.conv2", True, False), ("hg2.conv2 (+ residual)", True, True), ("hg3.conv2 (+ residual)", True, True)]        # (name, relu, residual)
FORMS = [("parent", "base", 0), ("rows", "new", 0x1000), ("flat G=1", "new", 0x2000 | 0x4000), ("flat G=4", "new", 0x2000 | 0x10000),
         ("flat G=8", "new", 0x2000 | 0x8000), ("choice", "new", 0)]
CH, D, H, W = 64, 6, 14, 14


def load(path):
    h = C.CDLL(path)
    h.drc_conv3d_k3_s16_fwd.restype, h.drc_conv3d_k3_s16_fwd.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return h


class Layer:
    def __init__(self, dev, N, relu, with_res, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.dev, self.N, self.relu = dev, N, relu
        w = torch.randn(CH, CH, 3, 3, 3, generator=g, device=dev) * (2.0 / (27 * CH)) ** 0.5
        self.wp, wexp = s16.pack_weight_s16(w)
        self.sc = ((torch.rand(CH, generator=g, device=dev) + 0.5) * (2.0 ** -wexp)).contiguous()
        self.sh = torch.randn(CH, generator=g, device=dev) * 0.1
        self.x16 = E.RS16(N, CH, D, H, W, 1, dev).from_dense(torch.relu(torch.randn(N, CH, D, H, W, generator=g, device=dev)))
        self.r16 = E.RS16(N, CH, D, H, W, 1, dev).from_dense(torch.randn(N, CH, D, H, W, generator=g, device=dev)) if with_res else None
        self.word = torch.zeros(1, dtype=torch.int32, device=dev)

    def out(self):
        return E.RS16(self.N, CH, D, H, W, 1, self.dev)

    def launch(self, lib, bits, y16):
        P = lambda t: C.c_void_p(t.data_ptr())
        prm = DrcS16ConvParams(P(self.x16.storage), P(self.wp), P(self.sc), P(self.sh), P(self.r16.storage) if self.r16 is not None else None,
                               P(y16.storage), None, None, None, self.N, D, H, W, CH, CH, int(self.relu), 0, 1 | bits, None, None, P(self.word))
        _lib.check(lib.drc_conv3d_k3_s16_fwd(C.byref(prm), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)), "s16 launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per round and form")
    ap.add_argument("--rois", type=int, nargs="+", default=[1024, 256, 192, 128, 64], help="batches to time")
    ap.add_argument("--log", help="also write the report to this file")
    a = ap.parse_args()
    if os.path.samefile(a.base_lib, _lib.LIB_PATH):
        raise SystemExit("--base-lib is this tree's own library")
    dev = torch.device("cuda:0")
    libs = {"base": load(os.path.abspath(a.base_lib)), "new": _lib.lib()}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"exp_flat_tiles_half: new {os.path.relpath(_lib.LIB_PATH, ROOT)}  base {a.base_lib}")
    # ---- 1. bits
    for i, (name, relu, with_res) in enumerate(LAYERS[:2]):
        L = Layer(dev, 37, relu, with_res, seed=11 + i)
        outs = {}
        for tag, lib, bits in FORMS:
            y = L.out()
            L.word.zero_()
            L.launch(libs[lib], bits, y)
            outs[tag] = (y.storage, int(L.word.item()))
        yb, wb = outs["parent"]
        assert yb.float().abs().max().item() > 0.01
        bad = [t for t, (y, w_) in outs.items() if not (torch.equal(y, yb) and w_ == wb)]
        say(f"bits {name} N=37: {len(FORMS)} forms {'EQUAL' if not bad else 'DIFFER ' + repr(bad)}  guard word {wb}")
        assert not bad, bad
    # ---- 2. time
    say(f"time: us per launch, {a.launches} launches per round, rounds interleaved {' / '.join(t for t, _, _ in FORMS)}")
    for N in a.rois:
        for i, (name, relu, with_res) in enumerate(LAYERS):
            L = Layer(dev, N, relu, with_res, seed=23 + i)
            y = L.out()
            res = {t: [] for t, _, _ in FORMS}
            for tag, lib, bits in FORMS:                    # clocks, caches, the libraries' one-time attribute calls
                for _w in range(10):
                    L.launch(libs[lib], bits, y)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for tag, lib, bits in FORMS:
                    for _w in range(3):
                        L.launch(libs[lib], bits, y)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _k in range(a.launches):
                        L.launch(libs[lib], bits, y)
                    e1.record()
                    torch.cuda.synchronize()
                    res[tag].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
            med = lambda v: sorted(v)[len(v) // 2]
            say(f"Config A N={N:4d} {name}")
            for tag, v in res.items():
                verdict = ""
                if tag != "parent":
                    verdict = "FASTER than the parent (slowest < its fastest)" if max(v) < min(res["parent"]) else \
                        ("SLOWER than the parent (fastest > its slowest)" if min(v) > max(res["parent"]) else "not outside the parent's spread")
                say(f"    {tag:10s} [{' '.join(f'{t:7.1f}' for t in v)}]  median {med(v):7.1f}  {verdict}")
            del L, y
    return 0


if __name__ == "__main__":
    sys.exit(main())

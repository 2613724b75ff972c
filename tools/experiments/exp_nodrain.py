"""The stride-2 / transposed split-f16 kernels (csrc/convs16d.hip, convs16u.hip) of this tree against ANOTHER build of the library -- the
parent commit's, built from a checkout of it -- in one process:

    python tools/experiments/exp_nodrain.py --base-lib <other tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--rounds 5] [--log FILE]

  1. bit equality: every case of tests/test_hip_s16_columns.py (one-column units in batches of 1024, the hourglass layers at the Config A / B
     shapes, ragged tiles, the cases that clamp) is launched through both libraries (same DrcS16ConvParams): whole RS16 storage and guard
     word must be equal; the unit-by-unit references of the tests are taken from the OTHER build.
  2. time: the hourglass' conv1 / conv3 / conv5 / conv6 at the bench's shapes (Config A at 1024 and 256 units, Config B at 64), both
     libraries in interleaved rounds, us per launch of each round; "faster" = the new library's slowest round is below the other's fastest.
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
from tests import test_hip_s16_columns as T  # noqa: E402

TIMED = [
    # name, (kind, cin, cout, D, H, W, relu, with_res), units
    ("conv1 A", ("s2", 32, 64, 12, 28, 28, True, False), (1024, 256)),
    ("conv3 A", ("s2", 64, 64, 6, 14, 14, True, False), (1024, 256)),
    ("conv5 A", ("up", 64, 64, 3, 7, 7, True, True), (1024, 256)),
    ("conv6 A", ("up", 64, 32, 6, 14, 14, False, True), (1024, 256)),
    ("conv1 B", ("s2", 32, 64, 24, 56, 56, True, False), (64,)),
    ("conv3 B", ("s2", 64, 64, 12, 28, 28, True, False), (64,)),
    ("conv5 B", ("up", 64, 64, 6, 14, 14, True, True), (64,)),
    ("conv6 B", ("up", 64, 32, 12, 28, 28, False, True), (64,)),
]


def load(path):
    h = C.CDLL(os.path.abspath(path))
    for name in ("drc_conv3d_k3s2_s16_fwd", "drc_deconv3d_k3s2_s16_fwd"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per round and library")
    ap.add_argument("--log", help="also write the report to this file")
    ap.add_argument("--no-equal", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    if os.path.samefile(a.base_lib, _lib.LIB_PATH):
        raise SystemExit("--base-lib is this tree's own library")
    dev = torch.device("cuda:0")
    new, base = _lib.lib(), load(a.base_lib)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"exp_nodrain: new {_lib.LIB_PATH}  base {a.base_lib}")
    if not a.no_equal:
        n = 0
        for cases, check in ((T.ONE_COLUMN, T.check_one_column), (T.NEIGHBOUR, T.check_neighbours)):
            for case in cases:
                y_new, w_new = check(dev, new, case, ref_lib=base)          # batch: new; unit by unit: base
                y_base, w_base = check(dev, base, case)                     # the other build on its own
                assert torch.equal(y_new.storage, y_base.storage), f"{case}: outputs of the two builds differ"
                assert int(w_new.item()) == int(w_base.item()), f"{case}: guard words of the two builds differ"
                n += 1
                del y_new, y_base
        say(f"bit equality: {n} cases, whole RS16 storage and guard word equal between the two builds")
        flush_log()
    ok_all = True
    if not a.no_time:
        say(f"time: us per launch, {a.launches} launches per round, rounds interleaved base / new")
        for name, case, units in TIMED:
            for N in units:
                L = T.Layer(dev, *case[:1], N, *case[1:], seed=7)
                y = L.out()
                res = {"base": [], "new": []}
                for lib in (base, new):                      # clocks, caches, the libraries' one-time attribute calls
                    for _w in range(10):
                        L.launch(lib, y)
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for tag, lib in (("base", base), ("new", new)):
                        for _w in range(3):
                            L.launch(lib, y)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        for _k in range(a.launches):
                            L.launch(lib, y)
                        e1.record()
                        torch.cuda.synchronize()
                        res[tag].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
                faster = max(res["new"]) < min(res["base"])
                ok_all &= faster
                fmt = lambda v: " ".join(f"{t:7.1f}" for t in v)
                say(f"{name} N={N:4d}  base [{fmt(res['base'])}]  new [{fmt(res['new'])}]  "
                    f"median {sorted(res['base'])[len(res['base']) // 2]:.1f} -> {sorted(res['new'])[len(res['new']) // 2]:.1f}  "
                    f"{'FASTER (slowest new < fastest base)' if faster else 'not outside the spread'}")
                del L, y
                flush_log()
    flush_log()
    return 0


if __name__ == "__main__":
    sys.exit(main())

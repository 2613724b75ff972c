"""The cost-volume layer dres0[0] (csrc/s16_cvrows.h; DESIGN 3.15: its assembly loop) of this tree against OTHER builds of the library in one
process -- the parent commit's, built from a checkout of it, and any other builds of this tree (a variant of the loop under test):

    python tools/experiments/exp_cvrows_asm.py --base-lib <parent tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--record]
        [--variant "NAME=<another libdisprcnn_hip.so>" ...] [--rounds 5] [--log FILE]

  1. bits: every shape of tests/test_hip_cvrows_pins.py through the three entry forms and every library: torch.equal of the whole RS16 output
     storage and of the guard word against the base library's dispatch entry (so the base's three forms are checked against each other
     too).  --record prints the DIGESTS table of that test, computed from the BASE library's outputs only.
  2. time: the layer at 1024 and 256 Config-A ROIs and 64 Config-B ROIs, through the library's dispatch and with the one-row form forced
     (dil = 0x800); all libraries in interleaved rounds, us per launch of each round.  "faster" = the new library's slowest round is below
     the other's fastest: said of new against base, and of new against each variant (what the variant leaves out pays).
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
from tests import test_hip_cvrows_pins as T  # noqa: E402

TIMED = [("Config A", (1024, 12, 28, 28, 0)), ("Config A", (256, 12, 28, 28, 0)), ("Config B", (64, 24, 56, 56, -12))]


class TimedLayer(T.Layer):
    """Random inputs made on the device: the closed form of a 1024-unit batch is computed on the host."""

    def __init__(self, dev, shape):
        N, D, H, W, lo4 = shape
        g = torch.Generator(device=dev).manual_seed(7)
        r = lambda *s: torch.rand(s, generator=g, device=dev) * 2 - 1
        self.dev, self.N, self.D, self.H, self.W, self.lo4 = dev, N, D, H, W, lo4
        self.wp, wexp = T.s16.pack_weight_s16(r(32, 64, 3, 3, 3) * (6.0 / (27 * 64)) ** 0.5)
        self.sc = ((r(32) * 0.5 + 1.0) * (2.0 ** -wexp)).contiguous()
        self.sh = r(32) * 0.1
        self.l16 = T.E.RS16(N, 32, 1, H, W, 0, dev).from_dense(r(N, 32, H, W))
        self.r16 = T.E.RS16(N, 32, 1, H, W, 0, dev).from_dense(r(N, 32, H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB", help="another build of this tree")
    ap.add_argument("--record", action="store_true", help="print the DIGESTS table from the base library's outputs")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per round and library")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--log", help="also write the report to this file")
    a = ap.parse_args()
    if os.path.samefile(a.base_lib, _lib.LIB_PATH):
        raise SystemExit("--base-lib is this tree's own library")
    dev = torch.device("cuda:0")
    libs = {"base": T.load(os.path.abspath(a.base_lib)), "new": _lib.lib()}
    for v in a.variant:
        name, path = v.split("=", 1)
        libs[name] = T.load(os.path.abspath(path))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"exp_cvrows_asm: new {os.path.relpath(_lib.LIB_PATH, ROOT)}  base {a.base_lib}  " + "  ".join(a.variant))
    # ---- 1. bits
    table, differ = {}, []
    for sid in T.SHAPES:
        L = T.Layer(dev, sid)
        yb, wb = L.run(libs["base"], "dispatch")
        assert yb.abs().max().item() > 0.01 and torch.isfinite(yb).all(), sid
        table[sid] = T.digest(yb, wb)
        for name, lib in libs.items():
            for entry in T.ENTRIES:
                y, w = L.run(lib, entry)
                if not (torch.equal(y, yb) and torch.equal(w, wb)):
                    differ.append((sid, name, entry, int((y != yb).sum().item())))
        say(f"bits {sid:14s} {T.SHAPES[sid]}: {len(libs)} libraries x {len(T.ENTRIES)} entry forms "
            f"{'EQUAL' if not [d for d in differ if d[0] == sid] else 'DIFFER ' + repr([d[1:] for d in differ if d[0] == sid])}  guard word {table[sid][1]}")
    if a.record:
        say("DIGESTS = {")
        for sid, (h, w) in table.items():
            say(f'    "{sid}": ("{h}", {w}),')
        say("}")
    assert not differ, differ
    if a.no_time:
        return 0
    # ---- 2. time
    say(f"time: us per launch, {a.launches} launches per round, rounds interleaved {' / '.join(libs)}")
    for cfg, shape in TIMED:
        L = TimedLayer(dev, shape)
        y = L.out()
        for entry in ("dispatch", "one-row"):
            res = {k: [] for k in libs}
            for lib in libs.values():                    # clocks, caches, the libraries' one-time attribute calls
                for _w in range(10):
                    L.launch(lib, entry, y)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for tag, lib in libs.items():
                    for _w in range(3):
                        L.launch(lib, entry, y)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _k in range(a.launches):
                        L.launch(lib, entry, y)
                    e1.record()
                    torch.cuda.synchronize()
                    res[tag].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
            med = lambda v: sorted(v)[len(v) // 2]
            say(f"{cfg} N={shape[0]:4d} {entry:8s}")
            for tag, v in res.items():
                verdict = ""
                if tag != "new":
                    verdict = "new FASTER (slowest new < fastest of this)" if max(res["new"]) < min(v) else "new not outside the spread"
                say(f"    {tag:14s} [{' '.join(f'{t:7.1f}' for t in v)}]  median {med(v):7.1f}  {verdict}")
        del L, y
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The split-f16 convolution kernels of this tree (weights held in AGPRs and read by the MFMAs directly) against ANOTHER build of
the library -- the parent commit's, built from a checkout of it -- in one process:

    python tools/experiments/exp_agpr.py --base-lib <other tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--rounds 5] [--log FILE] [--record]
                                         [--also NAME=<a third build>.so ...]

  1. bit equality: every case of tests/test_hip_s16_pins.py through both libraries: output storage and guard word must be equal.  --record
     prints the DIGESTS table of that test from the BASE library's outputs.
  2. time: every launch shape of the headline step (Config A) at 1024 and 256 ROIs and the Config B shapes at 64, the libraries in
     interleaved rounds, us per launch of each round; "faster" = the new library's slowest round is below the base's fastest, "slower" = its
     fastest is above the base's slowest.  The outputs and guard words of the timed launches must be equal as well.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from disprcnn_amd import _lib  # noqa: E402
from tests import test_hip_s16_pins as T  # noqa: E402


def shapes(N, D, H, W):
    """(name, file, spec) of the step's launches on a D x H x W volume: spec = (kind, N, cin, cout, D, H, W, relu, flag)."""
    return [
        ("dres0[0] cost volume", "s16_cvrows.h", ("cv2" if N * (H // 2) * -(-W // 28) >= 1024 else "cv1", N, 64, 32, D, H, W, 1, None)),
        ("32->32 plain", "convs16.hip", ("s1", N, 32, 32, D, H, W, 1, None)),
        ("32->32 residual", "convs16.hip", ("s1", N, 32, 32, D, H, W, 0, "res")),
        ("32->32 fused head", "convs16.hip", ("s1", N, 32, 32, D, H, W, 1, "head")),
        ("conv1 32->64 s2", "convs16d.hip", ("s2", N, 32, 64, D, H, W, 1, None)),
        ("conv2 64->64", "convs16.hip", ("s1", N, 64, 64, D // 2, H // 2, W // 2, 1, None)),
        ("conv2 64->64 residual", "convs16.hip", ("s1", N, 64, 64, D // 2, H // 2, W // 2, 1, "res")),
        ("conv3 64->64 s2", "convs16d.hip", ("s2", N, 64, 64, D // 2, H // 2, W // 2, 1, None)),
        ("conv4 64->64", "convs16.hip", ("s1", N, 64, 64, D // 4, H // 4, W // 4, 1, None)),
        ("conv5 64->64 up", "convs16u.hip", ("up", N, 64, 64, D // 4, H // 4, W // 4, 1, "res")),
        ("conv6 64->32 up", "convs16u.hip", ("up", N, 64, 32, D // 2, H // 2, W // 2, 0, "res")),
    ]


TIMED = [("A", 1024, 12, 28, 28, 0), ("A", 256, 12, 28, 28, 0), ("B", 64, 24, 56, 56, -12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--also", action="append", default=[], help="NAME=PATH of a further build to time (an experiment variant)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per round and library")
    ap.add_argument("--log", help="also write the report to this file")
    ap.add_argument("--record", action="store_true", help="print the DIGESTS table of tests/test_hip_s16_pins.py from the base library")
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    if os.path.samefile(a.base_lib, _lib.LIB_PATH):
        raise SystemExit("--base-lib is this tree's own library")
    dev = torch.device("cuda:0")
    libs = [("base", T.load(os.path.abspath(a.base_lib))), ("new", _lib.lib())]
    for spec in a.also:
        name, path = spec.split("=", 1)
        libs.append((name, T.load(os.path.abspath(path))))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"exp_agpr: new {os.path.relpath(_lib.LIB_PATH, ROOT)}  base {a.base_lib}  {' '.join(a.also)}")
    table = {}
    for cid in T.CASES:
        L = T.Launch(dev, cid)
        got = {name: L.run(lib) for name, lib in libs}
        table[cid] = T.digest(*got["base"])
        for name, _ in libs[1:]:
            assert torch.equal(got[name][0], got["base"][0]), f"{cid}: output of '{name}' differs from the base build's"
            assert int(got[name][1].item()) == int(got["base"][1].item()), f"{cid}: guard word of '{name}' differs from the base build's"
        assert got["base"][0].abs().max().item() > 0.1
    say(f"bit equality: {len(table)} cases, output storage and guard word equal between {', '.join(n for n, _ in libs)}")
    if a.record:
        say("DIGESTS = {")
        for cid, (h, w) in table.items():
            say(f'    "{cid}": ("{h}", {w}),')
        say("}")
    if a.no_time:
        return 0
    say(f"time: us per launch, {a.launches} launches per round, {a.rounds} rounds interleaved {' / '.join(n for n, _ in libs)}")
    for cfg, N, D, H, W, lo4 in TIMED:
        for name, fname, spec in shapes(N, D, H, W):
            L = T.Launch(dev, "timed", spec=spec, rand=True)
            cvlo = lo4 if spec[0] in ("cv1", "cv2") else 0
            outs = {}
            for tag, lib in libs:                          # clocks, caches, the libraries' one-time attribute calls; and the outputs to compare
                outs[tag] = (L.out(), torch.zeros(1, dtype=torch.int32, device=dev))
                for _w in range(5):
                    L.launch(lib, outs[tag][0], outs[tag][1], cvlo)
            torch.cuda.synchronize()
            for tag, _ in libs[1:]:
                assert torch.equal(outs[tag][0], outs["base"][0]) and torch.equal(outs[tag][1], outs["base"][1]), f"{cfg} {N} {name}: '{tag}' differs from base"
            y = outs["base"][0]
            del outs
            res = {tag: [] for tag, _ in libs}
            for _ in range(a.rounds):
                for tag, lib in libs:
                    for _w in range(3):
                        L.launch(lib, y, None, cvlo)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _k in range(a.launches):
                        L.launch(lib, y, None, cvlo)
                    e1.record()
                    torch.cuda.synchronize()
                    res[tag].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
            fmt = lambda v: " ".join(f"{t:7.1f}" for t in v)
            med = lambda v: sorted(v)[len(v) // 2]
            s = f"{cfg} N={N:4d} {name:22s} {fname:13s}"
            for tag, _ in libs:
                s += f" {tag} [{fmt(res[tag])}]"
            for tag, _ in libs[1:]:
                verdict = "FASTER" if max(res[tag]) < min(res["base"]) else "SLOWER" if min(res[tag]) > max(res["base"]) else "within the spread"
                s += f"  {tag}: median {med(res['base']):.1f} -> {med(res[tag]):.1f} {verdict}"
            say(s)
            del L, y
    return 0


if __name__ == "__main__":
    sys.exit(main())

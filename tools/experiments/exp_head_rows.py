"""The fused heads in the rows layout (width taps summed in the conv kernel, one gather for three heads) against ANOTHER build of
the library -- the parent commit's, built from a checkout of it -- in one process (the pattern of exp_agpr.py):

    python tools/experiments/exp_head_rows.py --base-lib <other tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--rounds 5] [--log FILE]

  head launch   base: 12-float slots | new: rows layout            at 1024 and 256 ROIs of Config A (12 x 28 x 28)
                also the new library writing the 12-float slots (the untouched layout inside the touched kernel; outputs must equal base's)
  tail          base: three drc_head_gather_fwd (cost1 -> cost2 -> cost3) | new: one drc_head_gather_rows_fwd        at 1024 ROIs
  Config B      the head launch at 64 ROIs of 24 x 56 x 56: 12-float slots through both libraries (must be equal, must not be slower)
us per launch (the tail: per chain), the libraries in interleaved rounds; "faster" = the new library's slowest round is below the base's
fastest, "slower" = its fastest is above the base's slowest."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from disprcnn_amd import _lib  # noqa: E402
from disprcnn_amd._lib import DrcS16ConvParams  # noqa: E402
from tests import test_hip_s16_pins as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--log")
    a = ap.parse_args()
    if os.path.samefile(a.base_lib, _lib.LIB_PATH):
        raise SystemExit("--base-lib is this tree's own library")
    dev = torch.device("cuda:0")
    base, new = T.load(os.path.abspath(a.base_lib)), _lib.lib()
    base.drc_head_gather_fwd.restype = C.c_int
    base.drc_head_gather_fwd.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float, C.c_void_p]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def head_launch(L, lib, y, rows):
        prm = DrcS16ConvParams(P(L.x16.storage), P(L.wp), P(L.sc), P(L.sh), None, None, None, None, None, L.N, L.D, L.H, L.W, 32, 32, 1, 0, 1,
                               P(y), P(L.hp), None, 1 if rows else 0)
        _lib.check(lib.drc_conv3d_k3_s16_fwd(C.byref(prm), stream()), "drc_conv3d_k3_s16_fwd")

    def timed(variants):
        """variants: [(tag, fn)] -> {tag: [us per call of each round]}, interleaved"""
        res = {tag: [] for tag, _ in variants}
        for tag, fn in variants:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for tag, fn in variants:
                for _w in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _k in range(a.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[tag].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
        return res

    def report(name, res):
        fmt = lambda v: " ".join(f"{t:7.1f}" for t in v)
        med = lambda v: sorted(v)[len(v) // 2]
        s = f"{name:34s}"
        for tag, v in res.items():
            s += f" {tag} [{fmt(v)}]"
        for tag, v in res.items():
            if tag == "base":
                continue
            verdict = "FASTER" if max(v) < min(res["base"]) else "SLOWER" if min(v) > max(res["base"]) else "within the spread"
            s += f"  {tag}: median {med(res['base']):.1f} -> {med(v):.1f} {verdict}"
        say(s)

    say(f"exp_head_rows: new {os.path.relpath(_lib.LIB_PATH, ROOT)}  base {a.base_lib}; us per launch, {a.launches} launches per round, {a.rounds} rounds interleaved")
    for N in (1024, 256):
        D, H, W = 12, 28, 28
        L = T.Launch(dev, "timed", spec=("s1", N, 32, 32, D, H, W, 1, "head"), rand=True)
        S_base, S_new = (torch.zeros(N, D, H, W, 12, device=dev) for _ in range(2))
        Tr = torch.zeros(N, D, H, W, 4, device=dev)
        head_launch(L, base, S_base, False)
        head_launch(L, new, S_new, False)
        head_launch(L, new, Tr, True)
        torch.cuda.synchronize()
        assert torch.equal(S_base, S_new), "the 12-float slots of the new build differ from the base build's"
        report(f"A N={N:4d} head launch", timed([("base", lambda: head_launch(L, base, S_base, False)), ("new-rows", lambda: head_launch(L, new, Tr, True)),
                                                   ("new-slots", lambda: head_launch(L, new, S_new, False))]))
        if N == 1024:
            c = [torch.empty(N, D, H, W, device=dev) for _ in range(3)]
            c3 = torch.empty(N, D, H, W, device=dev)
            T3 = [Tr, Tr.clone(), Tr.clone()]           # three buffers, as in the step (equal contents do not matter to the time)

            def tail_base():
                prev = None
                for k in range(3):
                    _lib.check(base.drc_head_gather_fwd(P(S_base), P(prev), P(c[k]), N, D, H, W, C.c_float(0.5), stream()), "drc_head_gather_fwd")
                    prev = c[k]

            def tail_new():
                _lib.check(new.drc_head_gather_rows_fwd(P(T3[0]), P(T3[1]), P(T3[2]), 0.5, 0.5, 0.5, 3, None, P(c3), N, D, H, W, stream()), "drc_head_gather_rows_fwd")

            tail_base()
            tail_new()
            torch.cuda.synchronize()
            d = (c[2] - c3).abs().max().item()
            say(f"A N=1024 cost3 of the two tails: max|difference| {d:.3e} at max|cost3| {c[2].abs().max().item():.3f}")
            assert d <= 1e-5 * max(1.0, c[2].abs().max().item())
            report("A N=1024 tail (3 gathers | 1)", timed([("base", tail_base), ("new-rows", tail_new)]))
            del c, c3, T3
        del L, S_base, S_new, Tr
    N, D, H, W = 64, 24, 56, 56
    L = T.Launch(dev, "timed", spec=("s1", N, 32, 32, D, H, W, 1, "head"), rand=True)
    S_base, S_new = (torch.zeros(N, D, H, W, 12, device=dev) for _ in range(2))
    head_launch(L, base, S_base, False)
    head_launch(L, new, S_new, False)
    torch.cuda.synchronize()
    assert torch.equal(S_base, S_new), "Config B: the 12-float slots of the new build differ from the base build's"
    report(f"B N={N:4d} head launch (slots)", timed([("base", lambda: head_launch(L, base, S_base, False)), ("new-slots", lambda: head_launch(L, new, S_new, False))]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The fused heads on flat tiles (planar partial sums, one gather that forms the width sums) against ANOTHER build of the
library -- the parent commit's, built from a checkout of it -- in one process (the pattern of exp_head_rows.py / exp_flat_tiles.py):

    python tools/experiments/exp_head_flat.py --base-lib <other tree>/disprcnn_amd/csrc/libdisprcnn_hip.so [--rounds 5] [--log FILE]

  head launch   base: row tiles, rows layout | new: flat tiles, planar layout          at 1024 and 256 ROIs of Config A (12 x 28 x 28)
                also the new library's own rows layout (the untouched form inside the touched kernel file; outputs must equal base's)
  gather        base: drc_head_gather_rows_fwd, three heads | new: drc_head_gather_planar_fwd, three heads (cost3 must be equal)
  heads of a step   3 head launches + 1 gather, each library's form
us per launch (the step: per chain), the libraries in interleaved rounds; "faster" = the new library's slowest round is below the base's
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

ROWS_LAYOUT, PLANAR = 1, 2


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
    gather_sig = [C.c_void_p] * 3 + [C.c_float] * 3 + [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    base.drc_head_gather_rows_fwd.restype, base.drc_head_gather_rows_fwd.argtypes = C.c_int, gather_sig
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def head_launch(L, lib, y, layout):
        prm = DrcS16ConvParams(P(L.x16.storage), P(L.wp), P(L.sc), P(L.sh), None, None, None, None, None, L.N, L.D, L.H, L.W, 32, 32, 1, 0, 1,
                               P(y), P(L.hp), None, layout)
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

    say(f"exp_head_flat: new {os.path.relpath(_lib.LIB_PATH, ROOT)}  base {a.base_lib}; us per launch, {a.launches} launches per round, {a.rounds} rounds interleaved")
    for N in (1024, 256):
        D, H, W = 12, 28, 28
        L = T.Launch(dev, "timed", spec=("s1", N, 32, 32, D, H, W, 1, "head"), rand=True)
        vox = N * D * H * W
        Tb = [torch.zeros(vox * 4, device=dev) for _ in range(3)]       # three buffers, as in the step (equal contents do not matter to the time)
        Tn = torch.zeros(vox * 4, device=dev)
        Sp = [torch.zeros(vox * 9, device=dev) for _ in range(3)]
        for k in range(3):
            head_launch(L, base, Tb[k], ROWS_LAYOUT)
            head_launch(L, new, Sp[k], PLANAR)
        head_launch(L, new, Tn, ROWS_LAYOUT)
        torch.cuda.synchronize()
        assert torch.equal(Tb[0], Tn), "the rows layout of the new build differs from the base build's"
        report(f"A N={N:4d} head launch", timed([("base", lambda: head_launch(L, base, Tb[0], ROWS_LAYOUT)), ("new-flat", lambda: head_launch(L, new, Sp[0], PLANAR)),
                                                   ("new-rows", lambda: head_launch(L, new, Tn, ROWS_LAYOUT))]))
        cb, cn = torch.empty(N, D, H, W, device=dev), torch.empty(N, D, H, W, device=dev)

        def gather_base():
            _lib.check(base.drc_head_gather_rows_fwd(P(Tb[0]), P(Tb[1]), P(Tb[2]), 0.5, 0.25, 0.5, 3, None, P(cb), N, D, H, W, stream()), "drc_head_gather_rows_fwd")

        def gather_new():
            _lib.check(new.drc_head_gather_planar_fwd(P(Sp[0]), P(Sp[1]), P(Sp[2]), 0.5, 0.25, 0.5, 3, None, P(cn), N, D, H, W, stream()), "drc_head_gather_planar_fwd")

        def step_base():
            for k in range(3):
                head_launch(L, base, Tb[k], ROWS_LAYOUT)
            gather_base()

        def step_new():
            for k in range(3):
                head_launch(L, new, Sp[k], PLANAR)
            gather_new()

        gather_base()
        gather_new()
        torch.cuda.synchronize()
        assert torch.equal(cb, cn), "cost3 of the planar path differs from the base build's rows path"
        say(f"A N={N:4d} cost3: flat + planar gather torch.equal to the base build's rows path (max|cost3| {cb.abs().max().item():.3f})")
        report(f"A N={N:4d} gather (3 heads)", timed([("base", gather_base), ("new-flat", gather_new)]))
        report(f"A N={N:4d} 3 heads + 1 gather", timed([("base", step_base), ("new-flat", step_new)]))
        del L, Tb, Tn, Sp, cb, cn
    return 0


if __name__ == "__main__":
    sys.exit(main())

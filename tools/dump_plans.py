"""Dump what the engine plans for a fixed sweep of layers, one JSON line per case.

    python tools/dump_plans.py            the full dump (some 3 MB): compare two trees with it, line for line
    python tools/dump_plans.py --golden > tests/golden/plans_golden.json

Plans are built on torch.device("cpu") (Blocked.geometry: no storage), so this needs the built library but no GPU.  A line of the full dump
holds the case, its record under the default switches ("default") and, per kernel-selection switch turned off ("off"), the fields of the
record that then differ -- a switch that is not listed leaves the plan as it is.  A record of an fp32 plan: kname, the nine flags,
needs_t16, pack_kind, the hex of the plan's DrcTapconvParams and the C entries run() / run_costvol() / run(y16=...) call with their extra
arguments.  The entries are computed from the flags by `entry_from_flags`, the if-chain ConvPlan.run() had before plans carried a kernel
record; where a plan has a record (plan.kernel) the record's own entries must say the same, or the dump fails.

The full dump is too large to commit; tests/golden/plans_golden.json holds, per case, [case, kname under the default switches, the first
12 hex digits of the SHA-256 of the case's line of the full dump] (tests/test_host_logic.py regenerates and compares it).
"""
import contextlib
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from disprcnn_amd import engine as E  # noqa: E402

FLAGS = ("slide", "fused_deconv", "down", "pointwise", "direct", "wino", "rb", "c2d", "deconv_direct")
DEV = torch.device("cpu")

# (name, dict, key): each is switched off in turn
SWITCHES = [("DIRECT", E.DIRECT, "enabled"), ("WINO", E.WINO, "enabled"), ("WINO.rb", E.WINO, "rb"), ("WINO2D", E.WINO2D, "enabled"),
            ("WINO2D.rb", E.WINO2D, "rb"), ("WINO2D.odd", E.WINO2D, "odd"), ("WINO2D.dilated", E.WINO2D, "dilated"), ("SLIDE", E.SLIDE, "enabled"),
            ("DOWN", E.DOWN, "enabled"), ("FUSED_DECONV", E.FUSED_DECONV, "enabled"), ("DECONV_DIRECT", E.DECONV_DIRECT, "enabled"),
            ("POINTWISE", E.POINTWISE, "enabled"), ("CONV2D_FILL", E.CONV2D_FILL, "enabled"), ("C16_TILE", E.C16_TILE, "enabled")]


@contextlib.contextmanager
def switched_off(d, key):
    saved = d[key]
    d[key] = False
    try:
        yield
    finally:
        d[key] = saved


def entry_from_flags(pl):
    """(run(), run_costvol(), run(y16=...)) entries of an fp32 plan from its flags: the dispatch chain of ConvPlan.run() / run_costvol() as it
    was before the kernel record, in its arm order.  The cout-tile argument was slide_ct / c2d_ct / down_ct / deconv_ct then, plan.ct now."""
    def ct(name):
        return getattr(pl, name) if hasattr(pl, name) else pl.ct
    if pl.wino and pl.c2d and pl.rb:
        run = "drc_conv2d_k3_wino_rb_fwd()"
    elif pl.wino and pl.c2d:
        run = "drc_conv2d_k3_wino_fwd(ct=%d)" % ct("slide_ct")
    elif pl.direct and pl.c2d:
        run = "drc_conv2d_k3_direct_fwd(ct=%d)" % ct("c2d_ct")
    elif pl.direct and pl.down:
        run = "drc_conv3d_k3s2_direct_fwd(ct=%d)" % ct("down_ct")
    elif pl.wino and pl.rb:
        run = "drc_conv3d_k3_wino_rb_fwd()"
    elif pl.wino:
        run = "drc_conv3d_k3_wino_fwd(ct=%d)" % ct("slide_ct")
    elif pl.direct and pl.slide:
        run = "drc_tapconv3d_direct_fwd(ct=%d)" % ct("slide_ct")
    elif pl.pointwise:
        run = "drc_conv2d_k1_fwd()"
    elif pl.deconv_direct:
        run = "drc_deconv3d_k3s2_direct_fwd(ct=%d)" % ct("deconv_ct")
    elif pl.fused_deconv:
        run = "drc_deconv3d_k3s2_fwd()"
    else:
        run = "drc_tapconv_fwd()"
    costvol = None
    if pl.wino and not pl.c2d:
        costvol = "drc_conv3d_k3_wino_rb_costvol_fwd()" if pl.rb else "drc_conv3d_k3_wino_costvol_fwd(ct=%d)" % ct("slide_ct")
    rs16 = "drc_deconv3d_k3s2_direct_s16_fwd()" if pl.deconv_direct else None
    return run, costvol, rs16


def entry_from_record(pl):
    k = pl.kernel
    arg = "(ct=%d)" % pl.ct if k.takes_ct else "()"
    return k.entry + arg, (k.costvol + arg if k.costvol else None), (k.rs16 + "()" if k.rs16 else None)


def points_from_flags(pl):
    """(points, axis) of the w16 check run() made from the flags (None: the plan reads `w`)."""
    if not pl.needs_t16:
        return None
    return [(16 if pl.c2d else 64) if pl.wino else (9 if pl.c2d else 27), 1 if pl.deconv_direct else 0]


def record32(pl):
    rec = {"kname": pl.kname}
    rec.update((f, bool(getattr(pl, f))) for f in FLAGS + ("needs_t16",))
    rec["pack_kind"], rec["w16_points"], rec["p"] = pl.pack_kind, points_from_flags(pl), bytes(pl.p).hex()
    rec["entry"], rec["entry_costvol"], rec["entry_rs16"] = entry_from_flags(pl)
    if hasattr(pl, "kernel"):
        k = pl.kernel
        if entry_from_record(pl) != (rec["entry"], rec["entry_costvol"], rec["entry_rs16"]):
            raise SystemExit("kernel record and flags disagree on the entry: %r vs %r (%s)" % (entry_from_record(pl), rec["entry"], pl.kname))
        if ([k.points, k.axis] if k.points else None) != rec["w16_points"] or (k.pack if k.pack != "pw" else "tap") != rec["pack_kind"]:
            raise SystemExit("kernel record and flags disagree on the packing (%s)" % pl.kname)
    return rec


def record16(pl):
    """An fp16-storage plan: ConvPlan16.run()'s chain over costvol_lo4 / tile / tile_x as it was before the plan stored one entry name."""
    if pl.costvol_lo4 is not None:
        entry = "drc_conv16_k3_costvol_fwd(lo4=%d)" % pl.costvol_lo4
    elif pl.tile:
        entry = "drc_conv16_k3_tile_fwd()"
    elif pl.tile_x:
        entry = pl.tile_x + "()"
    else:
        entry = "drc_conv16_fwd()"
    if hasattr(pl, "entry") and pl.entry != entry.split("(")[0]:
        raise SystemExit("ConvPlan16.entry and tile / tile_x / costvol_lo4 disagree: %r vs %r" % (pl.entry, entry))
    return {"kname": pl.kname, "tile": bool(pl.tile), "tile_x": pl.tile_x, "dense1": bool(pl.dense1), "flops": pl.flops, "entry": entry, "p": bytes(pl.p).hex()}


def geo(n, c, d, h, w, pd, ph, pw):
    return E.Blocked.geometry(n, c, d, h, w, pd, ph, pw, DEV)


def geo16(n, c, d, h, w):
    """A Blocked16 without storage (plans read the geometry only)."""
    g = E.Blocked16.__new__(E.Blocked16)
    g.N, g.C, g.D, g.H, g.W, g.pd, g.ph, g.pw = n, c, d, h, w, 1, 1, 1
    g.cb = (c + E.CB16 - 1) // E.CB16
    g.Dp, g.Hp, g.Wp = d + 2, h + 2, w + 2
    g.h_stride = g.Wp * E.CB16
    g.d_stride = g.Hp * g.h_stride
    g.cb_stride = g.Dp * g.d_stride
    g.n_stride = g.cb * g.cb_stride
    g.numel, g.storage, g.device = n * g.n_stride, None, DEV
    return g


BATCHES = (1, 2, 4, 12, 64, 256, 1024)
DIMS3 = ((2, 4, 4), (3, 7, 7), (6, 14, 14), (12, 28, 28), (24, 56, 56))
MAPS2 = ((7, 7), (14, 14), (28, 28), (56, 56), (54, 56), (112, 112), (94, 311), (24, 78), (12, 38))
CHANNELS2 = (32, 64, 128, 256, 512)


def cases():
    """(case name, record function, plan thunk) of the sweep, in a fixed order."""
    for stride in (1, 2):
        for n in BATCHES:
            for c in (32, 64):
                for d in DIMS3:
                    od = d if stride == 1 else tuple(v // 2 for v in d)
                    yield ("conv3d s%d n%d c%d %s" % (stride, n, c, "x".join(map(str, d))), record32,
                           lambda n=n, c=c, d=d, od=od, stride=stride: E.plan_conv3d(geo(n, c, *d, 1, 1, 1), geo(n, c, *od, 1, 1, 1), stride, c, True))
    for n in BATCHES:
        for cin, cout in ((64, 64), (64, 32)):
            for d in ((3, 7, 7), (6, 14, 14)):
                yield ("deconv3d n%d c%d-%d %s" % (n, cin, cout, "x".join(map(str, d))), record32,
                       lambda n=n, cin=cin, cout=cout, d=d: E.plan_deconv3d(geo(n, cin, *d, 1, 1, 1), geo(n, cout, *(2 * v for v in d), 1, 1, 1), cout, False))
    for k in (1, 3):
        for stride in (1, 2):
            for dil in ((1, 2, 4) if k == 3 else (1,)):
                for hw in MAPS2:
                    for c in CHANNELS2:
                        for n in (2, 32):
                            pad = dil * (k - 1) // 2
                            ohw = tuple((v - 1) // stride + 1 for v in hw)
                            yield ("conv2d k%d s%d d%d n%d c%d %dx%d" % (k, stride, dil, n, c, *hw), record32,
                                   lambda k=k, stride=stride, dil=dil, pad=pad, hw=hw, ohw=ohw, c=c, n=n: E.plan_conv2d(
                                       geo(n, c, 1, *hw, 0, max(dil, 1), max(dil, 1)), geo(n, c, 1, *ohw, 0, 1, 1), k, stride, pad, dil, c, True))
    for k in (1, 3):
        for hw in ((14, 14), (28, 28), (12, 38)):
            for c in (32, 128):
                yield ("deconv2d k%d c%d %dx%d" % (k, c, *hw), record32,
                       lambda k=k, hw=hw, c=c: E.plan_deconv2d(geo(2, c, 1, *hw, 0, 2, 2), geo(2, c, 1, 2 * hw[0], 2 * hw[1], 0, 2, 2), k, c, False))
    # the fp16-storage plans
    for n in (1, 4):
        for cin, cout in ((32, 32), (64, 32), (64, 64), (96, 64)):
            for d in ((3, 28, 28), (6, 14, 14), (12, 28, 28), (24, 20, 56), (24, 56, 56)):
                for stride in (1, 2):
                    od = d if stride == 1 else tuple(v // 2 for v in d)
                    yield ("conv3d16 s%d n%d c%d-%d %s" % (stride, n, cin, cout, "x".join(map(str, d))), record16,
                           lambda n=n, cin=cin, cout=cout, d=d, od=od, stride=stride: E.plan_conv3d16(geo16(n, cin, *d), geo16(n, cout, *od), stride, cout, True))
                yield ("deconv3d16 n%d c%d-%d %s" % (n, cin, cout, "x".join(map(str, d))), record16,
                       lambda n=n, cin=cin, cout=cout, d=d: E.plan_deconv3d16(geo16(n, cin, *d), geo16(n, cout, *(2 * v for v in d)), cout, False))
        for d in ((6, 14, 14), (12, 28, 28), (24, 56, 56), (24, 20, 56)):
            for lo4 in (0, -6):
                yield ("conv3d16_costvol n%d lo4=%d %s" % (n, lo4, "x".join(map(str, d))), record16,
                       lambda n=n, d=d, lo4=lo4: E.plan_conv3d16_costvol(geo16(n, 64, 1, d[1], d[2]), geo16(n, 32, *d), lo4, 32, True))
            yield ("conv3d16_cout1 n%d %s" % (n, "x".join(map(str, d))), record16, lambda n=n, d=d: E.plan_conv3d16_cout1(geo16(n, 32, *d)))


def dump_lines():
    """The dump as a list of JSON lines."""
    lines = []
    for name, record, thunk in cases():
        default = record(thunk())
        off = {}
        for sw, d, key in SWITCHES:
            with switched_off(d, key):
                rec = record(thunk())
            diff = {f: v for f, v in rec.items() if v != default[f]}
            if diff:
                off[sw] = diff
        lines.append(json.dumps({"case": name, "default": default, "off": off}, sort_keys=True))
    return lines


def golden_lines(lines):
    """The committed form of the dump: per line [case, default kname, digest of the line]."""
    out = []
    for line in lines:
        rec = json.loads(line)
        out.append(json.dumps([rec["case"], rec["default"]["kname"], hashlib.sha256(line.encode()).hexdigest()[:12]], separators=(",", ":")))
    return out


if __name__ == "__main__":
    lines = dump_lines()
    print("\n".join(golden_lines(lines) if "--golden" in sys.argv[1:] else lines))

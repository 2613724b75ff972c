"""Per-kernel instruction statistics of one csrc file's gfx950 code, read from the compiler's assembly (no GPU needed):

    python tools/isa_step_stats.py <file.hip> [kernel substring] [--json]

The file is compiled with the FLAGS of disprcnn_amd/csrc/build.py plus `--cuda-device-only -S` into a temporary directory.  Per kernel:
VGPR and AGPR counts, VGPR / SGPR spills, scratch bytes and scratch instructions, and the averages per STEADY-STATE STEP of

    mfma      matrix instructions (v_mfma_*, v_smfmac_*)
    srcA=a    those of them whose first source (the weights of the split-f16 convolutions) is an AGPR
    copies    v_accvgpr_* (AGPR <-> VGPR copies: a weight fragment held in an AGPR and copied back before its MFMA costs four)
    valu      every other v_* instruction except the lane moves
    lane      v_readlane_* / v_writelane_* (SGPR spills and their reloads)

A step is the code between two s_barrier with at least 40 MFMAs (one depth step of the walking kernels: 54 to 84 MFMAs; prologues, column
changes and drains hold fewer).  A kernel without such a step is reported by its whole-kernel totals (steps = 0).  Instructions are
classified by their opcode prefix only: the numbers are static counts of the generated code, not executed instructions.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from disprcnn_amd.csrc import build as B  # noqa: E402

STEP_MIN_MFMA = 40
KEYS = ("mfma", "mfma_srca_agpr", "copies", "valu", "lane")


def compile_to_asm(src, out_dir):
    src = src if os.path.exists(src) else os.path.join(B.HERE, src)
    out = os.path.join(out_dir, os.path.basename(src)[:-4] + ".s")
    cmd = [B.HIPCC] + B.FLAGS + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument", src, "-o", out]
    subprocess.check_call(cmd)
    return out


def short_name(mangled):
    """_ZN..14convs16_kernelILi2ELb0E..EEv.. -> convs16_kernel<2,false,..> (integer and bool template arguments, all these kernels have)."""
    m = re.match(r"_ZN?(?:\d+_GLOBAL__N_1)?(.*)", mangled)
    rest = m.group(1) if m else mangled
    names = []
    while True:
        m = re.match(r"(\d+)", rest)
        if not m:
            break
        n = int(m.group(1))
        names.append(rest[m.end():m.end() + n])
        rest = rest[m.end() + n:]
    if not names:
        return mangled
    name = "::".join(names)
    if rest.startswith("I"):
        args = []
        for kind, neg, val in re.findall(r"L([a-z])(n?)(\d+)E", rest[:rest.find("EE") + 1] if "EE" in rest else rest):
            args.append(("true" if val != "0" else "false") if kind == "b" else ("-" if neg else "") + val)
        name += "<" + ",".join(args) + ">"
    return name


def classify(op, operands):
    if op.startswith("v_mfma_") or op.startswith("v_smfmac_"):
        ops = [o.strip() for o in operands.split(",")]
        return "mfma_a" if len(ops) > 1 and ops[1].startswith("a") else "mfma_v"
    if op.startswith("v_accvgpr_"):
        return "copies"
    if op.startswith("v_readlane_") or op.startswith("v_writelane_"):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("scratch_"):
        return "scratch"
    if op == "s_barrier":
        return "barrier"
    return None


def _count(segment):
    c = {k: 0 for k in KEYS}
    c["scratch"] = 0
    for kind in segment:
        if kind in ("mfma_a", "mfma_v"):
            c["mfma"] += 1
            c["mfma_srca_agpr"] += kind == "mfma_a"
        elif kind in c:
            c[kind] += 1
    return c


def parse(asm_text):
    """-> list of per-kernel dicts, in the file's order."""
    meta = {}
    tail = asm_text[asm_text.find(".amdgpu_metadata"):] if ".amdgpu_metadata" in asm_text else ""
    for entry in re.split(r"\n  - (?=\.agpr_count:)", tail)[1:]:
        f = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
        if "name" in f:
            meta[f["name"]] = f
    kernels = []
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm_text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if name not in meta:
            continue
        kinds = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            parts = line.split(None, 1)
            kinds.append(classify(parts[0], parts[1] if len(parts) > 1 else ""))
        segments, cur = [], []
        for kind in kinds:
            if kind == "barrier":
                segments.append(cur)
                cur = []
            elif kind:
                cur.append(kind)
        segments.append(cur)
        total = _count([k for s in segments for k in s])
        steps = [c for c in map(_count, segments) if c["mfma"] >= STEP_MIN_MFMA]
        f = meta[name]
        k = {"name": short_name(name), "mangled": name,
             "vgprs": int(f.get("vgpr_count", 0)), "agprs": int(f.get("agpr_count", 0)),
             "vgpr_spills": int(f.get("vgpr_spill_count", 0)), "sgpr_spills": int(f.get("sgpr_spill_count", 0)),
             "scratch_bytes": int(f.get("private_segment_fixed_size", 0)), "scratch_insts": total["scratch"],
             "steps": len(steps), "total": {q: total[q] for q in KEYS}}
        src = steps if steps else [total]
        k["per_step"] = {q: sum(c[q] for c in src) / len(src) for q in KEYS}
        kernels.append(k)
    return kernels


def stats(src, substring=None):
    with tempfile.TemporaryDirectory(prefix="isa_step_stats_") as d:
        with open(compile_to_asm(src, d)) as f:
            ks = parse(f.read())
    return [k for k in ks if not substring or substring in k["name"] or substring in k["mangled"]]


def table(ks):
    lines = ["| kernel | steps | MFMA | srcA=a | `v_accvgpr_*` copies | other VALU | lane moves | VGPRs (AGPRs) | VGPR / SGPR spills | scratch B / insts |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for k in ks:
        p = k["per_step"]
        lines.append(f"| `{k['name']}` | {k['steps'] or 'whole kernel'} | {p['mfma']:.1f} | {p['mfma_srca_agpr']:.1f} | {p['copies']:.1f} | {p['valu']:.1f} | "
                     f"{p['lane']:.1f} | {k['vgprs']} ({k['agprs']}) | {k['vgpr_spills']} / {k['sgpr_spills']} | {k['scratch_bytes']} / {k['scratch_insts']} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("file", help="a .hip file (a path, or a name inside disprcnn_amd/csrc)")
    ap.add_argument("kernel", nargs="?", help="only kernels whose name contains this")
    ap.add_argument("--json", action="store_true", help="print the raw numbers as one JSON list")
    a = ap.parse_args()
    ks = stats(a.file, a.kernel)
    print(json.dumps(ks) if a.json else table(ks))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Build the reference's own PointNet++ GPU kernels for gfx950 into oracle/_ref/ (test infrastructure; authoring container only).

    python oracle/build_pn2_ref.py        ->  oracle/_ref/libpn2_ref.so

tests/pn2_oracle.py restates the reference's kernels in NumPy, and disprcnn_amd/pts/pointnet2.hip reimplements them.  This library
is the reference itself, so that both can be compared with it and a misreading they share shows.  The recipe, as build_ref.py's:

  1. the nine input files (pointnet2_lib/pointnet2/src/{sampling,ball_query,group_points,interpolate}_gpu.{cu,h}, cuda_utils.h) are
     pinned by sha256: anything but the surveyed sources is refused before a tool reads it;
  2. /opt/rocm/bin/hipify-perl translates each into a temporary directory (never inside the repo);
  3. one line is patched, checked word for word: sampling_gpu.h's `#include <ATen/cuda/CUDAContext.h>`, which hipify renames to a
     header ROCm torch does not ship and the kernels do not use, is deleted;
  4. hipcc compiles them with oracle/pn2_ref_binding.hip (our extern "C" entry points for ctypes).

Flags: `--offload-arch=gfx950 -O3 -fPIC -ffp-contract=off`.  `-ffp-contract=off` is our choice, not the reference's: its setup.py
passes nvcc only -O2, and nvcc contracts a*b+c into fused multiply-adds by default.  Our kernels build without contraction
(disprcnn_amd/csrc/build.py FLAGS), so the pin is the reference's source compiled the same way: both sides then evaluate the same
fp32 expressions, and comparing indices and values bit for bit is fair.  It is not a bit-exact copy of the reference as shipped.

Only the compiled library lands in oracle/_ref/ (git-ignored; it travels with the tree to the GPU machine).  The hipified text is
never written anywhere else.  Reference sources absent => nothing to do, the prebuilt library -- if present -- is used as is.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/disprcnn/modeling/pointnet_module/point_rcnn/lib/pointnet2_lib/pointnet2/src"
OUT = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT, "libpn2_ref.so")
BINDING = os.path.join(HERE, "pn2_ref_binding.hip")
HIPIFY = "/opt/rocm/bin/hipify-perl"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off"]

SHA256 = {
    "sampling_gpu.cu": "57d75315a624b10fa3367a14bd081136e156f4c99a05d6696e65d06e7bd28497",
    "sampling_gpu.h": "493afa85307d03c0f4b244d347a4e253bf63d5e49cf8546a8a4fe3d0f3d60e63",
    "ball_query_gpu.cu": "be3f98ea0521da854b2d84eecfc244f2d707c46ac90530b8a5346c35c58d6b5a",
    "ball_query_gpu.h": "e3b31787c538eb0729bd0ef0702d3943202c135377181f93131b13d21a00a711",
    "group_points_gpu.cu": "3886bf0b47a069f548bc94dc7eeed4508f84e3297192d7121be7d48c941b368c",
    "group_points_gpu.h": "94d5f4552a3ac4509f59087e64f5080686eeda47e6173f0f17c976cd97b53724",
    "interpolate_gpu.cu": "c893c96f62fc962139c58961a4076525d7b26469a790f509efec4aa569ed5af2",
    "interpolate_gpu.h": "a70d61b718adaa9c8fa16b94a58c77d5bfb5347ac48e1b3e744b0e07b5d75fc8",
    "cuda_utils.h": "7ace0019cea06178a57b275d3b1086b26cd5d0c83d646e8b8ae70c530e9e7bca",
}

# hipified file -> [(line number, exact line that is deleted)]
DELETE = {"sampling_gpu.h": [(5, "#include <ATen/cuda/HIPContext.h>")]}

_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SIGS = {   # extern "C" entry points of pn2_ref_binding.hip
    "pn2_ref_furthest_point_sampling": [_I, _I, _I, _P, _P, _P],
    "pn2_ref_gather_points": [_I, _I, _I, _I, _P, _P, _P],
    "pn2_ref_gather_points_grad": [_I, _I, _I, _I, _P, _P, _P],
    "pn2_ref_ball_query": [_I, _I, _I, _F, _I, _P, _P, _P],
    "pn2_ref_group_points": [_I, _I, _I, _I, _I, _P, _P, _P],
    "pn2_ref_group_points_grad": [_I, _I, _I, _I, _I, _P, _P, _P],
    "pn2_ref_three_nn": [_I, _I, _I, _P, _P, _P, _P],
    "pn2_ref_three_interpolate": [_I, _I, _I, _I, _P, _P, _P, _P],
    "pn2_ref_three_interpolate_grad": [_I, _I, _I, _I, _P, _P, _P, _P],
}


def load():
    """ctypes handle of the prebuilt library, None if it was never built.  A library that exists but does not load raises."""
    if not os.path.exists(LIB):
        return None
    import torch  # noqa: F401  (the HIP runtime torch uses must be loaded first)
    h = ctypes.CDLL(LIB)
    for name, args in SIGS.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = ctypes.c_int, args
    return h


def build(force=False, verbose=False):
    if not os.path.isdir(REF_SRC):
        return LIB if os.path.exists(LIB) else None
    for rel, want in SHA256.items():      # checked before the up-to-date shortcut: a changed source is never passed over silently
        got = hashlib.sha256(open(os.path.join(REF_SRC, rel), "rb").read()).hexdigest()
        if got != want:
            raise RuntimeError(f"{rel}: sha256 {got} is not the surveyed reference file's ({want}); refusing to translate it")
    if os.path.exists(LIB) and not force and os.path.getmtime(LIB) >= max(os.path.getmtime(BINDING), os.path.getmtime(__file__)):
        return LIB
    from torch.utils import cpp_extension
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="drc_pn2_ref_")
    try:
        for rel in SHA256:
            text = subprocess.run([HIPIFY, os.path.join(REF_SRC, rel)], check=True, capture_output=True, text=True).stdout
            lines = text.split("\n")
            for ln, old in DELETE.get(rel, []):
                if lines[ln - 1].strip() != old:
                    raise RuntimeError(f"{rel}:{ln} after hipify is {lines[ln - 1]!r}, not {old!r}: the patch does not apply")
                lines[ln - 1] = ""              # keep the line count, so compiler messages point at the reference's lines
            open(os.path.join(tmp, rel), "w").write("\n".join(lines))
        srcs = [os.path.join(tmp, r) for r in SHA256 if r.endswith(".cu")] + [BINDING]
        inc = [f"-I{p}" for p in cpp_extension.include_paths()] + [f"-I{tmp}"]
        objs = [os.path.join(tmp, f"{i}.o") for i in range(len(srcs))]
        jobs = [[HIPCC] + FLAGS + ["-x", "hip", "-c", s, "-o", o] + inc for s, o in zip(srcs, objs)]
        tmp_lib = os.path.join(tmp, "libpn2_ref.so")

        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd, cwd=tmp)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(len(srcs), 16, os.cpu_count() or 1))) as ex:
            list(ex.map(run, jobs))
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp_lib] + objs)
        shutil.copy(tmp_lib, LIB)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))

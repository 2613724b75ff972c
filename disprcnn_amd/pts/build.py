"""Build libdisprcnn_pts.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m disprcnn_amd.pts.build [--force]

The point ops live in their own library so that the regressor's kernel digest (disprcnn_amd/csrc/build.py:source_digest, which
the committed roofline profile is tied to) does not change when they do.  Same compiler flags as the main build.
"""
import os
import subprocess
import sys

from ..csrc.build import FLAGS, HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["points.hip", "pointnet2.hip", "boxes3d.hip", "pn2_mlp.hip", "rcnn_ops.hip", "frame_ops.hip", "kitti_eval.hip",
           "train_targets.hip", "pn2_mlp_bwd.hip", "proposal_target.hip", "solver.hip", "pn2_bn.hip", "match2d.hip", "frame_ops_train.hip",
           "det_train.hip", "body_train.hip", "input_ops.hip"]
HEADER = os.path.join(HERE, "..", "..", "include", "disprcnn_pts.h")
SHARED = [os.path.join(HERE, h) for h in ("box3d_pt.h", "box3d_iou.h", "mask_resize.h")]     # included by boxes3d.hip, rcnn_ops.hip, proposal_target.hip; det_train.hip, input_ops.hip
LIB = os.path.join(HERE, "libdisprcnn_pts.so")
MAX_JOBS = 16


def _sources():
    return [os.path.join(HERE, s) for s in SOURCES]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in _sources() + [HEADER, __file__] + SHARED)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    objs, jobs = [], []
    for src in _sources():
        obj = src[:-4] + ".o"
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(d) for d in [src, HEADER] + SHARED):
            jobs.append([HIPCC] + FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
    if jobs:
        from concurrent.futures import ThreadPoolExecutor

        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), MAX_JOBS, os.cpu_count() or 1))) as ex:
            list(ex.map(run, jobs))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)

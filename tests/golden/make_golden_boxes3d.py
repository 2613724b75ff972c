#!/usr/bin/env python3
"""Golden fixture for PointRCNN's 3D box ops, recorded from the REFERENCE's own code on CPU (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_boxes3d.py      -> boxes3d_ref_golden.npz

Reference code exercised:
  - its geometry: the helpers of point_rcnn/lib/utils/iou3d/src/iou3d_kernel.cu (everything before the first __global__, plus
    iou_normal) and pt_in_box3d_cpu of roipool3d/src/roipool3d.cpp.  Both files are pinned by sha256; the excerpts are compiled for
    the host in a temporary directory with `-ffp-contract=off` and `__device__` defined empty, next to a small driver of our own
    (DRIVER below) that emulates the mask and walk of iou3d.cpp's nms_gpu / nms_normal_gpu and the index rule of get_pooled_idx;
  - its Python: kitti_utils.boxes3d_to_bev_torch and enlarge_box3d, and iou3d_utils.boxes_iou3d_gpu (its torch steps, with the
    overlap served by the driver and `torch.cuda.FloatTensor` on CPU).
Nothing from the reference is written into the repository: only the inputs and the recorded outputs.

Checked here before anything is written: no IoU the NMS walks compare lies within 1e-4 of a threshold (exact zeros of disjoint
boxes at threshold 0 excepted), and no point lies within 1e-4 of a box face or of the max_dis limit, except the deliberate on-face
points at ry = 0 (cos and sin exact there).
"""
import ctypes
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/disprcnn/modeling/pointnet_module/point_rcnn/lib/utils"
SHA256 = {     # the surveyed sources: anything else is refused before a tool reads it
    "iou3d/src/iou3d_kernel.cu": "8881d38c94c3b3310e1b638b341718876c2ffdd731ad67a1b0dcc521736cb8cd",
    "roipool3d/src/roipool3d.cpp": "344e64c9c084be1d79b58909aa3be5a3aa2375b970d3a79642afda2652aef72c",
    "kitti_utils.py": "0e29aa260938ba31b51a7e177fe6cde98752d6bbc8baa3f459e627dedda230cc",
    "iou3d/iou3d_utils.py": "36e65e47867430c6ba3f7206bf9d4ff1ae32cd867fbc65d480d1f4896f705aa7",
}

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <algorithm>
using std::min;
using std::max;
#define __device__
#include "iou3d_helpers.inc"
#include "roipool3d_helpers.inc"

extern "C" {
void ref_pairwise(int na, const float* a, int nb, const float* b, int mode, float* out) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j)
            out[(long)i * nb + j] = mode == 0 ? box_overlap(a + i * 5, b + j * 5) : mode == 1 ? iou_bev(a + i * 5, b + j * 5)
                                                                                   : iou_normal(a + i * 5, b + j * 5);
}

// nms_gpu's walk over nms_kernel's / nms_normal_kernel's mask words.  A row's words are formed (as the kernel forms them: box i as
// box_a, every later box as box_b, `> thresh`) when the walk reads them, i.e. when box i is kept; the other rows are never read.
// offender[j] <- 1 when the IoU of a kept box with a later box j lies within `margin` of thresh (exact 0 at thresh 0 excepted).
int ref_nms(int n, const float* boxes, float thresh, int normal, long* keep, float margin, int* offender) {
    std::vector<char> removed(n, 0);
    int num = 0;
    for (int i = 0; i < n; ++i) {
        if (removed[i]) continue;
        keep[num++] = i;
        for (int j = i + 1; j < n; ++j) {
            const float v = normal ? iou_normal(boxes + i * 5, boxes + j * 5) : iou_bev(boxes + i * 5, boxes + j * 5);
            if (v > thresh) removed[j] = 1;
            if (offender && fabsf(v - thresh) < margin && !(thresh == 0.f && v == 0.f)) offender[j] = 1;
        }
    }
    return num;
}

void ref_pts_in_boxes(int n, const float* pts, int m, const float* boxes, int* flags) {
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j)
            flags[(long)i * n + j] = pt_in_box3d_cpu(pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2], boxes[i * 7], boxes[i * 7 + 1],
                                                     boxes[i * 7 + 2], boxes[i * 7 + 3], boxes[i * 7 + 4], boxes[i * 7 + 5], boxes[i * 7 + 6]);
}

// get_pooled_idx of one batch row: flags [M,N] -> idx [M,S], empty [M]
void ref_pool_idx(int n, int m, const int* flags, int S, int* idx, int* empty) {
    for (int b = 0; b < m; ++b) {
        int cnt = 0;
        for (int k = 0; k < n; ++k) {
            if (flags[(long)b * n + k]) {
                if (cnt < S) idx[(long)b * S + cnt++] = k;
                else break;
            }
        }
        if (cnt == 0) empty[b] = 1;
        else for (int k = cnt; k < S; ++k) idx[(long)b * S + k] = idx[(long)b * S + k % cnt];
    }
}
}
"""


def _read_pinned(rel):
    data = open(os.path.join(REF, rel), "rb").read()
    digest = hashlib.sha256(data).hexdigest()
    if digest != SHA256[rel]:
        raise SystemExit(f"{rel}: sha256 {digest} is not the surveyed source ({SHA256[rel]})")
    return data.decode()


def _excerpts():
    k = _read_pinned("iou3d/src/iou3d_kernel.cu")
    head = k[:k.index("__global__")]
    i0 = k.index("__device__ inline float iou_normal")
    i1 = k.index("__global__", i0)
    r = _read_pinned("roipool3d/src/roipool3d.cpp")
    p0 = r.index("int pt_in_box3d_cpu(")
    p1 = r.index("int pts_in_boxes3d_cpu(")
    return head + "\n" + k[i0:i1], r[p0:p1]


def build_driver(tmp):
    iou_src, pool_src = _excerpts()
    open(os.path.join(tmp, "iou3d_helpers.inc"), "w").write(iou_src)
    open(os.path.join(tmp, "roipool3d_helpers.inc"), "w").write(pool_src)
    open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
    so = os.path.join(tmp, "libbox3d_ref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(tmp, "driver.cpp")], cwd=tmp)
    lib = ctypes.CDLL(so)
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ref_pairwise.argtypes = [I, P, I, P, I, P]
    lib.ref_nms.argtypes = [I, P, Fl, I, P, Fl, P]
    lib.ref_nms.restype = I
    lib.ref_pts_in_boxes.argtypes = [I, P, I, P, P]
    lib.ref_pool_idx.argtypes = [I, I, P, I, P, P]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def pairwise(self, a, b, mode):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        out = np.zeros((a.shape[0], b.shape[0]), np.float32)
        self.lib.ref_pairwise(a.shape[0], _p(a), b.shape[0], _p(b), mode, _p(out))
        return out

    def nms(self, boxes_sorted, thresh, normal, margin=1e-4):
        """-> (kept positions, offenders: boxes whose IoU with a kept one lies within margin of thresh)"""
        b = np.ascontiguousarray(boxes_sorted, np.float32)
        keep = np.zeros(max(b.shape[0], 1), np.int64)
        off = np.zeros(max(b.shape[0], 1), np.int32)
        k = self.lib.ref_nms(b.shape[0], _p(b), float(thresh), int(normal), _p(keep), float(margin), _p(off))
        return keep[:k].copy(), off[:b.shape[0]].astype(bool)

    def flags(self, pts, boxes):
        p, b = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(boxes, np.float32)
        f = np.zeros((b.shape[0], p.shape[0]), np.int32)
        self.lib.ref_pts_in_boxes(p.shape[0], _p(p), b.shape[0], _p(b), _p(f))
        return f

    def pool_idx(self, flags, S):
        m, n = flags.shape
        idx, empty = np.zeros((m, S), np.int32), np.zeros(m, np.int32)
        self.lib.ref_pool_idx(n, m, _p(np.ascontiguousarray(flags, np.int32)), S, _p(idx), _p(empty))
        return idx, empty


def ref_python(ref):
    """kitti_utils and iou3d_utils, imported from the reference as they are; iou3d_cuda served by the host driver."""
    pkg = types.ModuleType("refutils")
    pkg.__path__ = [REF]
    sys.modules["refutils"] = pkg
    _read_pinned("kitti_utils.py")
    _read_pinned("iou3d/iou3d_utils.py")
    spec = importlib.util.spec_from_file_location("refutils.kitti_utils", os.path.join(REF, "kitti_utils.py"))
    ku = importlib.util.module_from_spec(spec)
    sys.modules["refutils.kitti_utils"] = ku
    spec.loader.exec_module(ku)
    sub = types.ModuleType("refutils.iou3d")
    sub.__path__ = [os.path.join(REF, "iou3d")]
    sys.modules["refutils.iou3d"] = sub

    def overlap(a, b, out):
        out.copy_(torch.from_numpy(ref.pairwise(a.numpy(), b.numpy(), 0)))
        return 1
    sys.modules["iou3d_cuda"] = types.SimpleNamespace(boxes_overlap_bev_gpu=overlap)
    torch.cuda.FloatTensor = lambda size: torch.empty(size, dtype=torch.float32)
    spec = importlib.util.spec_from_file_location("refutils.iou3d.iou3d_utils", os.path.join(REF, "iou3d", "iou3d_utils.py"))
    iu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(iu)
    return ku, iu


def rand_bev(r, n, span=40.0, size=(0.5, 5.0)):
    c = r.uniform(-span, span, (n, 2))
    s = r.uniform(size[0], size[1], (n, 2))
    a = r.uniform(-np.pi, np.pi, n)
    return np.concatenate([c - s / 2, c + s / 2, a[:, None]], 1).astype(np.float32)


def rand_b7(r, n):
    x, z = r.uniform(-30, 30, n), r.uniform(2, 80, n)
    h, w, l = r.uniform(1.2, 2.2, n), r.uniform(1.4, 2.0, n), r.uniform(3.0, 5.0, n)
    y = r.uniform(1.0, 2.0, n)
    ry = r.uniform(-np.pi, np.pi, n)
    return np.stack([x, y, z, h, w, l, ry], 1).astype(np.float32)


def cluster_bev(r, n, centers):
    """Proposal-like clusters: jittered copies of a few objects (heavy mutual overlap, the NMS regime)."""
    k = r.randint(0, len(centers), n)
    base = centers[k]
    jit = r.normal(0, 1, (n, 5)) * np.array([0.4, 0.4, 0.4, 0.4, 0.15])
    b = base + jit
    b[:, 2] = np.maximum(b[:, 2], b[:, 0] + 0.3)
    b[:, 3] = np.maximum(b[:, 3], b[:, 1] + 0.3)
    return b.astype(np.float32)


def nms_case(ref, r, n, thresholds, normal):
    """n boxes in score order and their keep lists.  Boxes whose IoU with a kept box lies within 1e-4 of a threshold are dropped
    until none is left; the list is drawn longer and its tail cut to n (a box's fate depends only on the boxes before it)."""
    if n == 0:
        return np.zeros((0, 5), np.float32), [np.zeros(0, np.int64) for _ in thresholds]
    centers = rand_bev(r, max(1, n // 40), span=30.0 * max(1.0, (n / 768) ** 0.5), size=(2.0, 5.0)).astype(np.float64)
    boxes = cluster_bev(r, n + n // 20 + 4, centers)
    while True:
        bad = np.zeros(boxes.shape[0], bool)
        for t in thresholds:
            bad |= ref.nms(boxes, t, normal)[1]
        if not bad.any():
            break
        boxes = boxes[~bad]
    assert boxes.shape[0] >= n, "too many boxes dropped"
    boxes = boxes[:n]
    keeps = []
    for t in thresholds:
        keep, bad = ref.nms(boxes, t, normal)
        assert not bad.any()
        keeps.append(keep)
    return boxes, keeps


def hand_bev():
    """Hand cases: identical, containment, disjoint, touching edges, multiples of pi/2 with coincident edges, zero area, ry = +-pi."""
    pi = np.float32(np.pi)
    a = np.array([[0, 0, 2, 2, 0], [0, 0, 2, 2, pi / 2], [0, 0, 4, 2, pi], [0, 0, 4, 2, -pi], [1, 1, 1, 3, 0], [0, 0, 2, 2, 0.3]], np.float32)
    b = np.array([[0, 0, 2, 2, 0], [0.5, 0.5, 1.5, 1.5, 0], [5, 5, 6, 6, 0], [2, 0, 4, 2, 0], [0, 0, 2, 2, pi], [1, -1, 3, 3, pi / 2],
                  [0, 0, 4, 2, 0], [1, 1, 1, 1, 0], [-1, -1, 3, 3, 0.7]], np.float32)
    return a, b


def roipool_case(r):
    """Two batch rows of 1800 points; per row, boxes holding 511, 512, 600, 1 and 0 points, and one box at ry = 0 with 4 points exactly
    on its faces (cos and sin exact).  The cluster boxes of row 1 are rotated."""
    B, N = 2, 1800
    pts = np.zeros((B, N, 3), np.float32)
    boxes = []
    for bi in range(B):
        p = np.zeros((N, 3))
        o = 0
        for xc, cnt in ((-10.0, 511), (0.0, 512), (10.0, 600)):
            p[o:o + cnt] = np.stack([r.uniform(xc - 1.5, xc + 1.5, cnt), r.uniform(0.2, 1.6, cnt), r.uniform(18.5, 21.5, cnt)], 1)
            o += cnt
        p[o] = [-15.0, 0.5, 40.0]                                                            # a lone point
        p[o + 1:o + 5] = [[10.0, 1.0, 30.0], [12.0, 1.0, 30.0], [11.0, 1.0, 29.5], [11.0, 0.0, 30.5]]   # on the faces of the last box
        o += 5
        p[o:] = np.stack([r.uniform(-25, 25, N - o), r.uniform(-1, 2.5, N - o), r.uniform(46, 60, N - o)], 1)   # background
        perm = r.permutation(N)                                                              # index order != spatial order
        pts[bi] = p[perm]
        ry = 0.3 * bi
        boxes.append([[-10.0, 1.8, 20.0, 2.0, 4.0, 4.0, ry], [0.0, 1.8, 20.0, 2.0, 4.0, 4.0, -ry], [10.0, 1.8, 20.0, 2.0, 4.0, 4.0, ry],
                      [-15.0, 1.0, 40.0, 1.0, 0.6, 0.6, 0.0], [0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0], [11.0, 1.0, 30.0, 1.0, 1.0, 2.0, 0.0]])
    return pts, np.asarray(boxes, np.float32)


def on_face_mask(pts):
    f = np.zeros(pts.shape[0], bool)
    for q in ([10.0, 1.0, 30.0], [12.0, 1.0, 30.0], [11.0, 1.0, 29.5], [11.0, 0.0, 30.5]):
        f |= (pts == np.float32(q)).all(1)
    return f


def main():
    r = np.random.RandomState(20261016)
    with tempfile.TemporaryDirectory() as tmp:
        ref = Ref(build_driver(tmp))
        ku, iu = ref_python(ref)
        out = {}
        # ---- pairwise BEV: random (Na 17 x Nb 257), KITTI-like rotated, and the hand cases
        a, b = rand_bev(r, 17), rand_bev(r, 257)
        a[:8] = b[:8] + r.normal(0, 0.3, (8, 5)).astype(np.float32)     # some overlap
        out.update(bev_a=a, bev_b=b, bev_overlap=ref.pairwise(a, b, 0), bev_iou=ref.pairwise(a, b, 1), bev_iou_normal=ref.pairwise(a, b, 2))
        ha, hb = hand_bev()
        out.update(hand_a=ha, hand_b=hb, hand_overlap=ref.pairwise(ha, hb, 0), hand_iou=ref.pairwise(ha, hb, 1))
        # ---- 3D IoU through the reference's Python
        a7, b7 = rand_b7(r, 40), rand_b7(r, 33)
        a7[:20] = b7[:20] + r.normal(0, 0.25, (20, 7)).astype(np.float32)
        ta, tb = torch.from_numpy(a7), torch.from_numpy(b7)
        out.update(b7_a=a7, b7_b=b7, iou3d=iu.boxes_iou3d_gpu(ta, tb).numpy(), bev_of_a=ku.boxes3d_to_bev_torch(ta).numpy(),
                   enlarged_a=ku.enlarge_box3d(ta.clone(), 1.0).numpy())
        # ---- NMS
        ths = (0.0, 0.1, 0.8, 1.0)
        for n in (0, 1, 63, 64, 65, 768, 9000):
            for normal in (False, True):
                boxes, keeps = nms_case(ref, r, n, ths, normal)
                tag = f"nms{'n' if normal else 'r'}_{n}"
                out[tag + "_boxes"] = boxes
                for t, k in zip(ths, keeps):
                    out[f"{tag}_keep_{t}"] = k.astype(np.int32)
        # ---- roipool3d
        pts, boxes = roipool_case(r)
        for w in (0.0, 1.0):
            flags, idx, empty = [], [], []
            for bi in range(pts.shape[0]):
                big = ku.enlarge_box3d(torch.from_numpy(boxes[bi]).clone(), w).numpy()
                f = ref.flags(pts[bi], big)
                ii, ee = ref.pool_idx(f, 512)
                flags.append(f)
                idx.append(ii)
                empty.append(ee)
                margins(pts[bi], big, on_face_mask(pts[bi]))
            out[f"pool_{w}_flags"] = np.packbits(np.asarray(flags, np.uint8), axis=-1)
            out[f"pool_{w}_idx"] = np.asarray(idx, np.int16)
            out[f"pool_{w}_empty"] = np.asarray(empty, np.int32)
        out.update(pool_pts=pts, pool_boxes=boxes)
    np.savez_compressed(os.path.join(HERE, "boxes3d_ref_golden.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", None))


def margins(pts, boxes, on_face):
    """Assert no point's in-box result changes when a box's faces and the max_dis limit move by 1e-4 (fp64), except the deliberate
    on-face points."""
    p = pts.astype(np.float64)
    for bx in boxes.astype(np.float64):
        cx, by, cz, h, w, l, ry = bx
        dx, dz = p[:, 0] - cx, p[:, 2] - cz
        xr = dx * np.cos(ry) - dz * np.sin(ry)
        zr = dx * np.sin(ry) + dz * np.cos(ry)

        def inside(d):
            return (np.abs(xr) <= l / 2 + d) & (np.abs(zr) <= w / 2 + d) & (np.abs(p[:, 1] - (by - h / 2)) <= h / 2 + d) & \
                   (np.abs(dx) <= 10 + d) & (np.abs(dz) <= 10 + d)
        bad = (inside(1e-4) != inside(-1e-4)) & ~on_face
        assert not bad.any(), f"points {np.nonzero(bad)[0][:5]} lie within 1e-4 of a face of box {bx}"


if __name__ == "__main__":
    main()

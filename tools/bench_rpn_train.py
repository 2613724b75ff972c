#!/usr/bin/env python3
"""Time one training step of PointRCNN's RPN (car config: 16 clouds of 768 points, BatchNorm on batch statistics) on one GPU with HIP
events, and the BatchNorm kernels of pts/pn2_bn.hip on the tensor of SA level 0.

    python tools/bench_rpn_train.py [--iters 20] [--warmup 3] [--batch 16]
    python tools/bench_rpn_train.py --only level0         # the BatchNorm entry points alone, for a `rocprofv3 --kernel-trace --stats` run

  * step: RPN.train()(clouds, labels) -> loss (forward), loss.backward() (backward), FusedSGD.step() (optimizer), each between its own
    pair of events; medians, min / max as the spread.  In a second pass of the same steps every BatchNorm call (statistics + apply in the
    forward, the three launches of the backward) is bracketed by events: `bn_share` is their sum over that pass's forward + backward.
  * level0: the three BatchNorm entry points on fp32 (16, 16, 768 * 32), the tensor of SA level 0's wider scale: 393 216 columns per
    channel.  Each is run `reps` times back to back between one pair of events.  Bytes are counted from the passes the kernels make
    over the tensor of T bytes: statistics read T; apply reads T and writes T; the backward reads gz, z, y (3 T), then reads them again
    and writes gy (4 T).  `hbm_fraction` is bytes / 8 TB/s (the HBM3E peak) over the measured time.  "hot" reuses one set of tensors
    (100 MB: it stays in the 256 MiB Infinity Cache, as it does in the training step, where the conv has just written y), "cold"
    walks over enough sets to exceed that cache, so every pass comes from HBM.
  * torch: torch.nn.functional.batch_norm(training=True) + relu, forward and backward through autograd, on the same tensor, against
    bn_act_train's forward and backward through autograd, alternating in one process.
Microseconds, one JSON line.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_rpn as BR  # noqa: E402
from bench_rcnn import stats, time_alternating, timed  # noqa: E402
from disprcnn_amd import engine as E  # noqa: E402
from disprcnn_amd.layers import pn2_mlp  # noqa: E402
from disprcnn_amd.pts import _lib  # noqa: E402
from disprcnn_amd.solver.fused import FusedSGD  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402

HBM_PEAK = 8.0e12           # bytes / s
L3_BYTES = 256 << 20


def build_model(dev):
    m = BR.build_model(BR.car_cfg(), dev)
    return m.train()


def labels(B, N, dev):
    g = torch.Generator().manual_seed(2)
    u = torch.rand(B, N, generator=g)
    cls = torch.where(u < 0.4, torch.ones(()), torch.where(u < 0.55, -torch.ones(()), torch.zeros(())))
    reg = torch.cat([torch.rand(B, N, 3, generator=g) * 4 - 2, torch.tensor([1.5, 1.6, 3.9]) * (0.85 + 0.3 * torch.rand(B, N, 3, generator=g)),
                     torch.rand(B, N, 1, generator=g) * 6.28 - 3.14], 2)
    targets = [BoxList(torch.tensor([[0.0, 0.0, 10.0, 10.0]]), (1242, 375), mode="xyxy") for _ in range(B)]
    return cls.to(dev), reg.to(dev).contiguous(), targets


class BnSpans:
    """Event pairs around every BatchNorm forward and backward while `on`."""

    def __init__(self):
        self.on, self.ev = False, []
        fwd, bwd = pn2_mlp._BnActTrain.forward, pn2_mlp._BnActTrain.backward
        pn2_mlp._BnActTrain.forward = staticmethod(self._wrap(fwd))
        pn2_mlp._BnActTrain.backward = staticmethod(self._wrap(bwd))

    def _wrap(self, fn):
        def run(*a):
            if not self.on:
                return fn(*a)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a)
            e.record()
            self.ev.append((s, e))
            return out
        return run

    def total(self):
        t = sum(s.elapsed_time(e) for s, e in self.ev) * 1e3
        n, self.ev = len(self.ev), []
        return t, n


def bench_step(B, iters, warmup, dev):
    spans = BnSpans()
    m = build_model(dev)
    opt = FusedSGD(m.parameters(), lr=1e-3, momentum=0.9)
    pts = BR.clouds(B, dev)
    cls, reg, targets = labels(B, pts.shape[1], dev)
    t = {"forward": [], "backward": [], "optimizer": [], "bn": [], "fwd_bwd_with_marks": []}
    n_bn = 0
    for it in range(warmup + 2 * iters):
        marks = it >= warmup + iters
        spans.on = marks
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        opt.zero_grad(set_to_none=True)
        ev[0].record()
        _, losses = m(pts, cls, reg, targets)
        loss = losses["rpn_loss_cls"] + losses["rpn_loss_reg"]
        ev[1].record()
        loss.backward()
        ev[2].record()
        opt.step()
        ev[3].record()
        torch.cuda.synchronize()
        if it < warmup:
            continue
        if marks:
            bn, n_bn = spans.total()
            t["bn"].append(bn)
            t["fwd_bwd_with_marks"].append(ev[0].elapsed_time(ev[2]) * 1e3)
        else:
            for k, (a, b) in zip(("forward", "backward", "optimizer"), ((0, 1), (1, 2), (2, 3))):
                t[k].append(ev[a].elapsed_time(ev[b]) * 1e3)
    out = {k: stats(v) for k, v in t.items()}
    out["step_median"] = round(sum(out[k]["median"] for k in ("forward", "backward", "optimizer")), 1)
    out["bn_calls"] = n_bn
    out["bn_share"] = round(out["bn"]["median"] / out["fwd_bwd_with_marks"]["median"], 3)
    out["loss"] = float(loss.detach())
    return out


def bench_level0(iters, warmup, reps, dev, shape=(16, 16, 768 * 32)):
    B, C, N = shape
    T = B * C * N * 4
    L = _lib.lib()
    n_sets = {"hot": 1, "cold": L3_BYTES // (4 * T) + 2}
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    mi = torch.empty(2, C, device=dev)
    gg, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(L.drc_pn2_bn_workspace_doubles(B, C, N), dtype=torch.float64, device=dev)
    st = E._stream_ptr(torch.device(dev))
    out = {"shape": list(shape), "tensor_bytes": T, "reps": reps}
    for mode, n in n_sets.items():
        sets = [dict(y=torch.randn(shape, device=dev), gz=torch.randn(shape, device=dev), z=torch.empty(shape, device=dev),
                     gy=torch.empty(shape, device=dev)) for _ in range(n)]
        p = E._ptr

        def f_stats():
            for i in range(reps):
                s = sets[i % n]
                _lib.check(L.drc_pn2_bn_stats(B, C, N, p(s["y"]), p(ws), 1e-5, 0.1, p(mi), p(rm), p(rv), st), "stats")

        def f_apply():
            for i in range(reps):
                s = sets[i % n]
                _lib.check(L.drc_pn2_bn_apply_fwd(B, C, N, 1, p(s["y"]), p(mi), p(gamma), p(beta), p(s["z"]), st), "apply")

        def f_bwd():
            for i in range(reps):
                s = sets[i % n]
                _lib.check(L.drc_pn2_bn_bwd(B, C, N, 1, p(s["gz"]), p(s["z"]), p(s["y"]), p(mi), p(gamma), p(ws), p(s["gy"]), p(gg), p(gb), st),
                           "bwd")
        f_stats()
        for s in sets:          # every set's z is the output of its own y
            L.drc_pn2_bn_apply_fwd(B, C, N, 1, p(s["y"]), p(mi), p(gamma), p(beta), p(s["z"]), st)
        res = {}
        for name, fn, nbytes in (("stats", f_stats, T), ("apply_fwd", f_apply, 2 * T), ("bwd", f_bwd, 7 * T)):
            us = stats([v / reps for v in timed(fn, iters, warmup)])
            res[name] = dict(us, bytes=nbytes, hbm_bound_us=round(nbytes / HBM_PEAK * 1e6, 2),
                             hbm_fraction=round(nbytes / HBM_PEAK * 1e6 / us["median"], 3))
        out[mode] = res
        del sets
        torch.cuda.empty_cache()
    return out


def bench_vs_torch(iters, warmup, dev, shape=(16, 16, 768 * 32)):
    C = shape[1]
    y = torch.randn(shape, device=dev).requires_grad_()
    gz = torch.randn(shape, device=dev)
    gamma, beta = (torch.rand(C, device=dev) + 0.5).requires_grad_(), (torch.randn(C, device=dev) * 0.1).requires_grad_()
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    keep = {}

    def clear():
        y.grad = gamma.grad = beta.grad = None

    def hip_fwd():
        keep["hip"] = pn2_mlp.bn_act_train(y, gamma, beta, rm, rv, 0.1, 1e-5, True)

    def torch_fwd():
        keep["torch"] = F.relu(F.batch_norm(y, rm, rv, gamma, beta, True, 0.1, 1e-5))

    def hip_bwd():
        clear()
        keep["hip"].backward(gz, retain_graph=True)

    def torch_bwd():
        clear()
        keep["torch"].backward(gz, retain_graph=True)
    fh, ft = time_alternating(hip_fwd, torch_fwd, iters, warmup)
    bh, bt = time_alternating(hip_bwd, torch_bwd, iters, warmup)
    return {"shape": list(shape), "forward": {"hip": fh, "torch": ft}, "backward": {"hip": bh, "torch": bt},
            "hip_total_median": round(fh["median"] + bh["median"], 1), "torch_total_median": round(ft["median"] + bt["median"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["level0", "vs_torch", "step"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rpn_train: needs the GPU; there is no CPU path to time")
    dev = "cuda"
    out = {"bench": "rpn_train", "batch": a.batch, "points": 768, "device": torch.cuda.get_device_name(0)}
    if a.only in (None, "level0"):
        out["level0"] = bench_level0(a.iters, a.warmup, a.reps, dev)
    if a.only in (None, "vs_torch"):
        out["vs_torch"] = bench_vs_torch(a.iters, a.warmup, dev)
    if a.only in (None, "step"):
        out["step"] = bench_step(a.batch, a.iters, a.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

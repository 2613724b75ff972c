#!/usr/bin/env python3
"""Time the optimizer step on the parameter sets of PSMNet and PointRCNN's RCNNNet, gradients in comm.GradientSync's flat buffer.

    python tools/bench_solver.py [--iters 50] [--warmup 5] [--sets psmnet,rcnn]

Per parameter set, optimizer (SGD with momentum 0.9, Adam; weight decay 1e-4) and with / without clipping (max_norm far above the norm,
so the values stay put and the scaled gradient is still written back), alternating in ONE process after a warm-up of both:
  * fused : disprcnn_amd.solver.FusedSGD / FusedAdam, ``step(max_norm=...)``;
  * torch : torch.optim.SGD / Adam (+ torch.nn.utils.clip_grad_norm_) on the SAME parameter and gradient tensors;
each with ONE group for all parameters (as bench.py builds its optimizer) and with one group PER parameter (as make_optimizer and the
reference build theirs).  Reported, in microseconds:
  * step    : device-event time around one step call, median with min / max as the repeat-to-repeat spread.  It includes the host's
              share where the host is slower than the device (an eager step is a handful of small kernels);
  * host    : wall time of the call itself (the enqueue);
  * launches, kernel_us : kernels of one step and the sum of their device times, read from the profiler's device trace
              ("not measured" with the reason when the trace is not available);
  * bytes, hbm_share : the bytes the step has to move (per element: SGD 20, +4 with the scaled gradient written back; Adam 28, +4;
              +4 for the norm's read of the gradient) and the time those take at the measured copy rate over kernel_us.  The step is
              bytes-bound: its arithmetic is a few flops per 20 to 36 bytes.
One JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_rcnn import stats  # noqa: E402
from disprcnn_amd.solver import FusedAdam, FusedSGD  # noqa: E402
from disprcnn_amd.utils.comm import GradientSync  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the measured device-to-device copy rate of the MI355X


def param_set(name, dev):
    if name == "psmnet":
        from disprcnn_amd.modeling.psmnet.stackhourglass import PSMNet
        net = PSMNet(48, 0)
    elif name == "rcnn":
        import copy
        from bench_rcnn_train import train_cfg
        from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet
        net = RCNNNet(copy.deepcopy(train_cfg()), None)
    else:
        raise ValueError(name)
    return [p for p in net.to(dev).parameters() if p.requires_grad]


def step_bytes(kind, clip, n):
    per = (20 if kind == "sgd" else 28) + (8 if clip else 0)
    return per * n


def alternating(fa, fb, iters, warmup):
    """device-event and host times of fa and fb, alternated"""
    for _ in range(warmup):
        fa()
        fb()
    dev, host = ([], []), ([], [])
    for _ in range(iters):
        for k, fn in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev[k].append(a.elapsed_time(b) * 1e3)
            host[k].append((t1 - t0) * 1e6)
    return [{"step": stats(dev[k]), "host": stats(host[k])} for k in (0, 1)]


def device_trace(fn):
    """(kernels, sum of their device times in us, {name: count}) of one call, from the profiler's device trace"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # the device track also carries copies, memsets and the span of the optimizer's own profiler annotation: kernels only
    ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA and not getattr(e, "is_user_annotation", False)
          and not e.name.lower().startswith(("memcpy", "memset", "optimizer.step#"))]
    if not ev:
        raise RuntimeError("the trace holds no kernels")
    names = {}
    for e in ev:
        names[e.name[:60]] = names.get(e.name[:60], 0) + 1
    return len(ev), round(sum(e.device_time for e in ev), 1), names


def bench_set(name, dev, iters, warmup):
    params = param_set(name, dev)
    n = sum(p.numel() for p in params)
    sync = GradientSync(params)
    sync.zero_grad()
    for p in params:                     # through the views: the flat buffer itself is GradientSync's business
        p.grad.normal_(0, 1e-3)
    out = {"tensors": len(params), "elements": n, "gradients": "views of one flat buffer",
           "misaligned_gradients": sum(1 for p in params if p.grad.data_ptr() % 16)}
    max_norm = 1e9
    for layout in ("one_group", "group_per_param"):
        groups = (lambda: [{"params": params}]) if layout == "one_group" else (lambda: [{"params": [p]} for p in params])
        for kind in ("sgd", "adam"):
            kw = dict(lr=1e-7, weight_decay=1e-4, **({"momentum": 0.9} if kind == "sgd" else {}))
            for clip in (False, True):
                fused = (FusedSGD if kind == "sgd" else FusedAdam)(groups(), **kw)
                ref = (torch.optim.SGD if kind == "sgd" else torch.optim.Adam)(groups(), **kw)

                def f_fused():
                    fused.step(max_norm=max_norm if clip else None)

                def f_torch():
                    if clip:
                        torch.nn.utils.clip_grad_norm_(params, max_norm)
                    ref.step()
                a, b = alternating(f_fused, f_torch, iters, warmup)
                nbytes = step_bytes(kind, clip, n)
                floor_us = nbytes / COPY_RATE * 1e6
                for r, fn in ((a, f_fused), (b, f_torch)):
                    try:
                        r["launches"], r["kernel_us"], names = device_trace(fn)
                        if fn is f_fused:
                            r["kernels"] = names
                        r["hbm_share"] = round(floor_us / r["kernel_us"], 3)
                        r["bytes_per_s"] = round(nbytes / (r["kernel_us"] * 1e-6), -9)
                    except Exception as ex:            # the numbers above stand without the trace
                        r["launches"] = r["kernel_us"] = f"not measured: {ex!r}"[:200]
                spread = b["step"]["max"] - b["step"]["min"]
                out[f"{layout}.{kind}.{'clip' if clip else 'noclip'}"] = {
                    "fused": a, "torch": b, "bytes": nbytes, "floor_us": round(floor_us, 1), "bound": "bytes",
                    "fused_within_torch_plus_spread": a["step"]["median"] <= b["step"]["median"] + spread}
                del fused, ref
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", default="psmnet,rcnn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_solver needs the GPU: a time taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"iters": a.iters, "unit": "us", "copy_rate_bytes_per_s": COPY_RATE}
    for name in a.sets.split(","):
        res[name] = bench_set(name, dev, a.iters, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the device input pipeline on one GPU: 2 KITTI pairs of 375 x 1242 resized to 600 x 1987 (MIN_SIZE_TRAIN 600), 8 instance masks
per view, one disparity map per pair.

    python tools/bench_input.py [--iters 20] [--warmup 3] [--host-iters 3]

Prints one JSON line, microseconds (medians): the byte upload, the image kernel (both views), the mask kernel (both views), the disparity
resizes and the whole DeviceBatchCollator call (GPU events, and wall clock with a synchronize), next to (a) the host path -- per-sample
transforms + to_image_list + the fp32 upload, wall clock -- and (b) the same gathers written as torch ops on the GPU.  The image kernel's
written bytes per second stand beside the 6.3 TB/s float4-copy rate of an MI355X.
"""
import argparse
import json
import os
import random
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from disprcnn_amd.data import device_input as D  # noqa: E402
from disprcnn_amd.data.collate_batch import DeviceBatchCollator, DoubleViewBatchCollator  # noqa: E402
from disprcnn_amd.data.transforms import build_transforms  # noqa: E402
from disprcnn_amd.structures.bounding_box import BoxList  # noqa: E402
from disprcnn_amd.structures.calib import Calib  # noqa: E402
from disprcnn_amd.structures.disparity import DisparityMap  # noqa: E402
from disprcnn_amd.structures.segmentation_mask import SegmentationMask, resize_flip_batch  # noqa: E402

H, W, OH, OW, PAIRS, G = 375, 1242, 600, 1987, 2, 8
COPY_RATE = 6.3e12
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]], dtype=np.float32)
P3 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]], dtype=np.float32)
CFG = SimpleNamespace(INPUT=SimpleNamespace(DO_RESIZE=True, MIN_SIZE_TRAIN=(600,), MAX_SIZE_TRAIN=10000, MIN_SIZE_TEST=600, MAX_SIZE_TEST=10000,
                                            FLIP_PROB_TRAIN=0.5, TO_BGR255=True, PIXEL_MEAN=[102.9801, 115.9465, 122.7717],
                                            PIXEL_STD=[1.0, 1.0, 1.0]), DATALOADER=SimpleNamespace(SIZE_DIVISIBILITY=0))


def samples(device=None):
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(PAIRS):
        imgs, targets = {}, {}
        for k in ("left", "right"):
            imgs[k] = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
            cx, cy = rng.uniform(100, W - 100, G), rng.uniform(120, 300, G)
            rx, ry = rng.uniform(20, 120, G), rng.uniform(15, 70, G)
            masks = np.stack([(((xx - cx[g]) / rx[g]) ** 2 + ((yy - cy[g]) / ry[g]) ** 2 <= 1) for g in range(G)]).astype(np.uint8)
            box = np.stack([cx - rx, cy - ry, cx + rx, cy + ry], 1).astype(np.float32)
            t = BoxList(torch.from_numpy(box), (W, H))
            t.add_field("labels", torch.ones(G, dtype=torch.int64))
            t.add_field("masks", SegmentationMask(torch.from_numpy(masks), (W, H)))
            t.add_field("calib", Calib(SimpleNamespace(P2=P2, P3=P3), (W, H)))
            if k == "left":
                t.add_map("disparity", DisparityMap(torch.from_numpy(rng.uniform(0, 80, size=(H, W)).astype(np.float32))))
            targets[k] = t.to(device) if device is not None else t
        out.append((imgs, targets, i))
    return out


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def walled(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    raw_cpu, raw_gpu = samples(), samples(dev)
    res = {"shape": f"{PAIRS} pairs {H}x{W} -> {OH}x{OW}, {G} masks per view", "device": torch.cuda.get_device_name(0)}

    # the pieces, on one view's worth of state each
    arrays = [s[0][k] for k in ("left", "right") for s in raw_cpu]
    pinned = torch.empty(sum(a.size for a in arrays), dtype=torch.uint8, pin_memory=True)
    np.concatenate([a.reshape(-1) for a in arrays], out=pinned.numpy())
    res["upload_bytes"] = pinned.numel()
    res["byte_upload_us"] = timed(lambda: pinned.to(dev, non_blocking=True), args.iters, args.warmup)
    bytes_dev = pinned.to(dev)
    lut, chan = D.make_lut(CFG.INPUT.PIXEL_MEAN, CFG.INPUT.PIXEL_STD, True)
    lut_dev = lut.to(dev)
    tables = D.build_tables([(H, W)] * PAIRS, [(OH, OW)] * PAIRS, [False, True])
    ints_dev = torch.from_numpy(tables.ints).to(dev)
    per_view = PAIRS * H * W * 3
    outs = [torch.empty((PAIRS, 3, OH, OW), dtype=torch.float32, device=dev) for _ in range(2)]

    def image_kernel():
        for v in range(2):
            D.launch_input_batch(bytes_dev[v * per_view:(v + 1) * per_view], ints_dev, tables, lut_dev, chan, outs[v])
    res["image_kernel_us"] = timed(image_kernel, args.iters, args.warmup)
    written = 2 * outs[0].numel() * 4
    res["image_written_bytes"] = written
    res["image_written_TBps"] = written / (res["image_kernel_us"] * 1e-6) / 1e12
    res["image_fraction_of_float4_copy_rate"] = written / (res["image_kernel_us"] * 1e-6) / COPY_RATE

    masks = {k: [s[1][k].get_field("masks").masks for s in raw_gpu] for k in ("left", "right")}

    def mask_kernel():
        for k in ("left", "right"):
            resize_flip_batch(masks[k], [(OW, OH)] * PAIRS, [False, True])
    res["mask_kernel_us"] = timed(mask_kernel, args.iters, args.warmup)
    disp = [s[1]["left"].get_map("disparity") for s in raw_gpu]
    res["disparity_resize_us"] = timed(lambda: [d.resize((OW, OH)) for d in disp], args.iters, args.warmup)

    collate = DeviceBatchCollator(CFG, True, dev, rng=random.Random(0))
    res["collator_gpu_targets_us"] = timed(lambda: collate(raw_gpu), args.iters, args.warmup)
    res["collator_gpu_targets_wall_us"] = walled(lambda: collate(raw_gpu), args.iters, 1)
    res["collator_cpu_targets_wall_us"] = walled(lambda: collate(raw_cpu), args.iters, 1)

    # (b) the same gathers as torch ops on the GPU (images only)
    yt, xt = (torch.from_numpy(t.astype(np.int64)).to(dev) for t in D.axis_tables((H, W), (OH, OW)))
    xt_f = xt.flip(0)
    chan_dev = torch.tensor(chan, device=dev)

    def torch_gathers():
        for v in range(2):
            out = torch.zeros((PAIRS, 3, OH, OW), dtype=torch.float32, device=dev)
            for i in range(PAIRS):
                src = bytes_dev[(v * PAIRS + i) * H * W * 3:(v * PAIRS + i + 1) * H * W * 3].view(H, W, 3)
                g = src.index_select(0, yt).index_select(1, xt_f if i else xt).index_select(2, chan_dev).permute(2, 0, 1).long()
                out[i] = torch.gather(lut_dev, 1, g.reshape(3, -1)).view(3, OH, OW)
    res["torch_gpu_gathers_us"] = timed(torch_gathers, args.iters, args.warmup)

    # (a) the host path: per-sample transforms, to_image_list, the fp32 upload (targets stay on the host)
    tr, host_collate = build_transforms(CFG, True), DoubleViewBatchCollator(0)

    def host_path():
        images, _, _ = host_collate([tr(im, tg) + (i,) for im, tg, i in raw_cpu])
        return {k: images[k].to(dev) for k in images}

    def host_images_only():
        images, _, _ = host_collate([tr(im, {k: BoxList(torch.zeros(0, 4), (W, H)) for k in im}) + (i,) for im, _, i in raw_cpu])
        return {k: images[k].to(dev) for k in images}
    res["host_path_wall_us"] = walled(host_path, args.host_iters, 1)
    res["host_path_images_only_wall_us"] = walled(host_images_only, args.host_iters, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

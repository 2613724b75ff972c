#!/usr/bin/env python3
"""Time PointRCNN's RCNN stage (car config: 512 ROIs per forward, 512 points x 133 channels per ROI) on one GPU with HIP events.

    python tools/bench_rcnn.py [--iters 30] [--warmup 5] [--batches 16,1]

Per batch size B (M = 512 // B ROIs per cloud), on the proposals of a real RPN run on seeded clouds, moved to the camera frame by
PointRCNN.proposals_to_camera (so that padding ROIs become the cubes at the centroid they are in the product):
  * pooling: the fused kernel (roipool3d_canonical) against roipool3d_canonical_unfused, the composition of the operators that existed
    before it, alternating in one process after a warm-up of both; medians, min / max as the spread, and the fused kernel's bytes/s
    (outputs written + rows gathered, from the shapes) over its event time;
  * the RCNNNet forward split per stage (pool, xyz_up + merge_down, SA 0 / 1 / 2, heads, decode + NMS + lists), and SA levels 0 and 1
    as TFLOP/s of their shared-MLP multiply-adds (x2) over the event-timed stage (index ops included, so a lower bound of the
    kernel's rate);
  * RCNNNet.refine against the BoxList path (forward, then the arg-max of every list on the host, as combine_2d_3d takes it);
  * RPN -> proposals_to_camera -> refine -> fields on the host for B clouds: PointRCNN's eval forward from the instance clouds on
    (InstancePointCloud needs 2D results and is not part of this figure), and its first two parts on their own.
Microseconds, one JSON line.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_rpn as BR  # noqa: E402
from disprcnn_amd.layers import pn2_mlp  # noqa: E402
from disprcnn_amd.layers import roipool3d as RP  # noqa: E402
from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.net.point_rcnn import PointRCNN  # noqa: E402

PEAK_TFLOPS = 157.0
HBM_TBPS = 6.29          # measured float4-copy rate of the part


def car_cfg():
    with open(os.path.join(ROOT, "tests", "golden", "rcnn_cfg_car.json")) as f:
        return BR.make_cfg({"MODEL": {"POINTRCNN": json.load(f)}})


def build_model(dev):
    torch.manual_seed(0)
    m = PointRCNN(car_cfg())
    rpn = BR.build_model(m.cfg, dev)
    m.rpn.load_state_dict(rpn.state_dict())
    with torch.no_grad():
        m.rcnn_net.reg_layer[-1].conv.weight.normal_(0, 0.05)
        m.rcnn_net.cls_layer[-1].conv.weight.normal_(0, 0.2)
    return m.to(dev).eval()


def camera_proposals(m, B, dev):
    pts = BR.clouds(B, dev)
    with torch.no_grad():
        out, _ = m.rpn(pts)
    mean = torch.tensor([1.5, 1.0, 20.0], device=dev).repeat(B, 1)
    rot = torch.full((B,), 0.1, dtype=torch.float64, device=dev)
    return pts, mean, rot, m.proposals_to_camera(out, mean, rot)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}


def time_alternating(fa, fb, iters, warmup):
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(iters):
        ta += timed(fa, 1, 0)
        tb += timed(fb, 1, 0)
    return stats(ta), stats(tb)


def pool_args(net, p):
    rc = net.cfg.RCNN
    return (p["rpn_xyz"].contiguous(), p["backbone_features"], p["seg_mask"], p["pts_depth"], p["roi_boxes3d"], rc.POOL_EXTRA_WIDTH, rc.NUM_POINTS)


def split_forward(net, p, st):
    """RCNNNet.forward restated with stage marks"""
    with st("pool"):
        xyz, pts, feat = net.pool(p)
    with st("xyz_up+merge_down"):
        x = pts
        for layer in net.xyz_up_layer:
            x = pn2_mlp.pointwise_mlp(x, None, layer.folded(), None, layer.relu)
        merge = net.merge_down_layer[0]
        f = pn2_mlp.pointwise_mlp(x, feat, merge.folded(), None, merge.relu)
    for k, module in enumerate(net.SA_modules):
        with st(f"sa{k}"):
            xyz, f = module(xyz, f)
    with st("heads"):
        cols = f[:, :, 0].t().unsqueeze(0).contiguous()
        out = {"rcnn_cls": net._head(net.cls_layer, cols)[0].t().contiguous(), "rcnn_reg": net._head(net.reg_layer, cols)[0].t().contiguous()}
    with st("decode+nms+lists"):
        lists = net.inference(out, p)
    return lists


def sa_flops(net, R, k):
    sa = net.cfg.RCNN.SA_CONFIG
    widths = [(128 if k == 0 else sa.MLPS[k - 1][-1]) + 3] + list(sa.MLPS[k])
    cols = R * sa.NPOINTS[k] * sa.NSAMPLE[k]
    return 2 * cols * sum(a * b for a, b in zip(widths[:-1], widths[1:]))


def lists_argmax(lists):
    return [(bl.get_field("box3d").bbox_3d[bl.get_field("box3d_score").argmax()].cpu(), bl.get_field("box3d_score").max().cpu()) for bl in lists]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="16,1")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = build_model(dev)
    net = m.rcnn_net
    res = {"iters": a.iters, "unit": "us"}
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            pts, mean, rot, p = camera_proposals(m, B, dev)
            M = p["roi_boxes3d"].shape[1]
            R, S, N, C = B * M, net.cfg.RCNN.NUM_POINTS, pts.shape[1], p["backbone_features"].shape[1]
            args = pool_args(net, p)
            fused, unfused = time_alternating(lambda: RP.roipool3d_canonical(*args), lambda: RP.roipool3d_canonical_unfused(*args), a.iters, a.warmup)
            empty = RP.roipool3d_canonical(*args)[3]
            nbytes = 4 * (R * S * (3 + 5 + C) + R * S * (3 + 2 + C))           # written + gathered
            r = {"rois": R, "empty_rois": int(empty.sum()), "padding_rois": int((p["roi_scores_raw"] == 0).sum()),
                 "pool_fused": fused, "pool_unfused": unfused, "pool_speedup": round(unfused["median"] / fused["median"], 2),
                 "pool_fused_TBps": round(nbytes / fused["median"] / 1e6, 3), "pool_fraction_of_hbm_copy": round(nbytes / fused["median"] / 1e6 / HBM_TBPS, 3)}
            stages = {}
            for it in range(a.warmup + a.iters):
                st = BR.Stages(it >= a.warmup)
                split_forward(net, p, st)
                torch.cuda.synchronize()
                for k, v in st.totals().items():
                    stages.setdefault(k, []).append(v)
            r["stages"] = {k: stats(v)["median"] for k, v in stages.items()}
            for k in (0, 1):
                r[f"sa{k}_tflops"] = round(sa_flops(net, R, k) / r["stages"][f"sa{k}"] / 1e6, 1)
                r[f"sa{k}_fraction_of_mfma_peak"] = round(r[f"sa{k}_tflops"] / PEAK_TFLOPS, 3)
            boxlist, refine = time_alternating(lambda: lists_argmax(net(p)[0]), lambda: [t.cpu() for t in net.refine(p)], a.iters, a.warmup)
            r["rcnn_boxlist_path"], r["rcnn_refine_path"] = boxlist, refine

            def whole():
                out, _ = m.rpn(pts)
                return [t.cpu() for t in net.refine(m.proposals_to_camera(out, mean, rot))]
            r["rpn_to_fields"] = stats(timed(whole, a.iters, a.warmup))
            r["rpn"] = stats(timed(lambda: m.rpn(pts), a.iters, a.warmup))
            out = m.rpn(pts)[0]
            r["proposals_to_camera"] = stats(timed(lambda: m.proposals_to_camera(out, mean, rot), a.iters, a.warmup))
            res[f"B{B}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()

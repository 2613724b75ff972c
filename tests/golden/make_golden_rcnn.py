#!/usr/bin/env python3
"""Golden fixture for PointRCNN's RCNN stage, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rcnn.py    -> rcnn_ref_golden.npz, rcnn_cfg_car.json

Reference code exercised (its own Python on torch-CPU): RCNNNet (net/rcnn_net.py) with its SA modules and pytorch_utils, roipool3d_utils,
kitti_utils (enlarge_box3d, rotate_pc_along_y_torch, boxes3d_to_bev_torch), Box3DPointRCNNPostProcess (net/rcnn_inference.py),
decode_bbox_target, iou3d_utils.nms_gpu, Box3DList, utils_3d.rotate_pc_along_y, under the reference's config defaults with
configs/kitti/car/vob/rcnn.yaml's POINTRCNN overrides.  The harness stand-ins are make_golden_rpn.py's (imported from it), plus
`roipool3d_cuda.forward` served by tests/box3d_oracle.py (selection in fp32, the gather dtype-preserving).

Inputs and weights are not stored: tests/rcnn_oracle.py builds them from seeds (make_inputs, random_state).  Three kinds of run:
  * the reference's ROI_SAMPLE_JIT forward on the seeded RPN-like dict: pins the pooling (selected indices, empty flags, the canonical
    coordinates) -- its pooled tensor must equal the oracle's gathers bit for bit;
  * the network on the oracle's fp32 pooled tensor given as proposals['pts_input'] (ROI_SAMPLE_JIT False), from the fp32 module and from
    module.double(): both see the same coordinates, hence the same FPS / ball-query indices, and their difference is the reference's
    own fp32 rounding error, stored per tensor as err32_max_* / err32_mean_* -- the yardstick of the tests' tolerances;
  * the post-process on (post_cls(rcnn_cls), rcnn_reg) of the fp32 run: lists, fallback flags, decoded boxes; the decode again in fp64
    with the fp32 run's bins.
fp64 level outputs are stored on recorded subsets (ROIs `lev_rois`, points `pts_*`) of the B = 2 batch to stay under the size limit,
with the reference's fp32 error on exactly those entries (err32_*_lev_*): a subset's mean is not the whole tensor's.

Checked before writing, else the seeds move on: no arg-max competitor within 1e-4, no sigmoid score within 1e-4 of SCORE_THRESH, no IoU
the NMS walk compares within 1e-4 of NMS_THRESH, no point within 1e-4 of a face of its enlarged box; and the cases the fixtures must
contain (an empty ROI, a padding ROI, fewer and more than S points, a fallback cloud that lands on the padding slot, a cloud where the
NMS drops a box).
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_rpn as MR  # noqa: E402  (installs the stand-ins and imports the reference's cfg)
from tests import box3d_oracle as BO  # noqa: E402
from tests import rcnn_oracle as CO  # noqa: E402
from tests import rpn_oracle as RO  # noqa: E402

rp = types.ModuleType("roipool3d_cuda")


def _roipool_forward(pts, boxes3d, feat, pooled, empty):
    S = pooled.shape[2]
    for b in range(pts.shape[0]):
        idx, e = BO.pooled_idx(BO.pts_in_boxes3d(MR._np32(pts[b]), MR._np32(boxes3d[b])), S)
        rows = torch.cat([pts[b], feat[b]], dim=1)
        for m in range(boxes3d.shape[1]):
            if not e[m]:
                pooled[b, m] = rows[torch.from_numpy(idx[m])]
        empty[b] = torch.from_numpy(e)


rp.forward = _roipool_forward
sys.modules["roipool3d_cuda"] = rp

from disprcnn.modeling.pointnet_module.point_rcnn.lib.net.rcnn_net import RCNNNet  # noqa: E402  (the reference)
from disprcnn.modeling.pointnet_module.point_rcnn.lib.utils.bbox_transform import decode_bbox_target  # noqa: E402
from disprcnn.structures.bounding_box_3d import Box3DList  # noqa: E402
from disprcnn.modeling.pointnet_module.point_rcnn.lib.utils.roipool3d import roipool3d_utils  # noqa: E402
from disprcnn.utils.utils_3d import rotate_pc_along_y  # noqa: E402

roipool3d_utils.roipool3d_cuda = rp         # make_golden_rpn's import of the reference bound its placeholder there

CAR = {"MASK_THRESH": 0.5, "AUG_DATA": True, "MEAN_SIZE": [[1.52563191462, 1.62856739989, 3.88311640418]],
       "RPN": {"FIXED": True, "LOSS_CLS": "BinaryCrossEntropy"},
       "RCNN": {"ENABLED": True, "CLS_FG_THRESH": 0.60, "REG_FG_THRESH": 0.55, "LOSS_CLS": "BinaryCrossEntropy", "ROI_PER_IMAGE": 16},
       "TRAIN": {"RPN_PRE_NMS_TOP_N": 9000, "RPN_POST_NMS_TOP_N": 512},
       "TEST": {"RPN_PRE_NMS_TOP_N": 9000, "RPN_POST_NMS_TOP_N": 100}}                     # configs/kitti/car/vob/rcnn.yaml
N_LEV_ROIS, N_LEV_PTS = 6, 4
T = torch.from_numpy


def run_net(model, pts_input, rois, dtype):
    """The reference on proposals['pts_input'] -> levels (hooks), rcnn_cls, rcnn_reg"""
    MR.DTYPE[0] = dtype
    lv, hooks = {}, []
    hooks.append(model.xyz_up_layer.register_forward_hook(lambda m, i, o: lv.__setitem__("xyz_up", o.detach().squeeze(3).clone())))
    hooks.append(model.merge_down_layer.register_forward_hook(lambda m, i, o: lv.__setitem__("merge_down", o.detach().squeeze(3).clone())))
    for k, m in enumerate(model.SA_modules):
        hooks.append(m.register_forward_hook(lambda mod, i, o, k=k: lv.__setitem__(f"sa{k}", o[1].detach().clone())))
    hooks.append(model.cls_layer.register_forward_hook(lambda m, i, o: lv.__setitem__("rcnn_cls", o.detach()[:, :, 0].clone())))
    hooks.append(model.reg_layer.register_forward_hook(lambda m, i, o: lv.__setitem__("rcnn_reg", o.detach()[:, :, 0].clone())))
    model.cfg.RCNN.ROI_SAMPLE_JIT = False
    with torch.no_grad():
        model({"pts_input": T(pts_input).to(dtype), "roi_boxes3d": T(rois).to(dtype), "roi_scores_raw": torch.zeros(rois.shape[:2])})
    model.cfg.RCNN.ROI_SAMPLE_JIT = True
    for h in hooks:
        h.remove()
    return lv


def run_jit(model, inp):
    """The reference's ROI_SAMPLE_JIT forward (fp32) -> its pooled, canonical pts_input (R,S,3+E+C)"""
    MR.DTYPE[0] = torch.float32
    cap = []
    orig = model._break_up_pc
    model._break_up_pc = lambda pc: (cap.append(pc.detach().clone()), orig(pc))[1]
    prop = {"rpn_xyz": T(inp["rpn_xyz"]), "rpn_features": T(inp["backbone_features"]).permute(0, 2, 1), "seg_mask": T(inp["seg_mask"]),
            "pts_depth": T(inp["pts_depth"]), "roi_boxes3d": T(inp["roi_boxes3d"]).clone(), "roi_scores_raw": T(inp["roi_scores_raw"])}
    with torch.no_grad():
        model(prop)
    del model._break_up_pc
    return cap[0].numpy()


def lists_of(result):
    out = []
    for bl in result:
        b3 = bl.get_field("box3d")
        assert b3.mode == "ry_lhwxyz"
        lab = bl.get_field("labels")
        out.append(dict(n=len(b3), len2d=len(bl), boxes=b3.bbox_3d.numpy().astype(np.float32), scores=bl.get_field("box3d_score").numpy().astype(np.float32),
                        labels=np.atleast_1d(np.asarray(lab if isinstance(lab, int) else lab.numpy())).astype(np.int64),
                        random=bl.get_field("random").numpy().astype(np.int64), has_iou="iou_score" in bl.extra_fields))
    return out


def box_group(out):
    """Box3DList conversions and the rotate-back of proposals (point_rcnn.py:303-312) on seeded boxes.  The *32 arrays are the reference's (its
    Box3DList keeps fp32 whatever it is given); the *64 arrays are tests/rcnn_oracle.py's fp64 evaluation of the same boxes, stored
    for scale and never used as a reference for the oracle itself."""
    rs = np.random.RandomState(77)
    n, B, M = 12, 3, 4
    b7 = np.concatenate([rs.normal(0, 3, (n, 3)), rs.uniform(1.0, 4.0, (n, 3)), rs.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)
    b7[-1] = 0
    mean = rs.normal(0, 5, (B, 3)).astype(np.float32)
    mean[:, 2] += 20
    rot = rs.uniform(-0.6, 0.6, B)
    bl = Box3DList(T(b7), (1, 1), "xyzhwl_ry")
    corners = bl.convert("corners")
    out.update(box_b7=b7, box_mean=mean, box_rot=rot, box_corners32=corners.bbox_3d.numpy(), box_back32=corners.convert("xyzhwl_ry").bbox_3d.numpy(),
               box_rylhw32=bl.convert("ry_lhwxyz").bbox_3d.numpy(), box_corners64=CO.box_corners(b7), box_rylhw64=CO.to_ry_lhwxyz(b7))
    rotator = rotate_pc_along_y(None, None, rot_angle=T(rot))
    c = Box3DList(T(b7).view(-1, 7), (1, 1), "xyzhwl_ry").convert("corners").bbox_3d.view(B, -1, 24)
    cam = Box3DList((rotator.rotate_back((c.view(B, -1, 3) + T(mean)[:, None, :]).permute(0, 2, 1)).permute(0, 2, 1)).contiguous(), (1, 1),
                    "corners").convert("xyzhwl_ry").bbox_3d.view(B, -1, 7)
    out.update(box_cam32=cam.numpy(), box_cam64=CO.rois_to_camera(b7.reshape(B, M, 7), mean, rot))


def main():
    pr = MR.ref_cfg.MODEL.POINTRCNN.clone()
    MR.merge(pr, CAR)
    sub = {"RPN": MR.plain(pr.RPN), "RCNN": MR.plain(pr.RCNN), "MEAN_SIZE": MR.plain(pr.MEAN_SIZE), "TRAIN": MR.plain(pr.TRAIN),
           "TEST": MR.plain(pr.TEST), "MASK_THRESH": pr.MASK_THRESH}
    cfg = RO.make_cfg(sub)
    rc = cfg.RCNN
    S = rc.NUM_POINTS
    model = RCNNNet(pr, MR.ref_cfg).eval()
    keys = list(model.state_dict().keys())
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}

    for wseed in range(1, 40):
        sd = CO.random_state(shapes, wseed)
        out = {"state_dict_keys": np.array(keys), "state_dict_shapes": np.array([json.dumps(shapes[k]) for k in keys]),
               "weight_seed": np.int64(wseed), "input_bump": np.int64(wseed - 1)}
        errs, ok = {}, True
        seen = dict(empty=False, padding=False, fewer=False, more=False, fallback_on_padding=False, nms_drop=False)
        for tag in CO.BATCHES:
            inp = CO.make_inputs(tag, wseed - 1)
            rois, B, M = inp["roi_boxes3d"], inp["roi_boxes3d"].shape[0], inp["roi_boxes3d"].shape[1]
            model.float().load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
            # 1. pooling: the reference's own JIT forward against the oracle's gathers
            p32 = CO.pool_canonical(inp, rc.POOL_EXTRA_WIDTH, S, rc.USE_DEPTH, np.float32)
            p64 = CO.pool_canonical(inp, rc.POOL_EXTRA_WIDTH, S, rc.USE_DEPTH, np.float64)
            ref_in = run_jit(model, inp)
            mine = CO.pts_input_of(p32)
            assert ref_in.shape == mine.shape == (B * M, S, 3 + 2 + CO.N_FEAT)
            assert np.array_equal(ref_in[..., 3:], mine[..., 3:]), "pooled mask / depth / features differ from the oracle's gathers"
            assert np.array_equal(ref_in[..., 1], mine[..., 1]), "canonical y differs"
            scale = np.abs(p64["xyz"][..., 0]) + np.abs(p64["xyz"][..., 2])         # |rotated| <= |dx| + |dz|, same order of magnitude
            dxz = np.abs(ref_in[..., [0, 2]].astype(np.float64) - p64["xyz"][..., [0, 2]])
            e_ref = float((dxz.max(2) / (np.finfo(np.float32).eps * np.maximum(scale, 1e-30))).max())
            seen["empty"] |= bool(p32["empty"].reshape(B, M)[:, 1].all())
            seen["padding"] |= bool((rois[:, M - 1] == 0).all())
            seen["fewer"] |= bool(((p32["count"] > 0) & (p32["count"] < S)).any())
            seen["more"] |= bool((p32["count"] > S).any())
            # 2. the network on the oracle's fp32 pooled tensor
            l32 = run_net(model, mine, rois, torch.float32)
            model.double()
            l64 = run_net(model, mine, rois, torch.float64)
            assert all(v.dtype == torch.float64 for v in l64.values()) and all(v.dtype == torch.float32 for v in l32.values())
            for name in l32:
                d = (l32[name].double() - l64[name]).abs()
                errs.setdefault(name, []).append((d.max().item(), d.mean().item(), l64[name].abs().max().item()))
            cls32, reg32 = l32["rcnn_cls"].numpy(), l32["rcnn_reg"].numpy()
            # 3. post-process and decode
            model.float()
            MR.DTYPE[0] = torch.float32
            pcls = CO.post_cls(tag, cls32)
            prop = {"roi_boxes3d": T(rois), "roi_scores_raw": T(inp["roi_scores_raw"])}
            ref_lists = lists_of(model.inference({"rcnn_cls": T(pcls), "rcnn_reg": T(reg32)}, prop))
            mine_lists, m_score, m_nms = CO.postprocess(rc, cfg.MEAN_SIZE[0], rois, inp["roi_scores_raw"], pcls, reg32)
            dec32 = decode_bbox_target(T(rois).view(-1, 7), T(reg32), anchor_size=model.inference.MEAN_SIZE, loc_scope=rc.LOC_SCOPE,
                                       loc_bin_size=rc.LOC_BIN_SIZE, num_head_bin=rc.NUM_HEAD_BIN, get_xz_fine=True,
                                       get_y_by_bin=rc.LOC_Y_BY_BIN, loc_y_scope=rc.LOC_Y_SCOPE, loc_y_bin_size=rc.LOC_Y_BIN_SIZE,
                                       get_ry_fine=True).numpy()
            bins = CO.decode_bins(reg32, rc)
            dec64 = CO.decode(rois.reshape(-1, 7), reg32, rc, cfg.MEAN_SIZE[0], np.float64, bins)
            d = np.abs(dec32.astype(np.float64) - dec64)
            errs.setdefault("dec_boxes", []).append((d.max(), d.mean(), np.abs(dec64).max()))
            am = CO.argmax_margin(reg32, rc)
            print(f"seed {wseed} {tag}: face margin {p32['margin']:.3g}, argmax {am:.3g}, score {m_score:.3g}, NMS {m_nms:.3g}; pooled xz err "
                  f"{e_ref:.2f} eps; counts {sorted(p32['count'].tolist())[:4]}..{p32['count'].max()}; cls [{cls32.min():.2f}, {cls32.max():.2f}]; "
                  f"lists {[(d['n'], int(d['random'][0])) for d in ref_lists]}")
            if min(p32["margin"], am, m_score, m_nms) < 1e-4:
                ok = False
                break
            assert e_ref <= 6.0, "the reference's canonical x / z lie outside the bound the tests use"
            for b, (a, m) in enumerate(zip(ref_lists, mine_lists)):          # the oracle's post-process against the reference's
                assert a["n"] == len(m["keep"]) and bool(a["random"][0]) == m["fallback"], (b, a["n"], m)
                assert np.allclose(a["boxes"], CO.to_ry_lhwxyz(m["boxes"]), rtol=0, atol=2e-5) and np.array_equal(a["scores"], m["scores"])
                n_sel = int((CO.sigmoid(pcls.reshape(B, M)[b]) > np.float32(rc.SCORE_THRESH)).sum())
                seen["nms_drop"] |= (not m["fallback"]) and a["n"] < n_sel
                seen["fallback_on_padding"] |= m["fallback"] and int(m["keep"][0]) == M - 1
            rs = np.random.RandomState(7)
            out.update({
                f"{tag}_sel_idx": p32["idx"].astype(np.int16), f"{tag}_empty": p32["empty"], f"{tag}_count": p32["count"].astype(np.int32),
                f"{tag}_canon_err_eps": np.float64(e_ref),
                f"{tag}_rcnn_cls": cls32, f"{tag}_rcnn_reg": reg32, f"{tag}_rcnn_cls64": l64["rcnn_cls"].numpy(), f"{tag}_rcnn_reg64": l64["rcnn_reg"].numpy(),
                f"{tag}_post_cls": pcls, f"{tag}_dec_bins": bins.astype(np.int8), f"{tag}_dec_boxes": dec32, f"{tag}_dec_boxes64": dec64,
                f"{tag}_keep": np.concatenate([m["keep"] for m in mine_lists]).astype(np.int32),
                f"{tag}_list_n": np.array([a["n"] for a in ref_lists], np.int32), f"{tag}_list_len2d": np.array([a["len2d"] for a in ref_lists], np.int32),
                f"{tag}_list_boxes": np.concatenate([a["boxes"] for a in ref_lists]), f"{tag}_list_scores": np.concatenate([a["scores"] for a in ref_lists]),
                f"{tag}_list_labels": np.concatenate([a["labels"] for a in ref_lists]),
                f"{tag}_list_random": np.array([a["random"][0] for a in ref_lists], np.int32),
                f"{tag}_list_random_len": np.array([len(a["random"]) for a in ref_lists], np.int32),
                f"{tag}_list_has_iou": np.array([a["has_iou"] for a in ref_lists]),
            })
            if tag == "b2":
                lev_rois = np.sort(np.concatenate([[1, 2, M - 1], rs.choice(np.arange(M, 2 * M), N_LEV_ROIS - 3, replace=False)]))
                out["b2_lev_rois"] = lev_rois.astype(np.int32)
                for k in ("xyz_up", "merge_down", "sa0", "sa1", "sa2"):
                    n = l64[k].shape[2]
                    sel = np.sort(rs.choice(n, min(N_LEV_PTS, n), replace=False))
                    out[f"b2_pts_{k}"] = sel.astype(np.int32)
                    out[f"b2_{k}64"] = l64[k].numpy()[lev_rois][:, :, sel]
                    d = np.abs(l32[k].numpy()[lev_rois][:, :, sel].astype(np.float64) - out[f"b2_{k}64"])      # the yardstick of this subset
                    out[f"err32_max_lev_{k}"], out[f"err32_mean_lev_{k}"] = np.float64(d.max()), np.float64(d.mean())
        if ok:
            break
    else:
        raise SystemExit("no seed met the margins")
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"the fixtures lack the cases {missing}"
    for name, e in errs.items():
        out[f"err32_max_{name}"] = np.float64(max(x[0] for x in e))
        out[f"err32_mean_{name}"] = np.float64(np.mean([x[1] for x in e]))
        out[f"absmax_{name}"] = np.float64(max(x[2] for x in e))
        print(f"{name}: err32 max {out[f'err32_max_{name}']:.3g} mean {out[f'err32_mean_{name}']:.3g} |v| <= {out[f'absmax_{name}']:.3g}")
    box_group(out)
    with open(os.path.join(HERE, "rcnn_cfg_car.json"), "w") as f:
        json.dump(sub, f, indent=1, sort_keys=True)
        f.write("\n")
    path = os.path.join(HERE, "rcnn_ref_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()

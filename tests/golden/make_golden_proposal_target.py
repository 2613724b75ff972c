#!/usr/bin/env python3
"""Golden fixture for PointRCNN's ProposalTargetLayer, recorded from the IMPORTED REFERENCE (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_proposal_target.py    -> proposal_target_golden.npz

Reference code exercised (its own Python on torch-CPU): ProposalTargetLayer (rpn/proposal_target_layer.py: forward, sample_rois_for_rcnn,
sample_bg_inds, aug_roi_by_noise_torch, random_aug_box3d, data_augmentation), iou3d_utils.boxes_iou3d_gpu, roipool3d_utils.roipool3d_gpu,
kitti_utils (boxes3d_to_bev_torch, enlarge_box3d, rotate_pc_along_y_torch), under the reference's config defaults with
configs/kitti/car/vob/rcnn.yaml's POINTRCNN overrides and each case's settings (tests/proposal_target_oracle.py: CASES).  The harness
stand-ins are make_golden_rcnn.py's (imported from it), plus `iou3d_cuda.boxes_overlap_bev_gpu` served by tests/box3d_oracle.py (fp32 run:
its restatement of the kernel; fp64 run: its fp64 polygon clip).

The reference's random calls inside its module are replaced by stand-ins that serve recorded draws in the layout
key[M] | pick[P] | noise[P][T][9] | aug[P][3] per cloud: the module's names `torch` and `np` are bound to shims that forward everything
else.  randperm(n) is the argsort of the foreground candidates' keys; randint and the fg-only rand come from `pick` in slot order;
np.random.rand() is the keep draw of the next iteration; random_aug_box3d's randint / rand(3) / rand(3) / rand(1) are that iteration's
draws [1], [2:5], [5:8], [8]; data_augmentation's three rand((B, P)) are the aug block's columns.  aug_roi_by_noise_torch is called one
ROI at a time (the reference's own loop body, on a one-row view) so that the shims know the slot.  The reference's own control flow then
produces the outputs.  What it never names is recorded from that control flow: a slot's source candidate (the row handed to the noise
loop, matched among the candidates), its iteration count (the keep draws it asked for), the class counts (its three nonzero calls) and
the foreground slot count (what randperm / the fg-only rand were asked for).

Every case is recorded twice, fp32 and fp64, from the same fp32 inputs and draws; their difference is the reference's own fp32 error,
stored per case and tensor as err32_max_* / err32_mean_*.  The cloud without a foreground and without a background candidate makes the
reference raise (asserted): the recording holds the other clouds, and that cloud's expected values are the oracle's.

Inputs and draws are not stored: tests/proposal_target_oracle.py builds them from seeds (make_inputs, make_draws).  Checked before
writing, else the seeds move on (`bump`): no compared IoU within 1e-4 of its threshold, no point within 1e-4 of a face of its enlarged
box, no angle within 1e-4 of a value where its sign or modulo flips, distinct keys, no keep draw within 1e-6 of 0.2, no flip draw within
1e-6 of 0.5, identical branches in the fp32 and fp64 runs; and the cases the fixture must contain.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_rcnn as MG  # noqa: E402  (installs the stand-ins and imports the reference)
from tests import box3d_oracle as BO  # noqa: E402
from tests import proposal_target_oracle as PO  # noqa: E402

MR = MG.MR
T = torch.from_numpy


def _overlap_bev(a, b, out):
    if MR.DTYPE[0] == torch.float32:
        out.copy_(T(BO.box_overlap(MR._np32(a), MR._np32(b))))
    else:
        an, bn = a.detach().numpy().astype(np.float64), b.detach().numpy().astype(np.float64)
        out.copy_(T(np.array([[BO.clip_overlap64(x, y) for y in bn] for x in an])))


MR.iou3d.boxes_overlap_bev_gpu = _overlap_bev

from disprcnn.modeling.pointnet_module.point_rcnn.lib.rpn import proposal_target_layer as PTL  # noqa: E402  (the reference)


class State:
    pass


ST = State()


def start(case, draws, nb):
    k = PO.CASES[case]
    ST.M, ST.P, ST.T = k["M"], k["P"], k["T"]
    ST.draws = [PO.split_draws(draws[b], ST.M, ST.P, ST.T) for b in range(nb)]
    ST.aug = np.stack([d[3] for d in ST.draws])            # (nb, P, 3)
    ST.cloud, ST.aug_calls = -1, 0
    ST.src = np.full((nb, ST.P), -1, np.int32)
    ST.n_iter = np.zeros((nb, ST.P), np.int32)
    ST.counts = np.zeros((nb, 4), np.int32)


def _dt(a):
    return T(np.ascontiguousarray(a, np.float32)).to(MR.DTYPE[0])


class TorchShim:
    def __getattr__(self, k):
        return getattr(torch, k)

    def max(self, *a, **k):                                # the module calls it once per cloud, on the cloud's IoU matrix
        ST.cloud += 1
        ST.phase, ST.cursor, ST.base, ST.nz = "sample", 0, 0, []
        return torch.max(*a, **k)

    def nonzero(self, x):                                  # fg, easy bg, hard bg, in the module's order
        r = torch.nonzero(x)
        ST.nz.append(r.view(-1).numpy().copy())
        if len(ST.nz) == 3:
            ST.counts[ST.cloud, :3] = [ST.nz[0].size, ST.nz[2].size, ST.nz[1].size]
        return r

    def randperm(self, n):
        fg = ST.nz[0]
        assert ST.phase == "sample" and fg.size == n
        ST.cursor = ST.counts[ST.cloud, 3] = min(ST.fg_per_image, n)
        return T(np.argsort(ST.draws[ST.cloud][0][fg], kind="stable"))

    def randint(self, low, high, size):
        assert low == 0
        if ST.phase == "sample":
            u = ST.draws[ST.cloud][1][ST.cursor:ST.cursor + size[0]]
            assert u.size == size[0]
            ST.cursor += size[0]
            return T(np.array([PO.pick_index(v, high) for v in u], np.int64))
        assert ST.phase == "noise" and high == 5 and tuple(size) == (1,)
        return torch.tensor([PO.pick_index(ST.draws[ST.cloud][2][ST.slot, ST.t, 1], 5)])

    def rand(self, *size, device=None):
        if isinstance(size[0], tuple):                     # data_augmentation: rotation, scale, flip
            col = ST.aug_calls
            ST.aug_calls += 1
            assert size[0] == ST.aug.shape[:2] and col < 3
            return _dt(ST.aug[:, :, col])
        if ST.phase == "sample":                           # the fg-only cloud: floor(rand * fg_num) is the module's own, in fp32
            assert size == (ST.P,) and ST.cursor == 0
            ST.cursor = ST.counts[ST.cloud, 3] = ST.P
            return T(np.ascontiguousarray(ST.draws[ST.cloud][1], np.float32))
        row = ST.draws[ST.cloud][2][ST.slot, ST.t]
        if size == (3,):
            ST.r3 += 1
            assert ST.r3 <= 2
            return _dt(row[2:5] if ST.r3 == 1 else row[5:8])
        assert size == (1,)
        return _dt(row[8:9])


class NpRandom:
    @staticmethod
    def rand():
        ST.t += 1
        ST.r3 = 0
        ST.n_iter[ST.cloud, ST.slot] += 1
        return float(ST.draws[ST.cloud][2][ST.slot, ST.t, 0])


class NpShim:
    random = NpRandom()

    def __getattr__(self, k):
        return getattr(np, k)


PTL.torch, PTL.np = TorchShim(), NpShim()


class Recorded(PTL.ProposalTargetLayer):
    def sample_rois_for_rcnn(self, roi_boxes3d, gt_boxes3d):
        ST.cand = roi_boxes3d
        out = super().sample_rois_for_rcnn(roi_boxes3d, gt_boxes3d)
        ST.noise_rois, ST.gt_raw = out[0].clone(), out[1].clone()
        return out

    def aug_roi_by_noise_torch(self, roi_boxes3d, gt_boxes3d, iou3d_src, aug_times=10):
        ST.phase = "noise"
        ious = []
        for k in range(roi_boxes3d.shape[0]):              # the reference's loop body, one ROI at a time
            ST.slot, ST.t = ST.base + k, -1
            hit = torch.nonzero((ST.cand[ST.cloud] == roi_boxes3d[k]).all(1)).view(-1)
            assert hit.numel() == 1
            ST.src[ST.cloud, ST.slot] = int(hit[0])
            _, iou = super().aug_roi_by_noise_torch(roi_boxes3d[k:k + 1], gt_boxes3d[k:k + 1], iou3d_src[k:k + 1], aug_times=aug_times)
            ious.append(iou)
        ST.base += roi_boxes3d.shape[0]
        return roi_boxes3d, torch.cat(ious)


def ref_cfg_of(case):
    k = PO.CASES[case]
    pr = MR.ref_cfg.MODEL.POINTRCNN.clone()
    MR.merge(pr, MG.CAR)
    MR.merge(pr, {"AUG_DATA": k["aug"], "RCNN": {"ROI_PER_IMAGE": k["P"], "ROI_FG_AUG_TIMES": k["T"], "NUM_POINTS": k["S"], "USE_DEPTH": k["depth"],
                                                "REG_AUG_METHOD": k["method"]}})
    return pr


def run_ref(case, inp, draws, dtype, clouds):
    """The reference's forward on the clouds `clouds` -> its dict plus what the shims recorded, as arrays"""
    MR.DTYPE[0] = dtype
    sel = np.asarray(clouds)
    start(case, draws[sel], len(sel))
    layer = Recorded(ref_cfg_of(case), MR.ref_cfg)
    ST.fg_per_image = int(np.round(layer.cfg.RCNN.FG_RATIO * ST.P))
    d = {"roi_boxes3d": T(inp["roi_boxes3d"][sel]).to(dtype), "rpn_xyz": T(inp["rpn_xyz"][sel]).to(dtype),
         "rpn_features": T(inp["backbone_features"][sel]).permute(0, 2, 1).to(dtype), "seg_mask": T(inp["seg_mask"][sel]).to(dtype),
         "pts_depth": T(inp["pts_depth"][sel]).to(dtype)}
    with torch.no_grad():
        out = layer(d, T(inp["gt_boxes3d"][sel]).to(dtype))
    res = {k: v.numpy() for k, v in out.items()}
    assert all(v.dtype == (np.float32 if dtype == torch.float32 else np.float64) for k, v in res.items() if k not in ("cls_label", "reg_valid_mask"))
    assert res["cls_label"].dtype == res["reg_valid_mask"].dtype == np.int64
    res.update(noise_rois=ST.noise_rois.numpy(), gt_raw=ST.gt_raw.numpy(), src_index=ST.src.copy(), n_iter=ST.n_iter.copy(), counts=ST.counts.copy())
    return res


FLOATS = ("noise_rois", "gt_iou", "roi_boxes3d", "gt_of_rois", "sampled_pts")
INTS = ("src_index", "n_iter", "counts", "cls_label", "reg_valid_mask")


def record(bump):
    """-> (arrays, seen) or None when a margin is missed"""
    out, seen = {}, {k: False for k in (
        "fg+hard+easy", "fg only", "hard only", "easy only", "hard+easy", "fewer fg", "more fg", "no candidate", "ends at 1", "runs all T",
        "kept original", "empty", "fewer than S", "more than S", "cls -1 in between", "flip", "no flip")}
    clouds = [b for b in range(PO.B) if b != PO.NONE_CLOUD]
    for case, k in PO.CASES.items():
        cfg = PO.case_cfg(MG_CFG, case)
        st = PO.settings(cfg)
        inp, draws = PO.make_inputs(case, bump), PO.make_draws(case, bump)
        M, P, Tn, S = k["M"], k["P"], k["T"], k["S"]
        o = PO.blocks(M, P, Tn)
        s32, p32 = PO.layer(st, inp, draws, np.float32)
        s64, p64 = PO.layer(st, inp, draws, np.float64)
        keys = draws[:, :M]
        noise = draws[:, o["noise"]:o["aug"]].reshape(PO.B, P, Tn, 9)
        aug = draws[:, o["aug"]:].reshape(PO.B, P, 3)
        margins = dict(iou=min(s32["margin"], s64["margin"]), label=min(PO.label_margin(st, s32), PO.label_margin(st, s64)),
                       face=min(p32["margin"], p64["margin"]), ry=min(p32["ry_margin"], p64["ry_margin"]) if k["aug"] else np.inf)
        print(f"bump {bump} case {case}: margins {margins}")
        if min(margins.values()) < 1e-4:
            return None
        if any(np.unique(keys[b]).size != M for b in range(PO.B)) or (Tn and np.abs(noise[..., 0].astype(np.float64) - 0.2).min() < 1e-6) \
                or np.abs(aug[..., 2].astype(np.float64) - 0.5).min() < 1e-6:
            return None
        for name in ("src_index", "n_iter", "counts", "kept"):
            assert np.array_equal(s32[name], s64[name]), f"{case}: the oracle's fp32 and fp64 runs differ in {name}"
        try:                                               # the reference ends the run on the cloud without a candidate
            run_ref(case, inp, draws, torch.float32, [PO.NONE_CLOUD])
            raise AssertionError("the reference did not raise on the cloud without a candidate")
        except NotImplementedError:
            seen["no candidate"] |= bool(s32["counts"][PO.NONE_CLOUD, 4])
        r32 = run_ref(case, inp, draws, torch.float32, clouds)
        r64 = run_ref(case, inp, draws, torch.float64, clouds)
        for name in INTS:
            assert np.array_equal(r32[name], r64[name]), f"{case}: the fp32 and fp64 runs of the reference took different branches ({name})"
        # pooled mask / depth / features are gathers: the reference's must equal the oracle's bit for bit (they are not stored)
        nb = len(clouds)
        mine = PO.reference_dict({n: (v[:nb * P] if isinstance(v, np.ndarray) and v.shape[:1] == (PO.B * P,) else v) for n, v in p32.items()},
                                 {"roi_iou": s32["roi_iou"][:nb]})
        assert r32["pts_feature"].shape == mine["pts_feature"].shape == (nb * P, S, 1 + int(k["depth"]) + k["C"])
        assert np.array_equal(r32["pts_feature"], mine["pts_feature"]), f"{case}: pooled features differ from the oracle's gathers"
        for name in FLOATS:
            d = np.abs(r32[name].astype(np.float64) - r64[name])
            assert d.max() < 1e-3, f"{case}: {name} differs by {d.max()} between the fp32 and fp64 runs: a branch"
            out[f"{case}_{name}64"] = r64[name]
            out[f"err32_max_{case}_{name}"], out[f"err32_mean_{case}_{name}"] = np.float64(d.max()), np.float64(d.mean())
            print(f"  {name}: err32 max {d.max():.3g} mean {d.mean():.3g} |v| <= {np.abs(r64[name]).max():.3g}")
        out[f"{case}_noise_rois"] = r32["noise_rois"]
        out[f"{case}_gt_raw"] = r32["gt_raw"]
        out[f"{case}_gt_iou"] = r32["gt_iou"]
        for name in INTS:
            out[f"{case}_{name}"] = r32[name]
        out[f"{case}_sel_idx"] = p32["idx"][:nb * P].astype(np.int16)
        out[f"{case}_empty"] = p32["empty_flag"][:nb * P]
        out[f"{case}_count"] = p32["count"][:nb * P].astype(np.int32)
        c, it = r32["counts"], r32["n_iter"]
        fgpi = int(np.round(st["fg_ratio"] * P))
        fg_slot = np.arange(P)[None] < c[:, 3:4]
        seen["fg+hard+easy"] |= bool(((c[:, 0] > 0) & (c[:, 1] > 0) & (c[:, 2] > 0)).any())
        seen["fg only"] |= bool(((c[:, 0] > 0) & (c[:, 1] == 0) & (c[:, 2] == 0)).any())
        seen["hard only"] |= bool(((c[:, 0] == 0) & (c[:, 1] > 0) & (c[:, 2] == 0)).any())
        seen["easy only"] |= bool(((c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 2] > 0)).any())
        seen["hard+easy"] |= bool(((c[:, 0] == 0) & (c[:, 1] > 0) & (c[:, 2] > 0)).any())
        both = (c[:, 0] > 0) & (c[:, 1] + c[:, 2] > 0)
        seen["fewer fg"] |= bool((both & (c[:, 0] < fgpi)).any())
        seen["more fg"] |= bool((both & (c[:, 0] > fgpi)).any())
        if Tn >= 10:
            seen["ends at 1"] |= bool((fg_slot & (it == 1)).any())
            seen["runs all T"] |= bool((fg_slot & (it == Tn)).any())
            seen["kept original"] |= bool((fg_slot & (it > 1) & s32["kept"][:nb]).any())
        cnt, emp = out[f"{case}_count"], out[f"{case}_empty"]
        seen["empty"] |= bool(emp.any())
        seen["fewer than S"] |= bool(((cnt > 0) & (cnt < S)).any())
        seen["more than S"] |= bool((cnt > S).any())
        iou = r32["gt_iou"]
        seen["cls -1 in between"] |= bool(((iou > st["cls_bg"]) & (iou < st["cls_fg"]) & (emp == 0)).any())
        if k["aug"]:
            seen["flip"] |= bool((aug[:nb, :, 2] < 0.5).any())
            seen["no flip"] |= bool((aug[:nb, :, 2] > 0.5).any())
    return out, seen


def main():
    import json
    global MG_CFG
    with open(os.path.join(HERE, "rcnn_cfg_car.json")) as f:
        MG_CFG = json.load(f)
    ks = PO.CASES.values()
    assert {k["N"] for k in ks} >= {1, 3} and {k["method"] for k in ks} == {"multiple", "single"} and {k["aug"] for k in ks} == {True, False}
    assert any(k["T"] == 0 for k in ks)
    for bump in range(40):
        got = record(bump)
        if got is not None:
            break
    else:
        raise SystemExit("no seed met the margins")
    out, seen = got
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"the fixture lacks the cases {missing}"
    out["input_bump"] = np.int64(bump)
    out["clouds"] = np.array([b for b in range(PO.B) if b != PO.NONE_CLOUD], np.int32)
    path = os.path.join(HERE, "proposal_target_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()

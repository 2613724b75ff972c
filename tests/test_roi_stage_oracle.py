"""tests/roi_stage_oracle.py tied to the pinned oracles (oracle/roi_oracle.py bit-pinned to the reference's ROIAlign kernel,
oracle/train_caller_oracle.py, oracle/post_oracle.py), its launch mirrors held to the caps the GPU cases of tests/test_hip_roi_stage.py are
named for, the conditions those cases state about their own inputs, and -- for every case -- the proof that its input is strong enough:
each plausible kernel mistake that applies to the case moves the reference by >= 10x the case's bound (a mistake a geometry cannot show must
leave the reference exactly unchanged; the ones a case is built for are named in its table and must clear)."""
import numpy as np
import pytest
import torch

from oracle import post_oracle as PO
from oracle import roi_oracle as RO
from oracle import train_caller_oracle as TO
from tests import resample_oracle as R
from tests import roi_stage_oracle as S


def _strong(name, ref, bound, mutants, must=()):
    best = 0.0
    for mname, mut in mutants.items():
        m = R.margin(ref, mut, bound)
        print(f"[{name}] {mname}: {m:.3g}x the bound")
        assert m == 0.0 or m >= 10.0, f"{name}: input too weak for mistake {mname!r} ({m:.3g}x)"
        assert mname not in must or m >= 10.0, f"{name}: built for mistake {mname!r}, which it does not show"
        best = max(best, m)
    assert best >= 10.0, f"{name}: no mistake clears 10x the bound"


def _small_rois():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_golden.npz"), allow_pickle=False)
    return z["small_rois"]


def _fwd_cases():
    """(name, input, rois, scale, ph, pw, sr, channels per thread, must)"""
    out = []
    for C in sorted(set(S.FWD_CHANNELS + S.FWD_NORM_CHANNELS)):
        for ph, pw, sr, scale in S.FWD_SETTINGS:
            must = ("swap23", "round_roi") + (("cg_off",) if C // S.fwd_cc(C) > 1 else ())
            out.append((f"C={C} {ph}x{pw} sr={sr} scale={scale}", S.fwd_input(C), _small_rois(), scale, ph, pw, sr, S.fwd_cc(C), must))
    w = S.FWD_WRAP
    out.append(("wrap", S.fwd_input(w["shape"][1], w["shape"][2:]), S.rois_of(w["rois"]), w["scale"], w["ph"], w["pw"], w["sr"], 4,
                ("swap23", "cg_off", "wrap_dropped")))
    return out


FWD = _fwd_cases()


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_fwd64_vs_pinned_oracle_and_strength(case):
    name, x, rois, scale, ph, pw, sr, cc, must = case
    ref, mag = S.roi_align_fwd64(x, rois, scale, ph, pw, sr)
    bound = S.fwd_tie_bound(mag, S.roi_grids(rois, scale, ph, pw, sr)) + 1e-300
    pinned = RO.roi_align(x, rois, scale, ph, pw, sr)
    m = R.margin(ref, pinned, bound)
    print(f"[fwd {name}] pinned float32 oracle off by {m:.3g} of (4 gh gw + 2) eps mag")
    assert m <= 1.0 and (mag >= np.abs(ref) - 1e-12).all()
    mut = {k: S.roi_align_fwd64(x, rois, scale, ph, pw, sr, (k,))[0] for k in S.ROI_MISTAKES}
    if x.shape[1] // cc > 1:
        mut["cg_off"] = S.roi_align_fwd64(x, rois, scale, ph, pw, sr, ("cg_off",), cc)[0]
    if name == "wrap":
        work = len(rois) * (x.shape[1] // cc) * ph * pw
        assert work == 1076480 > S.CAP and S.grid_for(work) == (4096, True)
        mut["wrap_dropped"] = S.wrap_dropped_fwd(ref, cc, R.SENT)
    else:
        assert not S.grid_for(len(rois) * (x.shape[1] // cc) * ph * pw)[1]
    _strong(f"fwd {name}", ref, bound, mut, must)


@pytest.mark.parametrize("C", S.FPN_CHANNELS)
@pytest.mark.parametrize("ph,pw,sr", S.FPN_SETTINGS)
def test_fpn_case(C, ph, pw, sr):
    feats, rois, levels, big = S.fpn_case(C)
    assert len(rois) == 24 and set(levels.tolist()) == {0, 1, 3} and (np.diff(levels) < 0).any()          # shuffled, level 2 empty
    (H, W), s = S.FPN_LEVELS[levels[big]]
    assert (rois[big, 3] - rois[big, 1]) * s > W and (rois[big, 4] - rois[big, 2]) * s > H
    assert S.fpn_cc(8) == 4 and S.fpn_cc(5) == 1
    for k in range(len(rois)):
        (H, W), s = S.FPN_LEVELS[levels[k]]
        ref, mag = S.roi_align_fwd64(feats[levels[k]], rois[k:k + 1], s, ph, pw, sr)
        bound = S.fwd_tie_bound(mag, S.roi_grids(rois[k:k + 1], s, ph, pw, sr)) + 1e-300
        assert R.margin(ref, RO.roi_align(feats[levels[k]], rois[k:k + 1], s, ph, pw, sr), bound) <= 1.0
        other = (levels[k] + 1) % 4                                                    # the roi pooled from a neighbouring level
        s2 = S.FPN_LEVELS[other][1]
        mut = {"swap23": S.roi_align_fwd64(feats[levels[k]], rois[k:k + 1], s, ph, pw, sr, ("swap23",))[0],
               "wrong level": S.roi_align_fwd64(feats[other], rois[k:k + 1], s2, ph, pw, sr)[0]}
        assert all(R.margin(ref, m, bound) >= 10.0 for m in mut.values()), k


@pytest.mark.parametrize("name", [c[0] for c in S.BWD_CASES])
def test_bwd64_is_the_transpose_and_strength(name):
    c = S.bwd_case(name)
    K = len(c["rois"])
    args = (c["rois"], c["scale"], c["ph"], c["pw"], c["sr"])
    x = R.uniform(f"adj:{name}", c["shape"])
    zero = np.zeros(c["shape"])
    gx, _, cnt = S.roi_align_bwd64(c["gout"], *args, c["shape"], zero)
    lhs = float((S.roi_align_fwd64(x, *args)[0] * c["gout"]).sum())
    rhs = float((x.astype(np.float64) * gx).sum())
    print(f"[bwd {name}] <fwd(x), g> {lhs:.12e}  <x, bwd(g)> {rhs:.12e}")
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-300)
    assert np.array_equal(cnt, c["cnt"]) and np.allclose(gx + c["init"], c["gin"], rtol=0, atol=1e-12) and (c["init"] != 0).all()
    work = K * c["shape"][1] * c["ph"] * c["pw"]
    assert S.grid_for(work)[1] == (name == "wrap")
    if name == "empty":
        assert K == 0 and np.array_equal(c["gin"], c["init"].astype(np.float64)) and not cnt.any()
        return
    bound = S.bwd_bound(c["mag"], c["cnt"])
    mut = {k: S.roi_align_bwd64(c["gout"], *args, c["shape"], c["init"], (k,))[0] for k in S.ROI_MISTAKES}
    mut["not accumulated"] = c["gin"] - c["init"]
    if name == "wrap":
        assert work == 1080000 > S.CAP
        mut["wrap_dropped"] = S.roi_align_bwd64(S.wrap_dropped_flat(c["gout"]), *args, c["shape"], c["init"])[0]
    _strong(f"bwd {name}", c["gin"], bound, mut, c["must"] + ("not accumulated",))


def test_bwd_cases_state_what_they_force():
    a = S.bwd_case("adaptive")
    grids = S.roi_grids(a["rois"], a["scale"], a["ph"], a["pw"], a["sr"])
    assert len(a["rois"]) == 8 and {g for gg in grids for g in gg} == {1, 2, 3} and any(gh != gw for gh, gw in grids)
    assert ((a["rois"][:, 3] - a["rois"][:, 1]) < 1).any() and ((a["rois"][:, 4] - a["rois"][:, 2]) < 1).any()
    for n in ("scaled.5", "scaled.25"):
        c = S.bwd_case(n)
        w = (c["rois"][:, 3] - c["rois"][:, 1])
        assert ((w >= 1) & (w * c["scale"] < 1)).any()                                 # max(., 1) before or after the scale differ
    o = S.bwd_case("outside")
    H, W = o["shape"][2:]
    g = [S.roi_geometry(r, 1.0, o["ph"], o["pw"], o["sr"], H, W) for r in o["rois"]]
    ys, xs = np.concatenate([q["yy"].ravel() for q in g[:4]]), np.concatenate([q["xx"].ravel() for q in g[:4]])
    for v, n in ((ys, H), (xs, W)):
        assert ((v >= -1) & (v <= 0)).any() and (v < -1).any() and (v > n).any() and ((v >= n - 1) & (v <= n)).any()
    assert g[4]["dead"].all() and not o["cnt"][1].any() and np.array_equal(o["gin"][1], o["init"][1].astype(np.float64))
    m = S.bwd_case("malformed")
    assert (m["rois"][:, 3] < m["rois"][:, 1]).sum() == 2 and (m["rois"][:, 4] < m["rois"][:, 2]).sum() == 2
    p = S.bwd_case("pileup")
    assert len(p["rois"]) == 64 and p["cnt"].max() >= 2000 and (p["cnt"][1].any((0,)) > 0).sum() <= 16
    assert len(S.bwd_case("wrap")["rois"]) == 6


# ------------------------------------------------------------------------------------------------ ROI pairing
@pytest.mark.parametrize("Rn", S.PAIR_R)
def test_pair_tables_hold_every_special(Rn):
    seen = set()
    for lb, rb, idx in S.pair_tables(Rn):
        assert lb.shape == rb.shape == (Rn, 4) and lb.dtype == np.float32
        rl, rr, geom = S.align_pairs(lb, rb, idx, S.PAIR_W, S.PAIR_H)
        for i in range(Rn):
            x1, y1, x2, y2 = (float(v) for v in lb[i])
            x1p, _, x2p, _ = (float(v) for v in rb[i])
            fl, ce = np.floor, np.ceil
            mw = geom[i, 2] - geom[i, 0]
            cx1, cx1p = max(0, int(fl(x1))), max(0, int(fl(x1p)))
            wl, wr = min(int(ce(x2)), S.PAIR_W - 1) - cx1, min(int(ce(x2p)), S.PAIR_W - 1) - cx1p
            if all(v == fl(v) for v in (x1, y1, x2, y2, x1p, x2p)):
                seen.add("integer")
            if x1 < 0 and y1 < 0:
                seen.add("negative")
            if x2 > S.PAIR_W and y2 > S.PAIR_H:
                seen.add("beyond")
            if wr > wl:
                seen.add("right wider")
            if mw < max(wl, wr) and mw == S.PAIR_W - cx1p < S.PAIR_W - cx1:
                seen.add("cut by x1p")
            if mw < max(wl, wr) and mw == S.PAIR_W - cx1 < S.PAIR_W - cx1p:
                seen.add("cut by x1")
            if x2 == S.PAIR_W - 1:
                seen.add("x2 on the border")
            if 0 < ce(x2) - x2 < 2e-4:
                seen.add("just below an integer")
            assert rl[i, 0] == idx[i] and rl[i, 3] - rl[i, 1] == mw == rr[i, 3] - rr[i, 1] and 0 <= rl[i, 1] and rl[i, 3] <= S.PAIR_W
    assert seen == {s[0] for s in S.PAIR_SPECIALS}
    assert np.float32(1240.9999) < 1241 and (Rn + 63) // 64 == {1: 1, 63: 1, 64: 1, 65: 2, 129: 3}[Rn]


# ------------------------------------------------------------------------------------------------ training targets
def _tgt_mutants(c):
    out = {}
    for k in ("keep_off", "inv_scale", "half_pixel", "no_pad"):
        t = S.train_targets64(c["disp"], c["gt"], c["probs"], c["M"], c["pad"], S.TGT_THRESH, c["lbox"], c["rois_l"], c["geom"], c["res"], (k,))
        out[k] = (t, S.mask_expect(t))
    return out


@pytest.mark.parametrize("name", list(S.TGT_CASES))
def test_targets_cases(name):
    c = S.tgt_case(name)
    ref, code, interp = c["ref"], c["code"], c["interp"]
    n = code.size
    work = len(c["idx"]) * c["res"] ** 2
    assert S.grid_for(work)[1] == (name == "wrap") and (name != "wrap" or work == 1103872 > S.CAP)
    share = {k: float((code == v).mean()) for k, v in (("skip", S.SKIP), ("interp", S.INTERP))}
    exact = float(np.mean([((q["ly"] == 0)[:, None] & (q["lx"] == 0)[None, :]).mean() if q else 0.0 for q in ref["rec"]]))
    ones = float(((code == S.ONE) | ((code == S.INTERP) & (interp == 1))).mean())
    print(f"[targets {name}] {n} pixels: left out {share['skip']:.4f}, rule 2 {exact:.3f}, rule 5 {share['interp']:.3f}, expected ones {ones:.3f}")
    assert share["skip"] <= 0.01 and (code == S.ZERO).any()
    # rule 5's comparator is float32 F.interpolate on the CPU; on an all-ones neighbourhood the exact answer is 1, and where it gives
    # 0.99999994 -> 0 it errs by itself.  That share counts against the 2e-3 the rule allows, so a case may spend at most half of it
    lost = float(((code == S.INTERP) & (interp == 0)).mean())
    print(f"[targets {name}] rule-5 pixels the CPU interpolation itself truncates to 0: {lost:.2e} of the case")
    assert lost <= 1e-3
    assert (code == S.ONE).any() if name.startswith("degenerate") else 0.05 <= ones <= 0.95              # an all-zero mask must not pass
    if name == "integer":
        assert exact >= 0.25 and set(c["idx"].tolist()) == {0, 1, 2}
        assert {int(g[2] - g[0]) - 1 for g in c["geom"]} | {int(r[4] - r[2]) - 1 for r in c["rois_l"]} == {7, 14, 21}
    if name == "general":
        assert share["interp"] >= 0.10
        boxes = [S.paste_box(b, c["M"], c["pad"]) for b in c["lbox"]]
        assert boxes[0][0] < 0 and boxes[0][1] < 0 and boxes[1][0] + boxes[1][2] > c["W"] and boxes[1][1] + boxes[1][3] > c["H"]
    if name.startswith("degenerate"):
        mw, hc = c["geom"][:, 2] - c["geom"][:, 0], c["rois_l"][:, 4] - c["rois_l"][:, 2]
        assert mw[0] == 1 and hc[1] == 1 and S.paste_box(c["lbox"][2], c["M"], c["pad"])[2:] == (1, 1)
    # every mistake: targets against their bound, masks against ten times the allowed 2e-3 share
    bound = S.target_bound(ref["mag"]) + 1e-300
    mut = _tgt_mutants(c)
    tm = {k: mut[k][0]["target"] for k in ("keep_off", "inv_scale", "half_pixel")}
    _strong(f"targets {name}", ref["target"], bound, tm, ("keep_off", "half_pixel") + (("inv_scale",) if c["res"] > 2 else ()))
    for k in ("half_pixel", "no_pad"):
        moved = S.mask_moved(code, interp, *mut[k][1])
        print(f"[targets {name}] masks under {k}: {moved:.4f} of the pixels change (allowed mismatch 2e-3)")
        if k == "no_pad" and c["pad"] > 0 and c["res"] > 2:                           # half_pixel already clears on the targets
            assert moved >= 2e-2, (name, k, moved)


@pytest.mark.parametrize("name", ["integer", "general", "wrap"])
def test_targets64_vs_caller_oracle(name):
    """oracle.train_caller_oracle.roi_targets (F.interpolate in float32, pinned to the reference's recorded scene): targets within the same
    12 eps mag as the kernel (the same float32 expression), masks under the rules"""
    c = S.tgt_case(name)
    worst, hard, soft = 0.0, 0, 0
    for r in range(len(c["idx"])):
        b = int(c["idx"][r])
        roi, roi_r, tgt, mk = TO.roi_targets([float(v) for v in c["lbox"][r]], [float(v) for v in c["rbox"][r]],
                                             torch.from_numpy(c["probs"][r].reshape(c["M"], c["M"])), torch.from_numpy(c["gt"][b]),
                                             torch.from_numpy(c["disp"][b]), c["res"])
        assert roi == tuple(int(v) for v in c["rois_l"][r, 1:]) and roi_r[0] == c["geom"][r, 1]
        worst = max(worst, R.margin(c["ref"]["target"][r], tgt.numpy(), S.target_bound(c["ref"]["mag"][r]) + 1e-300))
        h, s = S.mask_mismatch(c["code"][r], c["interp"][r], mk.numpy())
        hard, soft = hard + h, soft + s
    print(f"[targets64 vs roi_targets {name}] targets {worst:.3g} of the bound, masks: {hard} rule-2/3 breaks, {soft} rule-5 mismatches")
    assert worst <= 1.0 and hard == 0 and soft <= 2e-3 * c["code"].size


# ------------------------------------------------------------------------------------------------ paste and depth maps
@pytest.mark.parametrize("name", list(S.PASTE_CASES))
def test_paste_cases(name):
    c = S.PASTE_CASES[name]
    (H, W), counts = c["hw"], c["counts"]
    disp, boxes, masks = S.paste_inputs(name)
    ref, bound, covered = S.paste64(disp, boxes, counts, H, W, c["clamp0"], masks)
    assert S.blocks_for(H * W)[1] == (name == "wrap") and (name != "wrap" or H * W == 1054720 > S.CAP)
    assert not ref[~covered].any() and covered.any((1, 2)).tolist() == [n > 0 for n in counts]
    if name == "gap":
        assert counts == [2, 0, 3] and (ref >= 0).all() and (ref[covered] == 0).any() and (ref[covered] > 0).any()
        below = S.paste_surely_clamped(disp, boxes, counts, H, W)
        assert below.sum() >= 20 and not ref[below].any() and masks is not None and (masks == 0).any() and (masks == 1).any()
    if name.startswith("degenerate"):
        wh = {(b[2] - b[0] == 1, b[3] - b[1] == 1) for b in boxes}
        assert wh == {(True, False), (False, True), (True, True), (False, False)} and ((boxes[:, 5] - boxes[:, 4]) > (boxes[:, 2] - boxes[:, 0])).any()
        assert (boxes[:, 0] < 0).any() and (boxes[:, 1] < 0).any() and (boxes[:, 2] > W).any() and (boxes[:, 3] > H).any()
        assert any(tuple(b[2:4] - b[0:2]) == (2, 2) for b in boxes)
    if name == "wrap":
        assert covered.reshape(len(counts), -1)[:, S.CAP:].any(1).all()               # the second trip's pixels are covered in every image
    mut = {k: S.paste64(disp, boxes, counts, H, W, c["clamp0"], masks, (k,))[0] for k in ("wd_left", "no_offset")}
    if name == "wrap":
        mut["wrap_dropped"] = S.wrap_dropped_flat(ref, 0.0, H * W)
    _strong(f"paste {name}", ref, bound, mut, ("no_offset",) + (("wd_left",) if c["S"] > 1 else ()) + (("wrap_dropped",) if name == "wrap" else ()))
    # the float32 torch oracle on the boxes it can take (inside the image), within its own 1e-4
    r0 = 0
    for b, n in enumerate(counts):
        bx = boxes[r0:r0 + n]
        if n and (bx[:, :2] >= 0).all() and (bx[:, 2] <= W).all() and (bx[:, 3] <= H).all() and name != "wrap":
            lb, rb = torch.from_numpy(bx[:, :4].astype(np.float32)), torch.from_numpy(bx[:, [4, 1, 5, 3]].astype(np.float32))
            o = PO.disparity_map(lb, rb, torch.from_numpy(disp[r0:r0 + n]), H, W, c["clamp0"], None if masks is None else torch.from_numpy(masks[r0:r0 + n]))
            assert float(np.abs(o.numpy() - ref[b]).max()) <= 1e-4
        r0 += n


@pytest.mark.parametrize("name", list(S.DEPTH_CASES))
def test_depth_cases(name):
    c = S.DEPTH_CASES[name]
    H, W = c["hw"]
    disp, boxes, _ = S.paste_inputs(name, depth=True)
    k = np.full(len(boxes), S.FUXB)
    ref, bound, ok, inside = S.depth64(disp, boxes, k, H, W)
    assert not ref[~inside].any() and ok.mean() > 0.5 * inside.mean() > 0 and (name != "wrap" or (len(boxes) == 2 and H * W > S.CAP))
    mut = {m: np.where(ok, S.depth64(disp, boxes, k, H, W, (m,))[0], ref) for m in ("wd_left", "no_offset")}
    _strong(f"depth {name}", ref, np.where(ok, bound, 1.0), mut, ("no_offset",))


def test_grid_mirrors():
    assert S.grid_for(0) == (1, False) and S.grid_for(256) == (1, False) and S.grid_for(257) == (2, False)
    assert S.grid_for(S.CAP) == (4096, False) and S.grid_for(S.CAP + 1) == (4096, True) and S.blocks_for(S.CAP + 1) == (4096, True)
    assert S.grid_for(13 * 224 * 224) == (2548, False)                                # the largest launch of the rest of the suite
    assert [S.fwd_cc(C) for C in (1, 2, 3, 4, 5, 6, 7, 9, 12)] == [1, 1, 3, 4, 1, 3, 1, 3, 4]

"""GPU tests of the Stereo RPN's training step (csrc/srpn_train.hip, modeling/rpn/srpn_train.py, StereoRPN / DispRCNN in train mode):
the three sparse kernels against numpy / torch restatements (exact where they are gathers), the whole step against the fp64 oracle
(tests/srpn_train_oracle.py; bound 2 e32 + 2e-5 max|ref64|, e32 the oracle's own fp32-vs-fp64 error, no element excluded), against a dense
autograd witness, against the step recorded from the reference, and DispRCNN.train() with a frozen trunk.  The cases and their ReLU margin
are held on the host by tests/test_srpn_train_host.py.
"""
import numpy as np
import pytest
import torch

from tests import srpn_train_cases as CS
from tests import srpn_train_oracle as TO
from tests.head_kernels_oracle import active_pixels_np as np_active       # the hand-built masks and the numpy restatements of the kernels
from tests.head_kernels_oracle import batch_masks, col2im_np, gather_rows_np, image_a, row_coords
from tests.helpers import golden_npz

pytestmark = pytest.mark.gpu
F32 = np.float32
PRE_T, POST_T = 60, 20                                      # the recorded step's train limits: both cuts act


def ST():
    from disprcnn_amd.modeling.rpn import srpn_train
    return srpn_train


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def uniform(key, shape, lo=-1.0, hi=1.0):
    from disprcnn_amd.utils.synth import hash_uniform
    return hash_uniform(key, shape, lo, hi)


def check(got, ref64, ref32, what, rel=2e-5):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    e32 = np.abs(np.asarray(ref32, np.float64) - ref64).max(initial=0.0)
    err, mag = np.abs(got - ref64).max(initial=0.0), np.abs(ref64).max(initial=0.0)
    bound = 2 * e32 + rel * mag
    print(f"{what}: err {err:.3g} e32 {e32:.3g} bound {bound:.3g} (|ref| <= {mag:.3g})")
    assert np.isfinite(got).all() and err <= bound, what


# ------------------------------------------------------------------------------------------------ 1. active pixels
@pytest.mark.parametrize("cap", [8, 256])
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("N", [1, 2])
def test_active_pixels(N, L, cap):
    shapes, A = CS.SHAPES[:L], CS.A
    _, _, used = image_a(shapes, A, cap)
    assert used == (8 if cap == 8 else 4 + 4 * L)            # cap 8: exactly cap pixels; cap 256: the corners of every level
    out = None
    for which in (0, 1):                                     # the second call rewrites the same buffers completely
        pos, neg = batch_masks(which, N, shapes, A, cap)
        out = ST().active_pixels(cuda(pos), cuda(neg), N, A, shapes, cap, out=out)
        row_pix, counts, index = np_active(pos, neg, N, A, shapes, cap)
        assert np.array_equal(host(out[0]), row_pix) and np.array_equal(host(out[1]), counts) and np.array_equal(host(out[2]), index)
        assert counts.max() <= cap and (which == 0 or counts[0] == cap)
        maps = ST().index_maps(out[2], N, shapes)
        assert [tuple(m.shape) for m in maps] == [(N,) + tuple(s) for s in shapes]
        if which == 0:                                       # horizontal neighbours are consecutive rows of image 0
            m0 = host(maps[0])[0]
            assert m0[1, 1] >= 0 and m0[1, 2] == m0[1, 1] + 1 and m0[2, 1] >= 0 and m0[2, 2] == m0[2, 1] + 1 and m0[3, 3] == -1
    if N == 2:
        assert host(out[1])[1] == used


# ------------------------------------------------------------------------------------------------ 2. gather rows
@pytest.mark.parametrize("C", [8, 24])
def test_gather_rows(C):
    from disprcnn_amd import engine as E
    N, A, shapes, cap = 2, CS.A, CS.SHAPES, 32
    pos, neg = batch_masks(0, N, shapes, A, cap)
    pos[len(pos) // 2 + 7 * A] = 1                           # the second image: one pixel, so most of its rows are zero rows
    row_pix, counts, index = ST().active_pixels(cuda(pos), cuda(neg), N, A, shapes, cap)
    rp = host(row_pix)
    assert list(host(counts)) == [24, 1]
    dev = torch.device("cuda")
    hid_dense = [uniform(f"gr{C}:h{l}", (N, 4 * C, h, w)).cuda() for l, (h, w) in enumerate(shapes)]
    hidden = [E.Blocked(N, 4 * C, 1, h, w, 0, 0, 0, dev).from_dense(d) for d, (h, w) in zip(hid_dense, shapes)]
    fl = [uniform(f"gr{C}:l{l}", (N, C, h, w)).cuda() for l, (h, w) in enumerate(shapes)]
    fr = [uniform(f"gr{C}:r{l}", (N, C, h, w)).cuda() for l, (h, w) in enumerate(shapes)]
    gz = [uniform(f"gr{C}:gz{l}", (N, 2 * A, h, w)).cuda() for l, (h, w) in enumerate(shapes)]
    gb = [uniform(f"gr{C}:gb{l}", (N, 6 * A, h, w)).cuda() for l, (h, w) in enumerate(shapes)]
    s_obj, s_box = torch.tensor([0.37], device=dev), torch.tensor([-1.9], device=dev)
    T, Xcol, G = ST().gather_rows(row_pix, N, A, C, cap, shapes, hidden=[(h.storage, h.n_stride) for h in hidden], feats=(fl, fr),
                                  grads=(gz, gb), g_obj=s_obj, g_box=s_box)
    _, _, G_obj_only = ST().gather_rows(row_pix, N, A, C, cap, shapes, grads=(gz, gb), g_obj=s_obj, g_box=None)
    _, _, G_box_only = ST().gather_rows(row_pix, N, A, C, cap, shapes, grads=(gz, gb), g_obj=None, g_box=s_box)
    R = N * cap
    wT, wX, wG = gather_rows_np(rp, N, A, C, cap, shapes, hidden=[host(d) for d in hid_dense], feats=([host(f) for f in fl], [host(f) for f in fr]),
                                grads=([host(g) for g in gz], [host(g) for g in gb]), s_obj=host(s_obj)[0], s_box=host(s_box)[0])
    wT, wX, wG = torch.from_numpy(wT), torch.from_numpy(wX), torch.from_numpy(wG)
    edge = sum(y in (0, shapes[l][0] - 1) or x in (0, shapes[l][1] - 1) for _, _, l, y, x, _ in row_coords(rp, shapes, cap))
    assert edge >= 20 and (rp < 0).sum() == R - 25           # corners of every level; zero rows past the counts
    assert torch.equal(T.cpu(), wT) and torch.equal(Xcol.cpu(), wX) and torch.equal(G.cpu(), wG)
    live = torch.from_numpy(rp >= 0)
    assert (wX[:R][live] == 0).any() and not T.cpu()[~live].any() and not Xcol.cpu()[:R][~live].any() and not Xcol.cpu()[R:][~live].any()
    zero_box, zero_obj = wG.clone(), wG.clone()
    zero_box[:, 2 * A:], zero_obj[:, :2 * A] = 0, 0
    assert torch.equal(G_obj_only.cpu(), zero_box) and torch.equal(G_box_only.cpu(), zero_obj)


# ------------------------------------------------------------------------------------------------ 3. col2im
@pytest.mark.parametrize("C", [8, 24])
def test_col2im(C):
    N, A, shapes, cap = 2, CS.A, CS.SHAPES, 8                # cap 8: the neighbour / overlap pixels and the last level's corners;
    pos, neg = batch_masks(1, N, shapes, A, cap)             # image 0: exactly cap pixels on level 0; levels 1..3 have no active pixel
    row_pix, counts, index = ST().active_pixels(cuda(pos), cuda(neg), N, A, shapes, cap)
    rp = host(row_pix)
    R = N * cap
    dxcol = uniform(f"c2i{C}", (2 * R, 9 * C), -2.0, 2.0)
    dx = dxcol.cuda()
    dl, dr = ST().col2im(dx, index, N, A, C, cap, shapes)
    dl2, dr2 = ST().col2im(dx, index, N, A, C, cap, shapes)
    only_l, none_r = ST().col2im(dx, index, N, A, C, cap, shapes, want_right=False)
    ref64, ref32 = (col2im_np(dxcol.numpy(), rp, N, C, cap, shapes, dtype) for dtype in (np.float64, np.float32))
    active_levels = set()
    for view, got in enumerate((dl, dr)):
        for l in range(len(shapes)):
            g, r64, r32 = host(got[l]).astype(np.float64), ref64[view][l], ref32[view][l]
            e32, err = np.abs(r32 - r64).max(), np.abs(g - r64).max()
            print(f"view {view} level {l}: err {err:.3g} e32 {e32:.3g} max {np.abs(r64).max():.3g}")
            assert err <= 2 * e32 + 1e-6 * np.abs(r64).max()
            assert not g[r64 == 0].any()                     # all zeros where nothing is active (written, not left over)
            if np.abs(r64).max() > 0:
                active_levels.add(l)
    assert active_levels == {0, len(shapes) - 1}             # levels with no active pixel come back as zeros
    for a, b in zip(dl + dr, dl2 + dr2):
        assert torch.equal(a, b)
    assert none_r is None and all(torch.equal(a, b) for a, b in zip(only_l, dl))


# ------------------------------------------------------------------------------------------------ 4. StereoRPN.train()
def train_cfg(pre=PRE_T, post=POST_T):
    from disprcnn_amd.modeling.detector.disprcnn import default_cfg_2d
    cfg = default_cfg_2d()
    r = cfg.MODEL.RPN
    r.BATCH_SIZE_PER_IMAGE, r.POSITIVE_FRACTION, r.PRE_NMS_TOP_N_TRAIN, r.POST_NMS_TOP_N_TRAIN = CS.BATCH, CS.FRACTION, pre, post
    return cfg


def new_rpn(c, cfg=None):
    from disprcnn_amd.modeling.rpn.stereo_rpn import StereoRPN
    rpn = StereoRPN(cfg or train_cfg(), c.c)
    sd = rpn.state_dict()
    sd.update({k: torch.from_numpy(np.asarray(v)) for k, v in c.params.items()})
    rpn.load_state_dict(sd, strict=True)
    return rpn.cuda().train()


def rpn_inputs(c, grad=True):
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.image_list import ImageList
    images = ImageList(torch.zeros(c.n, 3, CS.IMG[1], CS.IMG[0]), [(h, w) for (w, h) in c.img_whs])
    fl = [cuda(f).requires_grad_(grad) for f in c.feats_left]
    fr = [cuda(f).requires_grad_(grad) for f in c.feats_right]
    lt = [BoxList(cuda(g), wh, mode="xyxy") for g, wh in zip(c.gt_left, c.img_whs)]
    rt = [BoxList(cuda(g), wh, mode="xyxy") for g, wh in zip(c.gt_right, c.img_whs)]
    return images, fl, fr, lt, rt


def run_step(rpn, c):
    images, fl, fr, lt, rt = rpn_inputs(c)
    rpn.zero_grad(set_to_none=True)
    lb, rb, losses = rpn(images, images, fl, fr, lt, rt, draws=cuda(c.draws))
    assert set(losses) == {"loss_objectness", "loss_rpn_box_reg"}
    (losses["loss_objectness"] + losses["loss_rpn_box_reg"]).backward()
    named = dict(rpn.named_parameters())
    return dict(losses={k: v.detach().clone() for k, v in losses.items()}, grads={k: named[k].grad.detach().clone() for k in TO.PARAMS},
                gleft=[f.grad.detach().clone() for f in fl], gright=[f.grad.detach().clone() for f in fr], left=lb, right=rb)


@pytest.mark.parametrize("name", ["full", "wide", "none"])
def test_stereo_rpn_training_step(name):
    c = CS.cached(name)
    r64, r32 = CS.cached_oracle(name, 64), CS.cached_oracle(name, 32)
    rpn = new_rpn(c)
    a = run_step(rpn, c)
    for k in ("loss_objectness", "loss_rpn_box_reg"):
        check(host(a["losses"][k]), r64[k], r32[k], f"{name} {k}")
    for k in TO.PARAMS:
        check(host(a["grads"][k]), r64["grads"][k], r32["grads"][k], f"{name} d/d {k}")
    for side in ("gleft", "gright"):
        for l in range(len(CS.SHAPES)):
            check(host(a[side][l]), r64[side][l], r32[side][l], f"{name} {side}[{l}]")
    if name == "none":
        assert all(v.item() == 0 for v in a["losses"].values()) and not any(g.any().item() for g in a["grads"].values())
        assert not any(g.any().item() for g in a["gleft"] + a["gright"])
    else:
        assert all(v.item() > 0 for v in a["losses"].values())
    b = run_step(rpn, c)                                     # a second run: the same bits everywhere
    for k in a["losses"]:
        assert torch.equal(a["losses"][k], b["losses"][k]), k
    for k in TO.PARAMS:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    for x, y in zip(a["gleft"] + a["gright"], b["gleft"] + b["gright"]):
        assert torch.equal(x, y)
    for x, y in zip(a["left"] + a["right"], b["left"] + b["right"]):
        assert torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("objectness"), y.get_field("objectness"))
    for bl in a["left"]:
        s = bl.get_field("objectness")
        assert 0 < len(bl) <= POST_T and (s[1:] <= s[:-1]).all().item()      # descending-score order
    with pytest.raises(RuntimeError):
        images, fl, fr, lt, rt = rpn_inputs(c, grad=False)
        rpn(images, images, [f.cpu() for f in fl], [f.cpu() for f in fr], lt, rt)


@pytest.mark.parametrize("name", ["full", "wide"])
def test_dense_autograd_head_is_a_second_witness(name):
    """the existing srpn_loss on a torch autograd head (F.conv2d) at the same weights, the same sample: the same gradients within the same
    bound"""
    from disprcnn_amd.layers import det2d_loss as D
    c = CS.cached(name)
    r64, r32 = CS.cached_oracle(name, 64), CS.cached_oracle(name, 32)
    rpn = new_rpn(c)
    images, fl, fr, lt, rt = rpn_inputs(c)
    ev = rpn.loss_evaluator
    with torch.no_grad():
        _, labels, reg, counts = ev.prepare_targets(rpn.anchor_generator(images, fl), lt, rt)
        pos, neg, n_sampled, _ = ev.fg_bg_sampler.sample(labels, counts, cuda(c.draws))
    assert np.array_equal(host(pos), c.pos) and np.array_equal(host(neg), c.neg)          # the host oracle's sample
    prm = {k: p for k, p in rpn.named_parameters()}
    logits, regs, _ = TO.head(prm, fl, fr, torch.float32)
    lo, lb, _ = D.srpn_loss(logits, regs, pos, neg, reg, n_sampled, beta=1.0 / 9)
    (lo + lb).backward()
    check(lo.item(), r64["loss_objectness"], r32["loss_objectness"], "dense loss_objectness")
    check(lb.item(), r64["loss_rpn_box_reg"], r32["loss_rpn_box_reg"], "dense loss_rpn_box_reg")
    for k in TO.PARAMS:
        check(host(prm[k].grad), r64["grads"][k], r32["grads"][k], f"dense d/d {k}")
    for side, fs in (("gleft", fl), ("gright", fr)):
        for l, f in enumerate(fs):
            check(host(f.grad), r64[side][l], r32[side][l], f"dense {side}[{l}]")


# ------------------------------------------------------------------------------------------------ 5. selection
def test_train_time_selection():
    z = golden_npz("srpn_train_golden.npz")
    c = CS.cached("full")
    assert (int(z["pre_nms"]), int(z["post_nms"])) == (PRE_T, POST_T)
    rpn = new_rpn(c)
    images, fl, fr, lt, rt = rpn_inputs(c, grad=False)
    lp, rp, _ = rpn(images, images, fl, fr, lt, rt, draws=cuda(c.draws))
    for i in range(c.n):                                     # the tolerance tests/test_hip_detector2d.py grants the eval proposals
        assert len(lp[i]) == z[f"prop_left{i}"].shape[0] == POST_T and lp[i].size == CS.IMG
        np.testing.assert_allclose(host(lp[i].get_field("objectness")), z[f"prop_score{i}"], rtol=0, atol=3e-5)
        np.testing.assert_allclose(host(lp[i].bbox), z[f"prop_left{i}"], rtol=0, atol=5e-3)
        np.testing.assert_allclose(host(rp[i].bbox), z[f"prop_right{i}"], rtol=0, atol=5e-3)
    # the eval forward's selection with the train limits on the same raw maps: bit for bit
    logits, regs, _ = rpn.head_train(fl, fr)
    rpn.eval()
    rpn.pre_nms_top_n, rpn.post_nms_top_n = PRE_T, POST_T
    rpn.proposals_dense = lambda *a, **k: rpn._decode(images, logits, regs)
    with torch.no_grad():
        le, re_, losses = rpn(images, images, fl, fr)
    assert losses == {}
    for x, y in zip(lp + rp, le + re_):
        assert torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("objectness"), y.get_field("objectness"))


# ------------------------------------------------------------------------------------------------ 6. eval unchanged
def test_eval_forward_is_unchanged_by_training():
    c = CS.cached("full")
    trained, fresh = new_rpn(c), new_rpn(c).eval()
    run_step(trained, c)
    trained.eval()
    images, fl, fr, _, _ = rpn_inputs(c, grad=False)
    with torch.no_grad():
        a, b = trained(images, images, fl, fr), fresh(images, images, fl, fr)
    assert a[2] == {} and b[2] == {} and len(a[0]) == c.n
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert len(x) > 0 and torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("objectness"), y.get_field("objectness"))


# ------------------------------------------------------------------------------------------------ 7. DispRCNN.train(), trunk frozen
DET_GT = [np.array([[8, 12, 40, 44], [48, 16, 112, 80]], F32), np.array([[40, 36, 72, 68], [81, 41, 126, 64], [16, 0, 80, 64]], F32)]


def test_disprcnn_training_with_a_frozen_trunk():
    from disprcnn_amd.modeling.detector import DispRCNN, default_cfg_2d
    from disprcnn_amd.solver.fused import FusedSGD
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.image_list import to_image_list
    from disprcnn_amd.utils import synth
    n, h, w = 2, 96, 160
    cfg = default_cfg_2d("R-50-FPN")
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TRAIN = 12000                # above the batch's anchor count: every anchor reaches the NMS
    m = DispRCNN(cfg)
    sd = m.state_dict()
    w_rpn = synth.synth_det_state({k[4:]: v for k, v in sd.items() if k.startswith("rpn.")}, gain={"head.cls_logits.weight": 0.5, "head.bbox_pred.weight": 0.02})
    w_heads = synth.synth_det_state({k[10:]: v for k, v in sd.items() if k.startswith("roi_heads.")}, gain=synth.DET_GAIN)
    bb = synth.synth_backbone_state({k[9:]: v for k, v in sd.items() if k.startswith("backbone.")})
    m.load_state_dict({**{"backbone." + k: v for k, v in bb.items()}, **{"rpn." + k: v for k, v in w_rpn.items()},
                       **{"roi_heads." + k: v for k, v in w_heads.items()}}, strict=True)
    m = m.cuda().train()
    left, right = synth.synth_images(n, h, w, tag="srpn:det")
    lr = {"left": left.cuda(), "right": right.cuda()}

    def targets():
        lt, rt = [], []
        for g in DET_GT:
            masks = np.zeros((len(g), h, w), np.uint8)
            for k, b in enumerate(g.astype(int)):
                masks[k, b[1]: b[3] + 1, b[0]: b[2] + 1] = 1
            l, r = BoxList(cuda(g), (w, h), mode="xyxy"), BoxList(cuda(g + np.array([-4, 0, -4, 0], F32)), (w, h), mode="xyxy")
            l.add_field("labels", torch.ones(len(g), dtype=torch.int64).cuda()), r.add_field("labels", torch.ones(len(g), dtype=torch.int64).cuda())
            l.add_field("masks", cuda(masks))
            lt.append(l), rt.append(r)
        return {"left": lt, "right": rt}
    tg = targets()
    with pytest.raises(NotImplementedError, match="trunk's backward"):        # a trainable backbone is refused first
        m(lr, tg)
    for p in m.backbone.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError):
        m(lr)
    # the parts on the eval backbone's features, which also gives the sizes of the box head's draws
    total = sum(hh * ww for hh, ww in CS.SHAPES) * CS.A
    d_rpn = uniform("srpn:det:rpn", (n * total,), 0.0, 1.0).cuda()
    li, ri = to_image_list(lr["left"]), to_image_list(lr["right"])
    lf, rf, levels = m.frozen_features(li, ri)
    assert [tuple(f.shape[2:]) for f in lf] == CS.SHAPES and not any(f.requires_grad for f in lf)
    lp, rp, _ = m.rpn(li, ri, lf, rf, tg["left"], tg["right"], blocked_levels=levels, draws=d_rpn)
    d_sample = uniform("srpn:det:sample", (sum(len(b) for b in lp),), 0.0, 1.0).cuda()
    x, _, _, _ = m.roi_heads.box({"left": lf, "right": rf}, {"left": lp, "right": rp}, tg, draws={"sample": d_sample})
    draws = {"rpn_sample": d_rpn, "sample": d_sample, "dropout": uniform("srpn:det:drop", (2, x.shape[0], 64), 0.0, 1.0).cuda()}

    def parts():
        lf, rf, levels = m.frozen_features(li, ri)
        lp, rp, pl = m.rpn(li, ri, lf, rf, tg["left"], tg["right"], blocked_levels=levels, draws=draws["rpn_sample"])
        _, _, _, dl = m.roi_heads(lf, rf, lp, rp, tg["left"], tg["right"], draws={"sample": draws["sample"], "dropout": draws["dropout"]})
        return {**dl, **pl}
    keys = {"loss_classifier", "loss_box_reg", "loss_mask", "loss_objectness", "loss_rpn_box_reg"}
    want = parts()
    m.zero_grad(set_to_none=True)
    losses = m(lr, tg, draws=draws)
    assert set(losses) == set(want) == keys
    for k in keys:
        print(k, losses[k].item())
        assert torch.equal(losses[k], want[k]), k
    assert all(losses[k].item() > 0 for k in keys)           # positives exist for both stages: every loss has something to learn
    opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=0.02, momentum=0.9)
    sum(losses.values()).backward()
    for k, p in m.named_parameters():
        if k.startswith("backbone."):
            assert p.grad is None, k
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
    assert all(p.grad.any().item() for k, p in m.named_parameters() if k.startswith("rpn."))
    opt.step()
    # the updated RPN proposes other boxes, so the box head's draws no longer fit: only the RPN's sample stays fixed from here on (the
    # two RPN losses are then functions of the weights alone)
    after = m(lr, tg, draws={"rpn_sample": d_rpn})
    assert set(after) == keys and all(after[k].item() != losses[k].item() for k in keys)
    m.rpn.eval()                                             # the reference's FIX_RPN: an eval sub-module contributes no losses
    assert set(m(lr, tg, draws={"rpn_sample": d_rpn})) == {"loss_classifier", "loss_box_reg", "loss_mask"}
    m.rpn.train()
    m.cfg.SOLVER = type("S", (), {"TRAIN_2D": False})()
    assert m(lr, tg, draws={"rpn_sample": d_rpn}) == {}

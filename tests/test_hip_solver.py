"""FusedSGD / FusedAdam on the MI355X against torch.optim.SGD / Adam on the CPU in fp64.

The bound is the project's standing one (tests/test_hip_pn2_mlp_bwd.py::check_bound): err <= 2 * e32 + 1e-6 * max|ref| per parameter
tensor and per state tensor, where e32 is the error of the SAME torch optimizer run in fp32 on the CPU.  The parameter set has the
sizes at which the chunked kernels can go wrong -- 1, 0, CH - 1, CH, CH + 1, 2 * CH + 3 elements (CH = drc_solver_chunk()) -- in three
groups with different learning rates and weight decays, and gradients drawn anew for every step.
"""
import copy

import numpy as np
import pytest
import torch

from tests import solver_oracle as SO
from tests.test_hip_pn2_mlp_bwd import check_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = np.float32
GROUPS = ((0, 1, 2), (3, 4), (5,))                     # tensor indices of the three groups
GROUP_LR = (0.05, 0.02, 0.1)
GROUP_WD = (5e-4, 0.0, 1e-3)
STEPS = 5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def chunk():
    from disprcnn_amd.pts import _lib
    return _lib.lib().drc_solver_chunk()


def numels():
    ch = chunk()
    return [1, 0, ch - 1, ch, ch + 1, 2 * ch + 3]


_CASE = {}


def case():
    """initial parameters and STEPS sets of gradients, made once and never changed"""
    if not _CASE:
        rs = np.random.RandomState(7)
        _CASE["init"] = [rs.normal(0, 1, n).astype(f32) for n in numels()]
        _CASE["grads"] = [[rs.normal(0, 1, n).astype(f32) for n in numels()] for _ in range(STEPS)]
    return _CASE["init"], _CASE["grads"]


def group_list(params, wd=None, one_group=False):
    if one_group:
        return [{"params": list(params)}]
    return [{"params": [params[i] for i in idx], "lr": lr, "weight_decay": w if wd is None else wd}
            for idx, lr, w in zip(GROUPS, GROUP_LR, GROUP_WD)]


def one_cycle_like(opt, s):
    """what OneCycleScheduler does to the groups between steps: another rate, another momentum / beta1"""
    for gi, g in enumerate(opt.param_groups):
        g["lr"] = GROUP_LR[gi % 3] * (1.0 + 0.3 * s)
        if "betas" in g:
            g["betas"] = (0.85 + 0.02 * s, g["betas"][1])
        else:
            g["momentum"] = 0.85 + 0.02 * s


def state_names(kind):
    return ("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq")


def run_torch(kind, dtype, kw, steps=STEPS, wd=None, one_group=False, hyper=None, max_norm=None, start=None, first_step=0):
    """torch.optim on the CPU in `dtype` -> dict(params, grads (as the step left them), norms, state..., opt)"""
    init, grads = case()
    params = [torch.nn.Parameter(torch.from_numpy(a).to(dtype).clone()) for a in init]         # from_numpy shares memory
    cls = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
    opt = cls(group_list(params, wd, one_group), **kw)
    if start is not None:
        with torch.no_grad():
            for p, a in zip(params, start["params"]):
                p.copy_(a.to(dtype))
        opt.load_state_dict(copy.deepcopy(start["sd"]))          # torch keeps tensors of the right dtype (and every step count) as they are
    norms = []
    for s in range(first_step, first_step + steps):
        for p, g in zip(params, grads[s]):
            p.grad = torch.from_numpy(g).to(dtype).clone()
        if hyper is not None:
            hyper(opt, s)
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm).double())
        opt.step()
    out = {"params": [p.detach().double() for p in params], "grads": [p.grad.double() for p in params], "norms": norms, "opt": opt}
    for name in state_names(kind):
        out[name] = [opt.state[p][name].double() if name in opt.state.get(p, {}) else None for p in params]
    return out


def flat_offsets(ns, phase):
    """element offsets into one flat buffer, with odd gaps so that the views' addresses take every residue mod 16 bytes"""
    offs, off = [], phase
    for i, n in enumerate(ns):
        offs.append(off)
        off += n + (1, 3, 2, 1, 3, 1)[i % 6]
    return offs, off


def run_fused(kind, kw, steps=STEPS, wd=None, one_group=False, hyper=None, max_norm=None, layout="separate", clip_call=False, start=None,
              first_step=0):
    """the fused optimizer on the GPU.  layout: "separate" (allocated gradients), "flat" (gradients are views of ONE flat buffer at odd
    element offsets) or "flat_params" (the parameters too).  clip_call: clip_grad_norm_() then step() instead of step(max_norm=)."""
    from disprcnn_amd.solver import FusedAdam, FusedSGD
    init, grads = case()
    ns = numels()
    if layout == "flat_params":
        offs, total = flat_offsets(ns, 3)
        pflat = torch.zeros(total, device=DEV)
        params = [torch.nn.Parameter(pflat[o:o + n]) for o, n in zip(offs, ns)]
        with torch.no_grad():
            for p, a in zip(params, init):
                p.copy_(torch.from_numpy(a))
    else:
        params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
    if start is not None:
        with torch.no_grad():
            for p, a in zip(params, start["params"]):
                p.copy_(a.to(torch.float32))
    gviews = None
    if layout != "separate":
        offs, total = flat_offsets(ns, 1)
        gflat = torch.zeros(total, device=DEV)
        gviews = [gflat[o:o + n] for o, n in zip(offs, ns)]
        assert len({v.data_ptr() % 16 for v in gviews}) == 4
    opt = (FusedSGD if kind == "sgd" else FusedAdam)(group_list(params, wd, one_group), **kw)
    if start is not None:
        opt.load_state_dict(copy.deepcopy(start["sd"]))          # torch keeps tensors of the right dtype (and every step count) as they are
    norms = []
    for s in range(first_step, first_step + steps):
        for i, (p, g) in enumerate(zip(params, grads[s])):
            if gviews is None:
                p.grad = torch.from_numpy(g).to(DEV)
            else:
                gviews[i].copy_(torch.from_numpy(g))
                p.grad = gviews[i]
        if hyper is not None:
            hyper(opt, s)
        if max_norm is not None and clip_call:
            norms.append(opt.clip_grad_norm_(max_norm).double().cpu())
            opt.step()
        else:
            opt.step(max_norm=max_norm)
            if max_norm is not None:
                norms.append(opt.total_norm.double().cpu())
    torch.cuda.synchronize()
    out = {"params": [p.detach().clone() for p in params], "grads": [p.grad.clone() for p in params], "norms": norms, "opt": opt}
    for name in state_names(kind):
        out[name] = [opt.state[p][name].clone() if name in opt.state.get(p, {}) else None for p in params]
    return out


def compare(kind, got, r64, r32, what=("params",), tag=""):
    for key in tuple(what) + state_names(kind):
        for i, (g, a, b) in enumerate(zip(got[key], r64[key], r32[key])):
            if a is None:
                assert g is None or not g.any(), (key, i)
                continue
            assert g is not None and g.shape == a.shape and bool(torch.isfinite(g).all()), (key, i)
            e32 = (b - a).abs().max().item() if a.numel() else 0.0
            check_bound(f"{tag}{key}[{i}] n={a.numel()}", g, a, e32)


def same_bits(a, b, keys):
    for key in keys:
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (key, i)


# ---- trajectories
@pytest.mark.parametrize("name,kind,kw,wd,one_group,hyper", [
    ("sgd momentum 0.9, weight decay 5e-4, one group", "sgd", dict(lr=0.05, momentum=0.9, weight_decay=5e-4), None, True, None),
    ("sgd momentum 0.9, three groups", "sgd", dict(lr=0.05, momentum=0.9), None, False, None),
    ("sgd momentum 0", "sgd", dict(lr=0.05, momentum=0.0), None, False, None),
    ("sgd cycled momentum", "sgd", dict(lr=0.05, momentum=0.9), None, False, one_cycle_like),
    ("adam weight decay 0", "adam", dict(lr=0.01), 0.0, False, None),
    ("adam weight decay > 0", "adam", dict(lr=0.01), None, False, None),
    ("adam cycled beta1", "adam", dict(lr=0.01), None, False, one_cycle_like),
])
def test_trajectory_matches_torch_in_fp64(name, kind, kw, wd, one_group, hyper):
    r64 = run_torch(kind, torch.float64, kw, wd=wd, one_group=one_group, hyper=hyper)
    r32 = run_torch(kind, torch.float32, kw, wd=wd, one_group=one_group, hyper=hyper)
    got = run_fused(kind, kw, wd=wd, one_group=one_group, hyper=hyper)
    compare(kind, got, r64, r32, tag=name + ": ")
    if kind == "adam":
        p = got["opt"].param_groups[0]["params"][0]
        assert float(got["opt"].state[p]["step"]) == STEPS
    if name == "sgd momentum 0":
        assert got["opt"].state_dict()["state"] == {}                       # as torch: no buffer without momentum


# ---- layout
@pytest.mark.parametrize("kind,kw,max_norm", [("sgd", dict(lr=0.05, momentum=0.9), 5.0), ("adam", dict(lr=0.01), None)])
def test_flat_buffer_views_at_odd_offsets_give_the_same_bits(kind, kw, max_norm):
    keys = ("params", "grads") + state_names(kind)
    a = run_fused(kind, kw, steps=3, max_norm=max_norm)
    b = run_fused(kind, kw, steps=3, max_norm=max_norm, layout="flat")
    c = run_fused(kind, kw, steps=3, max_norm=max_norm, layout="flat_params")
    a2 = run_fused(kind, kw, steps=3, max_norm=max_norm)
    same_bits(a, b, keys)
    same_bits(a, c, keys)
    same_bits(a, a2, keys)                                                   # and two runs give the same bits
    if max_norm is not None:
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a["norms"], b["norms"], c["norms"]))
    # the steps did something
    init, _ = case()
    assert all(not torch.equal(p.cpu(), torch.from_numpy(i)) for p, i in zip(a["params"], init) if i.size)


# ---- clipping
@pytest.mark.parametrize("kind,kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01))])
@pytest.mark.parametrize("clip_call", [False, True])
def test_clipping_above_the_norm_matches_clip_grad_norm_and_step(kind, kw, clip_call):
    max_norm = 5.0                      # the gradients' norm is about sqrt(5 * CH) >> 5
    r64 = run_torch(kind, torch.float64, kw, steps=3, max_norm=max_norm)
    r32 = run_torch(kind, torch.float32, kw, steps=3, max_norm=max_norm)
    got = run_fused(kind, kw, steps=3, max_norm=max_norm, clip_call=clip_call)
    assert len(got["norms"]) == 3 and all(n.item() > max_norm for n in r64["norms"])
    for s, (g, a, b) in enumerate(zip(got["norms"], r64["norms"], r32["norms"])):
        check_bound(f"total_norm step {s}", g.reshape(1), a.reshape(1), (b - a).abs().item())
    compare(kind, got, r64, r32, what=("params", "grads"))                   # .grad is left scaled, as clip_grad_norm_ leaves it


@pytest.mark.parametrize("kind,kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01))])
def test_clipping_below_the_norm_leaves_the_steps_bits(kind, kw):
    keys = ("params", "grads") + state_names(kind)
    plain = run_fused(kind, kw, steps=3)
    loose = run_fused(kind, kw, steps=3, max_norm=1e6)
    armed = run_fused(kind, kw, steps=3, max_norm=1e6, clip_call=True)
    same_bits(plain, loose, keys)
    same_bits(plain, armed, keys)
    init, grads = case()
    want = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads[2]))
    assert abs(loose["norms"][2].item() - want) <= 1e-6 * want


# ---- captured step
def test_captured_step_replays_with_pushed_learning_rates():
    from disprcnn_amd.solver import FusedSGD
    from disprcnn_amd.utils.graph import GraphedStep
    rs = np.random.RandomState(11)
    w0, b0, x0 = rs.normal(0, 1, (3, 5)).astype(f32), rs.normal(0, 1, 3).astype(f32), rs.normal(0, 1, (8, 5)).astype(f32)
    lrs = (0.05, 0.05, 0.05, 0.02, 0.08, 0.01)             # three warm-up steps at the first rate, then one rate per replay

    def make():
        w, b = torch.nn.Parameter(torch.from_numpy(w0).to(DEV)), torch.nn.Parameter(torch.from_numpy(b0).to(DEV))
        x = torch.from_numpy(x0).to(DEV)
        opt = FusedSGD([{"params": [w], "weight_decay": 1e-3}, {"params": [b]}], lr=lrs[0], momentum=0.9)

        def fn():
            opt.zero_grad()
            loss = (((x.unsqueeze(1) * w.unsqueeze(0)).sum(2) + b) ** 2).mean()          # elementwise and reductions only: no BLAS plan to differ
            loss.backward()
            opt.step()
            return loss
        return w, b, opt, fn

    def set_lr(opt, lr):
        for g in opt.param_groups:
            g["lr"] = lr

    w, b, opt, fn = make()
    eager_losses = []
    for lr in lrs:
        set_lr(opt, lr)
        eager_losses.append(fn().item())
    torch.cuda.synchronize()

    gw, gb, gopt, gfn = make()
    graphed = GraphedStep(gfn, warmup=3)
    losses = []
    for lr in lrs[3:]:
        set_lr(gopt, lr)
        gopt.push_hyper()
        losses.append(graphed().item())
    gopt.bump_versions()
    torch.cuda.synchronize()
    assert losses == eager_losses[3:]
    assert torch.equal(gw, w) and torch.equal(gb, b)
    assert torch.equal(gopt.state[gw]["momentum_buffer"], opt.state[w]["momentum_buffer"])
    assert not torch.equal(w.detach().cpu(), torch.from_numpy(w0))

    # under capture nothing is uploaded: a gradient that moved raises, and the capture ends cleanly
    kept, scratch = gw.grad, torch.zeros(4, device=DEV)
    gw.grad = torch.zeros_like(gw)
    torch.cuda.synchronize()
    before = gw.detach().clone()
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match=r"under stream capture.*zero_grad\(\).*push_hyper\(\)"):
        with torch.cuda.graph(g2):
            scratch.zero_()
            gopt.step()
    assert not torch.cuda.is_current_stream_capturing()
    set_lr(gopt, 0.5)
    g3 = torch.cuda.CUDAGraph()
    gw.grad = kept
    with pytest.raises(RuntimeError, match=r"under stream capture.*push_hyper\(\)"):
        with torch.cuda.graph(g3):
            scratch.zero_()
            gopt.step()
    del g2, g3
    torch.cuda.synchronize()
    assert torch.equal(gw, before)                           # neither attempt touched the weights
    gopt.step()                                              # and the optimizer still steps eagerly
    torch.cuda.synchronize()
    assert not torch.equal(gw, before)


# ---- checkpoints
def cpu_state_dict(sd):
    out = copy.deepcopy({"param_groups": sd["param_groups"], "state": {}})
    for i, s in sd["state"].items():
        out["state"][i] = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in s.items()}
    return out


@pytest.mark.parametrize("kind,kw", [("adam", dict(lr=0.01, weight_decay=1e-3)), ("sgd", dict(lr=0.05, momentum=0.9))])
def test_a_torch_checkpoint_continues_on_the_gpu(kind, kw):
    first = run_torch(kind, torch.float64, kw, steps=2)
    start = {"params": first["params"], "sd": cpu_state_dict(first["opt"].state_dict())}
    r64 = run_torch(kind, torch.float64, kw, steps=2, first_step=2, start=start)
    r32 = run_torch(kind, torch.float32, kw, steps=2, first_step=2, start=start)
    got = run_fused(kind, kw, steps=2, first_step=2, start=start)
    compare(kind, got, r64, r32, tag="torch -> fused: ")
    straight = run_torch(kind, torch.float64, kw, steps=4)
    same = all(torch.equal(a, b) for a, b in zip(straight["params"], r64["params"]))
    assert same, "the fp64 continuation is the straight fp64 run"


@pytest.mark.parametrize("kind,kw", [("adam", dict(lr=0.01, weight_decay=1e-3)), ("sgd", dict(lr=0.05, momentum=0.9))])
def test_a_gpu_checkpoint_continues_in_torch(kind, kw):
    """the state_dict() goes to torch AS IT COMES, through torch.save / torch.load: torch's Adam keeps loaded `step` tensors as they are and
    increments each parameter's in place, so a step tensor shared by the parameters would count once per parameter and step"""
    import io
    first = run_fused(kind, kw, steps=2)
    buf = io.BytesIO()
    torch.save(first["opt"].state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    if kind == "adam":
        steps = [s["step"] for s in sd["state"].values()]
        assert all(float(t) == 2.0 for t in steps) and len({t.data_ptr() for t in steps}) == len(steps)
    start = {"params": [p.cpu().double() for p in first["params"]], "sd": sd}
    r64 = run_torch(kind, torch.float64, kw, steps=2, first_step=2, start=start)
    r32 = run_torch(kind, torch.float32, kw, steps=2, first_step=2, start=start)
    got = run_fused(kind, kw, steps=2, first_step=2, start=start)
    if kind == "adam":
        for r in (r64, r32):
            assert [float(s["step"]) for s in r["opt"].state.values()] == [4.0] * len(r["opt"].state)
        live = first["opt"]
        assert all(float(live.state[p]["step"]) == 2.0 for g in live.param_groups for p in g["params"])       # ours did not move
    compare(kind, got, r64, r32, tag="fused -> torch: ")


# ---- version counter and caches
def test_step_bumps_versions_and_the_folded_cache_follows():
    from disprcnn_amd.modeling.pointnet_module.point_rcnn.lib.pointnet2_lib.pointnet2 import pytorch_utils as PU
    from disprcnn_amd.solver import FusedSGD
    torch.manual_seed(0)
    conv = PU.Conv1d(4, 6).eval().to(DEV)
    idle = torch.nn.Parameter(torch.ones(5, device=DEV))                     # in the optimizer, never given a gradient
    before = conv.folded()
    assert conv.folded() is before
    w, b = conv.conv.weight, conv.conv.bias
    w.grad, b.grad = torch.ones_like(w), torch.ones_like(b)
    opt = FusedSGD([w, b, idle], lr=0.25)
    v0 = (w._version, b._version, idle._version)
    w_old = w.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert w._version > v0[0] and b._version > v0[1] and idle._version == v0[2]
    assert torch.equal(idle, torch.ones(5, device=DEV)) and idle.grad is None and idle not in opt.state
    assert torch.equal(w, w_old - 0.25)
    after = conv.folded()
    assert after is not before
    assert torch.equal(after.wt, w.detach().reshape(6, 4).t())
    assert not torch.equal(after.wt, before.wt) and torch.equal(after.bias.float(), b.detach())


# ---- RCNNNet end to end
def test_rcnn_net_trains_with_make_optimizer():
    from disprcnn_amd.solver import FusedSGD, compute_losses, make_lr_scheduler, make_optimizer
    from tests import test_hip_rcnn_train as RT
    import warnings
    net = RT.new_net().train()
    cfg = SO.solver_cfg(BASE_LR=0.01, WEIGHT_DECAY=1e-4, OPTIMIZER="SGD", SCHEDULER="WarmupMultiStepLR")
    opt, uncert = make_optimizer(cfg, net)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make_lr_scheduler(cfg, opt)
    assert type(opt) is FusedSGD and uncert is None and len(opt.param_groups) == len(list(net.parameters()))
    prop = RT.proposals(RT.train_inputs())
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    losses = []
    for _ in range(2):
        opt.zero_grad()
        _, loss_dict = net(prop)
        loss = compute_losses(loss_dict, cfg, uncert)
        loss.backward()
        norm = opt.clip_grad_norm_(10.0)
        opt.step()
        sched.step()
        losses.append(loss.item())
        assert np.isfinite(norm.item()) and norm.item() > 0
        if len(losses) == 1:
            for k, p in net.named_parameters():
                assert p.grad is not None, k
                assert bool(torch.isfinite(p).all()), k
                assert not torch.equal(p.detach(), start[k]), f"{k} did not change"
    print("losses", losses)
    assert all(np.isfinite(v) for v in losses)
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())

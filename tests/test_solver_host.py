"""The solver's host side, without a GPU: the schedules and the group layout against the reference's recording
(tests/golden/solver_golden.npz, made by tests/golden/make_golden_solver.py), the alias imports, the chunk table, the checkpoint
layout, the refusals and the C ABI's arity."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import solver_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
G = np.load(os.path.join(HERE, "golden", "solver_golden.npz"))


@pytest.mark.parametrize("name", sorted(SO.SCHED_CASES))
def test_schedules_equal_the_reference_recording(name):
    from disprcnn_amd.solver import lr_scheduler as LS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lr, mom = SO.walk_schedule(name, LS, torch.optim.SGD, torch.optim.Adam)
    ref_lr, ref_mom = G[f"sched_{name}_lr"], G[f"sched_{name}_mom"]
    assert lr.shape == ref_lr.shape and lr.shape[0] == SO.SCHED_CASES[name][3] + 1 and lr.shape[1] == 2
    print(name, "max rel lr", np.abs(lr / ref_lr - 1).max(), "momentum", np.abs(mom / ref_mom - 1).max())
    np.testing.assert_allclose(lr, ref_lr, rtol=1e-12, atol=0)
    np.testing.assert_allclose(mom, ref_mom, rtol=1e-12, atol=0)


def test_the_recording_crosses_every_branch():
    """warm-up ends, milestones, the one-cycle's turn: the recorded values themselves show them"""
    lin = G["sched_warm_linear_lr"][:, 0]
    assert lin[0] == pytest.approx(0.02 / 3) and lin[4] == 0.02 and lin[6] == pytest.approx(0.002) and lin[9] == pytest.approx(0.0002)
    assert np.all(np.diff(lin[:5]) > 0)
    con = G["sched_warm_constant_lr"][:, 1]
    assert con[0] == pytest.approx(0.05 * 0.25) and con[2] == pytest.approx(0.05 * 0.25 * 0.5) and con[3] == pytest.approx(0.025)
    one, mom = G["sched_onecycle_sgd_lr"][:, 0], G["sched_onecycle_sgd_mom"][:, 0]
    assert one.argmax() == 2 and mom.argmin() == 2 and one.max() == pytest.approx(0.01) and mom.min() == pytest.approx(0.85)
    assert len(set(G["sched_onecycle_fixed_momentum_mom"][:, 0])) == 1


def test_schedulers_accept_the_fused_optimizers_and_refuse_others():
    from disprcnn_amd.solver import FusedAdam, FusedSGD, OneCycleScheduler, WarmupMultiStepLR
    p = [torch.nn.Parameter(torch.zeros(3))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sgd = FusedSGD(p, 0.1, momentum=0.9)
        s = OneCycleScheduler(sgd, 0.1, 10)
        assert not s.cycles_beta1 and sgd.param_groups[0]["momentum"] != 0.9
        adam = FusedAdam(p, 0.1)
        assert OneCycleScheduler(adam, 0.1, 10).cycles_beta1 and adam.param_groups[0]["betas"][1] == 0.999
        assert adam.param_groups[0]["betas"][0] != 0.9
        WarmupMultiStepLR(FusedSGD(p, 0.1), (3, 5))
    with pytest.raises(TypeError):
        OneCycleScheduler(object(), 0.1, 10)
    with pytest.raises(ValueError):
        WarmupMultiStepLR(sgd, (5, 3))
    with pytest.raises(ValueError):
        WarmupMultiStepLR(sgd, (3, 5), warmup_method="cosine")
    with pytest.raises(ValueError):
        OneCycleScheduler(sgd, 0.1, 10, base_momentum=[0.8, 0.9])


@pytest.mark.parametrize("name", sorted(SO.LAYOUT_CASES))
def test_make_optimizer_reproduces_the_recorded_group_layout(name):
    from disprcnn_amd.solver import FusedAdam, FusedSGD, make_optimizer
    over = SO.LAYOUT_CASES[name]
    opt, uncert = make_optimizer(SO.solver_cfg(**over), SO.small_model())
    assert type(opt) is (FusedSGD if over["OPTIMIZER"] == "SGD" else FusedAdam) and isinstance(opt, torch.optim.Optimizer)
    got = SO.layout_of(opt, uncert)
    for k, v in got.items():
        np.testing.assert_array_equal(v, G[f"layout_{name}_{k}"], err_msg=f"{name} {k}")
    if over["UNCERT_LOSS_WEIGHT"]:
        assert uncert.requires_grad and uncert.is_leaf and opt.param_groups[-1]["params"][0] is uncert
        assert opt.param_groups[-1]["weight_decay"] == 0 and torch.equal(uncert.detach(), torch.full((3,), -1.0))
    else:
        assert uncert is None
    # the frozen parameter is in no group
    assert 7 not in got["numel"].tolist()


def test_unknown_optimizer_and_scheduler_are_not_implemented():
    from disprcnn_amd.solver import FusedSGD, make_lr_scheduler, make_optimizer
    with pytest.raises(NotImplementedError):
        make_optimizer(SO.solver_cfg(OPTIMIZER="RMSprop"), SO.small_model())
    opt = FusedSGD([torch.nn.Parameter(torch.zeros(2))], 0.1, momentum=0.9)
    with pytest.raises(NotImplementedError):
        make_lr_scheduler(SO.solver_cfg(SCHEDULER="CosineAnnealingLR"), opt)
    from disprcnn_amd.solver import OneCycleScheduler, WarmupMultiStepLR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = make_lr_scheduler(SO.solver_cfg(), opt)
        o = make_lr_scheduler(SO.solver_cfg(SCHEDULER="OneCycleScheduler"), opt)
    assert type(w) is WarmupMultiStepLR and (w.milestones, w.gamma, w.warmup_iters, w.warmup_method) == ((6, 9), 0.1, 4, "linear")
    assert type(o) is OneCycleScheduler and o.total_steps == 10 and o.max_lrs == [0.01]


def test_reference_import_names_resolve_to_the_same_objects():
    from disprcnn.solver import make_lr_scheduler, make_optimizer
    from disprcnn.solver.lr_scheduler import OneCycleScheduler, WarmupMultiStepLR
    import disprcnn_amd.solver as real
    import disprcnn_amd.solver.lr_scheduler as real_ls
    assert make_optimizer is real.make_optimizer and make_lr_scheduler is real.make_lr_scheduler
    assert WarmupMultiStepLR is real_ls.WarmupMultiStepLR and OneCycleScheduler is real_ls.OneCycleScheduler
    import disprcnn.solver
    assert disprcnn.solver is real


def test_chunk_table_covers_every_element_once_in_a_fixed_order():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib
    from disprcnn_amd.solver.fused import chunk_table, state_offsets
    CH = _lib.lib().drc_solver_chunk()
    assert CH >= 256 and CH % 4 == 0
    numels = [1, 0, CH - 1, CH, CH + 1, 2 * CH + 3, 5]
    has_grad = [True, True, True, True, True, True, False]            # the last one has no gradient
    table = chunk_table(numels, has_grad, CH)
    assert table == chunk_table(numels, has_grad, CH) and table == sorted(table)
    seen = [np.zeros(n, np.int64) for n in numels]
    for t, s in table:
        assert s % CH == 0 and 0 <= s < numels[t]
        seen[t][s:s + CH] += 1
    for t, (n, gr) in enumerate(zip(numels, has_grad)):
        assert np.all(seen[t] == (1 if gr else 0)), t
    assert [t for t, _ in table] == [0, 2, 3, 4, 4, 5, 5, 5]
    offs, total = state_offsets(numels)
    assert all(o % 4 == 0 for o in offs) and total % 4 == 0
    assert all(o + n <= o2 for o, n, o2 in zip(offs, numels, offs[1:] + [total]))         # no two tensors share state


def _stepped(cls, params, **kw):
    """a torch optimizer after one step on seeded gradients"""
    opt = cls(params, **kw)
    g = torch.Generator().manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    opt.step()
    return opt


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_state_dict_has_torchs_keys_and_shapes(kind):
    from disprcnn_amd.solver import FusedAdam, FusedSGD
    shapes = [(3, 2), (5,), (1,)]
    tp = [torch.nn.Parameter(torch.ones(s)) for s in shapes]
    fp = [torch.nn.Parameter(torch.ones(s)) for s in shapes]
    if kind == "sgd":
        fresh_t, fused = torch.optim.SGD(tp, lr=0.1, momentum=0.9, weight_decay=1e-4), FusedSGD(fp, lr=0.1, momentum=0.9, weight_decay=1e-4)
    else:
        fresh_t, fused = torch.optim.Adam(tp, lr=0.1, weight_decay=1e-4), FusedAdam(fp, lr=0.1, weight_decay=1e-4)
    a, b = fresh_t.state_dict(), fused.state_dict()
    assert a["state"] == b["state"] == {}                                       # torch creates its state in the first step; so do we
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert a["param_groups"] == b["param_groups"]
    # a stepped torch checkpoint goes in and comes out with the same keys, shapes and values, as views of the flat buffers
    stepped = _stepped(type(fresh_t), tp, **{k: v for k, v in fresh_t.defaults.items() if k in ("lr", "momentum", "weight_decay")})
    sd = stepped.state_dict()
    fused.load_state_dict(sd)
    out = fused.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"]) and out["param_groups"] == sd["param_groups"]
    for i in sd["state"]:
        assert sorted(out["state"][i]) == sorted(sd["state"][i])
        for k, v in sd["state"][i].items():
            w = out["state"][i][k]
            assert w.shape == v.shape and w.dtype == v.dtype and torch.equal(w, v), (i, k)
    names = ("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq")
    for name in names:
        flat = fused._flat[name]
        assert all(fused.state[p][name].untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for p in fp)
        assert all(fused.state[p][name].data_ptr() % 16 == flat.data_ptr() % 16 for p in fp)       # offsets are multiples of 4 floats
    # and torch takes ours
    back = type(fresh_t)([torch.nn.Parameter(torch.ones(s)) for s in shapes], lr=0.1)
    back.load_state_dict(out)
    for i, p in enumerate(back.param_groups[0]["params"]):
        for name in names:
            assert torch.equal(back.state[p][name], sd["state"][i][name])
    if kind == "adam":
        _adam_state_dict_hands_out_one_step_tensor_per_parameter()


def _adam_state_dict_hands_out_one_step_tensor_per_parameter():
    """torch.optim.Adam keeps loaded `step` tensors as they are and increments each in place: a step tensor shared by the parameters
    would advance once per parameter"""
    import io
    from disprcnn_amd.solver import FusedAdam
    shapes = [(3, 2), (5,), (1,), (4,)]
    tp = [torch.nn.Parameter(torch.ones(s)) for s in shapes]
    fused = FusedAdam([torch.nn.Parameter(torch.ones(s)) for s in shapes], lr=0.1)
    fused.load_state_dict(_stepped(torch.optim.Adam, tp, lr=0.1).state_dict())
    sd = fused.state_dict()
    steps = [s["step"] for s in sd["state"].values()]
    assert len(steps) == 4 and all(float(t) == 1.0 and t.dtype == torch.float32 and t.device.type == "cpu" for t in steps)
    assert len({t.data_ptr() for t in steps}) == 4
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    for loaded in (sd, torch.load(buf)):
        ps = [torch.nn.Parameter(torch.ones(s)) for s in shapes]
        back = torch.optim.Adam(ps, lr=0.1)
        back.load_state_dict(loaded)
        for p in ps:
            p.grad = torch.ones_like(p)
        back.step()
        assert [float(back.state[p]["step"]) for p in ps] == [2.0] * 4
    assert all(float(fused.state[p]["step"]) == 1.0 for p in fused.param_groups[0]["params"])      # ours did not move


def _groups_are_fixed_at_construction():
    from disprcnn_amd.solver import FusedAdam, FusedSGD
    for cls in (FusedSGD, FusedAdam):
        opt = cls([{"params": [torch.nn.Parameter(torch.ones(3))]}, {"params": [torch.nn.Parameter(torch.ones(2))], "lr": 0.5}], lr=0.1)
        assert len(opt.param_groups) == 2
        with pytest.raises(NotImplementedError, match="add_param_group"):
            opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(4))]})
        assert len(opt.param_groups) == 2


def test_step_on_cpu_parameters_raises():
    from disprcnn_amd.solver import FusedAdam, FusedSGD
    for cls in (FusedSGD, FusedAdam):
        p = torch.nn.Parameter(torch.ones(4))
        p.grad = torch.ones(4)
        opt = cls([p], lr=0.1)
        with pytest.raises(RuntimeError, match="GPU only"):
            opt.step()
        with pytest.raises(RuntimeError, match="GPU only"):
            opt.clip_grad_norm_(1.0)
        assert torch.equal(p.detach(), torch.ones(4))


def test_what_is_not_built_raises():
    from disprcnn_amd.solver import FusedAdam, FusedSGD
    p = [torch.nn.Parameter(torch.ones(4))]
    for make in (lambda: FusedSGD(p, 0.1, momentum=0.9, nesterov=True), lambda: FusedSGD(p, 0.1, momentum=0.9, dampening=0.1),
                 lambda: FusedSGD(p, 0.1, maximize=True), lambda: FusedAdam(p, 0.1, amsgrad=True), lambda: FusedAdam(p, 0.1, maximize=True)):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(ValueError):
        FusedSGD([torch.nn.Parameter(torch.ones(4, dtype=torch.float64))], 0.1)
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.ones(4, dtype=torch.float16))], 0.1)
    with pytest.raises(ValueError):
        FusedSGD([torch.nn.Parameter(torch.ones(4, 6).t())], 0.1)
    # a value smuggled in through a group is refused where it would be used
    opt = FusedSGD(p, 0.1, momentum=0.9)
    opt.param_groups[0]["nesterov"] = True
    with pytest.raises(NotImplementedError):
        opt.push_hyper()
    _groups_are_fixed_at_construction()


def test_zero_grad_zeroes_in_place():
    from disprcnn_amd.solver import FusedSGD
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2)), torch.nn.Parameter(torch.ones(1))]
    flat = torch.full((9,), 7.0)
    ps[0].grad, ps[1].grad = flat[1:4], flat[4:8].view(2, 2)                    # tile flat[1:8]; ps[2] has no gradient
    opt = FusedSGD(ps, 0.1)
    ptrs = [p.grad.data_ptr() for p in ps[:2]]
    opt.zero_grad()
    assert flat.tolist() == [7.0] + [0.0] * 7 + [7.0] and ps[2].grad is None and [p.grad.data_ptr() for p in ps[:2]] == ptrs
    ps[0].grad, ps[1].grad = torch.ones(3), flat[4:8].view(2, 2).fill_(3.0)     # separate storages
    opt.zero_grad()
    assert not ps[0].grad.any() and not ps[1].grad.any() and flat[8] == 7.0
    opt.zero_grad(set_to_none=True)
    assert ps[0].grad is None and ps[1].grad is None


def test_header_and_bindings_agree_for_the_solver_symbols():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib, build
    assert "solver.hip" in build.SOURCES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "disprcnn_pts.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "solver.hip")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    names = [n for n in _lib.EXPORTED_SYMBOLS if n.startswith("drc_solver_")]
    assert sorted(names) == ["drc_solver_adam_step", "drc_solver_chunk", "drc_solver_grad_norm", "drc_solver_prepare", "drc_solver_sgd_step"]
    assert sorted(set(re.findall(r"\b(drc_solver_\w+)\s*\(", header))) == sorted(names)
    for name in names:
        assert hasattr(handle, name)
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        defn = re.search(r"\bint\s+%s\s*\(([^{;]*?)\)\s*\{" % name, src, re.S)
        assert decl and defn, name
        n_args = 0 if decl.group(1).strip() == "void" else len(decl.group(1).split(","))
        assert n_args == (0 if defn.group(1).strip() == "void" else len(defn.group(1).split(","))) == len(_lib._SIGS[name][1]), name
    for banned in ("hipMalloc", "hipMemcpy", "Synchronize", "atomicAdd", "atomicCAS"):
        assert banned not in src


def test_c_entries_refuse_bad_arguments_before_a_launch():
    import __graft_entry__ as g
    g.build()
    from disprcnn_amd.pts import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    a = ctypes.addressof(buf)
    assert L.drc_solver_grad_norm(-1, 1, a, a, a, None) == -1 and L.drc_solver_grad_norm(1, 1, None, a, a, None) == -1
    assert L.drc_solver_grad_norm(0, 0, None, None, None, None) == 0                       # nothing to do
    assert L.drc_solver_prepare(0, None, 8, 1.0, 1, 0, a, a, a, a, None) == -1             # an unknown flag
    assert L.drc_solver_prepare(1, None, 1, 1.0, 1, 0, a, a, a, a, None) == -1             # the norm without partials
    assert L.drc_solver_prepare(1, a, 1, -1.0, 1, 0, a, a, a, a, None) == -1 and L.drc_solver_prepare(1, a, 1, float("nan"), 1, 0, a, a, a, a, None) == -1
    assert L.drc_solver_prepare(0, None, 4, 0.0, 1, 1, None, a, a, a, None) == -1          # Adam without its tables
    assert L.drc_solver_sgd_step(1, 1, 1, a, a, None, a, None, 0, None) == -1 and L.drc_solver_sgd_step(0, 0, 0, None, None, None, None, None, 0, None) == 0
    assert L.drc_solver_adam_step(1, 1, 1, a, a, a, a, a, None, a, 0, None) == -1 and L.drc_solver_adam_step(1, 1, 0, a, a, a, a, a, a, a, 0, None) == -1


@pytest.mark.parametrize("n", [0, 3])
def test_compute_losses_is_the_reference_formula(n):
    from disprcnn_amd.solver import compute_losses
    rs = np.random.RandomState(3)
    vals = rs.uniform(0.1, 2.0, 3)
    losses = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in zip(("loss_a", "loss_b", "loss_c"), vals)}
    cfg = SO.solver_cfg(UNCERT_LOSS_WEIGHT=n)
    if n == 0:
        got = compute_losses(losses, cfg, None)
        assert got.item() == pytest.approx(vals.sum(), rel=1e-15)
        return
    u = rs.uniform(-1.0, 1.0, 3)
    uncert = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    got = compute_losses(losses, cfg, uncert)
    assert got.item() == pytest.approx(u.sum() + (vals * np.exp(-u)).sum(), rel=1e-14)
    got.backward()
    np.testing.assert_allclose(uncert.grad.numpy(), 1 - vals * np.exp(-u), rtol=1e-13)
    np.testing.assert_allclose([losses[k].grad.item() for k in losses], np.exp(-u), rtol=1e-13)
    with pytest.raises(AssertionError):
        compute_losses({"only": losses["loss_a"]}, cfg, uncert)

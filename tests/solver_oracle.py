"""What the solver's golden recorder (tests/golden/make_golden_solver.py, run on the reference) and the solver's tests share: the small
named model, the config, the schedule cases and the protocol that walks a scheduler.  Pure torch on the CPU."""
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

BASE_LRS = (0.02, 0.05)          # two groups, so that per-group values cannot be mixed up


def small_model():
    """Names with and without "bias", one parameter that does not require grad."""
    torch.manual_seed(0)
    m = nn.Sequential()
    m.add_module("conv", nn.Conv1d(3, 4, 1))
    m.add_module("bn", nn.BatchNorm1d(4))
    m.add_module("head", nn.Linear(4, 2))
    m.register_parameter("bias_scale", nn.Parameter(torch.ones(5)))           # "bias" inside a longer name counts too
    m.register_parameter("frozen", nn.Parameter(torch.ones(7), requires_grad=False))
    return m


def solver_cfg(**over):
    s = dict(BASE_LR=0.01, BIAS_LR_FACTOR=2, WEIGHT_DECAY=1e-4, WEIGHT_DECAY_BIAS=0.0, MOMENTUM=0.9, UNCERT_LOSS_WEIGHT=0, OPTIMIZER="SGD",
             SCHEDULER="WarmupMultiStepLR", STEPS=(6, 9), GAMMA=0.1, WARMUP_FACTOR=1.0 / 3, WARMUP_ITERS=4, WARMUP_METHOD="linear",
             MAX_ITER=10)
    s.update(over)
    return SimpleNamespace(SOLVER=SimpleNamespace(**s))


LAYOUT_CASES = {"sgd_uncert3": dict(OPTIMIZER="SGD", UNCERT_LOSS_WEIGHT=3), "adam": dict(OPTIMIZER="Adam", UNCERT_LOSS_WEIGHT=0)}

# name -> (scheduler, optimizer kind, keyword arguments, iterations).  Together they cross: the end of a linear and of a constant warm-up,
# each milestone, a milestone inside the warm-up, the turn of the one-cycle at pct_start (on and between iterations), a resume of each.
SCHED_CASES = {
    "constant": ("ConstantScheduler", "sgd", dict(), 3),
    "warm_linear": ("WarmupMultiStepLR", "sgd", dict(milestones=(6, 9), gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=4,
                                                     warmup_method="linear"), 12),
    "warm_constant": ("WarmupMultiStepLR", "sgd", dict(milestones=(2, 7), gamma=0.5, warmup_factor=0.25, warmup_iters=3,
                                                       warmup_method="constant"), 9),
    "warm_resume": ("WarmupMultiStepLR", "sgd", dict(milestones=(6, 9), gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=8,
                                                     warmup_method="linear", last_epoch=4), 7),
    "onecycle_sgd": ("OneCycleScheduler", "sgd", dict(max_lr=0.01, total_steps=10), 10),
    "onecycle_adam": ("OneCycleScheduler", "adam", dict(max_lr=0.03, total_steps=7, pct_start=0.4, div_factor=10.0,
                                                        final_div_factor=50.0, base_momentum=0.8, max_momentum=0.9), 7),
    "onecycle_fixed_momentum": ("OneCycleScheduler", "sgd", dict(max_lr=0.02, total_steps=6, cycle_momentum=False), 6),
    "onecycle_resume": ("OneCycleScheduler", "adam", dict(max_lr=0.01, total_steps=10, last_epoch=3), 6),
}


def walk_schedule(name, schedulers, make_sgd, make_adam):
    """-> (lr [n + 1, G], momentum [n + 1, G]) as float64: the groups' values after the scheduler's construction and after each of n
    iterations of ``optimizer.step(); scheduler.step()``.  `schedulers` is a module or namespace with the three classes."""
    cls, kind, kw, n = SCHED_CASES[name]
    params = [nn.Parameter(torch.zeros(2)), nn.Parameter(torch.zeros(3))]
    groups = [{"params": [p], "lr": lr} for p, lr in zip(params, BASE_LRS)]
    opt = make_sgd(groups, BASE_LRS[0], momentum=0.9) if kind == "sgd" else make_adam(groups, BASE_LRS[0])
    if kw.get("last_epoch", -1) != -1:                  # a resumed run: the checkpointed optimizer carries its initial rates
        for g, lr in zip(opt.param_groups, BASE_LRS):
            g["initial_lr"] = lr
    sched = getattr(schedulers, cls)(opt, **kw)

    def read():
        return ([float(g["lr"]) for g in opt.param_groups],
                [float(g["momentum"] if kind == "sgd" else g["betas"][0]) for g in opt.param_groups])
    rows = [read()]
    for _ in range(n):
        opt.step()
        sched.step()
        rows.append(read())
    return np.array([r[0] for r in rows], np.float64), np.array([r[1] for r in rows], np.float64)


def layout_of(optimizer, uncert):
    """The group layout as arrays: per group lr, weight decay, momentum | beta1, the parameter's numel; the defaults' lr; uncert."""
    gs = optimizer.param_groups
    assert all(len(g["params"]) == 1 for g in gs)
    return {"lr": np.array([g["lr"] for g in gs], np.float64), "weight_decay": np.array([g["weight_decay"] for g in gs], np.float64),
            "momentum": np.array([g["momentum"] if "momentum" in g else g["betas"][0] for g in gs], np.float64),
            "numel": np.array([g["params"][0].numel() for g in gs], np.int64), "default_lr": np.float64(optimizer.defaults["lr"]),
            "uncert": np.zeros(0, np.float32) if uncert is None else uncert.detach().cpu().numpy()}

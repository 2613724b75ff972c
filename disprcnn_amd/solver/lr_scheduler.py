"""Learning-rate schedules of the reference's configs (reference: solver/lr_scheduler.py), restated: a constant one, multi-step decay behind
a warm-up, and the one-cycle policy with cosine annealing that also cycles the momentum (SGD) or beta1 (Adam) against the rate.

All three are ``_LRScheduler``s: they write ``param_groups[i]['lr']`` (and the momentum) on the host.  With FusedSGD / FusedAdam those
values reach the kernels through ``optimizer.push_hyper()``, which ``step()`` calls itself and a captured step needs between replays.
tests/golden/solver_golden.npz holds the reference's values per iteration.
"""
import math
from bisect import bisect_right

from torch.optim import Optimizer
from torch.optim.lr_scheduler import _LRScheduler


class ConstantScheduler(_LRScheduler):
    def __init__(self, optimizer, last_epoch=-1):
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return self.base_lrs


class WarmupMultiStepLR(_LRScheduler):
    """base_lr * gamma^(milestones passed), times a warm-up factor during the first `warmup_iters` iterations: `warmup_factor` itself
    ("constant") or the line from `warmup_factor` at iteration 0 to 1 at `warmup_iters` ("linear")."""

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=500, warmup_method="linear", last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError(f"milestones must be increasing integers, got {milestones}")
        if warmup_method not in ("constant", "linear"):
            raise ValueError(f"warmup_method must be 'constant' or 'linear', got {warmup_method}")
        self.milestones = milestones
        self.gamma = gamma
        self.warmup_factor = warmup_factor
        self.warmup_iters = warmup_iters
        self.warmup_method = warmup_method
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        it = self.last_epoch
        factor = 1
        if it < self.warmup_iters:
            if self.warmup_method == "constant":
                factor = self.warmup_factor
            else:
                alpha = float(it) / self.warmup_iters
                factor = self.warmup_factor * (1 - alpha) + alpha
        decay = self.gamma ** bisect_right(self.milestones, it)
        return [base * factor * decay for base in self.base_lrs]


def annealing_cos(start, end, pct):
    """Half a cosine from `start` (pct 0) to `end` (pct 1)."""
    return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)


class OneCycleScheduler(_LRScheduler):
    """One cycle over `total_steps` iterations: the rate climbs on a half cosine from max_lr / div_factor to max_lr during the first
    `pct_start` of them and falls to max_lr / final_div_factor (default div_factor * 1e4) over the rest.  With `cycle_momentum` the
    group's momentum -- 'momentum' where the optimizer has one, else betas[0] -- moves the other way between max_momentum and
    base_momentum.  Call ``step()`` once per iteration.  `max_lr` is one number for all groups (as in the reference); the two momentum
    bounds may be lists with one value per group."""

    def __init__(self, optimizer, max_lr, total_steps, pct_start=0.3, div_factor=25.0, final_div_factor=None, cycle_momentum=True,
                 base_momentum=0.85, max_momentum=0.95, last_epoch=-1):
        if not isinstance(optimizer, Optimizer):
            raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
        self.optimizer = optimizer                           # the momentum helpers below need it before the base class stores it
        groups = optimizer.param_groups
        fresh = last_epoch == -1                             # a resumed run keeps what the checkpointed groups hold
        if final_div_factor is None:
            final_div_factor = div_factor * 1e4
        self.total_steps = total_steps
        self.pct_start = pct_start
        self.steps_up = float(total_steps * pct_start)
        self.steps_down = float(total_steps - self.steps_up)
        self.max_lrs = [max_lr] * len(groups)
        self.end_lrs = [max_lr / final_div_factor] * len(groups)
        if fresh:
            for g in groups:
                g["lr"] = max_lr / div_factor
        self.cycle_momentum = cycle_momentum
        if cycle_momentum:
            if "momentum" not in optimizer.defaults and "betas" not in optimizer.defaults:
                raise ValueError("cycle_momentum needs an optimizer with a momentum or betas")
            self.cycles_beta1 = "momentum" not in optimizer.defaults
            if fresh:
                for g, m in zip(groups, self._per_group("base_momentum", base_momentum, len(groups))):
                    self._set_momentum(g, m)
            self.base_momentums = [self._get_momentum(g) for g in groups]
            self.max_momentums = self._per_group("max_momentum", max_momentum, len(groups))
        super().__init__(optimizer, last_epoch)

    @staticmethod
    def _per_group(name, value, n):
        if isinstance(value, (list, tuple)):
            if len(value) != n:
                raise ValueError(f"expected {n} values for {name}, got {len(value)}")
            return list(value)
        return [value] * n

    def _get_momentum(self, group):
        return group["betas"][0] if self.cycles_beta1 else group["momentum"]

    def _set_momentum(self, group, value):
        if self.cycles_beta1:
            group["betas"] = (value, group["betas"][1])
        else:
            group["momentum"] = value

    def get_lr(self):
        """The rates of iteration last_epoch + 1; with cycle_momentum it also writes that iteration's momentum into the groups."""
        it = self.last_epoch + 1
        rising = it / self.total_steps <= self.pct_start
        pct = it / self.steps_up if rising else (it - self.steps_up) / self.steps_down
        if rising:
            lrs = [annealing_cos(base, mx, pct) for base, mx in zip(self.base_lrs, self.max_lrs)]
        else:
            lrs = [annealing_cos(mx, end, pct) for mx, end in zip(self.max_lrs, self.end_lrs)]
        if self.cycle_momentum:
            for g, lo, hi in zip(self.optimizer.param_groups, self.base_momentums, self.max_momentums):
                self._set_momentum(g, annealing_cos(hi, lo, pct) if rising else annealing_cos(lo, hi, pct))
        return lrs

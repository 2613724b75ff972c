"""make_optimizer / make_lr_scheduler from the config (reference: solver/build.py) and the trainer's loss weighting
(reference: engine/trainer.py:44-51; `disprcnn_amd.engine` is a module, not a package, so compute_losses lives with the solver).

The optimizers are the fused HIP ones (solver/fused.py); the grouping rules are the reference's.
"""
import torch

from .fused import FusedAdam, FusedSGD
from .lr_scheduler import OneCycleScheduler, WarmupMultiStepLR


def make_optimizer(cfg, model):
    """-> (optimizer, uncert).  One group per parameter that requires grad, in named_parameters() order: a name containing "bias" gets
    BASE_LR * BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS, every other BASE_LR and WEIGHT_DECAY.  With SOLVER.UNCERT_LOSS_WEIGHT = n != 0,
    `uncert` is a leaf of n log-variances starting at -1 on the model's device, in a last group that names no weight decay (so it gets the
    optimizer's default, 0).  As in the reference, that group's rate and the optimizer's default rate are those of the LAST parameter."""
    s = cfg.SOLVER
    n_uncert = int(s.UNCERT_LOSS_WEIGHT)
    groups, lr, device = [], s.BASE_LR, None
    for name, p in model.named_parameters():
        device = p.device if device is None else device
        if not p.requires_grad:
            continue
        bias = "bias" in name
        lr = s.BASE_LR * s.BIAS_LR_FACTOR if bias else s.BASE_LR
        groups.append({"params": [p], "lr": lr, "weight_decay": s.WEIGHT_DECAY_BIAS if bias else s.WEIGHT_DECAY})
    uncert = None
    if n_uncert != 0:
        uncert = torch.full((n_uncert,), -1.0, dtype=torch.float32, device=device or "cpu", requires_grad=True)
        groups.append({"params": [uncert], "lr": lr})
    if s.OPTIMIZER == "SGD":
        return FusedSGD(groups, lr, momentum=s.MOMENTUM), uncert
    if s.OPTIMIZER == "Adam":
        return FusedAdam(groups, lr), uncert
    raise NotImplementedError(f"SOLVER.OPTIMIZER {s.OPTIMIZER!r}: 'SGD' and 'Adam' are built")


def make_lr_scheduler(cfg, optimizer):
    s = cfg.SOLVER
    if s.SCHEDULER == "WarmupMultiStepLR":
        return WarmupMultiStepLR(optimizer, s.STEPS, s.GAMMA, warmup_factor=s.WARMUP_FACTOR, warmup_iters=s.WARMUP_ITERS,
                                 warmup_method=s.WARMUP_METHOD)
    if s.SCHEDULER == "OneCycleScheduler":
        # the cycle spans MAX_ITER from iteration 0, also when training resumes later (as the reference)
        return OneCycleScheduler(optimizer, s.BASE_LR, s.MAX_ITER)
    raise NotImplementedError(f"SOLVER.SCHEDULER {s.SCHEDULER!r}: 'WarmupMultiStepLR' and 'OneCycleScheduler' are built")


def compute_losses(loss_dict, cfg, uncert):
    """The scalar the trainer back-propagates: the plain sum of the losses, or with UNCERT_LOSS_WEIGHT = n != 0 (n must be the number
    of losses) the uncertainty weighting  sum_i uncert_i + sum_i loss_i * exp(-uncert_i),  losses in the dict's order."""
    losses = list(loss_dict.values())
    n = cfg.SOLVER.UNCERT_LOSS_WEIGHT
    if n == 0:
        return sum(losses)
    assert n == len(losses), f"{n} != {len(losses)}"
    return uncert.sum() + sum(loss * torch.exp(-u) for loss, u in zip(losses, uncert))

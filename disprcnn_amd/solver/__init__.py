"""The solver: fused SGD / Adam steps with gradient clipping on HIP, and the reference's optimizer and schedule factories
(reference: disprcnn/solver)."""
from .build import compute_losses, make_lr_scheduler, make_optimizer
from .fused import FusedAdam, FusedSGD
from .lr_scheduler import ConstantScheduler, OneCycleScheduler, WarmupMultiStepLR

__all__ = ["make_optimizer", "make_lr_scheduler", "compute_losses", "FusedSGD", "FusedAdam", "ConstantScheduler", "WarmupMultiStepLR",
           "OneCycleScheduler"]

from .transforms import Compose, Normalize, RandomHorizontalFlip, Resize, ToTensor
from .build import build_transforms

__all__ = ["Compose", "Resize", "RandomHorizontalFlip", "ToTensor", "Normalize", "build_transforms"]

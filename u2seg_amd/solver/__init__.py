from .build import FlatSGD, WarmupLR, WarmupMultiStepLR, build_lr_scheduler, build_optimizer

__all__ = ["FlatSGD", "WarmupLR", "WarmupMultiStepLR", "build_lr_scheduler", "build_optimizer"]

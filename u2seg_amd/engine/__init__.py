from .precise_bn import get_bn_modules, precise_bn_due, update_bn_stats
from .trainer import SimpleTrainer, default_argument_parser, launch_info

__all__ = ["SimpleTrainer", "default_argument_parser", "get_bn_modules", "launch_info", "precise_bn_due", "update_bn_stats"]

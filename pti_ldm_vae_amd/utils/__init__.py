from .config import (load_vae_config, parse_config, read_config, resolve_ar_settings, resolve_bool,
                     resolve_guard_settings)
from .distributed import setup_ddp
from .eval_metrics import compute_psnr, compute_ssim, serialize_args
from .losses import ensure_three_channels
from .metrics import compute_regression_metrics

__all__ = ["compute_psnr", "compute_regression_metrics", "compute_ssim", "ensure_three_channels", "load_vae_config", "parse_config",
           "read_config", "resolve_ar_settings", "resolve_bool", "resolve_guard_settings", "serialize_args", "setup_ddp"]

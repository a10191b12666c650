"""Evaluation metrics with the reference's signatures (``src/pti_ldm_vae/utils/eval_metrics.py``): ``compute_psnr``,
``compute_ssim`` and ``serialize_args``.

Both metrics come out of ONE fused HIP pass (``ops.image_metrics`` -> ``pti_image_metrics``); a caller that wants
several of them per batch should call ``ops.image_metrics`` once instead (``evaluate_vae`` does).  Device tensors only:
CPU tensors are refused, there is no CPU/PyTorch fallback in this package.
"""
from __future__ import annotations

from typing import Any

import torch

from .. import _lib, ops


def _device_metrics(pred: torch.Tensor, target: torch.Tensor, who: str, **kw) -> torch.Tensor:
    if not (pred.is_cuda and target.is_cuda):
        raise _lib.PtiError(f"{who}: expected device tensors, got {pred.device} / {target.device}. "
                            "There is no CPU/PyTorch fallback for the evaluation metrics.")
    return ops.image_metrics(pred, target, **kw)


def compute_psnr(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """PSNR per sample of two ``[B, C, H, W]`` batches -> ``[B]`` on the inputs' device:
    ``10 log10(data_range^2 / max(mse, 1e-12))`` (eval_metrics.py:6-19).  The inputs are used as given (no clamp)."""
    return _device_metrics(pred, target, "compute_psnr", data_range=data_range)[:, 2]


def compute_ssim(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, k1: float = 0.01,
                 k2: float = 0.03) -> torch.Tensor:
    """SSIM per sample of two ``[B, C, H, W]`` batches -> ``[B]`` on the inputs' device: 11x11 Gaussian window, sigma
    1.5, zero padding without renormalisation at the border (eval_metrics.py:22-63).  The reference function runs for
    ``C == 1`` only; here ``C > 1`` means the same window applied to each channel on its own and the mean over all
    channels."""
    return _device_metrics(pred, target, "compute_ssim", data_range=data_range, k1=k1, k2=k2)[:, 3]


def serialize_args(args: Any) -> dict[str, Any]:
    """Parsed CLI arguments -> JSON-serialisable primitives (eval_metrics.py:66-83): path-like values become strings,
    lists and tuples become lists of strings, everything else is kept."""
    out: dict[str, Any] = {}
    for name, value in vars(args).items():
        if hasattr(value, "__fspath__"):
            value = str(value)
        elif isinstance(value, (list, tuple)):
            value = [str(v) for v in value]
        out[name] = value
    return out

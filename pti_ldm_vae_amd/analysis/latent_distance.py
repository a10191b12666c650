"""Euclidean distances between single latent vectors on the host (reference
``src/pti_ldm_vae/analysis/latent_distance.py``: same functions, checks and error texts).  Whole distance matrices belong
on the device: ``ops.latent_pairwise``."""
from __future__ import annotations

import numpy as np


def latent_distance(vec_a: np.ndarray, vec_b: np.ndarray) -> float:
    """Euclidean distance of two 1-D latent vectors of one shape."""
    if vec_a.ndim != 1 or vec_b.ndim != 1:
        raise ValueError(f"Expected 1D latent vectors, got shapes {vec_a.shape} and {vec_b.shape}")
    if vec_a.shape != vec_b.shape:
        raise ValueError(f"Latent vectors must have the same shape, got {vec_a.shape} and {vec_b.shape}")
    diff = vec_a - vec_b
    return float(np.sqrt(np.dot(diff, diff)))


def _check_index(name: str, idx: int, n: int) -> None:
    if not 0 <= idx < n:
        raise ValueError(f"{name} must be in [0, {n - 1}], got {idx}")


def latent_distance_from_indices(latents: np.ndarray, idx_a: int, idx_b: int) -> float:
    """Distance of rows ``idx_a`` and ``idx_b`` of one ``[N, D]`` group."""
    if latents.ndim != 2:
        raise ValueError(f"Expected latents of shape [N, D], got shape {latents.shape}")
    n = latents.shape[0]
    if not (0 <= idx_a < n and 0 <= idx_b < n):
        raise ValueError(f"indices must be in [0, {n - 1}], got {idx_a} and {idx_b}")
    return latent_distance(latents[idx_a], latents[idx_b])


def latent_distance_cross(latents_a: np.ndarray, idx_a: int, latents_b: np.ndarray, idx_b: int) -> float:
    """Distance of row ``idx_a`` of one ``[N, D]`` group and row ``idx_b`` of another."""
    if latents_a.ndim != 2 or latents_b.ndim != 2:
        raise ValueError(f"Expected 2D latents for both groups, got shapes {latents_a.shape} and {latents_b.shape}")
    if latents_a.shape[1] != latents_b.shape[1]:
        raise ValueError(f"Latent dimensions must match between groups, got {latents_a.shape[1]} and {latents_b.shape[1]}")
    _check_index("idx_a", idx_a, latents_a.shape[0])
    _check_index("idx_b", idx_b, latents_b.shape[0])
    return latent_distance(latents_a[idx_a], latents_b[idx_b])

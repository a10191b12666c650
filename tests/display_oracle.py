"""fp64 numpy restatement of ``pti_display_planes`` (test helper, like ``tests/eval_metrics_oracle.py``): the semantics
that ``include/pti_vae.h`` states for the display normalisation, written the slow and obvious way.

Per plane: the foreground is ``v != 0`` (``-0.0`` is background), it is SORTED, the two percentiles are numpy's linear
method spelled out in fp64 (``vi = (n - 1) q / 100``, ``lo = floor(vi)``, ``hi = min(lo + 1, n - 1)``,
``p = s[lo] + (s[hi] - s[lo]) (vi - lo)``), the map ``clip((v - p_low) / (p_high - p_low + 1e-8), 0, 1)`` is taken in
fp64 and rounded to fp32 once, values below ``1e-3`` (fp32) and the background become 0.  The canvas is built with
``np.rot90`` and ``np.concatenate``.  The reference's ``normalize_batch_for_display``
(``src/pti_ldm_vae/utils/visualization.py:6-40``, restated in ``pti_ldm_vae_amd/utils/visualization.py``) does the same
arithmetic in fp32; ``tests/test_display_cpu.py`` pins this file to it.

``case(seed, h, w)`` is the seeded generator of the tests: a z-scored ellipse on a zero background and a noisy copy of
it as the "reconstruction".
"""
from __future__ import annotations

import numpy as np

FLOOR = np.float32(1e-3)
NEAR_FLOOR = 1e-6      # a pixel whose value lies this close to FLOOR may fall on either side of it: left out of a comparison
MAX_LEFT_OUT = 4       # ... at most this many per plane


def percentile(sorted_values: np.ndarray, q: float) -> float:
    """numpy's ``method="linear"`` on an ascending fp32 vector, in fp64."""
    n = sorted_values.size
    vi = (n - 1) * float(q) / 100.0
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    s_lo, s_hi = float(sorted_values[lo]), float(sorted_values[hi])
    return s_lo + (s_hi - s_lo) * (vi - lo)


def plane_stats(plane: np.ndarray, low: float = 2, high: float = 98):
    """-> ``(n, p_low, p_high)`` of one fp32 plane; ``(0, 0.0, 0.0)`` without a foreground."""
    plane = np.asarray(plane, dtype=np.float32)
    values = np.sort(plane[plane != 0], kind="stable")
    if values.size == 0:
        return 0, 0.0, 0.0
    return int(values.size), percentile(values, low), percentile(values, high)


def normalize_plane(plane: np.ndarray, low: float = 2, high: float = 98) -> np.ndarray:
    """One fp32 ``[h, w]`` plane -> the mapped fp32 plane."""
    plane = np.asarray(plane, dtype=np.float32)
    n, p_low, p_high = plane_stats(plane, low, high)
    out = np.zeros(plane.shape, dtype=np.float32)
    if n == 0:
        return out
    foreground = plane != 0
    x = np.clip((plane.astype(np.float64) - p_low) / (p_high - p_low + 1e-8), 0.0, 1.0).astype(np.float32)
    out[foreground] = x[foreground]
    out[out < FLOOR] = 0.0
    return out


def to_uint8(canvas: np.ndarray) -> np.ndarray:
    """``(uint8)(x * 255.0f)``: the fp32 product, truncated."""
    return (np.asarray(canvas, dtype=np.float32) * np.float32(255.0)).astype(np.uint8)


def sources(a: np.ndarray, b: np.ndarray | None, nsrc: int):
    """The ``nsrc`` source batches ``[n, h, w]``: ``a``; ``a, b``; ``a, b, |a - b|`` (fp32 difference)."""
    a = np.asarray(a, dtype=np.float32)
    out = [a]
    if nsrc >= 2:
        b = np.asarray(b, dtype=np.float32)
        out.append(b)
    if nsrc == 3:
        out.append(np.abs(a - b))
    return out


def display_planes(a, b=None, nsrc=1, low=2, high=98, rot90=0):
    """-> ``(canvas fp32 [n, ho, nsrc * wo], stats fp64 [n, nsrc, 3])``."""
    srcs = sources(a, b, nsrc)
    n = srcs[0].shape[0]
    stats = np.zeros((n, nsrc, 3), dtype=np.float64)
    rows = []
    for i in range(n):
        parts = []
        for s, src in enumerate(srcs):
            stats[i, s] = plane_stats(src[i], low, high)
            parts.append(np.rot90(normalize_plane(src[i], low, high), k=rot90))
        rows.append(np.concatenate(parts, axis=1))
    return np.stack(rows), stats


def compare(got: np.ndarray, want: np.ndarray, tol: float = 1e-6):
    """Largest ``|got - want|`` over the pixels of ONE plane, leaving out those whose wanted value lies within
    ``NEAR_FLOOR`` of the floor -> ``(max abs error, number left out)``.  The caller asserts both."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    near = np.abs(want - float(FLOOR)) <= NEAR_FLOOR
    err = np.abs(got - want)[~near]
    return (float(err.max()) if err.size else 0.0), int(near.sum())


def case(seed: int, h: int, w: int, noise: float = 0.1):
    """-> ``(image, reconstruction)`` fp32 ``[h, w]``: normal noise inside an ellipse, z-scored over the ellipse, zero
    outside; the reconstruction adds ``noise`` * normal noise everywhere inside the ellipse."""
    rng = np.random.default_rng(seed)
    yy = np.linspace(-1.0, 1.0, h)[:, None] if h > 1 else np.zeros((1, 1))
    xx = np.linspace(-1.0, 1.0, w)[None, :] if w > 1 else np.zeros((1, 1))
    mask = (xx / 0.80) ** 2 + (yy / 0.64) ** 2 <= 1.0
    raw = rng.normal(size=(h, w)) + 2.0 * np.exp(-(xx ** 2 + yy ** 2) * 4.0)
    inside = raw[mask]
    std = inside.std() if inside.size > 1 and inside.std() > 0 else 1.0
    image = np.where(mask, (raw - inside.mean()) / std, 0.0).astype(np.float32)
    recon = np.where(mask, image + noise * rng.normal(size=(h, w)), 0.0).astype(np.float32)
    return image, recon

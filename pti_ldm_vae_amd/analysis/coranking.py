"""At which scale a 2-D projection of the latents can be believed: the co-ranking curves of Lee & Verleysen and a Shepard
figure, for every neighbourhood size at once.

``rho(i, j)`` is the rank of row ``j`` seen from row ``i`` in the latent space, ``r(i, j)`` the rank in the projection, both
``1 .. n - 1`` under ``projection_quality``'s order (distance, then column; -0 is 0).  Over the ordered pairs ``i != j`` and
with ``m = max(rho, r)``, three histograms: ``H_eq[m]`` (``rho = r``), ``H_in[m]`` (``r < rho``: an intrusion) and
``H_ex[m]`` (``rho < r``: an extrusion).  From their exact integer prefix sums, in fp64:

* ``Q_NX(K) = sum_{m <= K} (H_eq + H_in + H_ex)[m] / (K n)``: the mean share of the ``K`` nearest rows the two spaces have in
  common (``projection_quality``'s ``neighborhood_preservation``, for every ``K``);
* ``B_NX(K) = (sum_{m <= K} H_ex[m] - sum_{m <= K} H_in[m]) / (K n)``: positive where the projection tears neighbourhoods
  apart (extrusive), negative where it crushes them together (intrusive);
* ``R_NX(K) = ((n - 1) Q_NX(K) - K) / (n - 1 - K)``, ``K <= n - 2``: ``Q_NX`` rescaled so that a random projection scores 0;
* ``LCMC(K) = Q_NX(K) - K / (n - 1)``; ``K_max`` its lowest maximiser; ``Q_local`` / ``Q_global`` the means of ``Q_NX`` up to
  and past ``K_max``; ``AUC_logK = sum_K R_NX(K) / K  /  sum_K 1 / K``: one scale-free score.

Per row the Spearman coefficient ``1 - 6 S_i / (m (m^2 - 1))``, ``S_i = sum_j (rho - r)^2``, ``m = n - 1`` (exact in this
form: the keys have no ties); ``rank_correlation`` is its mean.  The Shepard figure: Kruskal's stress-1 at the best scale,
``sqrt(1 - (sum d_high d_low)^2 / (sum d_high^2 sum d_low^2))``, and a ``bins x bins`` histogram of the distance pairs.

On the device (csrc/coranking.hip): the two distance matrices as ``projection_quality`` forms them, ``ops.full_ranks`` on
each, ``ops.coranking_fold`` and ``ops.shepard_fold``; one packed copy brings 3 n + n + 3 n + bins^2 + 2 numbers to the
host.  The curves are functions of integers: exact, and the same bits on every run.  Limits: 4 .. 8192 rows, 2 .. 128 bins."""
from __future__ import annotations

import math

import numpy as np

MAX_ROWS, MIN_ROWS, MIN_BINS, MAX_BINS = 8192, 4, 2, 128


def curves_from_histograms(hist, n: int) -> dict:
    """``hist``: integers ``[3, n]`` (``H_eq``, ``H_in``, ``H_ex``; bin 0 is not used) -> ``Q_NX`` / ``B_NX`` / ``LCMC``
    (fp64 ``[n - 1]``, entry ``K - 1`` for ``K = 1 .. n - 1``), ``R_NX`` (``[n - 2]``), ``k_max``, ``q_local``, ``q_global``
    (``None`` when ``k_max = n - 1``) and ``auc_logk_rnx``.  Pure numpy."""
    n = int(n)
    hist = np.asarray(hist)
    if n < MIN_ROWS or hist.shape != (3, n):
        raise ValueError(f"curves_from_histograms: expected three histograms of n = {n} >= {MIN_ROWS} bins, got {hist.shape}")
    h = hist.astype(np.int64)
    if (h < 0).any() or h[:, 0].any() or int(h.sum()) != n * (n - 1):
        raise ValueError(f"curves_from_histograms: the histograms must hold the n (n - 1) = {n * (n - 1)} ordered pairs in "
                         f"bins 1 .. n - 1, got {int(h.sum())}")
    k = np.arange(1, n, dtype=np.int64)
    cum = np.cumsum(h[:, 1:], axis=1)                      # exact
    q = (cum[0] + cum[1] + cum[2]) / (k * n)
    b = (cum[2] - cum[1]) / (k * n)
    r = ((n - 1) * q[:-1] - k[:-1]) / (n - 1 - k[:-1])
    lcmc = q - k / (n - 1)
    k_max = int(np.argmax(lcmc)) + 1                       # the first of equal maxima
    return {"Q_NX": q, "B_NX": b, "R_NX": r, "LCMC": lcmc, "k_max": k_max,
            "q_local": math.fsum(q[:k_max]) / k_max,
            "q_global": math.fsum(q[k_max:]) / (n - 1 - k_max) if k_max < n - 1 else None,
            "auc_logk_rnx": math.fsum(r / k[:-1]) / math.fsum(1.0 / k[:-1])}


def stress_from_sums(sums):
    """``sums``: fp64 ``[n, 3]``, per row the sums of ``d_high^2``, ``d_low^2`` and ``d_high d_low`` -> Kruskal's stress-1 with
    the projection scaled to fit best (so its units do not matter), or ``None`` when either space has no extent or a sum
    is not finite.  The rows are folded by ``math.fsum``.  Pure numpy."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != 3:
        raise ValueError(f"stress_from_sums: expected [n, 3] sums, got {sums.shape}")
    hh, ll, hl = (math.fsum(sums[:, c]) for c in range(3))
    if not (math.isfinite(hh) and math.isfinite(ll) and math.isfinite(hl)) or hh <= 0.0 or ll <= 0.0:
        return None
    return math.sqrt(max(0.0, 1.0 - (hl * hl) / (hh * ll)))


def row_spearman(sqdiff, n: int) -> np.ndarray:
    """``S_i`` -> the Spearman coefficient of row ``i``'s two rankings of the other ``n - 1`` rows."""
    m = int(n) - 1
    return 1.0 - 6.0 * np.asarray(sqdiff, dtype=np.float64) / (m * (m * m - 1))


def curve_samples(n: int) -> list[int]:
    """The neighbourhood sizes a summary lists: 1, 2, 5, 10, 20, 50, 100, ... below ``n``."""
    out, decade = [], 1
    while decade < n:
        out += [v * decade for v in (1, 2, 5) if v * decade < n]
        decade *= 10
    return out


def bin_edges(scale: float, bins: int) -> np.ndarray:
    """The ``bins + 1`` edges of ``ops.shepard_fold``'s bins for one matrix (all 0 when the matrix is all zero)."""
    return np.arange(bins + 1) / scale if scale > 0 else np.zeros(bins + 1)


def coranking_curves(high, low, *, bins: int = 64, device) -> tuple[dict, dict]:
    """-> (report, arrays).  ``high`` ``[n, d]``: the latent rows as given to the projection; ``low`` ``[n, 2]``; numpy arrays
    or device tensors.  The report: ``n``, ``bins``, ``auc_logk_rnx``, ``k_max``, ``q_local``, ``q_global``,
    ``rank_correlation``, ``stress`` (``None`` where undefined, never NaN).  The arrays: the curves ``Q_NX``, ``B_NX``,
    ``LCMC`` ``[n - 1]`` and ``R_NX`` ``[n - 2]``, ``histograms`` int64 ``[3, n]``, ``sqdiff`` int64 and ``spearman`` ``[n]``,
    ``shepard_sums`` ``[n, 3]``, ``shepard_hist`` int64 ``[bins, bins]`` (rows: latent distance) and its
    ``shepard_edges_high`` / ``shepard_edges_low`` ``[bins + 1]``."""
    import torch

    from .. import ops
    from .projection_quality import _device_rows
    who = "coranking_curves"
    bins = int(bins)
    if not MIN_BINS <= bins <= MAX_BINS:
        raise ValueError(f"{who}: bins = {bins}; {MIN_BINS} .. {MAX_BINS}")
    device = torch.device(device)
    x, y = _device_rows(high, "high", device, who), _device_rows(low, "low", device, who)
    n = x.shape[0]
    if y.shape[0] != n:
        raise ValueError(f"{who}: high has {n} rows, low {y.shape[0]}")
    if n > MAX_ROWS:
        raise ValueError(f"{who}: {n} rows; at most {MAX_ROWS} (the distance matrices and one row's keys in LDS)")
    if n < MIN_ROWS:
        raise ValueError(f"{who}: {n} rows; at least {MIN_ROWS}")
    if y.shape[1] > ops.PROJECTION_MAX_COLS:
        raise ValueError(f"{who}: low has {y.shape[1]} columns; a projection has at most {ops.PROJECTION_MAX_COLS}")
    dist_high, dist_low = ops.latent_pairwise(x), ops.projection_distances(y)
    hist, sqdiff = ops.coranking_fold(ops.full_ranks(dist_high), ops.full_ranks(dist_low))
    sums, shepard, scale = ops.shepard_fold(dist_high, dist_low, bins)
    host = torch.cat([hist.reshape(-1).long(), sqdiff, sums.reshape(-1).view(torch.int64), shepard.reshape(-1).long(),
                      scale.view(torch.int32).long()]).cpu().numpy()
    cuts = np.cumsum([3 * n, n, 3 * n, bins * bins])
    hist, sqdiff, sums, shepard, scale = np.split(host, cuts)
    scale = scale.astype(np.int32).view(np.float32)
    arrays = curves_from_histograms(hist.reshape(3, n), n)
    report = {"n": n}
    report.update({key: arrays.pop(key) for key in ("auc_logk_rnx", "k_max", "q_local", "q_global")})
    spearman = row_spearman(sqdiff, n)
    sums = sums.view(np.float64).reshape(n, 3)
    report.update(rank_correlation=math.fsum(spearman) / n, stress=stress_from_sums(sums), bins=bins)
    arrays.update(histograms=hist.reshape(3, n), sqdiff=sqdiff, spearman=spearman, shepard_sums=sums,
                  shepard_hist=shepard.reshape(bins, bins), shepard_edges_high=bin_edges(float(scale[0]), bins),
                  shepard_edges_low=bin_edges(float(scale[1]), bins))
    return report, arrays

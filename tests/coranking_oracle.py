"""Plain numpy restatement of the co-ranking curves and the Shepard figure (``pti_ldm_vae_amd.analysis.coranking``) and of
the three device ops under them (csrc/coranking.hip).  Everything is stated on DISTANCE MATRICES and on rank tables, with
loops and ``math.fsum`` where the package uses prefix sums, so the two share no arithmetic.

Order within a row and ``rank(i, j)``: ``projection_quality_oracle.rank_table``."""
import math

import numpy as np

from projection_quality_oracle import golden_inputs, pairwise, rank_table  # noqa: F401  (re-exported for the tests)


def full_ranks(dist, row_offset=0):
    """``ops.full_ranks``: int16 [m, n] of the rows ``row_offset .. row_offset + m - 1``."""
    dist = np.asarray(dist)
    return rank_table(dist, np.arange(row_offset, row_offset + dist.shape[0])).astype(np.int16)


def coranking_fold(rank_high, rank_low):
    """``ops.coranking_fold`` -> (int64 [3, n] histograms, int64 [m] squared rank differences), entry by entry."""
    rh, rl = np.asarray(rank_high, dtype=np.int64), np.asarray(rank_low, dtype=np.int64)
    m, n = rh.shape
    hist, sq = np.zeros((3, n), dtype=np.int64), np.zeros(m, dtype=np.int64)
    for i in range(m):
        for a, b in zip(rh[i].tolist(), rl[i].tolist()):
            if 1 <= a <= n - 1 and 1 <= b <= n - 1:
                hist[0 if a == b else (1 if b < a else 2), max(a, b)] += 1
                sq[i] += (a - b) ** 2
    return hist, sq


def curves(hist, n):
    """The curves from the histograms by their definitions: one exact Python-integer sum per K."""
    h = [[int(v) for v in row] for row in np.asarray(hist)]
    q, b, lcmc, r = [], [], [], []
    for k in range(1, n):
        eq, intr, ext = (sum(h[c][1:k + 1]) for c in range(3))
        q.append((eq + intr + ext) / (k * n))
        b.append((ext - intr) / (k * n))
        lcmc.append(q[-1] - k / (n - 1))
        if k <= n - 2:
            r.append(((n - 1) * q[-1] - k) / (n - 1 - k))
    k_max = 1 + max(range(n - 1), key=lambda t: (lcmc[t], -t))
    return {"Q_NX": np.array(q), "B_NX": np.array(b), "R_NX": np.array(r), "LCMC": np.array(lcmc), "k_max": k_max,
            "q_local": math.fsum(q[:k_max]) / k_max,
            "q_global": math.fsum(q[k_max:]) / (n - 1 - k_max) if k_max < n - 1 else None,
            "auc_logk_rnx": math.fsum(v / (t + 1) for t, v in enumerate(r)) / math.fsum(1.0 / (t + 1) for t in range(n - 2))}


def row_spearman(sqdiff, n):
    m = n - 1
    return np.array([1.0 - 6.0 * int(s) / (m * (m * m - 1)) for s in sqdiff])


def shepard_scale(dist, bins):
    """fp32 ``bins / largest finite entry``, 0 when that entry is 0."""
    d = np.asarray(dist, dtype=np.float32)
    top = np.float32(np.where(np.isfinite(d), d, np.float32(0)).max())
    return np.float32(bins) / top if top > 0 else np.float32(0)


def shepard_bins(dist, scale, bins):
    """``min(bins - 1, int(v * scale))`` with the product in fp32; +inf and NaN go to the last bin."""
    d = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = d * np.float32(scale)
    assert t.dtype == np.float32
    last = ~(t < np.float32(bins - 1))
    return np.where(last, bins - 1, np.where(last, 0, t).astype(np.int64)).clip(min=0)


def shepard_fold(dist_high, dist_low, bins):
    """``ops.shepard_fold`` -> (per-row [fsum d_high^2, fsum d_low^2, fsum d_high d_low] over j != i, per-row sums of the
    terms' magnitudes, int64 [bins, bins] histogram, the two fp32 scales)."""
    dh, dl = np.asarray(dist_high, dtype=np.float32), np.asarray(dist_low, dtype=np.float32)
    n = dh.shape[0]
    scale = np.array([shepard_scale(dh, bins), shepard_scale(dl, bins)], dtype=np.float32)
    bh, bl = shepard_bins(dh, scale[0], bins), shepard_bins(dl, scale[1], bins)
    off = ~np.eye(n, dtype=bool)
    hist = np.zeros((bins, bins), dtype=np.int64)
    np.add.at(hist, (bh[off], bl[off]), 1)
    a, b = np.asarray(dist_high).astype(np.float64), np.asarray(dist_low).astype(np.float64)   # fp64 input: summed as given
    sums, mags = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        keep = off[i]
        for c, term in enumerate((a[i] * a[i], b[i] * b[i], a[i] * b[i])):      # a product of two fp32 values is exact in fp64
            sums[i, c], mags[i, c] = math.fsum(term[keep]), math.fsum(np.abs(term[keep]))
    return sums, mags, hist, scale


def stress(sums):
    hh, ll, hl = (math.fsum(np.asarray(sums)[:, c]) for c in range(3))
    if not all(math.isfinite(v) for v in (hh, ll, hl)) or hh <= 0.0 or ll <= 0.0:
        return None
    return math.sqrt(max(0.0, 1.0 - (hl * hl) / (hh * ll)))


def report_from_distances(dist_high, dist_low, bins=64):
    """The whole report from two distance matrices -> (report, arrays): the statement ``coranking_curves`` is held to."""
    dist_high, dist_low = np.asarray(dist_high), np.asarray(dist_low)
    n = dist_high.shape[0]
    hist, sq = coranking_fold(rank_table(dist_high), rank_table(dist_low))
    arrays = curves(hist, n)
    report = {"n": n}
    report.update({key: arrays.pop(key) for key in ("auc_logk_rnx", "k_max", "q_local", "q_global")})
    spearman = row_spearman(sq, n)
    sums, _, shist, _ = shepard_fold(dist_high, dist_low, bins)
    report.update(rank_correlation=math.fsum(spearman) / n, stress=stress(sums), bins=bins)
    arrays.update(histograms=hist, sqdiff=sq, spearman=spearman, shepard_sums=sums, shepard_hist=shist)
    return report, arrays

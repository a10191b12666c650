"""Host arithmetic of the disentanglement report: from the integer tables of ``ops.tied_ranks`` / ``ops.rank_moments`` /
``ops.joint_histogram`` to Spearman's rho, mutual information, MIG, modularity, SAP and interpretability.  Nothing here
needs a GPU.

Columns are ordered channels first: column ``c < L`` is latent channel ``c``, column ``L + q`` is attribute ``q``.  A term whose
denominator is zero is ``None`` (JSON ``null``), never NaN; it is left out of its mean and named in ``excluded``.
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np


def bin_edges(lo, hi, bins) -> np.ndarray:
    """The ``bins`` LEFT edges numpy gives a float32 column whose extremes are ``lo`` and ``hi`` -- ``np.histogram(x,
    bins)[1][:-1]`` -- widened to fp64.  A constant column gets numpy's ``lo - 0.5 .. hi + 0.5``."""
    return np.histogram_bin_edges(np.array([lo, hi], dtype=np.float32), bins)[:-1].astype(np.float64)


def edge_tables(lo, hi, bins) -> np.ndarray:
    """``bin_edges`` of every column: ``lo``, ``hi`` [M] -> fp64 [M, bins]."""
    return np.stack([bin_edges(a, b, bins) for a, b in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist())])


def spearman_matrix(sums, gram, n, na, l) -> list:
    """Spearman's rho of every (attribute, channel) from the moments of the doubled ranks: ``sums`` [M], ``gram`` [M, M] with
    ``M = l + na`` -> [na][l].  ``(n Sxy - Sx Sy) / sqrt((n Sxx - Sx^2) (n Syy - Sy^2))`` in Python integers with one square
    root (the factor 2 of the ranks cancels); ``None`` where a factor is 0, i.e. a side is constant."""
    sums = np.asarray(sums).tolist()
    gram = np.asarray(gram).tolist()
    if len(sums) != l + na or len(gram) != l + na:
        raise ValueError(f"spearman_matrix: expected {l + na} columns, got sums {len(sums)} / gram {len(gram)}")
    n = int(n)
    var = [n * int(gram[k][k]) - int(sums[k]) ** 2 for k in range(l + na)]
    out = []
    for q in range(na):
        row = []
        for c in range(l):
            den = var[c] * var[l + q]
            num = n * int(gram[l + q][c]) - int(sums[l + q]) * int(sums[c])
            row.append(num / math.sqrt(den) if den > 0 else None)
        out.append(row)
    return out


def mutual_information(counts):
    """``counts`` int [na, L, B, B] (``[q, c, bin_a, bin_z]``) -> ``(mi, h)``: fp64 MI [na, L] in nats and the attribute
    entropies H [na], both from the integer tables: ``MI = sum (k / n) log(k n / (row col))``."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 4 or counts.shape[2] != counts.shape[3]:
        raise ValueError(f"mutual_information: expected counts [na, L, B, B], got {counts.shape}")
    na, l = counts.shape[:2]
    mi, h = np.zeros((na, l), np.float64), np.zeros(na, np.float64)
    for q in range(na):
        for c in range(l):
            t = counts[q, c]
            n = int(t.sum())
            rows, cols = t.sum(1), t.sum(0)
            ia, iz = np.nonzero(t)
            k = t[ia, iz].astype(np.float64)
            ratio = (k * n) / (rows[ia] * cols[iz]).astype(np.float64)   # both sides are exact integers below 2^53
            mi[q, c] = max(float(np.sum(k / n * np.log(ratio))), 0.0)
            if c == 0:
                p = rows[rows > 0].astype(np.float64) / n
                h[q] = max(float(-np.sum(p * np.log(p))), 0.0)
    return mi, h


EULER_GAMMA = 0.5772156649015328606


def ksg_scale(cols) -> np.ndarray:
    """What the k-nearest-neighbour estimator sees: every column (a ROW of ``cols`` [M, N]) divided by its population
    standard deviation -- fp64 arithmetic on the fp32 data, rounded back to fp32, ``sklearn.preprocessing.scale(x,
    with_mean=False)``.  A column whose deviation is below ``10 eps`` (fp64) -- a constant column -- is left unscaled, as
    sklearn leaves it."""
    x = np.asarray(cols, dtype=np.float32).astype(np.float64)
    if x.ndim != 2:
        raise ValueError(f"ksg_scale: expected columns [M, N], got {x.shape}")
    std = x.std(axis=1)
    std[~(std >= 10.0 * np.finfo(np.float64).eps)] = 1.0
    return (x / std[:, None]).astype(np.float32)


def digamma_table(n) -> np.ndarray:
    """``psi(m) = -gamma + H_(m - 1)`` at the integers ``m = 1 .. n`` as fp64 ``[n + 1]``, indexed by ``m`` (entry 0, the pole,
    is ``-inf``); the harmonic numbers are one running fp64 sum.  No scipy needed."""
    n = int(n)
    if n < 1:
        raise ValueError(f"digamma_table: n = {n} (n >= 1)")
    table = np.full(n + 1, -np.inf)
    table[1] = -EULER_GAMMA
    table[2:] = np.cumsum(1.0 / np.arange(1, n, dtype=np.float64)) - EULER_GAMMA
    return table


def ksg_mutual_information(nx, ny, n, k) -> np.ndarray:
    """The Kraskov-Stoegbauer-Grassberger estimate (estimator 1, scikit-learn's ``_compute_mi_cc``) from the integer range
    counts of ``ops.ksg_counts``: ``nx``, ``ny`` int [na, L, n] -> fp64 MI [na, L] in nats,
    ``max(0, psi(n) + psi(k) - mean_i psi(nx_i + 1) - mean_i psi(ny_i + 1))``.  The mean is taken over the per-row terms
    ``(psi(n) - psi(nx_i + 1)) + (psi(k) - psi(ny_i + 1))``: where every ``nx_i = n - 1`` and ``ny_i = k - 1`` -- a constant
    column against one without ties -- each term, and with it the estimate, is 0.0 exactly."""
    nx, ny = np.asarray(nx), np.asarray(ny)
    n, k = int(n), int(k)
    if nx.shape != ny.shape or nx.ndim != 3 or nx.shape[2] != n:
        raise ValueError(f"ksg_mutual_information: expected nx, ny [na, L, {n}], got {nx.shape} and {ny.shape}")
    if not 1 <= k <= n - 1:
        raise ValueError(f"ksg_mutual_information: k = {k} with n = {n} (1 <= k <= n - 1)")
    if nx.min() < 0 or ny.min() < 0 or nx.max() > n - 1 or ny.max() > n - 1:
        raise ValueError(f"ksg_mutual_information: a count outside 0 .. {n - 1}")
    psi = digamma_table(n)
    terms = (psi[n] - psi[nx.astype(np.int64) + 1]) + (psi[k] - psi[ny.astype(np.int64) + 1])
    return np.maximum(terms.mean(axis=2), 0.0)


def _top_two_gap(values):
    """Largest minus second largest of the defined values; ``None`` with fewer than two."""
    top = sorted((v for v in values if v is not None), reverse=True)
    return top[0] - top[1] if len(top) >= 2 else None


def _mean(values):
    kept = [v for v in values if v is not None]
    return sum(kept) / len(kept) if kept else None


def scores(mi, h, pearson, names) -> dict:
    """-> ``{"scores", "per_attribute", "per_channel", "excluded"}`` from MI [na, L], H [na] and Pearson's r [na][L]
    (``ar_metrics.pearson_matrix``: ``None`` where a side is constant).

    * ``mig``: per attribute ``(MI top1 - MI top2 over the channels) / H[q]``;
    * ``modularity``: per channel ``1 - (sum_q MI^2 - max_q MI^2) / (max_q MI^2 (na - 1))``;
    * ``sap``: per attribute the top-two gap of ``r^2`` over the channels whose ``r`` is defined;
    * ``interpretability``: per attribute ``r^2`` at the channel of largest MI (lowest index on ties).

    An entry is ``None`` when its denominator is zero: ``H[q] = 0``, a channel without any MI, ``na < 2`` (modularity),
    fewer than two channels (the gaps), an undefined ``r``.  The score is the mean of the defined entries (``None`` when
    there is none); ``excluded`` names the others per score."""
    mi = np.asarray(mi, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    na, l = mi.shape
    mig, sap, interp = [], [], []
    for q in range(na):
        row = [float(v) for v in mi[q]]
        gap = _top_two_gap(row)
        mig.append(gap / float(h[q]) if gap is not None and h[q] > 0.0 else None)
        sap.append(_top_two_gap([None if r is None else r * r for r in pearson[q]]))
        r = pearson[q][int(np.argmax(mi[q]))]
        interp.append(None if r is None or not h[q] > 0.0 else r * r)
    modularity = []
    for c in range(l):
        sq = mi[:, c] ** 2
        top = float(sq.max())
        modularity.append(1.0 - (float(sq.sum()) - top) / (top * (na - 1)) if na >= 2 and top > 0.0 else None)
    channels = [f"channel {c}" for c in range(l)]
    entries = {"mig": (mig, names), "modularity": (modularity, channels), "sap": (sap, names),
               "interpretability": (interp, names)}
    return {"scores": {k: _mean(v) for k, (v, _) in entries.items()},
            "per_attribute": {"mig": mig, "sap": sap, "interpretability": interp},
            "per_channel": {"modularity": modularity},
            "excluded": {k: [str(lab) for val, lab in zip(v, labels) if val is None] for k, (v, labels) in entries.items()}}


def best_channel(rho_row):
    """argmax |rho| over the channels, the lowest index on ties; ``None`` when no channel has a defined rho."""
    best, top = None, -1.0
    for c, r in enumerate(rho_row):
        if r is not None and abs(r) > top:
            best, top = c, abs(r)
    return best


def disentanglement_report(names, channels, n, sums, gram, counts, pearson, *, mi=None) -> dict:
    """The ``scores``, ``attributes``, matrices, ``entropy`` and ``excluded`` blocks of ``disentanglement.json``.  ``mi``
    [na, L] (``ksg_mutual_information``) takes the place of the histogram MI in ``mutual_information`` and under the scores;
    the histogram MI is then kept as ``mutual_information_binned``.  The entropies stay the histogram ones: a differential
    entropy cannot normalise MIG."""
    counts = np.asarray(counts)
    na, l = counts.shape[:2]
    rho = spearman_matrix(sums, gram, n, na, l)
    binned, h = mutual_information(counts)
    if mi is None:
        mi = binned
    else:
        mi = np.asarray(mi, dtype=np.float64)
        if mi.shape != (na, l):
            raise ValueError(f"disentanglement_report: expected mi [{na}, {l}], got {mi.shape}")
    s = scores(mi, h, pearson, list(names))
    per_attr = {}
    for q, name in enumerate(names):
        ch = int(channels[q])
        mapped = 0 <= ch < l
        best = best_channel(rho[q])
        per_attr[name] = {"latent_channel": ch, "spearman_rho": rho[q][ch] if mapped else None,
                          "best_channel_spearman": best, "mapped_channel_is_best": bool(mapped and best == ch),
                          "mig": s["per_attribute"]["mig"][q], "sap": s["per_attribute"]["sap"][q]}
    report = {"scores": s["scores"], "attributes": per_attr, "spearman_rho": rho, "mutual_information": mi.tolist(),
              "pearson_r": pearson, "entropy": h.tolist(), "excluded": s["excluded"]}
    if mi is not binned:
        report["mutual_information_binned"] = binned.tolist()
    return report


def save_heatmaps(path, rho, mi, names, channels, mi_title="mutual information (nats)") -> Path:
    """|rho| and MI heat maps side by side: attributes down, channels across, the mapped cell of every attribute outlined
    (matplotlib, Agg; the drawing style of ``ar_metrics.save_tau_heatmap``).  ``mi_title``: the MI panel's title."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.patches import Rectangle
    grids = [np.abs(np.array([[np.nan if v is None else v for v in row] for row in rho], dtype=np.float64)),
             np.array(mi, dtype=np.float64)]
    na, l = grids[0].shape
    fig, axes = plt.subplots(1, 2, figsize=(2 * (1.5 + 0.6 * l), 1.2 + 0.5 * na))
    for ax, grid, title, cmap, vmax in zip(axes, grids, ("|Spearman rho|: attribute vs channel mean", mi_title),
                                           ("viridis", "magma"), (1.0, None)):
        im = ax.imshow(np.ma.masked_invalid(grid), cmap=cmap, vmin=0.0, vmax=vmax, aspect="auto")
        ax.set_xticks(range(l), [str(c) for c in range(l)])
        ax.set_yticks(range(na), list(names))
        ax.set_xlabel("latent channel")
        ax.set_title(title)
        for q, ch in enumerate(channels):
            if 0 <= int(ch) < l:
                ax.add_patch(Rectangle((int(ch) - 0.5, q - 0.5), 1.0, 1.0, fill=False, edgecolor="black", linewidth=2.0))
        fig.colorbar(im, ax=ax)
    fig.tight_layout()
    path = Path(path)
    fig.savefig(path, dpi=120)
    plt.close(fig)
    return path

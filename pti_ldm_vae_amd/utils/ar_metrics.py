"""Host arithmetic of the attribute-ordering report: from the pair counts of ``ops.rank_agreement`` to concordance, Kendall's
tau-b and the full-set AR term; Pearson's r; the heat map.  Nothing here needs a GPU.

``counts[q][c]`` (``ops.RANK_CLASSES`` order) = (concordant C, discordant D, z-tied Tz, a-tied Ta, both-tied) over the
N (N - 1) / 2 unordered pairs.  A ratio whose denominator is zero is ``None`` (JSON ``null``), never NaN.
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import torch


def order_statistics(counts, loss_sum) -> dict:
    """``counts`` int [na, L, 5], ``loss_sum`` float [na] -> plain lists:

    * ``pairs`` [na][L] = C + D + Tz: the UNORDERED pairs whose attribute values differ -- half of what the training
      kernel's ``counts`` reports, which runs over ordered pairs (the value depends on the attribute only);
    * ``concordance`` [na][L] = C / pairs;
    * ``kendall_tau_b`` [na][L] = (C - D) / sqrt((C + D + Tz) (C + D + Ta));
    * ``ar_loss`` [na] = loss_sum / pairs, 0 when no pair qualifies, as in the training kernel."""
    counts = np.asarray(counts, dtype=np.int64)
    loss_sum = np.asarray(loss_sum, dtype=np.float64)
    if counts.ndim != 3 or counts.shape[2] != 5 or loss_sum.shape != (counts.shape[0],):
        raise ValueError(f"order_statistics: expected counts [na, L, 5] and loss_sum [na], got {counts.shape} / {loss_sum.shape}")
    pairs, conc, tau, ar_loss = [], [], [], []
    for q in range(counts.shape[0]):
        rp, rc, rt = [], [], []
        for c in range(counts.shape[1]):
            cc, dd, tz, ta, _ = (int(v) for v in counts[q, c])
            p = cc + dd + tz
            den = p * (cc + dd + ta)                      # Python integers: exact
            rp.append(p)
            rc.append(cc / p if p > 0 else None)
            rt.append((cc - dd) / math.sqrt(den) if den > 0 else None)
        pairs.append(rp)
        conc.append(rc)
        tau.append(rt)
        ar_loss.append(float(loss_sum[q]) / rp[0] if rp[0] > 0 else 0.0)
    return {"pairs": pairs, "concordance": conc, "kendall_tau_b": tau, "ar_loss": ar_loss}


def pearson_matrix(z, attrs) -> list:
    """Pearson's r of every (attribute, channel) in fp64 via torch: ``z`` [N, L], ``attrs`` [na, N] -> [na][L]; ``None``
    where either side is constant."""
    z = torch.as_tensor(np.asarray(z)).to(torch.float64)
    a = torch.as_tensor(np.asarray(attrs)).to(torch.float64)
    zc, ac = z - z.mean(0, keepdim=True), a - a.mean(1, keepdim=True)
    cov = ac @ zc                                                      # [na, L]
    den = torch.sqrt((ac * ac).sum(1)[:, None] * (zc * zc).sum(0)[None, :])
    return [[float(cov[q, c] / den[q, c]) if float(den[q, c]) > 0.0 else None for c in range(z.shape[1])]
            for q in range(a.shape[0])]


def best_channel(tau_row):
    """argmax |tau_b| over the channels, the lowest index on ties; ``None`` when no channel has a defined tau."""
    best, top = None, -1.0
    for c, t in enumerate(tau_row):
        if t is not None and abs(t) > top:
            best, top = c, abs(t)
    return best


def attribute_report(names, channels, deltas, counts, loss_sum, pearson) -> dict:
    """The ``attributes`` block and the matrices of ``ar_metrics.json``."""
    stats = order_statistics(counts, loss_sum)
    per_attr = {}
    for q, name in enumerate(names):
        ch = int(channels[q])
        best = best_channel(stats["kendall_tau_b"][q])
        mapped = 0 <= ch < len(stats["pairs"][q])
        per_attr[name] = {
            "latent_channel": ch, "delta": float(deltas[q]), "pairs": stats["pairs"][q][0],
            "concordance": stats["concordance"][q][ch] if mapped else None,
            "kendall_tau_b": stats["kendall_tau_b"][q][ch] if mapped else None,
            "pearson_r": pearson[q][ch] if mapped else None,
            "ar_loss": stats["ar_loss"][q], "best_channel": best, "mapped_channel_is_best": bool(mapped and best == ch)}
    return {"attributes": per_attr, "kendall_tau_b": stats["kendall_tau_b"], "concordance": stats["concordance"],
            "pearson_r": pearson, "counts": np.asarray(counts, dtype=np.int64).tolist()}


def save_tau_heatmap(path, tau, names, channels) -> Path:
    """tau-b heat map: attributes down, channels across, the mapped cell of every attribute outlined (matplotlib, Agg)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.patches import Rectangle
    grid = np.array([[np.nan if v is None else v for v in row] for row in tau], dtype=np.float64)
    na, l = grid.shape
    fig, ax = plt.subplots(figsize=(1.5 + 0.6 * l, 1.2 + 0.5 * na))
    im = ax.imshow(np.ma.masked_invalid(grid), cmap="coolwarm", vmin=-1.0, vmax=1.0, aspect="auto")
    ax.set_xticks(range(l), [str(c) for c in range(l)])
    ax.set_yticks(range(na), list(names))
    ax.set_xlabel("latent channel")
    ax.set_title("Kendall tau-b: attribute vs channel mean")
    for q, ch in enumerate(channels):
        if 0 <= int(ch) < l:
            ax.add_patch(Rectangle((int(ch) - 0.5, q - 0.5), 1.0, 1.0, fill=False, edgecolor="black", linewidth=2.0))
    fig.colorbar(im, ax=ax)
    fig.tight_layout()
    path = Path(path)
    fig.savefig(path, dpi=120)
    plt.close(fig)
    return path

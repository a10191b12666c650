"""Plain numpy restatement of the disentanglement report (``pti_tied_ranks`` / ``pti_rank_moments`` / ``pti_joint_histogram`` +
``utils/disentanglement.py``).  numpy only: the GPU tests import it where scipy and sklearn may be missing.

Everything is spelled out: doubled average ranks by broadcasting (two boolean [n, n] tables per column), edges from
``np.histogram_bin_edges``, bins from ``np.digitize``, joint histograms with ``np.add.at``, Spearman's rho as Pearson's r of the
ranks in fp64, MI from probabilities.  ``report`` takes switches that MUTATE the definition (tests/test_disentanglement_cpu.py
shows that every one of them is caught).  Columns are ordered channels first, then attributes.

``tools/make_disentanglement_golden.py`` records ``tests/golden/disentanglement_golden.npz`` from ``report``.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "disentanglement_golden.npz")
TABLES = ("edges", "rank2", "sums", "gram", "bins", "counts")
FLOATS = ("spearman_rho", "mutual_information", "entropy", "pearson_r", "scores", "mig", "sap", "interpretability", "modularity")
SCORES = ("mig", "modularity", "sap", "interpretability")

# name, n, L, na, seed, kind, bins, (ldz - n, lda - n) of the GPU run
CASES = [
    ("n2", 2, 1, 1, 21, "plain", 2, (0, 0)),                # a single pair of rows
    ("n3", 3, 2, 1, 22, "plain", 2, (0, 0)),
    ("n65", 65, 3, 2, 23, "plain", 2, (0, 0)),              # crosses a wavefront; the smallest bin count
    ("n257", 257, 10, 6, 24, "plain", 20, (0, 0)),          # one past a 256 tile; the AR config's L and na
    ("n1030", 1030, 16, 16, 25, "plain", 32, (0, 0)),       # all 32 columns; the largest bin count; ragged tiles
    ("n2500", 2500, 10, 6, 26, "plain", 20, (12, 60)),      # two row chunks of the histogram; padded strides
    ("n97_const", 97, 5, 3, 27, "const", 20, (0, 0)),       # a constant channel and a constant attribute
    ("n300_edges", 300, 4, 3, 28, "edges", 20, (0, 0)),     # integers 0..20 on every edge, 0.0 / -0.0, a 5-valued attribute
]


def make_case(name, n, l, na, seed, kind="plain", bins=20):
    """Seeded inputs: z is rounded to 0.01 (some ties), attributes are integers 0..39 (many ties), attribute q follows
    channel (3 q + 1) % L loosely so that the scores are not all noise, a tenth of the rows are copies of other rows."""
    rng = np.random.default_rng(seed)
    z = np.round(rng.normal(0.0, 1.0, (n, l)), 2).astype(np.float32)
    channels = np.array([(3 * q + 1) % l for q in range(na)], np.int32)
    attrs = np.stack([np.clip(np.round(20.0 + 8.0 * z[:, channels[q]] + rng.normal(0.0, 4.0, n)), 0, 39) for q in range(na)])
    attrs = attrs.astype(np.float32)
    for k in range(n // 10):
        src, dst = rng.integers(0, n, 2)
        z[dst], attrs[:, dst] = z[src], attrs[:, src]
    if kind == "const":
        z[:, 2] = 0.3
        attrs[1] = 7.0
    if kind == "edges":
        z[:, 0] = rng.integers(0, 21, n).astype(np.float32)
        z[:2, 0] = (0.0, 20.0)                                      # both ends occur: the 20 edges are 0, 1, .. 19
        z[:, 1] = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), n)
        z[2:4, 1] = (0.0, -0.0)
        attrs[0] = rng.integers(0, 5, n).astype(np.float32)
    return SimpleNamespace(name=name, n=n, l=l, na=na, bins=bins, z=z, attrs=attrs, channels=channels)


def all_cases():
    return [make_case(*spec[:7]) for spec in CASES]


def columns(z, attrs):
    """[L + na, n] float32: channels first, then attributes."""
    return np.concatenate([np.asarray(z, np.float32).T, np.asarray(attrs, np.float32)])


def rank2_of(x, *, ordinal=False):
    """2 x the average rank of every value: 2 #{x_j < x_i} + #{x_j == x_i} + 1 (``ordinal``: ties broken by position)."""
    x = np.asarray(x, np.float32)
    less = (x[None, :] < x[:, None]).sum(1).astype(np.int64)
    equal = (x[None, :] == x[:, None]).sum(1).astype(np.int64)
    if ordinal:
        idx = np.arange(x.size)
        before = ((x[None, :] == x[:, None]) & (idx[None, :] < idx[:, None])).sum(1).astype(np.int64)
        return (2 * (less + before) + 2).astype(np.int32)
    return (2 * less + equal + 1).astype(np.int32)


def edges_of(x, bins):
    """The ``bins`` left edges of numpy's histogram of the float32 column, as fp64."""
    return np.histogram_bin_edges(np.asarray(x, np.float32), bins)[:-1].astype(np.float64)


def bins_of(x, edges, *, strict=False, open_last=None):
    """#{k: edges[k] <= x} - 1.  ``strict``: edges[k] < x (the minimum is clipped into bin 0).  ``open_last``: the right
    end of the range -- numpy's last bin without its closed right side: the maximum falls out (bin = len(edges))."""
    x = np.asarray(x, np.float32)
    if open_last is not None:
        return np.digitize(x, np.append(edges, open_last)) - 1
    if strict:
        return np.maximum(np.digitize(x, edges, right=True) - 1, 0)
    return np.digitize(x, edges) - 1


def _nan_gap(values):
    v = np.sort(values[~np.isnan(values)])[::-1]
    return v[0] - v[1] if v.size >= 2 else np.nan


def _nan_mean(values):
    values = np.asarray(values, np.float64)
    return float(np.mean(values[~np.isnan(values)])) if np.any(~np.isnan(values)) else np.nan


def report(z, attrs, bins, *, ordinal_ranks=False, strict_edges=False, open_last_bin=False, log2_mi=False,
           unsorted_top_two=False, modularity_over_na=False):
    """-> dict of the integer tables (``TABLES``) and the fp64 results (``FLOATS``; NaN where undefined).  ``scores`` is
    [4] in ``SCORES`` order.  The keyword switches are the mutations; all False is the definition."""
    z = np.asarray(z, np.float32)
    attrs = np.asarray(attrs, np.float32)
    n, l = z.shape
    na = attrs.shape[0]
    cols = columns(z, attrs)
    m = l + na
    rank2 = np.stack([rank2_of(c, ordinal=ordinal_ranks) for c in cols])
    r64 = rank2.astype(np.int64)
    sums, gram = r64.sum(1), r64 @ r64.T
    edges = np.stack([edges_of(c, bins) for c in cols])
    b = np.stack([bins_of(c, e, strict=strict_edges, open_last=float(c.max()) if open_last_bin and c.max() > c.min() else None)
                  for c, e in zip(cols, edges)])
    counts = np.zeros((na, l, bins, bins), np.int32)
    for q in range(na):
        for c in range(l):
            keep = (b[l + q] < bins) & (b[c] < bins)
            np.add.at(counts[q, c], (b[l + q][keep], b[c][keep]), 1)

    ranks = rank2.astype(np.float64) / 2.0
    rc = ranks - ranks.mean(1, keepdims=True)
    zc = cols.astype(np.float64) - cols.astype(np.float64).mean(1, keepdims=True)
    rho, pearson = np.full((na, l), np.nan), np.full((na, l), np.nan)
    for q in range(na):
        for c in range(l):
            for out, v in ((rho, rc), (pearson, zc)):
                den = np.sqrt(np.sum(v[l + q] ** 2) * np.sum(v[c] ** 2))
                if den > 0:
                    out[q, c] = np.sum(v[l + q] * v[c]) / den

    log = np.log2 if log2_mi else np.log
    mi, h = np.zeros((na, l)), np.zeros(na)
    for q in range(na):
        for c in range(l):
            total = counts[q, c].sum()                      # marginals from the integer sums: a constant column has p = 1.0
            p = counts[q, c].astype(np.float64) / total     # exactly, and with it MI = 0 exactly
            pa, pz = counts[q, c].sum(1, keepdims=True) / total, counts[q, c].sum(0, keepdims=True) / total
            nz = p > 0
            mi[q, c] = max(np.sum(p[nz] * log(p[nz] / (pa * pz)[nz])), 0.0)
        pa = np.bincount(b[l + q][b[l + q] < bins], minlength=bins).astype(np.float64)
        pa = pa[pa > 0] / pa.sum()
        h[q] = max(-np.sum(pa * np.log(pa)), 0.0)           # the entropy stays in nats: log2_mi does not renormalise it

    r2 = pearson ** 2
    mig, sap, interp = np.full(na, np.nan), np.full(na, np.nan), np.full(na, np.nan)
    for q in range(na):
        if unsorted_top_two:
            gap_mi = mi[q, 0] - mi[q, 1] if l >= 2 else np.nan
            ok = r2[q][~np.isnan(r2[q])]
            gap_r2 = ok[0] - ok[1] if ok.size >= 2 else np.nan
        else:
            gap_mi, gap_r2 = _nan_gap(mi[q]), _nan_gap(r2[q])
        mig[q] = gap_mi / h[q] if h[q] > 0 else np.nan
        sap[q] = gap_r2
        interp[q] = r2[q, int(np.argmax(mi[q]))] if h[q] > 0 else np.nan
    modularity = np.full(l, np.nan)
    for c in range(l):
        sq = mi[:, c] ** 2
        if na >= 2 and sq.max() > 0:
            modularity[c] = 1.0 - (sq.sum() - sq.max()) / (sq.max() * (na if modularity_over_na else na - 1))
    scores = np.array([_nan_mean(mig), _nan_mean(modularity), _nan_mean(sap), _nan_mean(interp)])
    return dict(edges=edges, rank2=rank2, sums=sums, gram=gram, bins=b.astype(np.uint8), counts=counts, spearman_rho=rho,
                mutual_information=mi, entropy=h, pearson_r=pearson, scores=scores, mig=mig, sap=sap, interpretability=interp,
                modularity=modularity)


def load_golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}

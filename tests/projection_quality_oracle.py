"""Plain numpy restatement of the projection-quality report (``pti_ldm_vae_amd.analysis.projection_quality``) and of its two
device ops (csrc/projection_quality.hip).  Everything is stated on DISTANCE MATRICES, so the same code rates scikit-learn's
fp64 distances, numpy fp32 distances and the device's own matrices copied back.

Order within a row: (distance, column), -0 taken as 0 -- for an fp32 matrix exactly ``umap_knn``'s 64-bit key (the bits of
the distance above the column), for any other dtype a stable sort of the values.  ``rank(i, j) = 1 + #{l != i : key(i, l) <
key(i, j)}``."""
import math

import numpy as np

MAX_ROWS, MIN_ROWS, MAX_NEIGHBORS, MAX_CLASSES = 8192, 4, 255, 2048


def row_order(dist):
    """-> int64 [n, n]: the columns of every row in ascending key order (the diagonal competes)."""
    dist = np.asarray(dist)
    n = dist.shape[1]
    if dist.dtype == np.float32:
        bits = np.ascontiguousarray(dist).view(np.uint32).astype(np.uint64)
        bits[bits == 0x80000000] = 0
        keys = (bits << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
        return np.argsort(keys, axis=1, kind="stable").astype(np.int64)
    return np.argsort(dist.astype(np.float64) + 0.0, axis=1, kind="stable").astype(np.int64)


def rank_table(dist, rows=None):
    """-> int64 [r, n]: ``rank(i, j)`` for every j (0 at the row's own column).  ``dist`` holds the rows ``rows`` of the
    matrix (all of them, in order, when ``rows`` is None)."""
    order = row_order(dist)
    r, n = order.shape
    own_col = np.arange(r) if rows is None else np.asarray(rows, dtype=np.int64)
    pos = np.empty_like(order)
    pos[np.arange(r)[:, None], order] = np.arange(n)[None, :]
    own = pos[np.arange(r), own_col][:, None]
    rank = pos - (own < pos) + 1
    rank[np.arange(r), own_col] = 0
    return rank


def neighbor_ranks(dist, nbr_idx, rows=None):
    """``ops.neighbor_ranks``: int32 [r, m]; 0 for the row's own index, -1 for an index outside [0, n).  With ``rows``,
    ``dist`` and ``nbr_idx`` hold only those rows of the call."""
    nbr = np.asarray(nbr_idx, dtype=np.int64)
    rank = rank_table(dist, rows)
    r, n = rank.shape
    ok = (nbr >= 0) & (nbr < n)
    got = rank[np.arange(r)[:, None], np.where(ok, nbr, 0)]
    return np.where(ok, got, -1).astype(np.int32)


def nearest_others(dist, k):
    """-> int64 [n, k]: the k nearest OTHER rows of every row, ascending by key."""
    order = row_order(dist)
    n = order.shape[0]
    return order[order != np.arange(n)[:, None]].reshape(n, n - 1)[:, :k]


def segment_row_sums(dist, seg):
    """``ops.segment_row_sums`` with every entry summed exactly (``math.fsum`` of the values widened to fp64)."""
    d = np.asarray(dist).astype(np.float64)
    seg = [int(v) for v in seg]
    out = np.zeros((d.shape[0], len(seg) - 1))
    for i in range(d.shape[0]):
        for g in range(len(seg) - 1):
            out[i, g] = math.fsum(d[i, seg[g]:seg[g + 1]])
    return out


def pairwise(x, dtype=np.float64):
    """Euclidean distances of the rows of ``x``, accumulated as differences in ``dtype``; an exactly zero diagonal."""
    x = np.asarray(x, dtype=dtype)
    d = np.stack([np.sqrt(((x - row) ** 2).sum(axis=1, dtype=dtype)) for row in x]).astype(dtype)
    np.fill_diagonal(d, 0.0)
    return d


def admitted(neighbors, n):
    """-> (the k with k < n / 2 in the order given, {k: reason} of the others): scikit-learn's condition."""
    keep, out = [], {}
    for k in neighbors:
        k = int(k)
        if k < 1:
            out[k] = "k must be at least 1"
        elif 2 * k >= n:
            out[k] = f"k = {k} is not below n / 2 = {n / 2:g}"
        elif k not in keep:
            keep.append(k)
    return keep, out


def rank_sums(dist_high, dist_low, ks):
    """The integers under the three rank figures -> dict of int64 arrays [n, K]: ``trust_excess`` (sum over the k nearest in
    ``dist_low`` of max(0, rank in ``dist_high`` - k)), ``cont_excess`` (the spaces swapped), ``shared`` (|kNN_high and kNN_low|)."""
    n = np.asarray(dist_high).shape[0]
    out = {name: np.zeros((n, len(ks)), dtype=np.int64) for name in ("trust_excess", "cont_excess", "shared")}
    if not ks:
        return out
    kmax = max(ks)
    r_hl = neighbor_ranks(dist_high, nearest_others(dist_low, kmax)).astype(np.int64)
    r_lh = neighbor_ranks(dist_low, nearest_others(dist_high, kmax)).astype(np.int64)
    for c, k in enumerate(ks):
        out["trust_excess"][:, c] = np.maximum(r_hl[:, :k] - k, 0).sum(axis=1)
        out["cont_excess"][:, c] = np.maximum(r_lh[:, :k] - k, 0).sum(axis=1)
        out["shared"][:, c] = (r_hl[:, :k] <= k).sum(axis=1)
    return out


def label_codes(labels):
    """-> (classes in sorted order -- by ``str`` when the labels do not compare --, int64 codes [n])."""
    labels = [v.item() if isinstance(v, np.generic) else v for v in labels]
    try:
        classes = sorted(set(labels))
    except TypeError:
        classes = sorted(set(labels), key=str)
    index = {c: i for i, c in enumerate(classes)}
    return classes, np.array([index[v] for v in labels], dtype=np.int64)


def silhouette(dist, codes, n_classes):
    """scikit-learn's silhouette_samples on a distance matrix (fsum of the fp64-widened entries): a = own sum / (size - 1),
    b = min over the other labels of sum / size, s = (b - a) / max(a, b), 0 for a singleton and where a = b = 0."""
    order = np.argsort(codes, kind="stable")
    sizes = np.bincount(codes, minlength=n_classes)
    seg = np.concatenate([[0], np.cumsum(sizes)])
    sums = segment_row_sums(np.asarray(dist)[:, order], seg)
    return silhouette_from_sums(sums, codes, sizes)


def silhouette_from_sums(sums, codes, sizes):
    n = len(codes)
    rows = np.arange(n)
    own_size = sizes[codes]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[rows, codes] / (own_size - 1)
        mean = sums / sizes[None, :]
        mean[rows, codes] = np.inf
        b = mean.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s[own_size == 1] = 0.0
    return np.nan_to_num(s, nan=0.0)


def knn_agreement_counts(dist, codes, ks):
    """-> int64 [n, K]: how many of a row's k nearest other rows carry its label."""
    if not ks:
        return np.zeros((len(codes), 0), dtype=np.int64)
    near = nearest_others(dist, max(ks))
    same = codes[near] == codes[:, None]
    return np.stack([same[:, :k].sum(axis=1) for k in ks], axis=1).astype(np.int64)


def _ratio(excess_total, n, k):
    return 1.0 - float(excess_total) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def report_from_distances(dist_high, dist_low, high_dims, neighbors=(5, 15, 40), labels=None):
    """The whole report from two distance matrices -> (report dict, per-point arrays): the statement that
    ``projection_quality`` is held to."""
    dist_high, dist_low = np.asarray(dist_high), np.asarray(dist_low)
    n = dist_high.shape[0]
    ks, excluded = admitted(neighbors, n)
    sums = rank_sums(dist_high, dist_low, ks)
    report = {"n": n, "high_dims": int(high_dims), "neighbors": list(ks), "excluded": excluded,
              "trustworthiness": {}, "continuity": {}, "neighborhood_preservation": {}, "labels": {}}
    points = {"trustworthiness_local": np.zeros((n, len(ks))), "continuity_local": np.zeros((n, len(ks)))}
    for c, k in enumerate(ks):
        report["trustworthiness"][k] = _ratio(sums["trust_excess"][:, c].sum(), n, k)
        report["continuity"][k] = _ratio(sums["cont_excess"][:, c].sum(), n, k)
        report["neighborhood_preservation"][k] = float(sums["shared"][:, c].sum()) / (n * k)
        points["trustworthiness_local"][:, c] = 1.0 - sums["trust_excess"][:, c] * (2.0 / (k * (2.0 * n - 3.0 * k - 1.0)))
        points["continuity_local"][:, c] = 1.0 - sums["cont_excess"][:, c] * (2.0 / (k * (2.0 * n - 3.0 * k - 1.0)))
    for name, values in (labels or {}).items():
        classes, codes = label_codes(values)
        entry = {"classes": classes, "knn_agreement_latent": {}, "knn_agreement_projection": {},
                 "silhouette_latent": None, "silhouette_projection": None}
        for tag, dist in (("latent", dist_high), ("projection", dist_low)):
            counts = knn_agreement_counts(dist, codes, ks)
            for c, k in enumerate(ks):
                entry[f"knn_agreement_{tag}"][k] = float(counts[:, c].sum()) / (n * k)
            if 2 <= len(classes) <= MAX_CLASSES:
                s = silhouette(dist, codes, len(classes))
                entry[f"silhouette_{tag}"] = float(s.sum() / n)
                points[f"silhouette_{tag}_{name}"] = s
        report["labels"][name] = entry
    return report, points


def report(high, low, neighbors=(5, 15, 40), labels=None, dtype=np.float64):
    """``report_from_distances`` on numpy distances of the fp32-rounded rows, computed in ``dtype``."""
    high, low = np.asarray(high, np.float32), np.asarray(low, np.float32)
    return report_from_distances(pairwise(high, dtype), pairwise(low, dtype), high.shape[1], neighbors, labels)


def has_row_ties(dist):
    """Whether any row holds two equal off-diagonal distances (scikit-learn breaks such ties by an unstable sort)."""
    d = np.asarray(dist, dtype=np.float64).copy()
    np.fill_diagonal(d, -1.0)
    s = np.sort(d, axis=1)[:, 1:]
    return bool((np.diff(s, axis=1) == 0).any())


def golden_inputs(seed, n, d, noise):
    """Seeded fp32 rows of three loose clusters, a noisy linear 2-D projection of them, and two label sets."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((3, d)) * 1.5
    group = np.arange(n) % 3
    high = (centre[group] + rng.standard_normal((n, d))).astype(np.float32)
    low = (high.astype(np.float64) @ rng.standard_normal((d, 2)) / np.sqrt(d) + noise * rng.standard_normal((n, 2))).astype(np.float32)
    patient = [f"p{v:02d}" for v in rng.integers(0, max(2, n // 6), size=n)]
    patient[-3:] = ["single0", "single1", "single2"]       # labels with one row: silhouette 0
    return high, low, {"group": [("edente", "dente", "other")[g] for g in group], "patient": patient}

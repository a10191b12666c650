"""numpy oracle of the two-sample permutation tests (csrc/two_sample.hip, analysis/two_sample.py): int64 / fp64 throughout,
nothing shared with the code under test but ``permutation_masks`` (the labellings are an input, equal by construction)."""
import numpy as np

from pti_ldm_vae_amd.analysis.two_sample import fixed_strata, permutation_masks

HALF_ZONE = 1e-9          # an entry whose fp64 value lies this close to a half-integer may round either way on the device


def forms_loops(w, masks):
    """(A, R, C) of every labelling from the definition, by explicit loops (tiny cases only)."""
    n = len(w)
    out = []
    for s in masks:
        a = r = c = 0
        for i in range(n):
            for j in range(n):
                a += int(s[i]) * int(w[i][j]) * int(s[j])
                r += int(s[i]) * int(w[i][j])
                c += int(s[j]) * int(w[i][j])
        out.append((a, r, c))
    return np.array(out, dtype=np.int64)


def forms(w, masks):
    """A = s^T W s, R = s . (W 1), C = s . (W^T 1) per row s of masks -> int64 [P, 3].  Exact below 2^63."""
    w = np.asarray(w).astype(np.int64)
    s = (np.asarray(masks) != 0).astype(np.int64)
    t = s @ w
    return np.stack([(t * s).sum(1), s @ w.sum(1), s @ w.sum(0)], axis=1)


def pairwise(z):
    """fp32 Euclidean distances, differences first (the bits are NOT the device's; the GPU tests hand the device's matrix on)."""
    z = np.asarray(z, dtype=np.float32)
    d = z[:, None, :] - z[None, :, :]
    return np.sqrt((d * d).sum(-1, dtype=np.float32)).astype(np.float32)


def lower_median(dist):
    n = dist.shape[0]
    tri = np.asarray(dist, dtype=np.float32)[np.triu_indices(n, 1)]
    k = (tri.size - 1) // 2
    return np.partition(tri, k)[k]


def kernel_matrix(dist, kind, scale, bandwidths=(0.5, 1.0, 2.0)):
    """-> (int64 [n, n] in [0, 65535], bool [n, n]: the entries within HALF_ZONE of a half-integer before rounding)."""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    n = d.shape[0]
    scale = float(np.float32(scale))
    if not scale > 0.0:
        return np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=bool)
    if kind == "energy":
        v = 65535.0 * d / scale
    else:
        acc = np.zeros_like(d)
        for b in bandwidths:
            sigma = float(b) * scale
            acc = acc + np.exp(-(d * d) / (2.0 * sigma * sigma))
        v = 65535.0 * (acc / float(len(bandwidths)))
    near = np.abs(v - np.floor(v) - 0.5) < HALF_ZONE
    w = np.clip(np.rint(v), 0, 65535).astype(np.int64)
    eye = np.eye(n, dtype=bool)
    w[eye] = 0
    near[eye] = False
    return w, near


def knn_table(dist, k):
    """The k nearest columns of every row by (distance, column), the diagonal competing like any other: pti_umap_knn's order."""
    return np.argsort(np.asarray(dist, dtype=np.float32), axis=1, kind="stable")[:, :k].astype(np.int32)


def knn_indicator(knn_idx, n):
    w = np.zeros((n, n), dtype=np.int64)
    for i, row in enumerate(np.asarray(knn_idx)):
        for j in row:
            if 0 <= j < n and j != i:
                w[i, j] = 1
    return w


def statistics(table, n_a, n_b, kind, neighbors=0):
    """fp64 statistic per labelling from the integer table [P + 2, 3] (observed, relabellings, all-ones)."""
    table = np.asarray(table, dtype=np.int64)
    total = int(table[-1, 0])
    out = []
    for a, r, c in table[:-1].tolist():
        b = total - r - c + a
        x = r + c - 2 * a
        if kind == "mmd":
            out.append(float(a) / float(n_a * (n_a - 1)) + float(b) / float(n_b * (n_b - 1)) - float(x) / float(n_a * n_b))
        elif kind == "energy":
            out.append(float(x) / float(n_a * n_b) - float(a) / float(n_a * n_a) - float(b) / float(n_b * n_b))
        else:
            out.append(float(a + b) / float((n_a + n_b) * neighbors))
    return np.array(out, dtype=np.float64)


def two_sample(dist, n_a, n_b, *, permutations=9999, seed=0, strata=None, neighbors=5, bandwidths=(0.5, 1.0, 2.0)):
    """The whole test from the pooled fp32 distance matrix -> dict per test of the integer table, ``exceed``, ``p_value``,
    ``statistic`` (reported units), the null distribution and the weight matrix; plus ``masks`` and the fixed-row counts."""
    dist = np.asarray(dist, dtype=np.float32)
    n = n_a + n_b
    masks = permutation_masks(n_a, n_b, permutations, seed, strata)
    table = np.concatenate([masks, np.ones((1, n), dtype=np.uint8)])
    median, dmax = float(lower_median(dist)), float(dist.max())
    mats = {"mmd": kernel_matrix(dist, "gaussian", median, bandwidths)[0], "energy": kernel_matrix(dist, "energy", dmax)[0],
            "knn": knn_indicator(knn_table(dist, neighbors + 1), n)}
    units = {"mmd": 1.0 / 65535.0, "energy": dmax / 65535.0, "knn": 1.0}
    out = {"masks": masks, "fixed": fixed_strata(n_a, n_b, strata), "median": median, "max": dmax}
    for kind, w in mats.items():
        tab = forms(w, table)
        raw = statistics(tab, n_a, n_b, kind, neighbors)
        exceed = int((raw[1:] >= raw[0]).sum())
        out[kind] = {"forms": tab, "exceed": exceed, "p_value": (1 + exceed) / (permutations + 1),
                     "statistic": float(raw[0] * units[kind]), "null": raw[1:] * units[kind], "w": w}
    return out

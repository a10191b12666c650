"""fp64 numpy statement of the device-side UMAP (csrc/umap.hip), stage by stage: the k nearest neighbours of
a distance matrix ordered by (distance, column), umap-learn's ``smooth_knn_dist`` / ``compute_membership_strengths`` / fuzzy
union (``set_op_mix_ratio = 1``, ``local_connectivity = 1``, ``bandwidth = 1``) as a thresholded CSR graph with the integer
edge schedule, and the layout epoch in its buffered (Jacobi) form with the counter-based negative sampling.  Beside them a
numpy trustworthiness and a sequential, in-place, umap-learn-style layout from the same graph, start, schedule and hash:
the quality reference.  ``find_ab_params`` is the package's own numpy fit (pinned to scipy in ``tests/test_umap_cpu.py``).

Functions that take ``dtype`` run the same statements in fp32 throughout with ``np.float32``: the plain fp32 restatement
whose distance from the fp64 result sets the tests' bounds.

    python tests/umap_oracle.py        # measures every bound on the CPU, writes tests/golden/umap_golden.npz (minutes)
"""
from __future__ import annotations

import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pti_ldm_vae_amd.analysis.latent_space import find_ab_params  # noqa: E402,F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umap_golden.npz")
U32 = np.uint32
MIN_DIST = 0.5                                             # the project's default: a, b = find_ab_params(1.0, 0.5)
SEED = 42
TRUST_K = 15

# name -> (rows, n_neighbors, n_epochs, seed of the rows).  Seeds and epoch counts are chosen so that no weight lies within
# the graph bound of the threshold wmax / n_epochs (``build`` asserts it): with k = 200 of 300 rows the weights are dense
# around 1 / 200, so that case thresholds at 1 / 20.
CASES = {"n3k2": (3, 2, 200, 21), "n97dup": (97, 15, 200, 22), "n300k40": (300, 40, 200, 24), "n300k200": (300, 200, 20, 23),
         "n700hub": (700, 15, 200, 24), "n1030k40": (1030, 40, 200, 25)}
EPOCH_CASES = ("n97dup", "n300k40", "n700hub")

Graph = namedtuple("Graph", "indptr indices weights rate rho sigma wmax row")


# ---- inputs ------------------------------------------------------------------------------------------------------------
def make_rows(name: str) -> np.ndarray:
    """Seeded fp32 rows.  ``n3k2``: three points.  ``n97dup``: Gaussian rows, then 57 points of an integer grid (exact
    distance ties), rows 0-2 identical (zero distances).  ``n300*``: 12 overlapping Gaussian clusters in 50 columns.
    ``n700hub`` / ``n1030k40``: row 0 at the origin, row i near axis i at radius about 1 -- the origin is every row's
    nearest neighbour, so its row of the symmetric graph holds every other row."""
    n, _, _, seed = CASES[name]
    rng = np.random.default_rng(seed)
    if name == "n3k2":
        rows = rng.normal(0.0, 1.0, (3, 5))
    elif name == "n97dup":
        rows = rng.normal(0.0, 2.0, (n, 4))
        rows[40:] = rng.integers(-3, 4, (n - 40, 4))
        rows[1] = rows[0]
        rows[2] = rows[0]
    elif name.startswith("n300"):
        rows = rng.normal(0.0, 1.5, (12, 50))[rng.integers(0, 12, n)] + rng.normal(0.0, 1.0, (n, 50))
    else:
        rows = 0.01 * rng.normal(0.0, 1.0, (n, n))
        rows[np.arange(1, n), np.arange(1, n)] += 1.0 + 0.05 * rng.uniform(-1.0, 1.0, n - 1)
        rows[0] = 0.0
    return rows.astype(np.float32)


def distances(rows: np.ndarray) -> np.ndarray:
    """fp32 [n, n] Euclidean distances, fp64 sums of squared differences; exact zeros on the diagonal and for duplicates."""
    x = np.asarray(rows, np.float64)
    return np.stack([np.sqrt(((x[i] - x) ** 2).sum(-1)) for i in range(len(x))]).astype(np.float32)


def pca_init(rows: np.ndarray) -> np.ndarray:
    """The first two principal components, each min-max scaled to [0, 10] (umap-learn's rescaling of any init), fp32."""
    x = np.asarray(rows, np.float64)
    x = x - x.mean(axis=0)
    u, s, _ = np.linalg.svd(x, full_matrices=False)
    y = np.zeros((len(x), 2))
    y[:, :min(2, len(s))] = (u * s)[:, :2]
    y *= np.where(y[np.argmax(np.abs(y), axis=0), np.arange(2)] < 0, -1.0, 1.0)
    return scale_init(y)


def scale_init(y: np.ndarray) -> np.ndarray:
    y = np.asarray(y, np.float64)
    span = np.ptp(y, axis=0)
    return (10.0 * (y - y.min(axis=0)) / np.where(span > 0, span, 1.0)).astype(np.float32)


# ---- stage 1: neighbours -------------------------------------------------------------------------------------------------
def knn(dist: np.ndarray, k: int):
    """The k smallest entries of every row ascending by (distance, column) -> (int32 [n, k], fp32 [n, k]).  One 64-bit key
    per entry: the bits of the non-negative fp32 distance above the column."""
    d = np.ascontiguousarray(np.asarray(dist, np.float32) + np.float32(0.0))
    n = d.shape[1]
    key = (d.view(U32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    key = np.sort(key, axis=1)[:, :k]
    return (key & np.uint64(0xFFFFFFFF)).astype(np.int32), (key >> np.uint64(32)).astype(U32).view(np.float32)


# ---- stage 2: the graph ----------------------------------------------------------------------------------------------------
def smooth_knn(knn_dist: np.ndarray, tol=1e-5, dtype=np.float64):
    """``smooth_knn_dist`` -> (rho fp32 [n], sigma [n]).  rho: the smallest non-zero distance of the row (0 if none).
    sigma: from 1, doubling while no upper bound is known and bisecting after, at most 64 rounds, stop at
    |sum_{j=1..k-1} (d_j - rho > 0 ? exp(-(d_j - rho) / sigma) : 1) - log2 k| < tol; then floored at 1e-3 times the
    row's mean distance (rho > 0) or the mean of all kNN distances (rho = 0)."""
    d = np.asarray(knn_dist, np.float32)
    n, k = d.shape
    target, tol = dtype(np.log2(np.float64(k))), dtype(tol)
    mean_all = d.astype(np.float64).mean()
    rho, sigma = np.zeros(n, np.float32), np.zeros(n, dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(n):
            nz = d[i][d[i] > 0]
            if nz.size:
                rho[i] = nz[0]
            dd = d[i, 1:].astype(dtype) - dtype(rho[i])
            pos = dd > 0
            lo, hi, mid = dtype(0.0), dtype(np.inf), dtype(1.0)
            for _ in range(64):
                psum = np.where(pos, np.exp(-dd / mid), dtype(1.0)).sum(dtype=dtype)
                if abs(psum - target) < tol:
                    break
                if psum > target:
                    hi = mid
                    mid = (lo + hi) / dtype(2.0)
                else:
                    lo = mid
                    mid = mid * dtype(2.0) if np.isinf(hi) else (lo + hi) / dtype(2.0)
            floor = dtype(1e-3) * dtype(d[i].astype(np.float64).mean() if rho[i] > 0 else mean_all)
            sigma[i] = max(mid, floor)
    return rho, sigma


def strengths(knn_idx, knn_dist, rho, sigma, dtype=np.float64) -> np.ndarray:
    """``compute_membership_strengths`` scattered into a dense [n, n] matrix: 0 for the row itself, 1 for d - rho <= 0,
    exp(-(d - rho) / sigma) otherwise."""
    n, k = knn_idx.shape
    dd = np.asarray(knn_dist, np.float32).astype(dtype) - rho.astype(dtype)[:, None]
    with np.errstate(over="ignore", under="ignore"):
        val = np.where(dd > 0, np.exp(-np.maximum(dd, 0) / sigma.astype(dtype)[:, None]), dtype(1.0))
    val = np.where(knn_idx == np.arange(n)[:, None], dtype(0.0), val).astype(dtype)
    a = np.zeros((n, n), dtype)
    a[np.arange(n)[:, None], knn_idx] = val
    return a


def rates(weights32: np.ndarray, wmax32) -> np.ndarray:
    """floor(w * 2^20 / wmax) of fp32 weights as int32: exact (a quotient of two 24-bit numbers never lies within 2^-53 of
    an integer it does not reach)."""
    return np.floor(weights32.astype(np.float64) * 1048576.0 / np.float64(wmax32)).astype(np.int32)


def fuzzy_graph(knn_idx, knn_dist, n_epochs: int, tol=1e-5, dtype=np.float64) -> Graph:
    """w = a + a^T - a o a^T, entries with w * n_epochs < wmax dropped, as CSR with ascending columns; ``weights`` fp32
    (``dense_weights`` gives them unrounded), ``rate`` from the fp32 weights."""
    rho, sigma = smooth_knn(knn_dist, tol, dtype)
    w = dense_weights(knn_idx, knn_dist, rho, sigma, dtype)
    wmax = w.max()
    keep = (w > 0) & (w * dtype(n_epochs) >= wmax)
    row, col = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    w32 = w[row, col].astype(np.float32)
    return Graph(indptr, col.astype(np.int32), w32, rates(w32, np.float32(wmax)), rho, sigma, float(wmax), row.astype(np.int32))


def dense_weights(knn_idx, knn_dist, rho, sigma, dtype=np.float64) -> np.ndarray:
    a = strengths(knn_idx, knn_dist, rho, sigma, dtype)
    return a + a.T - a * a.T


def fires(rate: np.ndarray, e: int) -> np.ndarray:
    """The edge with this rate is sampled in epoch e: umap-learn's epochs_per_sample = wmax / w in integer form."""
    r = rate.astype(np.int64)
    return (((e + 1) * r) >> 20) > ((e * r) >> 20)


# ---- stage 3: the layout ---------------------------------------------------------------------------------------------------
def lowbias32(h: np.ndarray) -> np.ndarray:
    h = np.asarray(h).astype(U32)
    with np.errstate(over="ignore"):
        h ^= h >> U32(16)
        h *= U32(0x7FEB352D)
        h ^= h >> U32(15)
        h *= U32(0x846CA68B)
        h ^= h >> U32(16)
    return h


def negatives(p: np.ndarray, s: int, e: int, seed: int, n: int, nsr: int) -> np.ndarray:
    """The negative vertex of sample s of the edge at CSR position p in epoch e."""
    base = lowbias32(np.array([(seed + e) & 0xFFFFFFFF], dtype=np.uint64))[0]
    h = lowbias32(base ^ ((p.astype(np.uint64) * np.uint64(nsr) + np.uint64(s)) & np.uint64(0xFFFFFFFF)).astype(U32))
    return ((h.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _pull(y, i, j, a, b, repel, dtype):
    """clip4(g * (y_i - y_j)) per pair: g_att (repel False) or g_rep (True); 0 where the two points coincide."""
    diff = y[i] - y[j]
    d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
    ok = d2 > 0
    d2s = np.where(ok, d2, dtype(1.0))
    if repel:
        g = dtype(2.0) * b / ((dtype(0.001) + d2s) * (a * np.power(d2s, b) + dtype(1.0)))
    else:
        g = dtype(-2.0) * a * b * np.power(d2s, b - dtype(1.0)) / (a * np.power(d2s, b) + dtype(1.0))
    g = np.where(ok, g, dtype(0.0)).astype(dtype)
    return np.clip(g[:, None] * diff, dtype(-4.0), dtype(4.0))


def epoch_jacobi(g: Graph, y, a, b, alpha, e: int, seed: int, nsr: int = 5, dtype=np.float64) -> np.ndarray:
    """One buffered epoch: y_out[i] = y[i] + alpha (2 sum_fired clip4(g_att (y_i - y_j)) + sum_fired sum_s clip4(g_rep (y_i - y_v)))."""
    y = np.asarray(y, dtype)
    a, b = dtype(a), dtype(b)
    p = np.nonzero(fires(g.rate, e))[0]
    i, j = g.row[p], g.indices[p]
    acc = np.zeros_like(y)
    np.add.at(acc, i, dtype(2.0) * _pull(y, i, j, a, b, False, dtype))
    for s in range(nsr):
        np.add.at(acc, i, _pull(y, i, negatives(p, s, e, seed, len(y), nsr), a, b, True, dtype))
    return y + dtype(alpha) * acc


def layout_jacobi(g: Graph, y0, a, b, n_epochs: int, seed: int, nsr: int = 5, stop=None, dtype=np.float64) -> np.ndarray:
    y = np.asarray(y0, dtype)
    for e in range(n_epochs if stop is None else stop):
        y = epoch_jacobi(g, y, a, b, 1.0 - e / n_epochs, e, seed, nsr, dtype)
    return y


def layout_sequential(g: Graph, y0, a, b, n_epochs: int, seed: int, nsr: int = 5) -> np.ndarray:
    """umap-learn's ``optimize_layout_euclidean`` sweep (in place, edge by edge, both ends of an edge move) over the same
    graph, start, schedule and negative samples.  Plain Python floats: only the quality reference."""
    y = [[float(v[0]), float(v[1])] for v in np.asarray(y0, np.float64)]
    n = len(y)

    def clip(v):
        return 4.0 if v > 4.0 else (-4.0 if v < -4.0 else v)

    for e in range(n_epochs):
        alpha = 1.0 - e / n_epochs
        p = np.nonzero(fires(g.rate, e))[0]
        heads, tails = g.row[p].tolist(), g.indices[p].tolist()
        neg = np.stack([negatives(p, s, e, seed, n, nsr) for s in range(nsr)], axis=1).tolist() if nsr else [[]] * len(heads)
        for t in range(len(heads)):
            cur, oth = y[heads[t]], y[tails[t]]
            dx, dy = cur[0] - oth[0], cur[1] - oth[1]
            d2 = dx * dx + dy * dy
            if d2 > 0.0:
                pw = math.pow(d2, b)
                gc = -2.0 * a * b * (pw / d2) / (a * pw + 1.0)
                mx, my = clip(gc * dx) * alpha, clip(gc * dy) * alpha
                cur[0] += mx
                cur[1] += my
                oth[0] -= mx
                oth[1] -= my
            for v in neg[t]:
                oth = y[v]
                dx, dy = cur[0] - oth[0], cur[1] - oth[1]
                d2 = dx * dx + dy * dy
                if d2 > 0.0:
                    gc = 2.0 * b / ((0.001 + d2) * (a * math.pow(d2, b) + 1.0))
                    cur[0] += clip(gc * dx) * alpha
                    cur[1] += clip(gc * dy) * alpha
    return np.array(y)


# ---- measures --------------------------------------------------------------------------------------------------------------
def trustworthiness(x, y, k: int = TRUST_K) -> float:
    """sklearn.manifold.trustworthiness (Euclidean): 1 - 2 / (n k (2n - 3k - 1)) sum_i sum_{j in kNN_Y(i)} max(0, r_X(i, j) - k)."""
    dx, dy = (np.stack([np.sqrt(((v[i] - v) ** 2).sum(-1)) for i in range(len(v))]) for v in (np.asarray(x, np.float64), np.asarray(y, np.float64)))
    n = len(dx)
    np.fill_diagonal(dx, np.inf)
    np.fill_diagonal(dy, np.inf)
    order = np.argsort(dx, axis=1, kind="stable")
    rank = np.zeros((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], order] = np.arange(1, n + 1)
    near = np.argsort(dy, axis=1, kind="stable")[:, :k]
    excess = rank[np.arange(n)[:, None], near] - k
    return float(1.0 - excess[excess > 0].sum() * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))))


def rel_dev(got, want) -> float:
    """max |got - want| / max |want|."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def span_dev(got, want) -> float:
    """max |got - want| over the largest extent of the layout ``want``."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.ptp(want, axis=0).max())


def case_graph(name: str, tol=1e-5, dtype=np.float64):
    """-> (fp32 distances, kNN indices, kNN distances, the graph) of a named case."""
    _, k, n_epochs, _ = CASES[name]
    dist = distances(make_rows(name))
    idx, kd = knn(dist, k)
    return dist, idx, kd, fuzzy_graph(idx, kd, n_epochs, tol, dtype)


def graph_bounds(name: str) -> dict:
    """The graph bounds of one case: twice the larger of the fp32 restatement's deviation from the fp64 oracle and the
    effect of the search's own stopping slack (1e-5 against 1e-10), for sigma and for the weights; and the distance of the
    nearest oracle weight from the threshold wmax / n_epochs, in units of wmax."""
    _, k, n_epochs, _ = CASES[name]
    _, idx, kd, g = case_graph(name)
    w = dense_weights(idx, kd, g.rho, g.sigma)
    out = {}
    devs = {"sigma": [], "w": []}
    for kw in (dict(tol=1e-10), dict(dtype=np.float32)):
        rho2, sigma2 = smooth_knn(kd, **kw)
        assert np.array_equal(rho2, g.rho)
        devs["sigma"].append(rel_dev(sigma2, g.sigma))
        devs["w"].append(rel_dev(dense_weights(idx, kd, rho2, sigma2, kw.get("dtype", np.float64)), w))
    for key, (tol_dev, f32_dev) in devs.items():
        out[f"{key}_dev_tol_{name}"], out[f"{key}_dev_fp32_{name}"] = tol_dev, f32_dev
        out[f"{key}_bound_{name}"] = 2.0 * max(tol_dev, f32_dev)
    out[f"thr_gap_{name}"] = float(np.abs(w[w > 0] - g.wmax / n_epochs).min() / g.wmax)
    out[f"graph_checksum_{name}"] = np.array([float(g.indptr[-1]), float(g.weights.astype(np.float64).sum()),
                                              float(g.rate.astype(np.int64).sum()), float(g.sigma.sum())])
    return out


def restarted_epochs(g: Graph, y0, a, b, n_epochs: int, step, stop: int = 10) -> float:
    """Epochs 0 .. stop - 1 one at a time, each from the fp64 trajectory rounded to fp32: the largest ``span_dev`` of
    ``step(e, y32)`` from the fp64 epoch on the same start.  Ten epochs compared pointwise without the dynamics between
    them (which amplify a last-bit difference about sixfold per epoch while alpha is near 1)."""
    y, worst = np.asarray(y0, np.float64), 0.0
    for e in range(stop):
        y32 = y.astype(np.float32)
        y = epoch_jacobi(g, y32, a, b, 1.0 - e / n_epochs, e, SEED)
        worst = max(worst, span_dev(step(e, y32), y))
    return worst


def epoch_bounds(name: str, a: float, b: float) -> dict:
    """1 and 10 epochs from the case's scaled PCA start: the fp64 layouts, and twice the fp32 restatement's deviation;
    the same for the ten epochs taken one at a time (``restarted_epochs``)."""
    _, _, n_epochs, _ = CASES[name]
    g = case_graph(name)[3]
    y0 = pca_init(make_rows(name))
    out = {f"y0_{name}": y0}
    dev = restarted_epochs(g, y0, a, b, n_epochs, lambda e, y32: epoch_jacobi(g, y32, a, b, 1.0 - e / n_epochs, e, SEED, dtype=np.float32))
    out[f"restart_fp32_dev_{name}"], out[f"restart_bound_{name}"] = dev, 2.0 * dev
    for stop in (1, 10):
        want = layout_jacobi(g, y0, a, b, n_epochs, SEED, stop=stop)
        got = layout_jacobi(g, y0, a, b, n_epochs, SEED, stop=stop, dtype=np.float32)
        out[f"y{stop}_{name}"] = want
        out[f"epoch_fp32_dev_{stop}_{name}"] = span_dev(got, want)
        out[f"epoch_bound_{stop}_{name}"] = 2.0 * span_dev(got, want)
    return out


def quality(a: float, b: float) -> dict:
    """The gate of the full run on n300k40: trustworthiness of the start, of the Jacobi layout, of the sequential layout,
    and the spread of the latter over five negative-sampling seeds."""
    name = "n300k40"
    rows, n_epochs = make_rows(name), CASES[name][2]
    g = case_graph(name)[3]
    y0 = pca_init(rows)
    t_seq = trustworthiness(rows, layout_sequential(g, y0, a, b, n_epochs, SEED))
    seeds = [trustworthiness(rows, layout_sequential(g, y0, a, b, n_epochs, s)) for s in (1, 2, 3, 4, 5)]
    return {"trust_start": trustworthiness(rows, y0), "trust_jacobi": trustworthiness(rows, layout_jacobi(g, y0, a, b, n_epochs, SEED)),
            "trust_seq": t_seq, "trust_seq_seeds": np.array(seeds), "trust_margin": 3.0 * float(np.ptp(seeds))}


def build() -> dict:
    """Everything the golden file holds; deterministic."""
    a, b = find_ab_params(1.0, MIN_DIST)
    out = {"ab": np.array([a, b]), "rows_n97dup": make_rows("n97dup")}
    for name in CASES:
        out.update(graph_bounds(name))
        # the sparsity pattern is compared exactly: no weight may sit within the bound of the threshold
        assert out[f"thr_gap_{name}"] > out[f"w_bound_{name}"], (name, out[f"thr_gap_{name}"], out[f"w_bound_{name}"])
    for name in EPOCH_CASES:
        out.update(epoch_bounds(name, a, b))
    out.update(quality(a, b))
    return out


if __name__ == "__main__":
    gold = build()
    np.savez_compressed(GOLDEN, **gold)
    for key, v in gold.items():
        if np.ndim(v) == 0 or np.size(v) <= 5:
            print(key, v)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")

"""fp64 numpy statement of the device-side UMAP transform (csrc/umap.hip), stage by stage: the PCA model and
its projection of new rows through the centred cross Gram matrix, the k nearest TRAINING rows of every new row,
umap-learn's transform preamble (``rho = 0``, the sigma search, bipartite strengths, the thresholded integer schedule, the
weighted-mean start point) and the layout of new rows against a frozen embedding, rounded to fp32 after every epoch.
Beside them the quality measure of the full path: the share of a new row's nearest training rows that stay its nearest
training points in the plane.  Inputs, kNN, schedule, hash and the pair forces are those of ``umap_oracle``.

Functions that take ``dtype`` run the same statements in fp32 throughout with ``np.float32``: the plain fp32 restatement
whose distance from the fp64 result sets the tests' bounds.

    python tests/umap_transform_oracle.py    # measures every bound on the CPU, writes tests/golden/umap_transform_golden.npz
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np

import umap_oracle as O
from umap_oracle import fires, knn, make_rows, negatives, rates, rel_dev, span_dev  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umap_transform_golden.npz")
SEED = O.SEED
INITIAL_ALPHA = 0.25                                       # umap-learn's transform: the fit's initial alpha / 4
SHARE_K = 15
QUALITY_SEEDS = (42, 1, 2, 3, 4, 5)
QUALITY_FIT = (40, 200)                                    # n_neighbors, n_epochs of the fit behind the quality case
QUALITY_T = 100
QUALITY_T_DEFAULT = QUALITY_FIT[1] // 3                    # what transform(new) runs after that fit

# name -> (row set of umap_oracle, training rows, k, transform epochs)
CASES = {"t97": ("n97dup", 70, 15, 100), "t300k40": ("n300k40", 220, 40, 100), "t300k200": ("n300k40", 220, 200, 100),
         "thub": ("n700hub", 600, 15, 100)}
T_SHORT = {"t97": 10}                                      # a second epoch count at which slots are dropped
EPOCH_CASES = ("t97", "t300k40", "thub")

TGraph = namedtuple("TGraph", "indices weights w32 rate sigma wmax y0")


# ---- inputs ------------------------------------------------------------------------------------------------------------
def split(name: str):
    """-> (training rows, new rows), fp32.  ``t97``: the new rows end in copies of training rows 0, 45 and 45: exact zero
    distances (row 0 has two duplicates among the training rows, so its copy sees three)."""
    rows_name, n_train = CASES[name][:2]
    rows = make_rows(rows_name)
    train, new = rows[:n_train], rows[n_train:]
    if name == "t97":
        new = np.concatenate([new, train[[0, 45, 45]]])
    return train, new


def cross_distances(new: np.ndarray, train: np.ndarray) -> np.ndarray:
    """fp32 [m, n] Euclidean distances from new rows to training rows, fp64 sums of squared differences."""
    x, t = np.asarray(new, np.float64), np.asarray(train, np.float64)
    return np.stack([np.sqrt(((row - t) ** 2).sum(-1)) for row in x]).astype(np.float32)


def train_embedding(name: str) -> np.ndarray:
    """The frozen embedding of the operator-level cases: the training rows' scaled PCA start, fp32 [n, 2]."""
    return O.pca_init(split(name)[0])


# ---- PCA model -----------------------------------------------------------------------------------------------------------
def pca_fit(x: np.ndarray, c: int, dtype=np.float64):
    """-> (embedding [N, c], mean [D], axes [N, c] = U signs / sqrt(lambda)) by the Gram route of ``fit_pca``; ``dtype`` is
    that of the centring and of the Gram matrix, the eigen-decomposition is fp64 either way."""
    x = np.asarray(x, dtype)
    mean = x.mean(axis=0, dtype=dtype)
    xc = x - mean
    lam, u = np.linalg.eigh((xc @ xc.T).astype(np.float64))
    lam, u = np.clip(lam[::-1], 0.0, None)[:c], u[:, ::-1][:, :c].copy()
    signs = np.sign(u[np.argmax(np.abs(u), axis=0), np.arange(c)])
    signs[signs == 0] = 1.0
    keep = lam > max(x.shape) * np.finfo(np.float64).eps * lam.max()
    return u * signs * np.sqrt(lam), mean, np.where(keep, u * signs / np.sqrt(np.where(keep, lam, 1.0)), 0.0)


def pca_transform(new: np.ndarray, x: np.ndarray, mean: np.ndarray, axes: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(new - mean) (x - mean)^T in ``dtype``, times the axes in fp64 -> fp64 [m, c]."""
    cross = (np.asarray(new, dtype) - mean.astype(dtype)) @ (np.asarray(x, dtype) - mean.astype(dtype)).T
    return cross.astype(np.float64) @ axes


# ---- the transform graph -------------------------------------------------------------------------------------------------
def smooth_rho0(knn_dist: np.ndarray, tol=1e-5, dtype=np.float64) -> np.ndarray:
    """``smooth_knn_dist`` with ``local_connectivity - 1 = 0``: rho = 0 for every row, sigma from 1, doubling while no upper
    bound is known and bisecting after, at most 64 rounds, stop at |sum_{t=1..k-1} (d_t > 0 ? exp(-d_t / sigma) : 1) -
    log2 k| < tol; floored at 1e-3 times the mean of ALL distances."""
    d = np.asarray(knn_dist, np.float32)
    m, k = d.shape
    target, tol = dtype(np.log2(np.float64(k))), dtype(tol)
    floor = dtype(1e-3) * dtype(d.astype(np.float64).mean())
    sigma = np.zeros(m, dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(m):
            dd = d[i, 1:].astype(dtype)
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
            sigma[i] = max(mid, floor)
    return sigma


def transform_graph(knn_idx, knn_dist, y_train, n_epochs: int, tol=1e-5, dtype=np.float64) -> TGraph:
    """``weights`` [m, k] in ``dtype`` (1 for d <= 0, exp(-d / sigma) otherwise; no self exclusion), ``w32`` the same
    rounded to fp32; ``wmax``, the threshold ``w n_epochs >= wmax`` and ``rate`` (0 where dropped) from the fp32 weights;
    ``y0`` = sum_t w_t Y[idx_t] / sum_t w_t over all k slots, rounded to fp32."""
    d = np.asarray(knn_dist, np.float32).astype(dtype)
    sigma = smooth_rho0(knn_dist, tol, dtype)
    with np.errstate(under="ignore"):
        w = np.where(d > 0, np.exp(-d / sigma[:, None]), dtype(1.0)).astype(dtype)
    w32 = w.astype(np.float32)
    wmax = w32.max()
    keep = (w32 > 0) & (w32.astype(np.float64) * n_epochs >= np.float64(wmax))
    rate = np.where(keep, rates(w32, wmax), 0).astype(np.int32)
    y = np.asarray(y_train, np.float32).astype(dtype)[knn_idx]                          # [m, k, 2]
    y0 = ((w[:, :, None] * y).sum(axis=1, dtype=dtype) / w.sum(axis=1, dtype=dtype)[:, None]).astype(np.float32)
    return TGraph(np.asarray(knn_idx, np.int32), w, w32, rate, sigma, float(wmax), y0)


# ---- the layout ------------------------------------------------------------------------------------------------------------
def epoch(indices, rate, y, y_train, a, b, alpha, e: int, seed: int, nsr: int = 5, dtype=np.float64) -> np.ndarray:
    """One epoch, unrounded: y[i] + alpha sum_fired (clip4(g_att (y_i - Y[idx])) + sum_s clip4(g_rep (y_i - Y[v]))); slot t
    of row i has position p = i k + t; a slot whose index lies outside [0, n) never fires."""
    y, yt = np.asarray(y, dtype), np.asarray(y_train, np.float32).astype(dtype)
    (m, k), n = indices.shape, len(yt)
    a, b = dtype(a), dtype(b)
    fire = fires(rate, e) & (rate > 0) & (indices >= 0) & (indices < n)
    i, t = np.nonzero(fire)
    p = i * k + t
    both = np.concatenate([y, yt])
    acc = np.zeros_like(y)
    np.add.at(acc, i, O._pull(both, i, m + indices[i, t], a, b, False, dtype))
    for s in range(nsr):
        np.add.at(acc, i, O._pull(both, i, m + negatives(p, s, e, seed, n, nsr), a, b, True, dtype))
    return y + dtype(alpha) * acc


def alpha_at(e: int, n_epochs: int) -> float:
    return INITIAL_ALPHA * (1.0 - e / n_epochs)


def layout(indices, rate, y0, y_train, a, b, n_epochs: int, seed: int, start: int = 0, stop=None, nsr: int = 5,
           dtype=np.float64, round_last: bool = True) -> np.ndarray:
    """Epochs start .. stop - 1; the points are rounded to fp32 after every epoch (part of the statement: it is what makes
    one launch equal to many) -> fp32 [m, 2].  ``round_last=False`` leaves the last epoch's result in ``dtype``: what a
    rounded result is compared with."""
    y = np.asarray(y0, np.float32)
    stop = n_epochs if stop is None else stop
    for e in range(start, stop):
        y = epoch(indices, rate, y, y_train, a, b, alpha_at(e, n_epochs), e, seed, nsr, dtype)
        if round_last or e + 1 < stop:
            y = y.astype(np.float32)
    return y


def train_span(y_train) -> float:
    return float(np.ptp(np.asarray(y_train, np.float64), axis=0).max())


def tspan_dev(got, want, y_train) -> float:
    """max |got - want| over the largest extent of the training embedding."""
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max() / train_span(y_train))


def restarted_epochs(tg: TGraph, y_train, a, b, n_epochs: int, step, stop: int = 10) -> float:
    """Epochs 0 .. stop - 1 one at a time, each from the oracle's (fp32) trajectory: the largest ``tspan_dev`` of
    ``step(e, y32)`` from the unrounded fp64 epoch on the same start."""
    y32, worst = tg.y0, 0.0
    for e in range(stop):
        want = epoch(tg.indices, tg.rate, y32, y_train, a, b, alpha_at(e, n_epochs), e, SEED)
        worst = max(worst, tspan_dev(step(e, y32), want, y_train))
        y32 = want.astype(np.float32)
    return worst


# ---- measures --------------------------------------------------------------------------------------------------------------
def neighbour_share(new, train, y_new, y_train, k: int = SHARE_K) -> float:
    """The mean share of each new row's k nearest training rows (fp64 Euclidean) that are among its k nearest training
    points in the plane; ties go by the lower row."""
    def near(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.argsort(np.stack([((row - b) ** 2).sum(-1) for row in a]), axis=1, kind="stable")[:, :k]
    lat, plane = near(new, train), near(y_new, y_train)
    return float(np.mean([len(set(p) & set(q)) / k for p, q in zip(lat, plane)]))


def case_graph(name: str, n_epochs=None, tol=1e-5, dtype=np.float64):
    """-> (fp32 cross distances, kNN indices, kNN distances, the frozen embedding, the transform graph) of a named case."""
    train, new = split(name)
    dist = cross_distances(new, train)
    idx, kd = knn(dist, CASES[name][2])
    yt = train_embedding(name)
    return dist, idx, kd, yt, transform_graph(idx, kd, yt, CASES[name][3] if n_epochs is None else n_epochs, tol, dtype)


def graph_bounds(name: str) -> dict:
    """Twice the larger of the fp32 restatement's deviation from the fp64 oracle and the effect of the search's stopping
    slack (1e-5 against 1e-10) for sigma, the weights (both relative to their maximum) and the start points (as a share of
    the training span); the distance of the nearest weight from the threshold wmax / T in units of wmax, for every T of
    the case; the number of dropped slots."""
    _, idx, kd, yt, g = case_graph(name)
    out, devs = {}, {"sigma": [], "w": [], "y0": []}
    for kw in (dict(tol=1e-10), dict(dtype=np.float32)):
        g2 = transform_graph(idx, kd, yt, CASES[name][3], **kw)
        devs["sigma"].append(rel_dev(g2.sigma, g.sigma))
        devs["w"].append(rel_dev(g2.weights, g.weights))
        devs["y0"].append(tspan_dev(g2.y0, g.y0, yt))
    for key, (tol_dev, f32_dev) in devs.items():
        out[f"{key}_dev_tol_{name}"], out[f"{key}_dev_fp32_{name}"] = tol_dev, f32_dev
        out[f"{key}_bound_{name}"] = 2.0 * max(tol_dev, f32_dev)
    for t in (CASES[name][3],) + ((T_SHORT[name],) if name in T_SHORT else ()):
        out[f"thr_gap_{t}_{name}"] = float(np.abs(g.weights - g.wmax / t).min() / g.wmax)
        out[f"dropped_{t}_{name}"] = int((transform_graph(idx, kd, yt, t).rate == 0).sum())
    out[f"y0_{name}"] = g.y0
    out[f"zeros_{name}"] = int((kd == 0).sum())
    return out


def store_dev(want, y_train) -> float:
    """Half an ulp of fp32 at the largest coordinate of ``want`` as a share of the training span: what storing a result as
    fp32 moves it by at most."""
    return float(np.spacing(np.float32(np.abs(want).max()))) / 2.0 / train_span(y_train)


def epoch_bounds(name: str, a: float, b: float) -> dict:
    """1 and 10 epochs from the oracle's start: the oracle's layouts (the last epoch left unrounded), and twice the fp32
    restatement's deviation as a share of the training span; the same for the ten epochs taken one at a time.  Few slots
    fire in the first epochs (in epoch 0 only those of weight wmax), so the restatement samples the rounding of the fp32
    result on a handful of rows; the deviation is therefore taken as at least ``store_dev``, the half ulp that the fp32
    output format itself allows."""
    _, _, _, yt, g = case_graph(name)
    t = CASES[name][3]
    out = {}
    dev = restarted_epochs(g, yt, a, b, t, lambda e, y32: epoch(g.indices, g.rate, y32, yt, a, b, alpha_at(e, t), e, SEED, dtype=np.float32))
    out[f"restart_fp32_dev_{name}"] = dev
    for stop in (1, 10):
        want = layout(g.indices, g.rate, g.y0, yt, a, b, t, SEED, stop=stop, round_last=False)
        got = layout(g.indices, g.rate, g.y0, yt, a, b, t, SEED, stop=stop, dtype=np.float32)
        out[f"y{stop}_{name}"] = want
        out[f"epoch_fp32_dev_{stop}_{name}"] = tspan_dev(got, want, yt)
        out[f"epoch_bound_{stop}_{name}"] = 2.0 * max(tspan_dev(got, want, yt), store_dev(want, yt))
    out[f"store_dev_{name}"] = store_dev(out[f"y10_{name}"], yt)
    out[f"restart_bound_{name}"] = 2.0 * max(dev, out[f"store_dev_{name}"])
    return out


def quality_fit(a: float, b: float):
    """The fit behind the quality case, all on the CPU: ``umap_oracle``'s graph and buffered layout of the training rows of
    ``t300k40`` -> (training rows, new rows, fitted embedding fp32)."""
    train, new = split("t300k40")
    k, n_epochs = QUALITY_FIT
    idx, kd = knn(O.distances(train), k)
    g = O.fuzzy_graph(idx, kd, n_epochs)
    return train, new, O.layout_jacobi(g, O.pca_init(train), a, b, n_epochs, SEED).astype(np.float32)


def quality(a: float, b: float) -> dict:
    """The gates of the public path on ``t300k40``: the neighbour share at the start points, and for six negative-sampling
    seeds after ``QUALITY_T`` epochs and after the default a 200-epoch fit gives (``QUALITY_T_DEFAULT`` = 200 // 3);
    gate = the smallest of the six minus their spread."""
    train, new, yt = quality_fit(a, b)
    idx, kd = knn(cross_distances(new, train), QUALITY_FIT[0])
    out = {}
    for t, tag in ((QUALITY_T, ""), (QUALITY_T_DEFAULT, "_default")):
        g = transform_graph(idx, kd, yt, t)
        shares = [neighbour_share(new, train, layout(g.indices, g.rate, g.y0, yt, a, b, t, s), yt) for s in QUALITY_SEEDS]
        out.update({"share_start": neighbour_share(new, train, g.y0, yt), f"share_seeds{tag}": np.array(shares),
                    f"share_gate{tag}": min(shares) - float(np.ptp(shares))})
    return out


def pca_bounds() -> dict:
    """``PcaModel.transform`` on the rows of ``t300k40`` with 50 components: twice the deviation of the restatement with an
    fp32 centring and Gram matrix from the fp64 one, relative to the largest projection."""
    train, new = split("t300k40")
    emb, mean, axes = pca_fit(train, 50)
    emb32, mean32, axes32 = pca_fit(train, 50, np.float32)
    want = pca_transform(new, train, mean, axes)
    got = pca_transform(new, train, mean32, axes32, np.float32)
    dev = max(rel_dev(got, want), rel_dev(pca_transform(train, train, mean32, axes32, np.float32), emb))
    return {"pca_fp32_dev": dev, "pca_bound": 2.0 * dev}


def build() -> dict:
    """Everything the golden file holds; deterministic."""
    a, b = O.find_ab_params(1.0, O.MIN_DIST)
    out = {"ab": np.array([a, b])}
    for name in CASES:
        out.update(graph_bounds(name))
        for t in (CASES[name][3],) + ((T_SHORT[name],) if name in T_SHORT else ()):
            # the dropped slots are compared exactly: no weight may sit within 100 bounds of the threshold
            assert out[f"thr_gap_{t}_{name}"] > 100.0 * out[f"w_bound_{name}"], (name, t, out[f"thr_gap_{t}_{name}"], out[f"w_bound_{name}"])
    for name in EPOCH_CASES:
        out.update(epoch_bounds(name, a, b))
    out.update(quality(a, b))
    assert min(out["share_gate"], out["share_gate_default"]) > out["share_start"], (out["share_gate"], out["share_gate_default"], out["share_start"])
    out.update(pca_bounds())
    return out


if __name__ == "__main__":
    gold = build()
    np.savez_compressed(GOLDEN, **gold)
    for key, v in gold.items():
        if np.ndim(v) == 0 or np.size(v) <= 6:
            print(key, v)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")

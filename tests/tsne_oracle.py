"""fp64 numpy statement of exact t-SNE as scikit-learn computes it (``sklearn.manifold._t_sne``: ``_joint_probabilities``
with ``_utils._binary_search_perplexity``, ``_kl_divergence``, ``_gradient_descent`` and the two-stage schedule of
``TSNE._tsne``), in dense form and without importing sklearn.  ``tests/test_tsne_cpu.py`` pins it to sklearn's own
functions; ``tests/test_gpu_tsne.py`` checks ``ops.tsne_affinities`` / ``ops.tsne_step`` (csrc/tsne.hip) against it.

Every function takes ``dtype``: with ``np.float32`` the same statements run in fp32 throughout -- the plain fp32
restatement whose distance from the fp64 result sets the tests' bounds.

    python tests/tsne_oracle.py        # writes tests/golden/tsne_golden.npz (about a minute)
"""
from __future__ import annotations

import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)                      # sklearn's MACHINE_EPSILON
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_golden.npz")

# name -> (rows, perplexity, seed, clusters, duplicates and an outlier)
CASES = {"n97": (97, 30.0, 11, 5, False), "n257": (257, 5.0, 12, 6, False), "n97dup": (97, 30.0, 13, 5, True),
         "n300": (300, 30.0, 14, 6, False)}
STEP_CASES = [(name, scale, exag) for name in ("n97", "n300") for scale in (1e-4, 10.0) for exag in (12.0, 1.0)]


def make_rows(name: str) -> np.ndarray:
    """Seeded Gaussian clusters in 50 columns, fp32 [n, 50].  ``n97dup``: rows 0-2 identical, row 3 offset by +1000."""
    n, _, seed, clusters, dup = CASES[name]
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (clusters, 50))
    rows = centres[rng.integers(0, clusters, n)] + rng.normal(0.0, 1.0, (n, 50))
    if dup:
        rows[1] = rows[0]
        rows[2] = rows[0]
        rows[3] += 1000.0
    return rows.astype(np.float32)


def squared_distances(rows: np.ndarray) -> np.ndarray:
    """fp32 [n, n] squared Euclidean distances, computed in fp64 from differences; exact zeros on the diagonal."""
    x = np.asarray(rows, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return d2.astype(np.float32)


def step_embedding(name: str, scale: float) -> np.ndarray:
    """The seeded fp32 [n, 2] embedding of a one-step case: N(0, scale^2)."""
    n, _, seed, _, _ = CASES[name]
    return (np.random.default_rng(seed + 1000).standard_normal((n, 2)) * scale).astype(np.float32)


def pca_init(rows: np.ndarray) -> np.ndarray:
    """sklearn's ``init="pca"``: the first two principal components, scaled to a population std of 1e-4 in column 0, fp32."""
    x = np.asarray(rows, np.float64)
    x = x - x.mean(axis=0)
    u, s, _ = np.linalg.svd(x, full_matrices=False)
    y = u[:, :2] * s[:2]
    y *= np.sign(y[np.argmax(np.abs(y), axis=0), np.arange(2)])
    return (y / y[:, 0].std() * 1e-4).astype(np.float32)


def conditional_probabilities(d2, perplexity, tol=1e-5, dtype=np.float64) -> np.ndarray:
    """``_binary_search_perplexity`` on a full matrix, all rows at once: beta from 1, at most 100 steps, doubling / halving
    while a bound is infinite and bisection after, stop at |H - log(perplexity)| <= tol.  sklearn holds the tolerance,
    the perplexity and the 1e-8 that replaces a zero row sum as C floats; so does this."""
    d = np.asarray(d2, np.float32).astype(dtype)
    n = d.shape[0]
    tol, tiny = dtype(np.float32(tol)), dtype(np.float32(1e-8))
    target = dtype(np.log(np.float64(np.float32(perplexity))))
    beta, lo, hi = np.ones(n, dtype), np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
    cond = np.zeros((n, n), dtype)
    active = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for _ in range(100):
            if active.size == 0:
                break
            b, da = beta[active], d[active]
            p = np.exp(-da * b[:, None])
            p[np.arange(active.size), active] = 0
            s = p.sum(axis=1)
            s[s == 0] = tiny
            p /= s[:, None]
            diff = np.log(s) + b * (da * p).sum(axis=1) - target
            cond[active] = p
            done = np.abs(diff) <= tol
            up = active[(diff > 0) & ~done]
            dn = active[~(diff > 0) & ~done]
            lo[up] = beta[up]
            beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2, (beta[up] + hi[up]) / 2)
            hi[dn] = beta[dn]
            beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] / 2, (beta[dn] + lo[dn]) / 2)
            active = active[~done]
    return cond


def joint_probabilities(d2, perplexity, tol=1e-5, dtype=np.float64) -> np.ndarray:
    """``_joint_probabilities`` as a dense [n, n] matrix: max((p_j|i + p_i|j) / sum, eps), zero diagonal."""
    cond = conditional_probabilities(d2, perplexity, tol, dtype)
    p = cond + cond.T
    p = np.maximum(p / np.maximum(p.sum(), dtype(EPS)), dtype(EPS))
    np.fill_diagonal(p, 0)
    return p


def condensed(p: np.ndarray) -> np.ndarray:
    """The upper triangle in scipy's ``squareform`` order."""
    return p[np.triu_indices(p.shape[0], 1)]


def kl_and_grad(P, Y, exaggeration=1.0, dtype=np.float64):
    """``_kl_divergence`` with one degree of freedom on a dense P -> (KL(exaggeration * P || Q), gradient [n, 2])."""
    p = np.asarray(P, dtype) * dtype(exaggeration)
    y = np.asarray(Y, dtype)
    diff = y[:, None, :] - y[None, :, :]
    num = 1 / (1 + (diff ** 2).sum(-1))
    np.fill_diagonal(num, 0)
    q = np.maximum(num / num.sum(), dtype(EPS))
    off = ~np.eye(len(y), dtype=bool)
    kl = (p[off] * np.log(np.maximum(p[off], dtype(EPS)) / q[off])).sum()
    grad = 4 * (((p - q) * num)[:, :, None] * diff).sum(axis=1)
    return kl, grad


def one_step(P, y, update, gains, exaggeration, momentum, lr, dtype=np.float64):
    """One iteration of ``_gradient_descent`` -> (KL at y, |gain * grad|, new y, new update, new gains)."""
    kl, grad = kl_and_grad(P, y, exaggeration, dtype)
    inc = update * grad < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    grad = grad * gains
    update = dtype(momentum) * update - dtype(lr) * grad
    return kl, np.sqrt((grad.astype(np.float64) ** 2).sum()), y + update, update, gains


def learning_rate(n: int, early_exaggeration: float = 12.0) -> float:
    return max(n / early_exaggeration / 4.0, 50.0)


def descend(P, Y0, max_iter=1000, exploration_n_iter=250, early_exaggeration=12.0, dtype=np.float64):
    """``TSNE._tsne`` (sklearn 1.7, ``learning_rate="auto"``): momentum 0.5 with exaggeration for ``exploration_n_iter``
    iterations, then 0.8 without up to ``max_iter``; every 50 iterations stop on |grad| <= 1e-7 or when KL has not improved
    for more than ``exploration_n_iter`` (stage 1) / 300 (stage 2) iterations -> (Y, KL at the returned Y, iterations run)."""
    y = np.asarray(Y0, dtype).copy()
    lr = learning_rate(len(y), early_exaggeration)
    update, gains = np.zeros_like(y), np.ones_like(y)
    it = 0
    for stop, momentum, exag, patience in ((min(exploration_n_iter, max_iter), 0.5, early_exaggeration, exploration_n_iter),
                                           (max_iter, 0.8, 1.0, 300)):
        best, best_it = np.inf, it
        for i in range(it, stop):
            kl, norm, y, update, gains = one_step(P, y, update, gains, exag, momentum, lr, dtype)
            it = i + 1
            if (i + 1) % 50 == 0:
                if kl < best:
                    best, best_it = kl, i
                elif i - best_it > patience:
                    break
                if norm <= 1e-7:
                    break
    return y, float(kl_and_grad(P, y, 1.0, dtype)[0]), it


def rel_dev(got, want) -> float:
    """max |got - want| / max |want|."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def host_sums(p32: np.ndarray) -> np.ndarray:
    """{sum P log P, sum P} of an fp32 P in fp64: what ``ops.tsne_affinities`` returns beside P."""
    p = p32.astype(np.float64)
    nz = p[p > 0]
    return np.array([(nz * np.log(nz)).sum(), nz.sum()])


def build() -> dict:
    """Everything the golden file holds; deterministic."""
    out = {"rows_n97": make_rows("n97")}
    for name, (n, perplexity, _, _, _) in CASES.items():
        d2 = squared_distances(make_rows(name))
        p = joint_probabilities(d2, perplexity)
        dev_tol = rel_dev(p, joint_probabilities(d2, perplexity, tol=1e-10))
        dev_f32 = rel_dev(joint_probabilities(d2, perplexity, dtype=np.float32), p)
        out[f"aff_dev_tol_{name}"], out[f"aff_dev_fp32_{name}"] = dev_tol, dev_f32
        out[f"aff_bound_{name}"] = 2.0 * max(dev_tol, dev_f32)
        if n < 100:
            out[f"p_{name}"] = p
        out[f"p_checksum_{name}"] = np.array([p.sum(), (p * np.arange(n)[:, None]).sum(), p.max()])
    for name, scale, exag in STEP_CASES:
        n, perplexity = CASES[name][:2]
        p32 = joint_probabilities(squared_distances(make_rows(name)), perplexity).astype(np.float32)
        y = step_embedding(name, scale)
        lr = learning_rate(n)
        zero, one = np.zeros((n, 2)), np.ones((n, 2))
        kl, norm, _, upd, _ = one_step(p32, y, zero, one, exag, 0.5, lr)
        kl32, norm32, _, upd32, _ = one_step(p32, y, zero.astype(np.float32), one.astype(np.float32), exag, 0.5, lr, np.float32)
        tag = f"{name}_{scale:g}_{exag:g}"
        out[f"step_kl_{tag}"], out[f"step_norm_{tag}"], out[f"step_update_{tag}"] = kl, norm, upd
        # ONE bound per case, twice the largest relative deviation of the fp32 restatement over the three quantities: KL
        # and the norm are single numbers, and one fp32 draw of a single number can land arbitrarily close to the fp64
        # value (the norm of n97 / 10 / 12 does, at 2e-9), which says nothing about the arithmetic's error scale
        devs = np.array([rel_dev(upd32, upd), abs(float(kl32) - kl) / abs(kl), abs(float(norm32) - norm) / abs(norm)])
        out[f"step_fp32_dev_{tag}"] = devs
        out[f"step_bound_{tag}"] = 2.0 * devs.max()
    # trajectories at n = 300
    rows = make_rows("n300")
    p = joint_probabilities(squared_distances(rows), CASES["n300"][1])
    y0 = pca_init(rows)
    out["y0_n300"] = y0
    y10, _, _ = descend(p, y0, max_iter=10, exploration_n_iter=5)
    y10_32, _, _ = descend(p.astype(np.float32), y0, max_iter=10, exploration_n_iter=5, dtype=np.float32)
    out["y10_n300"], out["traj_bound_n300"] = y10, 2.0 * rel_dev(y10_32, y10)
    _, kl_full, iters = descend(p, y0)
    out["kl_full_n300"], out["iters_full_n300"] = kl_full, iters
    rng = np.random.default_rng(99)
    kls = [descend(p, (y0 * (1.0 + 1e-6 * rng.standard_normal(y0.shape))).astype(np.float32))[1] for _ in range(5)]
    out["kl_perturbed_n300"] = np.array(kls)
    out["kl_spread_n300"] = (max(kls) - min(kls)) / kl_full
    return out


if __name__ == "__main__":
    gold = build()
    np.savez_compressed(GOLDEN, **gold)
    for k, v in gold.items():
        if np.ndim(v) == 0 or np.size(v) <= 5:
            print(k, v)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")

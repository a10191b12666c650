"""Shared by ``tools/make_latent_golden.py`` and the latent-analysis tests: the seeded inputs of
``tests/golden/latent_analysis_golden.npz`` (so that the D = 40 960 case is regenerated instead of stored), the plain fp32
CPU restatement whose error is recorded beside every expected array, and the error measures."""
from __future__ import annotations

import numpy as np
import torch

PATIENTS = [str(100 + i) for i in range(1, 10)]
COUNTS_A = [12, 1, 6, 5, 0, 8, 4, 7, 5]      # 48 rows; one patient with a single row, one absent
COUNTS_B = [5, 6, 1, 7, 4, 0, 9, 3, 5]       # 40 rows
SPECTRUM = [1.0, 0.7, 0.5, 0.35, 0.25, 0.18]  # patient-level directions: a decaying spectrum for the PCA case
PCA_COMPONENTS = len(SPECTRUM)


def make_latents(seed: int, d: int):
    """-> (a [48, d] fp32, ids_a, b [40, d] fp32, ids_b): every row = a shared offset (about 3, scale 2) + patient-level
    noise along six directions of decaying weight + sample noise of 0.01 / 0.05 / 0.2, so that near-duplicate rows
    with a large common mean occur.  Rows come in shuffled patient order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    offset = 3.0 + 2.0 * rng.standard_normal(d)
    directions = rng.standard_normal((len(SPECTRUM), d))
    coeff = rng.standard_normal((len(PATIENTS), len(SPECTRUM))) * np.asarray(SPECTRUM)
    centre = coeff @ directions

    def group(counts):
        ids = [p for p, c in zip(PATIENTS, counts) for _ in range(c)]
        order = rng.permutation(len(ids))
        ids = [ids[i] for i in order]
        scale = rng.choice([0.01, 0.05, 0.2], size=len(ids))
        rows = np.stack([offset + centre[PATIENTS.index(p)] + s * rng.standard_normal(d) for p, s in zip(ids, scale)])
        return rows.astype(np.float32), ids

    a, ids_a = group(COUNTS_A)
    b, ids_b = group(COUNTS_B)
    return a, ids_a, b, ids_b


def rel_err(got, ref) -> float:
    """Largest elementwise |got - ref| / |ref| (absolute where ref == 0); NaN positions must coincide."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    g, r = got[ok], ref[ok]
    return float(np.max(np.abs(g - r) / np.where(r == 0, 1.0, np.abs(r))))


def component_err(got, ref) -> float:
    """Largest per-column relative L2 error."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.linalg.norm(got - ref, axis=0) / np.linalg.norm(ref, axis=0)))


def sign_rule(proj):
    """Flip each column so that its entry of largest magnitude is positive (sklearn svd_flip, u-based; the columns of
    U sqrt(lambda) and of U share the position of that entry)."""
    proj = np.array(proj, dtype=np.float64)
    top = np.argmax(np.abs(proj), axis=0)
    signs = np.sign(proj[top, np.arange(proj.shape[1])])
    signs[signs == 0] = 1.0
    return proj * signs


def segments(ids):
    """-> (row order grouped by PATIENTS, offsets [len(PATIENTS) + 1])."""
    order = [i for p in PATIENTS for i, q in enumerate(ids) if q == p]
    counts = [sum(1 for q in ids if q == p) for p in PATIENTS]
    return order, [0] + list(np.cumsum(counts))


# ---- plain fp32 CPU restatement (torch): direct differences, two-pass std, fp32 Gram -> fp64 eigh ----
def fp32_cdist(a, b):
    a, b = torch.from_numpy(np.ascontiguousarray(a)).float(), torch.from_numpy(np.ascontiguousarray(b)).float()
    return torch.stack([((b - row) ** 2).sum(dim=1).sqrt() for row in a]).numpy()


def fp32_metrics(a, b):
    a, b = torch.from_numpy(np.ascontiguousarray(a)).float(), torch.from_numpy(np.ascontiguousarray(b)).float()
    if len(a) == 0 or len(b) == 0:
        return [float("nan")] * 4

    def std(x):
        if len(x) < 2:
            return 0.0
        return float(((x - x.mean(dim=0)) ** 2).mean(dim=0).sqrt().mean())

    centre = float(((a.mean(dim=0) - b.mean(dim=0)) ** 2).sum().sqrt())
    return [centre, std(a), std(b), float(fp32_cdist(a.numpy(), b.numpy()).astype(np.float64).mean())]


def fp32_pca(x, k):
    x = torch.from_numpy(np.ascontiguousarray(x)).float()
    xc = x - x.mean(dim=0)
    gram = (xc @ xc.t()).double().numpy()
    lam, u = np.linalg.eigh(gram)
    lam, u = np.clip(lam[::-1], 0, None), u[:, ::-1]
    return sign_rule(u[:, :k] * np.sqrt(lam[:k])), lam[:k] / np.trace(gram)

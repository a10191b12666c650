"""Is the difference between two groups of latent rows more than chance?  Three two-sample permutation tests on one pooled
distance matrix: the unbiased MMD^2 of a Gaussian kernel mixture, the energy distance, and Schilling-Henze's
share of nearest neighbours with the same label.

Every test is a bilinear form of a fixed matrix ``W`` in the 0/1 group labelling ``s``.  ``W`` is quantised ONCE to integers
in [0, 65535] (``ops.two_sample_kernel`` / ``ops.knn_indicator``), so for every relabelling the three sums
``A = s^T W s``, ``R = s . (W 1)``, ``C = s . (W^T 1)`` are exact integers (``ops.permutation_forms``, the int8 matrix cores)
and the p-value is a count.  A permutation test is valid for any fixed kernel, so the quantisation costs resolution
(2^-17 of the kernel's range per entry), not validity.  The labellings come from ``permutation_masks`` on the host; the
statistics are formed on the host in fp64 from the integers.
"""
from __future__ import annotations

import numpy as np
import torch

LEVELS = 65536
TESTS = ("mmd", "energy", "knn")
_CHUNK = 256


def _strata_index(n_a: int, n_b: int, strata):
    """-> [(rows of the stratum ascending, how many of them are A-rows)] in order of first appearance."""
    n = n_a + n_b
    strata = list(strata)
    if len(strata) != n:
        raise ValueError(f"permutation_masks: strata must name all {n} pooled rows, got {len(strata)}")
    rows: dict = {}
    for i, key in enumerate(strata):
        rows.setdefault(key, []).append(i)
    return [(np.asarray(idx, dtype=np.int64), sum(1 for i in idx if i < n_a)) for idx in rows.values()]


def fixed_strata(n_a: int, n_b: int, strata=None) -> tuple[int, int]:
    """(strata, rows) that no relabelling can change: the strata that hold rows of one group only."""
    if strata is None:
        return 0, 0
    one_sided = [idx for idx, count in _strata_index(n_a, n_b, strata) if count in (0, len(idx))]
    return len(one_sided), int(sum(len(idx) for idx in one_sided))


def permutation_masks(n_a: int, n_b: int, permutations: int, seed: int, strata=None) -> np.ndarray:
    """The labellings of a permutation test -> uint8 ``[permutations + 1, n_a + n_b]`` of 0/1, 1 = group A; the pooled rows
    hold A first.  Row 0 is the observed labelling.  Every further row draws one key per pooled row from
    ``numpy.random.Generator(PCG64(seed))`` (``rng.random(n)``) and gives label A to the ``n_a`` smallest keys (equal keys:
    the lower row first).  With ``strata`` (one patient id per pooled row) label A goes, within each stratum, to as many of
    its smallest keys as the stratum holds A-rows; a stratum with rows of one group only keeps its labels."""
    n_a, n_b, permutations = int(n_a), int(n_b), int(permutations)
    if n_a < 1 or n_b < 1:
        raise ValueError(f"permutation_masks: both groups need rows, got n_a={n_a} n_b={n_b}")
    if permutations < 1:
        raise ValueError(f"permutation_masks: permutations must be at least 1, got {permutations}")
    n = n_a + n_b
    groups = None if strata is None else _strata_index(n_a, n_b, strata)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    masks = np.zeros((permutations + 1, n), dtype=np.uint8)
    masks[0, :n_a] = 1
    for start in range(1, permutations + 1, _CHUNK):
        rows = min(_CHUNK, permutations + 1 - start)
        keys = rng.random((rows, n))                       # row r of the block is the r-th further rng.random(n)
        block = masks[start:start + rows]
        line = np.arange(rows)[:, None]
        if groups is None:
            block[line, np.argsort(keys, axis=1, kind="stable")[:, :n_a]] = 1
            continue
        for idx, count in groups:
            if count in (0, len(idx)):
                block[:, idx] = masks[0, idx]
            else:
                block[line, idx[np.argsort(keys[:, idx], axis=1, kind="stable")[:, :count]]] = 1
    return masks


def _finite(v):
    v = float(v)
    return v if np.isfinite(v) else None


def evaluate_forms(forms, n_a: int, n_b: int, kind: str, *, neighbors: int = 0, unit: float | None = 1.0,
                    scale=None, bandwidths=None) -> tuple[dict, np.ndarray]:
    """One test's report entry and null distribution from the exact integer table ``forms`` int64 ``[P + 2, 3]`` =
    ``(A, R, C)`` of: the observed labelling, the ``P`` relabellings, and the all-ones labelling (whose ``A`` is the matrix
    total ``T``).  With ``B = T - R - C + A`` and the cross term ``X = R + C - 2 A``, in fp64:
    ``mmd``: ``A / (n_a (n_a - 1)) + B / (n_b (n_b - 1)) - X / (n_a n_b)``; ``energy``: ``X / (n_a n_b) - A / n_a^2 - B / n_b^2``;
    ``knn``: ``(A + B) / (n neighbors)``.  ``p = (1 + #{relabellings with statistic >= observed}) / (P + 1)``, the comparison
    on these fp64 values; ``unit`` scales what is REPORTED (quantum -> the kernel's own units), ``None`` = the test is
    undefined (zero scale) and every value is null."""
    forms = np.asarray(forms, dtype=np.int64)
    perms = forms.shape[0] - 2
    total = int(forms[-1, 0])
    a, r, c = forms[:-1, 0], forms[:-1, 1], forms[:-1, 2]
    b = total - r - c + a
    x = r + c - 2 * a
    af, bf, xf = a.astype(np.float64), b.astype(np.float64), x.astype(np.float64)
    n = n_a + n_b
    if kind == "mmd":
        raw = af / float(n_a * (n_a - 1)) + bf / float(n_b * (n_b - 1)) - xf / float(n_a * n_b)
    elif kind == "energy":
        raw = xf / float(n_a * n_b) - af / float(n_a * n_a) - bf / float(n_b * n_b)
    elif kind == "knn":
        raw = (a + b).astype(np.float64) / float(n * neighbors)
    else:
        raise ValueError(f"evaluate_forms: kind must be one of {TESTS}, got {kind!r}")
    entry = {"statistic": None, "p_value": None, "null_mean": None, "null_std": None, "z": None, "permutations": perms,
             "exceed": None, "scale": None if scale is None else _finite(scale),
             "bandwidths": None if bandwidths is None else [float(v) for v in bandwidths],
             "levels": 2 if kind == "knn" else LEVELS}
    if unit is None:
        return entry, np.full(perms, np.nan)
    exceed = int(np.count_nonzero(raw[1:] >= raw[0]))
    null = raw[1:] * float(unit)
    stat, mean, std = float(raw[0] * float(unit)), float(null.mean()), float(null.std())
    entry.update(statistic=_finite(stat), p_value=(1 + exceed) / (perms + 1), null_mean=_finite(mean), null_std=_finite(std),
                 z=_finite((stat - mean) / std) if std > 0.0 else None, exceed=exceed)
    return entry, null


def check_arguments(n_a: int, n_b: int, permutations: int, neighbors: int, bandwidths) -> None:
    n = n_a + n_b
    if n_a < 2 or n_b < 2:
        raise ValueError(f"two_sample_tests: each group needs at least 2 rows, got {n_a} and {n_b}")
    if n > 8192:
        raise ValueError(f"two_sample_tests: at most 8192 pooled rows, got {n}")
    if not 1 <= permutations <= 65534:
        raise ValueError(f"two_sample_tests: permutations must be 1 .. 65534, got {permutations}")
    if not (1 <= neighbors <= 255 and neighbors + 1 < n):
        raise ValueError(f"two_sample_tests: neighbors must be 1 .. 255 and below n - 1 = {n - 1}, got {neighbors}")
    if not 1 <= len(bandwidths) <= 8 or not all(0.0 < float(b) < float("inf") for b in bandwidths):
        raise ValueError(f"two_sample_tests: bandwidths must be 1 .. 8 positive finite values, got {bandwidths!r}")


def build_report(entries: dict, n_a: int, n_b: int, seed: int, neighbors: int, strata) -> dict:
    fixed = fixed_strata(n_a, n_b, strata)
    return {"n_a": n_a, "n_b": n_b, "stratified": strata is not None, "fixed_strata": fixed[0], "fixed_rows": fixed[1],
            "seed": int(seed), "neighbors": int(neighbors), "tests": entries}


def two_sample_tests(latents_a, latents_b, *, permutations: int = 9999, seed: int = 0, strata_a=None, strata_b=None,
                     neighbors: int = 5, bandwidths=(0.5, 1, 2), device=None) -> tuple[dict, dict]:
    """The three permutation tests of rows ``latents_a`` [n_a, D] against ``latents_b`` [n_b, D] (arrays or tensors) on
    ``device`` -> ``(report, arrays)``.  The rows are pooled A first; one ``ops.latent_pairwise`` call gives the distances,
    ``ops.distance_median`` the Gaussian scale, ``ops.two_sample_kernel`` / ``ops.umap_knn`` + ``ops.knn_indicator`` the three
    integer matrices; ONE mask table (``permutation_masks`` plus an all-ones row for the matrix totals) serves the three
    ``ops.permutation_forms`` calls, and one packed copy brings everything to the host.  ``strata_a`` / ``strata_b`` (a
    patient id per row, both or neither) restrict the relabellings to exchanges within a patient.

    ``report``: ``n_a``, ``n_b``, ``stratified``, ``fixed_strata``, ``fixed_rows``, ``seed``, ``neighbors`` and per test
    (``tests["mmd" | "energy" | "knn"]``) ``statistic``, ``p_value``, ``null_mean``, ``null_std``, ``z``, ``permutations``,
    ``exceed`` and the quantum ``scale``, ``bandwidths``, ``levels``.  Undefined values (all rows equal: zero scale; a null
    distribution without spread: ``z``) are None, never NaN.  ``arrays``: ``null_<test>`` fp64 [P], ``forms_<test>`` int64
    [P + 2, 3] (observed, relabellings, all-ones), ``masks`` uint8 [P + 1, n] and ``witness`` fp64 [n], the per-row
    ``mean_{j in A} w_ij - mean_{j in B} w_ij`` of the Gaussian matrix in kernel units.  Deterministic for a seed."""
    from .. import ops
    if device is None:
        device = torch.device("cuda")
    if (strata_a is None) != (strata_b is None):
        raise ValueError("two_sample_tests: give strata for both groups or for neither")
    rows = []
    for name, x in (("latents_a", latents_a), ("latents_b", latents_b)):
        t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
        if t.dim() != 2 or not t.is_floating_point():
            raise ValueError(f"two_sample_tests: {name} must be a floating-point [rows, D] matrix, got {tuple(t.shape)} {t.dtype}")
        rows.append(t.to(device=device, dtype=torch.float32))
    if rows[0].shape[1] != rows[1].shape[1]:
        raise ValueError(f"two_sample_tests: the groups have {rows[0].shape[1]} and {rows[1].shape[1]} columns")
    n_a, n_b = rows[0].shape[0], rows[1].shape[0]
    permutations, neighbors = int(permutations), int(neighbors)
    bandwidths = [float(b) for b in bandwidths]
    check_arguments(n_a, n_b, permutations, neighbors, bandwidths)
    n = n_a + n_b
    strata = None if strata_a is None else list(strata_a) + list(strata_b)
    masks = permutation_masks(n_a, n_b, permutations, seed, strata)
    table = torch.from_numpy(np.concatenate([masks, np.ones((1, n), dtype=np.uint8)])).to(device)

    dist = ops.latent_pairwise(torch.cat(rows))
    scales = torch.empty(2, dtype=torch.float32, device=device)
    ops.distance_median(dist, out=scales[0])
    w_gauss = ops.two_sample_kernel(dist, "gaussian", scale=scales[0], bandwidths=bandwidths)
    w_energy = ops.two_sample_kernel(dist, "energy", scale_out=scales[1])
    knn_idx, _ = ops.umap_knn(dist, neighbors + 1)
    w_knn = ops.knn_indicator(knn_idx, n)
    forms = [ops.permutation_forms(w, table) for w in (w_gauss, w_energy, w_knn)]
    sums = ops.segment_row_sums(w_gauss.to(torch.float32), [0, n_a, n])          # entries <= 65535: exact in fp32
    packed = torch.cat([f.reshape(-1) for f in forms] + [sums.reshape(-1).view(torch.int64),
                                                         scales.to(torch.float64).view(torch.int64)]).cpu().numpy()
    per = (permutations + 2) * 3
    tables = [packed[i * per:(i + 1) * per].reshape(-1, 3) for i in range(3)]
    sums = packed[3 * per:3 * per + 2 * n].view(np.float64).reshape(n, 2)
    median, dmax = (float(v) for v in packed[3 * per + 2 * n:].view(np.float64))

    entries, arrays = {}, {"masks": masks}
    spec = (("mmd", tables[0], dict(unit=1.0 / 65535.0 if median > 0.0 else None, scale=median, bandwidths=bandwidths)),
            ("energy", tables[1], dict(unit=dmax / 65535.0 if dmax > 0.0 else None, scale=dmax)),
            ("knn", tables[2], dict(neighbors=neighbors)))
    for name, forms_host, extra in spec:
        entries[name], arrays[f"null_{name}"] = evaluate_forms(forms_host, n_a, n_b, name, **extra)
        arrays[f"forms_{name}"] = forms_host.copy()
    arrays["witness"] = (sums[:, 0] / float(n_a) - sums[:, 1] / float(n_b)) / 65535.0
    return build_report(entries, n_a, n_b, seed, neighbors, strata), arrays

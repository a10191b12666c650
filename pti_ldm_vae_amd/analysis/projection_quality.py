"""How faithful a 2-D projection of the latents is, and how separate the labelled groups are in either space.

``projection_quality(high, low, ...)`` rates any projection -- whichever backend made it -- from data the analysis already has
on the device: the two ``n x n`` distance matrices (``ops.latent_pairwise`` for the latents; ``ops.projection_distances`` for the
projection, formed in fp64 and rounded once), exact neighbour tables (``ops.umap_knn``), and
two streaming passes over the matrices, ``ops.neighbor_ranks`` (integer ranks) and ``ops.segment_row_sums`` (per-label fp64
sums; csrc/projection_quality.hip).  Per admitted ``k``:

* ``trustworthiness`` (scikit-learn's ``manifold.trustworthiness``): are the neighbours the picture shows real?
* ``continuity``: the same with the spaces swapped -- are real neighbours kept together?
* ``neighborhood_preservation``: the mean share of the ``k`` nearest rows the two spaces have in common.

Per label set (``group``, ``patient``): the share of a row's ``k`` nearest other rows that carry its label, and scikit-learn's
silhouette, each in the latent space and in the projection.  Ties in a row go to the lower column (``umap_knn``'s order).
All counts are integers summed exactly; the ratios are formed on the host in fp64.  Limits: 4 .. 8192 rows, ``k`` <= 255,
at most 2048 classes for a silhouette, Euclidean distances in fp32."""
from __future__ import annotations

import numpy as np
import torch

MAX_ROWS, MIN_ROWS, MAX_NEIGHBORS, MAX_CLASSES = 8192, 4, 255, 2048


def _device_rows(x, name: str, device, who: str = "projection_quality") -> torch.Tensor:
    """-> fp32 device matrix; a non-finite value is refused (for a device tensor through one read-back)."""
    if isinstance(x, torch.Tensor):
        if x.dim() != 2:
            raise ValueError(f"{who}: {name}: expected a matrix, got {tuple(x.shape)}")
        t = x.to(device, torch.float32)
        finite = bool(torch.isfinite(t).all())
    else:
        a = np.asarray(x)
        if a.ndim != 2:
            raise ValueError(f"{who}: {name}: expected a matrix, got {a.shape}")
        a = np.ascontiguousarray(a, dtype=np.float32)
        finite = bool(np.isfinite(a).all())
        t = torch.from_numpy(a).to(device)
    if not finite:
        raise ValueError(f"{who}: {name} holds a non-finite value")
    return t


def admitted_neighbors(neighbors, n: int) -> tuple[list[int], dict[int, str]]:
    """-> (the ``k`` with ``k < n / 2`` in the order given, ``{k: reason}`` of the others): scikit-learn's condition."""
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


def label_codes(labels) -> tuple[list, np.ndarray]:
    """-> (classes in sorted order -- by ``str`` when the labels do not compare --, int64 codes ``[n]``)."""
    labels = [v.item() if isinstance(v, np.generic) else v for v in labels]
    try:
        classes = sorted(set(labels))
    except TypeError:
        classes = sorted(set(labels), key=str)
    index = {c: i for i, c in enumerate(classes)}
    return classes, np.array([index[v] for v in labels], dtype=np.int64)


def nearest_others(dist: torch.Tensor, k: int) -> torch.Tensor:
    """The ``k`` nearest OTHER rows of every row of ``dist``, ascending by (distance, column) -> int32 ``[n, k]``:
    ``umap_knn`` with ``k + 1`` columns minus the row's own index wherever it stands (with duplicate rows it need not be
    first); a row whose own index is absent keeps the first ``k``.  No host sync."""
    from .. import ops
    idx, _ = ops.umap_knn(dist, k + 1)
    n = idx.shape[0]
    own = idx == torch.arange(n, device=idx.device, dtype=idx.dtype)[:, None]
    pos = torch.where(own.any(dim=1), own.int().argmax(dim=1), torch.full((n,), k, device=idx.device))
    cols = torch.arange(k, device=idx.device)[None, :]
    return idx.gather(1, cols + (cols >= pos[:, None]).long()).contiguous()


def _silhouette(sums: np.ndarray, b: np.ndarray, codes: np.ndarray, sizes: np.ndarray) -> np.ndarray:
    """``sums``: the own-label distance sum of every row, ``b``: the smallest mean distance to another label."""
    own = sizes[codes]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums / (own - 1)
        s = (b - a) / np.maximum(a, b)
    s[own == 1] = 0.0
    return np.nan_to_num(s, nan=0.0)


def projection_quality(high, low, *, neighbors=(5, 15, 40), labels=None, device) -> tuple[dict, dict]:
    """-> (report, per-point arrays).  ``high`` ``[n, d]``: the latent rows as given to the projection (before any PCA);
    ``low`` ``[n, 2]``; numpy arrays or device tensors.  ``labels``: ``{name: sequence of n hashable labels}``.

    The report: ``n``, ``high_dims``, ``neighbors`` (the admitted ``k``), ``excluded`` (``{k: reason}`` for ``k >= n / 2``),
    ``trustworthiness`` / ``continuity`` / ``neighborhood_preservation`` (``{k: value}``) and ``labels`` (``{name: {classes,
    knn_agreement_latent, knn_agreement_projection, silhouette_latent, silhouette_projection}}``; a silhouette is ``None`` with
    fewer than 2 classes or more than 2048).  No value is ever NaN.  The arrays: ``trustworthiness_local`` and
    ``continuity_local`` ``[n, K]`` (their column means are the global values) and ``silhouette_latent_<name>`` /
    ``silhouette_projection_<name>`` ``[n]``.  All device results reach the host in one packed copy."""
    from .. import ops
    neighbors = [int(k) for k in neighbors]
    if neighbors and max(neighbors) > MAX_NEIGHBORS:
        raise ValueError(f"projection_quality: at most {MAX_NEIGHBORS} neighbours, got {max(neighbors)}")
    device = torch.device(device)
    x, y = _device_rows(high, "high", device), _device_rows(low, "low", device)
    n = x.shape[0]
    if y.shape[0] != n:
        raise ValueError(f"projection_quality: high has {n} rows, low {y.shape[0]}")
    if n > MAX_ROWS:
        raise ValueError(f"projection_quality: {n} rows; at most {MAX_ROWS} (the distance matrices and one row in LDS)")
    if n < MIN_ROWS:
        raise ValueError(f"projection_quality: {n} rows; at least {MIN_ROWS}")
    if y.shape[1] > ops.PROJECTION_MAX_COLS:
        raise ValueError(f"projection_quality: low has {y.shape[1]} columns; a projection has at most {ops.PROJECTION_MAX_COLS}")
    label_sets = []
    for name, values in (labels or {}).items():
        if len(values) != n:
            raise ValueError(f"projection_quality: label set {name!r} has {len(values)} entries for {n} rows")
        label_sets.append((name,) + label_codes(values))
    ks, excluded = admitted_neighbors(neighbors, n)
    dists = (ops.latent_pairwise(x), ops.projection_distances(y))

    packed = []                                            # int64 device vectors; fp64 results travel as their bits
    if ks:
        kmax = max(ks)
        knn = tuple(nearest_others(d, kmax) for d in dists)
        r_hl = ops.neighbor_ranks(dists[0], knn[1]).long()   # rank in the latent space of the projection's neighbours
        r_lh = ops.neighbor_ranks(dists[1], knn[0]).long()
        for k in ks:
            packed += [(r_hl[:, :k] - k).clamp_(min=0).sum(dim=1), (r_lh[:, :k] - k).clamp_(min=0).sum(dim=1),
                       (r_hl[:, :k] <= k).sum(dim=1)]
    for _, classes, codes in label_sets:
        dcodes = torch.from_numpy(codes).to(device)
        order = torch.from_numpy(np.argsort(codes, kind="stable")).to(device)
        sizes = np.bincount(codes, minlength=len(classes))
        seg = [0] + [int(v) for v in np.cumsum(sizes)]
        for space in range(2):
            if ks:
                same = (dcodes[knn[space].long()] == dcodes[:, None]).long().cumsum(dim=1)
                packed += [same[:, k - 1].sum().reshape(1) for k in ks]
            if 2 <= len(classes) <= MAX_CLASSES:
                sums = ops.segment_row_sums(dists[space].index_select(1, order), seg)      # fp64 [n, classes]
                own = sums.gather(1, dcodes[:, None])[:, 0]
                mean = sums / torch.from_numpy(sizes).to(device, torch.float64)[None, :]
                mean.scatter_(1, dcodes[:, None], float("inf"))
                packed += [own.view(torch.int64), mean.min(dim=1).values.view(torch.int64)]
    host = torch.cat([p.reshape(-1) for p in packed]).cpu().numpy() if packed else np.zeros(0, np.int64)

    at = 0

    def take(count, as_float=False):
        nonlocal at
        v = host[at:at + count]
        at += count
        return v.view(np.float64) if as_float else v

    report = {"n": n, "high_dims": int(x.shape[1]), "neighbors": list(ks), "excluded": excluded,
              "trustworthiness": {}, "continuity": {}, "neighborhood_preservation": {}, "labels": {}}
    points = {"trustworthiness_local": np.zeros((n, len(ks))), "continuity_local": np.zeros((n, len(ks)))}
    for c, k in enumerate(ks):
        scale = 2.0 / (k * (2.0 * n - 3.0 * k - 1.0))
        trust, cont, shared = take(n), take(n), take(n)
        report["trustworthiness"][k] = 1.0 - float(trust.sum()) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
        report["continuity"][k] = 1.0 - float(cont.sum()) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
        report["neighborhood_preservation"][k] = float(shared.sum()) / (n * k)
        points["trustworthiness_local"][:, c] = 1.0 - trust * scale
        points["continuity_local"][:, c] = 1.0 - cont * scale
    for name, classes, codes in label_sets:
        sizes = np.bincount(codes, minlength=len(classes))
        entry = {"classes": classes, "knn_agreement_latent": {}, "knn_agreement_projection": {},
                 "silhouette_latent": None, "silhouette_projection": None}
        for tag in ("latent", "projection"):
            for k in ks:
                entry[f"knn_agreement_{tag}"][k] = float(take(1)[0]) / (n * k)
            if 2 <= len(classes) <= MAX_CLASSES:
                s = _silhouette(take(n, True), take(n, True), codes, sizes)
                entry[f"silhouette_{tag}"] = float(s.sum() / n)
                points[f"silhouette_{tag}_{name}"] = s
        report["labels"][name] = entry
    return report, points

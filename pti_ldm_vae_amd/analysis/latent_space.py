"""Latent-space analysis of a trained VAE (reference ``src/pti_ldm_vae/analysis/latent_space.py``: same names, signatures,
error texts and output files).

What differs is where the arithmetic runs.  The latents of all images stay on the device as one ``[N, D]`` matrix
(D = 4 096 .. 40 960); the per-patient distance statistics of all patients come out of ONE ``ops.latent_group_stats``
call, and PCA takes the centred Gram matrix ``Xc Xc^T`` from ``ops.latent_pairwise(mode="dot", center=mean)`` and
diagonalises that N x N matrix in fp64 on the host.  Only results cross to the host.  The default UMAP and t-SNE are
host libraries fed with the PCA output; ``reduce_dimensionality_tsne(backend="hip")`` is exact t-SNE on the device
(``ops.tsne_affinities`` / ``ops.tsne_step``, csrc/tsne.hip) and ``reduce_dimensionality_umap(backend="hip")`` UMAP on the
device (``ops.umap_knn`` / ``ops.umap_graph`` / ``ops.umap_epoch``, csrc/umap.hip); its ``UmapResult.transform`` places new rows
into the fitted embedding (``PcaModel.transform``, ``ops.umap_knn_cross`` / ``ops.umap_transform_graph`` /
``ops.umap_transform_layout``)."""
from __future__ import annotations

import os
from glob import glob
from pathlib import Path

import numpy as np
import torch

# plotly.express.colors.qualitative.Plotly + Dark24, the palette the reference cycles through (fixed here: plotly is optional)
PATIENT_PALETTE = (
    "#636EFA", "#EF553B", "#00CC96", "#AB63FA", "#FFA15A", "#19D3F3", "#FF6692", "#B6E880", "#FF97FF", "#FECB52",
    "#2E91E5", "#E15F99", "#1CA71C", "#FB0D0D", "#DA16FF", "#222A2A", "#B68100", "#750D86", "#EB663B", "#511CFB",
    "#00A08B", "#FB00D1", "#FC0080", "#B2828D", "#6C7C32", "#778AAE", "#862A16", "#A777F1", "#620042", "#1616A7",
    "#DA60CA", "#6C4516", "#0D2A63", "#AF0038")


def extract_patient_id_from_filename(filename: str) -> str:
    """``"1000_HA_2021_02_545.tif" -> "545"``: the last ``_``-separated part of the name without its extension."""
    stem = filename.rsplit(".", 1)[0] if "." in filename else filename
    return stem.split("_")[-1]


def load_image_paths(data_dir: str, max_images: int | None = None, extensions: list[str] | None = None) -> list[str]:
    """Sorted paths of the files in ``data_dir`` with one of ``extensions`` (default ``.tif`` / ``.tiff``; the leading
    dot is optional), capped to the first ``max_images``."""
    found: list[str] = []
    for ext in extensions if extensions is not None else [".tif", ".tiff"]:
        found.extend(glob(os.path.join(data_dir, f"*{ext if ext.startswith('.') else '.' + ext}")))
    found.sort()
    return found if max_images is None else found[:max_images]


def find_ab_params(spread: float = 1.0, min_dist: float = 0.5) -> tuple[float, float]:
    """umap-learn's ``find_ab_params`` without scipy: the least-squares fit of ``1 / (1 + a x^(2b))`` to the curve that is 1
    below ``min_dist`` and ``exp(-(x - min_dist) / spread)`` above it, on 300 points of [0, 3 spread] -> (a, b).  A damped
    Gauss-Newton iteration from (1, 1), the start ``scipy.optimize.curve_fit`` uses."""
    x = np.linspace(0.0, 3.0 * spread, 300)
    target = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    logx = np.log(np.where(x > 0, x, 1.0))

    def residual(a, b):
        return 1.0 / (1.0 + a * x ** (2.0 * b)) - target

    a, b, damp = 1.0, 1.0, 1e-3
    r = residual(a, b)
    for _ in range(500):
        xb = x ** (2.0 * b)
        f2 = (1.0 / (1.0 + a * xb)) ** 2
        jac = np.stack([-xb * f2, -2.0 * a * logx * xb * f2], axis=1)
        grad, hess = jac.T @ r, jac.T @ jac
        while True:
            step = np.linalg.solve(hess + damp * np.diag(np.diag(hess)), -grad)
            a2, b2 = a + step[0], b + step[1]
            r2 = residual(a2, b2) if a2 > 0 and b2 > 0 else None
            if r2 is not None and r2 @ r2 <= r @ r:
                damp = max(damp / 10.0, 1e-15)
                break
            damp *= 10.0
            if damp > 1e15:
                return float(a), float(b)
        a, b, r = a2, b2, r2
        if np.abs(step).max() <= 1e-14 * max(a, b):
            break
    return float(a), float(b)


class PcaModel:
    """What ``LatentSpaceAnalyzer.fit_pca`` returns: ``embedding_`` fp64 [N, c] (the projections of the training rows, what
    ``reduce_dimensionality_pca`` returns), ``explained_variance_ratio_`` [c], ``mean_`` fp64 [D], and ``transform`` for new
    rows.  The model keeps its own fp32 copy of the training rows on the device (134 MB at 8192 x 4096), so a later change
    of the caller's latents does not reach it: a new row is projected through its centred dot products with them, the
    principal axes are never formed."""

    def __init__(self, rows: torch.Tensor, mean: torch.Tensor, embedding, ratio, u_signed, lam) -> None:
        self._rows, self._mean = rows, mean
        self.embedding_, self.explained_variance_ratio_ = embedding, ratio
        self.mean_ = mean.cpu().double().numpy()
        n, d = rows.shape
        keep = lam > max(n, d) * np.finfo(np.float64).eps * (lam.max() if lam.size else 0.0)
        self._axes = np.where(keep, u_signed / np.sqrt(np.where(keep, lam, 1.0)), 0.0)       # [N, c]: U signs / sqrt(lambda)

    def transform(self, new_rows) -> np.ndarray:
        """-> fp64 [m, c].  The centred cross Gram matrix ``Xnew_c Xc^T`` comes from the device
        (``ops.latent_pairwise(mode="dot", center=mean)``); times ``U signs / sqrt(lambda)`` in fp64 on the host, which is
        ``Xnew_c V``.  A column whose ``lambda`` is not above ``max(N, D) eps lambda_max`` comes out as zero."""
        from .. import ops
        if new_rows.ndim != 2 or new_rows.shape[1] != self._rows.shape[1]:
            raise ValueError(f"Expected [m, {self._rows.shape[1]}] rows (the columns of the fit), got {tuple(new_rows.shape)}")
        if isinstance(new_rows, torch.Tensor):
            x = new_rows.to(self._rows.device, torch.float32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(new_rows, dtype=np.float32)).to(self._rows.device)
        cross = ops.latent_pairwise(x, self._rows, mode="dot", center=self._mean).cpu().double().numpy()
        return cross @ self._axes


class UmapResult:
    """What ``reduce_dimensionality_umap(backend="hip")`` returns beside the embedding (there is no umap-learn model):
    ``embedding_`` fp64 [N, 2] on the host, the curve parameters ``a_`` / ``b_``, ``n_epochs_`` and ``graph_``, the fuzzy
    graph as the device CSR of ``ops.umap_graph``.  With the keyword-only state ``reduce_dimensionality_umap`` adds (the
    ``PcaModel``, the PCA'd training rows and the fp32 embedding on the device, ``n_neighbors``, the seed, whether
    ``n_epochs`` was defaulted) it can ``transform`` new rows."""

    def __init__(self, embedding, a, b, n_epochs, graph, *, pca=None, train_pca=None, train_embedding=None,
                 n_neighbors=None, seed=None, n_epochs_defaulted=None):
        self.embedding_, self.a_, self.b_, self.n_epochs_, self.graph_ = embedding, a, b, n_epochs, graph
        self._pca, self._train_pca, self._train_embedding = pca, train_pca, train_embedding
        self._n_neighbors, self._seed, self._n_epochs_defaulted = n_neighbors, seed, n_epochs_defaulted

    def transform(self, new_latents, n_epochs: int | None = None, random_state: int | None = None) -> np.ndarray:
        """New rows ``[m, D]`` into the fitted embedding -> fp64 [m, 2]; the fit does not change (umap-learn's
        ``UMAP.transform``).  The rows go through the fit's PCA, find their ``n_neighbors`` nearest training rows there
        (exactly), get umap-learn's transform graph and start at the weighted mean of their neighbours' points; then
        ``n_epochs`` epochs against the frozen embedding in one launch.  ``n_epochs=None``: 100 when the fit's was
        defaulted (umap-learn's rule up to 10000 rows), else ``max(1, fit n_epochs // 3)``; 1 <= n_epochs <= 2000.
        ``random_state=None``: the fit's seed.  At most 8192 new rows, not chunked: the sigma floor and the largest weight
        are taken over all of them.  The same arguments give the same bits."""
        from .. import ops
        if self._pca is None or self._train_pca is None or self._train_embedding is None:
            raise RuntimeError("this UmapResult carries no fitted state to transform with: only the result of "
                               "reduce_dimensionality_umap(backend='hip') does")
        if new_latents.ndim != 2:
            raise ValueError(f"Expected 2D array, got {new_latents.ndim}D array")
        m = len(new_latents)
        if not 1 <= m <= 8192:
            raise ValueError(f"transform places 1 to 8192 new rows at once, got {m} (chunks would not reproduce the whole: "
                             f"the sigma floor and the largest weight are taken over all new rows)")
        if n_epochs is None:
            n_epochs = 100 if self._n_epochs_defaulted else max(1, self.n_epochs_ // 3)
        n_epochs = int(n_epochs)
        if not 1 <= n_epochs <= 2000:
            raise ValueError(f"transform needs 1 <= n_epochs <= 2000, got {n_epochs}")
        seed = self._seed if random_state is None else random_state
        new_pca = self._pca.transform(new_latents)
        dev = self._train_pca.device
        dist = ops.latent_pairwise(torch.from_numpy(np.ascontiguousarray(new_pca, dtype=np.float32)).to(dev), self._train_pca)
        knn_idx, knn_dist = ops.umap_knn_cross(dist, self._n_neighbors)
        tg = ops.umap_transform_graph(knn_idx, knn_dist, self._train_embedding, n_epochs)
        ops.umap_transform_layout(tg, self._train_embedding, tg.y0, tg.y0, a=self.a_, b=self.b_, n_epochs=n_epochs,
                                  seed=int(seed) & 0xFFFFFFFF)
        return tg.y0.cpu().double().numpy()


def _is_device_tensor(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host_metrics(p1: np.ndarray, p2: np.ndarray) -> tuple[float, float, float, float]:
    """fp64 numpy: centre distance, mean population std of each side (0 for one row), mean of all cross distances."""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    gap = p1.mean(axis=0) - p2.mean(axis=0)
    center = float(np.sqrt(np.dot(gap, gap)))
    std1 = float(p1.std(axis=0).mean()) if len(p1) > 1 else 0.0
    std2 = float(p2.std(axis=0).mean()) if len(p2) > 1 else 0.0
    total = 0.0
    for row in p1:                                          # differences, never |a|^2 + |b|^2 - 2ab
        diff = p2 - row
        total += float(np.sqrt(np.einsum("ij,ij->i", diff, diff)).sum())
    return center, std1, std2, total / (len(p1) * len(p2))


def compute_distance_metrics(points1, points2) -> tuple[float, float, float, float] | None:
    """``(center_distance, std1, std2, mean_cross_distance)`` of two point clouds ``[N1, D]`` / ``[N2, D]``, or ``None``
    when one is empty.  Device tensors go through ``ops.latent_group_stats`` (one segment); anything else is computed
    in fp64 numpy."""
    if len(points1) == 0 or len(points2) == 0:
        return None
    if _is_device_tensor(points1) and _is_device_tensor(points2):
        from .. import ops
        seg1 = torch.tensor([0, points1.shape[0]], dtype=torch.int32, device=points1.device)
        seg2 = torch.tensor([0, points2.shape[0]], dtype=torch.int32, device=points1.device)
        row = ops.latent_group_stats(points1, seg1, points2, seg2)[0].cpu().tolist()
        return row[0], row[1], row[2], row[3]
    if isinstance(points1, torch.Tensor):
        points1 = points1.detach().cpu().numpy()
    if isinstance(points2, torch.Tensor):
        points2 = points2.detach().cpu().numpy()
    return _host_metrics(np.array(points1), np.array(points2))


def segmented_distance_metrics_host(points1, seg1, points2, seg2) -> np.ndarray:
    """fp64 numpy statement of ``ops.latent_group_stats``: ``[patients, 4]``, NaN rows for patients without rows on one side."""
    points1, points2 = np.asarray(points1), np.asarray(points2)
    out = np.full((len(seg1) - 1, 4), np.nan)
    for e in range(len(seg1) - 1):
        a, b = points1[seg1[e]:seg1[e + 1]], points2[seg2[e]:seg2[e + 1]]
        if len(a) and len(b):
            out[e] = _host_metrics(a, b)
    return out


def group_rows_by_patient(ids1: list[str], ids2: list[str]) -> tuple[list[str], list[int], list[int], list[int], list[int]]:
    """-> (sorted patients of either group, row order 1, offsets 1, row order 2, offsets 2): ``order`` lists each group's
    row indices patient by patient (original order inside a patient), ``offsets[p] .. offsets[p + 1]`` are patient p's."""
    patients = sorted(set(ids1) | set(ids2))
    slot = {p: i for i, p in enumerate(patients)}

    def one(ids):
        rows: list[list[int]] = [[] for _ in patients]
        for i, p in enumerate(ids):
            rows[slot[p]].append(i)
        order = [i for r in rows for i in r]
        offsets = [0]
        for r in rows:
            offsets.append(offsets[-1] + len(r))
        return order, offsets

    order1, off1 = one(ids1)
    order2, off2 = one(ids2)
    return patients, order1, off1, order2, off2


def write_group_statistics(patients, counts1, counts2, metrics_lat, metrics_proj, name1: str, name2: str, output_dir) -> None:
    """``distance_metrics.txt`` and ``exams_sorted_by_distance.txt`` in the reference's text format.  ``metrics_*``:
    ``[patients, 4]``; a patient without rows in one group is left out."""
    output_dir = Path(output_dir)
    ranked = []
    with open(output_dir / "distance_metrics.txt", "w") as f:
        f.write("Distance Metrics per Exam (Latent Space and Projection)\n")
        f.write("=" * 60 + "\n\n")
        for p, exam in enumerate(patients):
            if counts1[p] == 0 or counts2[p] == 0:
                continue
            lat, proj = [float(v) for v in metrics_lat[p]], [float(v) for v in metrics_proj[p]]
            f.write(f"{exam}\n")
            f.write(f"  - n_{name1}: {counts1[p]}, n_{name2}: {counts2[p]}\n")
            for tag, m, end in (("Latent", lat, "\n"), ("Projection", proj, "\n\n")):
                f.write(f"  - [{tag}] center_dist: {m[0]:.3f}, std_{name1}: {m[1]:.3f}, std_{name2}: {m[2]:.3f}, "
                        f"mean_cross_dist: {m[3]:.3f}{end}")
            ranked.append((exam, lat[0]))
    ranked.sort(key=lambda item: item[1])
    with open(output_dir / "exams_sorted_by_distance.txt", "w") as f:
        f.write("Exams sorted by latent space center distance\n")
        f.write("=" * 60 + "\n\n")
        for exam, dist in ranked:
            f.write(f"{exam}: {dist:.3f}\n")


class LatentSpaceAnalyzer:
    """Encode images to latents, reduce them (PCA, then optionally t-SNE / UMAP) and compare two groups per patient.

    ``vae_model``: a model with ``encode_deterministic``; ``device``: the HIP device; ``transform``: what turns paths
    into network inputs -- either an object with ``loader(paths, batch_size)`` that yields device batches
    ``[b, C, H, W]`` (``analyze_static.TiffPreprocess``), or a callable ``path -> [C, H, W]`` tensor as in the reference."""

    def __init__(self, vae_model: torch.nn.Module, device: torch.device, transform) -> None:
        self.vae = vae_model
        self.device = device
        self.transform = transform
        self.vae.eval()

    # ---- encoding ----
    def _batches(self, image_paths: list[str], batch_size: int):
        if hasattr(self.transform, "loader"):
            yield from self.transform.loader(image_paths, batch_size)
            return
        for i in range(0, len(image_paths), batch_size):
            yield torch.stack([torch.as_tensor(self.transform(p)) for p in image_paths[i:i + batch_size]]).to(self.device)

    def encode_images(self, image_paths: list[str], max_images: int | None = None, batch_size: int = 8,
                      show_progress: bool = True, return_device: bool = False):
        """-> (latents ``[N, D]``, patient ids).  Deterministic (``z_mu``) and bit-exactly independent of the batch size.
        Every batch's ``z_mu`` is written, flattened in (C, H, W) order, into one preallocated device matrix; the host
        gets it in ONE copy at the end -- or not at all with ``return_device=True``, which returns the device matrix."""
        if len(image_paths) == 0:
            raise ValueError("image_paths cannot be empty")
        if max_images is not None:
            image_paths = image_paths[:max_images]
        batches = self._batches(list(image_paths), batch_size)
        if show_progress:
            try:
                from tqdm import tqdm
                batches = tqdm(batches, total=-(-len(image_paths) // batch_size), desc="Encoding images", unit="batch")
            except ImportError:
                pass
        matrix, row = None, 0
        with torch.no_grad():
            for batch in batches:
                z = self.vae.encode_deterministic(batch.to(self.device)).flatten(start_dim=1)
                if matrix is None:
                    matrix = torch.empty(len(image_paths), z.shape[1], dtype=torch.float32, device=z.device)
                matrix[row:row + z.shape[0]].copy_(z)
                row += z.shape[0]
        if row != len(image_paths):
            raise RuntimeError(f"encoded {row} of {len(image_paths)} images")
        ids = [extract_patient_id_from_filename(os.path.basename(p)) for p in image_paths]
        return (matrix if return_device else matrix.cpu().numpy()), ids

    # ---- dimensionality reduction ----
    def _to_device_matrix(self, x) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            return x.to(self.device, torch.float32)
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)

    def reduce_dimensionality_pca(self, latent_vectors, n_components: int = 50) -> tuple[np.ndarray, np.ndarray]:
        """-> (projections ``[N, n_components]`` fp64, explained-variance ratios).  The column mean and the centred Gram
        matrix ``G = Xc Xc^T`` are computed on the device; ``G = U diag(lambda) U^T`` in fp64 on the host, and the
        projections are ``U sqrt(lambda)`` -- what ``PCA(svd_solver="full").fit_transform`` returns.  Signs: the entry of
        largest magnitude of each column of U is positive (sklearn's ``svd_flip``, u-based)."""
        model = self.fit_pca(latent_vectors, n_components)
        return model.embedding_, model.explained_variance_ratio_

    def fit_pca(self, latent_vectors, n_components: int = 50) -> PcaModel:
        """``reduce_dimensionality_pca`` that keeps what it fitted -> ``PcaModel``: ``embedding_`` and
        ``explained_variance_ratio_`` are that function's two results, ``transform`` projects new rows."""
        from .. import ops
        if latent_vectors.ndim != 2:
            raise ValueError(f"Expected 2D array, got {latent_vectors.ndim}D array")
        n, d = latent_vectors.shape
        if not 1 <= n_components <= min(n, d):
            raise ValueError(f"n_components={n_components} must be between 1 and min(n_samples, n_features)={min(n, d)}")
        x = self._to_device_matrix(latent_vectors)
        if x is latent_vectors:                                # the caller's own device tensor: the model keeps a copy of its own
            x = x.clone()
        mean = x.mean(dim=0)
        gram = ops.latent_pairwise(x, mode="dot", center=mean).cpu().double().numpy()
        lam, u = np.linalg.eigh(gram)
        lam, u = np.clip(lam[::-1], 0.0, None), u[:, ::-1]
        total = float(np.trace(gram))
        lam, u = lam[:n_components], u[:, :n_components].copy()
        top = np.argmax(np.abs(u), axis=0)
        signs = np.sign(u[top, np.arange(n_components)])
        signs[signs == 0] = 1.0
        return PcaModel(x, mean, u * signs * np.sqrt(lam), (lam / total if total > 0 else np.zeros_like(lam)), u * signs, lam)

    @staticmethod
    def _check_reduction_input(latent_vectors, pca_components: int) -> int:
        if latent_vectors.ndim != 2:
            raise ValueError(f"Expected 2D array, got {latent_vectors.ndim}D array")
        n_samples = len(latent_vectors)
        if n_samples < pca_components:
            raise ValueError(f"Need at least {pca_components} samples for PCA with {pca_components} components, "
                             f"got {n_samples} samples. Reduce pca_components or provide more samples.")
        return n_samples

    def reduce_dimensionality_umap(self, latent_vectors, n_components: int = 2, n_neighbors: int = 40, min_dist: float = 0.5,
                                   random_state: int = 42, pca_components: int = 50, backend: str = "umap-learn",
                                   n_epochs: int | None = None) -> tuple[np.ndarray, object]:
        """PCA, then UMAP -> (reduced ``[N, n_components]``, the fitted UMAP model).

        ``backend="umap-learn"``: the host library; ``n_epochs`` is not used.  ``backend="hip"``: UMAP on the device
        (``ops.umap_knn`` / ``ops.umap_graph`` / ``ops.umap_epoch``), no host library; ``n_components`` must be 2,
        3 <= N <= 8192, ``n_neighbors`` at most 256, ``n_epochs`` at most 2000 (None: 500, umap-learn's choice up to
        10000 rows).  It starts from the first two principal components, each scaled to [0, 10]; ``random_state`` seeds
        the negative sampling: the same seed gives the same bits.  Returns ``(Y fp64 [N, 2], UmapResult)``."""
        if backend not in ("umap-learn", "hip"):
            raise ValueError(f"backend must be 'umap-learn' or 'hip', got {backend!r}")
        n_samples = self._check_reduction_input(latent_vectors, pca_components)
        if n_neighbors >= n_samples:
            raise ValueError(f"n_neighbors ({n_neighbors}) must be < n_samples ({n_samples}). "
                             f"Reduce n_neighbors or provide more samples.")
        if backend == "hip":
            if n_components != 2:
                raise ValueError(f"backend='hip' computes n_components=2 only, got {n_components}")
            defaulted, n_epochs = n_epochs is None, 500 if n_epochs is None else int(n_epochs)
            if not 2 <= n_neighbors <= 256 or not 3 <= n_samples <= 8192 or not 1 <= n_epochs <= 2000:
                raise ValueError(f"backend='hip' needs 2 <= n_neighbors <= 256, 3 <= n_samples <= 8192 and 1 <= n_epochs <= "
                                 f"2000, got n_neighbors={n_neighbors}, n_samples={n_samples}, n_epochs={n_epochs}")
            pca = self.fit_pca(latent_vectors, pca_components)
            return self._umap_device(pca.embedding_, n_neighbors, min_dist, n_epochs, random_state, pca, defaulted)
        try:
            import umap
        except ImportError as e:
            raise ImportError("Please install umap-learn: pip install umap-learn") from e
        vectors_pca, _ = self.reduce_dimensionality_pca(latent_vectors, pca_components)
        model = umap.UMAP(n_components=n_components, random_state=random_state, n_neighbors=n_neighbors, min_dist=min_dist)
        return model.fit_transform(vectors_pca), model

    @staticmethod
    def umap_init(vectors_pca: np.ndarray) -> np.ndarray:
        """The start of the device UMAP: the first two PCA columns, each min-max scaled to [0, 10] (umap-learn's rescaling
        of any initialisation), rounded to fp32 -> ``[N, 2]`` fp32."""
        y = np.zeros((len(vectors_pca), 2))
        y[:, :min(2, vectors_pca.shape[1])] = vectors_pca[:, :2]
        span = np.ptp(y, axis=0)
        return (10.0 * (y - y.min(axis=0)) / np.where(span > 0, span, 1.0)).astype(np.float32)

    @staticmethod
    def umap_layout(graph, y0: torch.Tensor, a: float, b: float, n_epochs: int, seed: int, negative_sample_rate: int = 5,
                    stop: int | None = None) -> torch.Tensor:
        """Epochs 0 .. ``stop`` - 1 (all ``n_epochs`` by default) of the layout from ``y0`` -> Y fp32 [N, 2] on the device.
        One launch per epoch on the current stream, ``alpha = 1 - e / n_epochs``, nothing comes back to the host."""
        from .. import ops
        y = [y0.to(torch.float32).contiguous().clone(), torch.empty(y0.shape[0], 2, dtype=torch.float32, device=y0.device)]
        cur = 0
        for e in range(n_epochs if stop is None else stop):
            ops.umap_epoch(graph, y[cur], y[cur ^ 1], a=a, b=b, alpha=1.0 - e / n_epochs, epoch=e, seed=seed,
                           negative_sample_rate=negative_sample_rate)
            cur ^= 1
        return y[cur]

    def _umap_device(self, vectors_pca: np.ndarray, n_neighbors: int, min_dist: float, n_epochs: int, seed: int,
                     pca: PcaModel | None = None, n_epochs_defaulted: bool = False) -> tuple[np.ndarray, UmapResult]:
        from .. import ops
        a, b = find_ab_params(1.0, min_dist)
        train_pca = self._to_device_matrix(vectors_pca)
        dist = ops.latent_pairwise(train_pca)
        knn_idx, knn_dist = ops.umap_knn(dist, n_neighbors)
        graph = ops.umap_graph(knn_idx, knn_dist, n_epochs)
        y0 = torch.from_numpy(self.umap_init(vectors_pca)).to(dist.device)
        y_dev = self.umap_layout(graph, y0, a, b, n_epochs, int(seed) & 0xFFFFFFFF)
        y = y_dev.cpu().double().numpy()
        return y, UmapResult(y, a, b, n_epochs, graph, pca=pca, train_pca=train_pca, train_embedding=y_dev,
                             n_neighbors=n_neighbors, seed=seed, n_epochs_defaulted=n_epochs_defaulted)

    def reduce_dimensionality_tsne(self, latent_vectors, n_components: int = 2, perplexity: int = 30, random_state: int = 42,
                                   pca_components: int = 50, backend: str = "sklearn", max_iter: int = 1000,
                                   exploration_n_iter: int = 250, early_exaggeration: float = 12.0) -> np.ndarray:
        """PCA, then t-SNE -> reduced ``[N, n_components]`` fp64 on the host.

        ``backend="sklearn"``: ``sklearn.manifold.TSNE(init="pca")`` on the host (Barnes-Hut); the last three parameters
        are not used.  ``backend="hip"``: exact t-SNE on the device (``ops.tsne_affinities`` / ``ops.tsne_step``) with
        sklearn's schedule and defaults, no host library; ``n_components`` must be 2 and N at most 8192.  It starts from
        the first two principal components scaled to a standard deviation of 1e-4, ``random_state`` is accepted and
        unused: the result is a pure function of the input, bit for bit.  The last KL value is kept in
        ``self.tsne_kl_divergence_``."""
        if backend not in ("sklearn", "hip"):
            raise ValueError(f"backend must be 'sklearn' or 'hip', got {backend!r}")
        n_samples = self._check_reduction_input(latent_vectors, pca_components)
        if perplexity >= n_samples:
            raise ValueError(f"perplexity ({perplexity}) must be < n_samples ({n_samples}). "
                             f"Reduce perplexity or provide more samples.")
        if perplexity < 5:
            print(f"Warning: perplexity={perplexity} is very low. Consider using 5-50 for better results.")
        if backend == "hip":
            if n_components != 2:
                raise ValueError(f"backend='hip' computes n_components=2 only, got {n_components}")
            vectors_pca, _ = self.reduce_dimensionality_pca(latent_vectors, pca_components)
            return self._tsne_device(vectors_pca, perplexity, max_iter, exploration_n_iter, early_exaggeration)
        try:
            from sklearn.manifold import TSNE
        except ImportError as e:
            raise ImportError("Please install scikit-learn: pip install scikit-learn") from e
        vectors_pca, _ = self.reduce_dimensionality_pca(latent_vectors, pca_components)
        return TSNE(n_components=n_components, perplexity=perplexity, init="pca", random_state=random_state).fit_transform(vectors_pca)

    @staticmethod
    def tsne_init(vectors_pca: np.ndarray) -> np.ndarray:
        """sklearn's ``init="pca"`` for rows that are PCA projections already: their first two columns ARE their principal
        axes; scaled to a population std of 1e-4 in column 0, rounded to fp32 -> ``[N, 2]`` fp32."""
        y = np.zeros((len(vectors_pca), 2))
        y[:, :min(2, vectors_pca.shape[1])] = vectors_pca[:, :2]
        std = float(y[:, 0].std())
        return (y / std * 1e-4 if std > 0 else y).astype(np.float32)

    def tsne_descend(self, p: torch.Tensor, sums: torch.Tensor, y0: torch.Tensor, max_iter: int = 1000,
                     exploration_n_iter: int = 250, early_exaggeration: float = 12.0) -> tuple[torch.Tensor, float]:
        """sklearn 1.7's ``TSNE._tsne`` schedule (``learning_rate="auto"``) on the device -> (Y fp32 [N, 2] on the device,
        KL at that Y; also kept in ``self.tsne_kl_divergence_``).  Momentum 0.5 with exaggeration for ``exploration_n_iter``
        iterations, then 0.8 without up to ``max_iter``.  Two launches per iteration, enqueued in order on the current
        stream; every 50th iteration also writes the two-double record {KL, gradient norm}, which then comes to the host
        for sklearn's stopping rule: |grad| <= 1e-7, or no KL improvement for more than ``exploration_n_iter`` (stage 1) /
        300 (stage 2) iterations.  The returned KL is evaluated at the returned Y by one more force pass (sklearn's
        ``kl_divergence_`` is the value one update earlier)."""
        from .. import ops
        n = p.shape[0]
        lr = max(n / early_exaggeration / 4.0, 50.0)
        y = [y0.to(torch.float32).contiguous().clone(), torch.empty(n, 2, dtype=torch.float32, device=p.device)]
        update, gains = torch.zeros_like(y[0]), torch.ones_like(y[0])
        record = torch.zeros(2, dtype=torch.float64, device=p.device)
        it, cur = 0, 0
        for stop, momentum, exaggeration, patience in ((min(exploration_n_iter, max_iter), 0.5, early_exaggeration, exploration_n_iter),
                                                       (max_iter, 0.8, 1.0, 300)):
            best, best_it = float("inf"), it
            for i in range(it, stop):
                check = (i + 1) % 50 == 0
                ops.tsne_step(p, y[cur], y[cur ^ 1], update, gains, record, sums=sums, exaggeration=exaggeration,
                              momentum=momentum, lr=lr, with_record=check)
                cur ^= 1
                it = i + 1
                if check:
                    kl, grad_norm = record.cpu().tolist()
                    if kl < best:
                        best, best_it = kl, i
                    elif i - best_it > patience:
                        break
                    if grad_norm <= 1e-7:
                        break
        ops.tsne_step(p, y[cur], y[cur ^ 1], update.clone(), gains.clone(), record, sums=sums, exaggeration=1.0, momentum=0.8,
                      lr=lr, with_record=True)                              # only its record is used
        self.tsne_kl_divergence_ = record.cpu().tolist()[0]
        return y[cur], self.tsne_kl_divergence_

    def _tsne_device(self, vectors_pca: np.ndarray, perplexity: float, max_iter: int, exploration_n_iter: int,
                     early_exaggeration: float) -> np.ndarray:
        from .. import ops
        dist = ops.latent_pairwise(self._to_device_matrix(vectors_pca))
        p, sums = ops.tsne_affinities(dist.square_(), perplexity)
        y, _ = self.tsne_descend(p, sums, torch.from_numpy(self.tsne_init(vectors_pca)).to(p.device), max_iter,
                                 exploration_n_iter, early_exaggeration)
        return y.cpu().double().numpy()

    # ---- projection quality ----
    def projection_quality(self, latent_vectors, projection, *, neighbors=(5, 15, 40), labels=None) -> tuple[dict, dict]:
        """How faithful ``projection`` ``[N, 2]`` is to ``latent_vectors`` ``[N, D]`` (the rows as given to the reduction,
        before any PCA) and how separate the ``labels`` are in either space -> ``(report, per-point arrays)``:
        ``analysis.projection_quality`` on this analyzer's device."""
        from .projection_quality import projection_quality
        return projection_quality(latent_vectors, projection, neighbors=neighbors, labels=labels, device=self.device)

    def projection_curves(self, latent_vectors, projection, bins: int = 64) -> tuple[dict, dict]:
        """At which scale ``projection`` ``[N, 2]`` can be believed: the co-ranking curves ``Q_NX`` / ``B_NX`` / ``R_NX`` /
        ``LCMC`` for every neighbourhood size and the Shepard figure -> ``(report, arrays)``:
        ``analysis.coranking_curves`` on this analyzer's device."""
        from .coranking import coranking_curves
        return coranking_curves(latent_vectors, projection, bins=bins, device=self.device)

    def group_separation_test(self, latents_a, latents_b, **options) -> tuple[dict, dict]:
        """Do two groups of latent rows differ by more than chance?  Permutation tests of the unbiased MMD^2, the energy
        distance and the same-label neighbour share -> ``(report, arrays)``: ``analysis.two_sample_tests`` on this
        analyzer's device."""
        from .two_sample import two_sample_tests
        return two_sample_tests(latents_a, latents_b, device=self.device, **options)

    # ---- colours ----
    def create_patient_colormap(self, patient_ids: list[str]) -> tuple[dict[str, int], dict[str, str]]:
        """-> (patient -> index in sorted order, patient -> hex colour, cycling through ``PATIENT_PALETTE``)."""
        patients = sorted(set(patient_ids))
        return ({p: i for i, p in enumerate(patients)},
                {p: PATIENT_PALETTE[i % len(PATIENT_PALETTE)] for i, p in enumerate(patients)})

    def save_color_legend(self, exam_to_id: dict[str, int], exam_to_color: dict[str, str], output_path: Path) -> None:
        with open(output_path, "w") as f:
            f.write("Color Legend for Exams\n")
            f.write("=" * 60 + "\n\n")
            for exam in sorted(exam_to_id, key=exam_to_id.get):
                f.write(f"{exam_to_id[exam]}: {exam} — {exam_to_color[exam]}\n")

    # ---- statistics ----
    def _segmented_metrics(self, points1, seg1, points2, seg2) -> np.ndarray:
        """``[patients, 4]`` from one ``ops.latent_group_stats`` call; the rows are already grouped by patient."""
        from .. import ops
        s1 = torch.tensor(seg1, dtype=torch.int32, device=self.device)
        s2 = torch.tensor(seg2, dtype=torch.int32, device=self.device)
        return ops.latent_group_stats(self._to_device_matrix(points1), s1, self._to_device_matrix(points2), s2).cpu().double().numpy()

    @staticmethod
    def _take_rows(points, order):
        if isinstance(points, torch.Tensor):
            return points.index_select(0, torch.tensor(order, dtype=torch.int64, device=points.device))
        return np.asarray(points)[np.asarray(order, dtype=np.int64)]

    def compute_group_statistics(self, projections: list, latent_vectors_list: list, output_dir: Path) -> None:
        """``projections`` / ``latent_vectors_list``: two ``(vectors, ids, name)`` tuples each (numpy arrays or device
        tensors).  Rows are grouped by patient id, patients sorted; one device call gives the four metrics of every
        patient in latent space, a second one in the projection; writes ``distance_metrics.txt`` and
        ``exams_sorted_by_distance.txt``.  Anything but two groups: nothing is written, as in the reference."""
        if len(projections) != 2 or len(latent_vectors_list) != 2:
            return
        (proj1, ids1, name1), (proj2, ids2, name2) = projections
        lat1, lat2 = latent_vectors_list[0][0], latent_vectors_list[1][0]
        patients, order1, seg1, order2, seg2 = group_rows_by_patient(list(ids1), list(ids2))
        counts1 = [seg1[p + 1] - seg1[p] for p in range(len(patients))]
        counts2 = [seg2[p + 1] - seg2[p] for p in range(len(patients))]
        if not order1 or not order2:
            nan = np.full((len(patients), 4), np.nan)
            write_group_statistics(patients, counts1, counts2, nan, nan, name1, name2, output_dir)
            return
        metrics_lat = self._segmented_metrics(self._take_rows(lat1, order1), seg1, self._take_rows(lat2, order2), seg2)
        metrics_proj = self._segmented_metrics(self._take_rows(proj1, order1), seg1, self._take_rows(proj2, order2), seg2)
        write_group_statistics(patients, counts1, counts2, metrics_lat, metrics_proj, name1, name2, output_dir)

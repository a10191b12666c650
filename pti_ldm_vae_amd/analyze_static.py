#!/usr/bin/env python3
"""Static latent-space analysis of a trained VAE -- the counterpart of the reference's ``vae_scripts/analyze_static.py``.

    python -m pti_ldm_vae_amd.analyze_static --vae-weights W.pth --config-file CFG.json --folder-edente DIR [--folder-dente DIR]

Same options and defaults, plus ``--method pca`` (the projection is the first two principal components; also the
fallback, with a warning, when umap-learn / scikit-learn is not installed), ``--cache-dir``, ``--batch-size``,
``--tsne-backend hip`` (``--method tsne`` as exact t-SNE on the device: deterministic, no host library) and
``--umap-backend hip`` (``--method umap`` on the device: deterministic for a ``--seed``, no host library) and
``--umap-fit-group edente`` (with ``--umap-backend hip`` and two groups: UMAP is fitted on the edentulous group alone and
the dentulous group is placed into that embedding, as the reference does; the default ``all`` fits on both).
Outputs in ``--output-dir``: ``<method>_projection.png`` (matplotlib; ``.html`` through plotly when that fails),
``color_legend.txt`` with ``--color-by-patient``, and with two groups ``distance_metrics.txt``,
``exams_sorted_by_distance.txt`` and ``latents.npz`` (latents, ids, paths and projection of each group).
``--quality [--quality-neighbors K ...]`` rates the projection, whichever method and backend made it
(``analysis.projection_quality``: trustworthiness, continuity and neighbourhood preservation per ``K``, and how separate the
groups and a patient's exams are in the latent space and in the picture) into ``projection_quality.json``,
``projection_quality.npz`` and ``<method>_projection_quality.png``; without it nothing changes.
``--quality-curves [--quality-bins B]`` says at which scale the picture can be believed (``analysis.coranking_curves``: the
co-ranking curves Q_NX, B_NX, R_NX for every neighbourhood size, their scale-free score, the rank correlation per point and
a Shepard diagram with its stress) into ``projection_curves.json``, ``projection_curves.npz`` and
``<method>_projection_curves.png``; it is independent of ``--quality``, and without it nothing changes either.
``--group-test`` asks whether the two groups differ by more than chance (``analysis.two_sample``: permutation tests of the
unbiased MMD^2, the energy distance and the same-label neighbour share on the latents, exact integer arithmetic on the
device) into ``group_test.json``, ``group_test.npz`` and ``group_test.png``; without it nothing changes.

Images are encoded deterministically in batches on the HIP engine; each image's latent is cached on disk in the
reference's layout (``analysis.LatentCache``), so a second run on the same folders encodes nothing."""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

from .analysis import LatentCache, LatentSpaceAnalyzer, load_image_paths


class _Args(argparse.Namespace):
    """The namespace ``parse_args`` fills.  ``--tsne-backend``, ``--umap-backend``, ``--umap-fit-group``, ``--quality``,
    ``--quality-neighbors``, ``--quality-curves``, ``--quality-bins`` and the ``--group-test`` family live here as class defaults and enter the instance
    only when they are given, so a command line without them parses to exactly the attributes it always had."""

    tsne_backend = "sklearn"
    umap_backend = "umap-learn"
    umap_fit_group = "all"
    quality = False
    quality_neighbors = (5, 15, 40)
    quality_curves = False
    quality_bins = 64
    group_test = False
    group_test_permutations = 9999
    group_test_stratify = "none"
    group_test_neighbors = 5
    group_test_seed = 0


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="Static Latent Space Analysis (UMAP, t-SNE or PCA; MI355X, HIP engine)")
    parser.add_argument("--vae-weights", type=str, required=True, help="Path to VAE weights file")
    parser.add_argument("--config-file", type=str, required=True, help="Path to model config file")
    parser.add_argument("--folder-edente", type=str, required=True, help="Path to edentulous image group folder")
    parser.add_argument("--folder-dente", type=str, default=None, help="Path to dentulous image group folder (optional)")
    parser.add_argument("--output-dir", type=str, default="projections", help="Output directory for projections")
    parser.add_argument("--max-images", type=int, default=1000, help="Maximum number of images per group")
    parser.add_argument("--patch-size", type=int, nargs=2, default=[256, 256], help="Image patch size (H W)")
    parser.add_argument("--color-by-patient", action="store_true", help="Color points by patient ID instead of group")
    parser.add_argument("--method", type=str, choices=["umap", "tsne", "pca"], default="umap",
                        help="Dimensionality reduction method (default: umap)")
    parser.add_argument("--n-neighbors", type=int, default=40, help="UMAP n_neighbors parameter")
    parser.add_argument("--min-dist", type=float, default=0.5, help="UMAP min_dist parameter")
    parser.add_argument("--perplexity", type=int, default=30, help="t-SNE perplexity parameter")
    parser.add_argument("--tsne-backend", type=str, choices=["sklearn", "hip"], default=argparse.SUPPRESS,
                        help="t-SNE implementation: sklearn (host, Barnes-Hut; default) or hip (exact, on the device, "
                             "deterministic, needs no host library)")
    parser.add_argument("--umap-backend", type=str, choices=["umap-learn", "hip"], default=argparse.SUPPRESS,
                        help="UMAP implementation: umap-learn (host; default) or hip (on the device, deterministic for a "
                             "--seed, needs no host library)")
    parser.add_argument("--umap-fit-group", type=str, choices=["all", "edente"], default=argparse.SUPPRESS,
                        help="Rows UMAP is fitted on: all (both groups together; default) or edente (the edentulous group "
                             "alone, the dentulous group is then placed into its embedding; needs --umap-backend hip)")
    parser.add_argument("--quality", action="store_true", default=argparse.SUPPRESS,
                        help="Also rate the projection: trustworthiness, continuity, neighbourhood preservation and the "
                             "separation of groups / patients in both spaces (projection_quality.json / .npz and "
                             "<method>_projection_quality.png)")
    parser.add_argument("--quality-neighbors", type=int, nargs="+", default=argparse.SUPPRESS, metavar="K",
                        help="Neighbour counts of --quality (default: 5 15 40; each at most 255, those not below half the "
                             "number of images are listed as excluded)")
    parser.add_argument("--quality-curves", action="store_true", default=argparse.SUPPRESS,
                        help="Also say at which scale the projection can be believed: the co-ranking curves Q_NX, B_NX, R_NX "
                             "for every neighbourhood size, AUC_logK, the rank correlation and a Shepard diagram with its "
                             "stress (projection_curves.json / .npz and <method>_projection_curves.png)")
    parser.add_argument("--quality-bins", type=int, default=argparse.SUPPRESS, metavar="B",
                        help="Bins per axis of the Shepard diagram of --quality-curves (default: 64; 2 .. 128)")
    parser.add_argument("--group-test", action="store_true", default=argparse.SUPPRESS,
                        help="Also test whether the two groups differ by more than chance: permutation tests of the unbiased "
                             "MMD^2, the energy distance and the same-label nearest-neighbour share on the latents "
                             "(group_test.json / .npz / .png); needs --folder-dente")
    parser.add_argument("--group-test-permutations", type=int, default=argparse.SUPPRESS, metavar="P",
                        help="Relabellings of --group-test (default: 9999; 1 .. 65534)")
    parser.add_argument("--group-test-stratify", type=str, choices=["none", "patient"], default=argparse.SUPPRESS,
                        help="Relabel freely (none; default) or only within a patient (patient)")
    parser.add_argument("--group-test-neighbors", type=int, default=argparse.SUPPRESS, metavar="K",
                        help="Nearest neighbours of --group-test's neighbour test (default: 5)")
    parser.add_argument("--group-test-seed", type=int, default=argparse.SUPPRESS,
                        help="Seed of --group-test's relabellings (default: 0)")
    parser.add_argument("--seed", type=int, default=42, help="Random seed for reproducibility")
    parser.add_argument("--subtitle", type=str, default=None, help="Optional subtitle for the plot")
    parser.add_argument("--dpi", type=int, default=300, help="DPI for output PNG (default: 300)")
    parser.add_argument("--cache-dir", type=str, default="cache/latents", help="Root of the per-image latent cache")
    parser.add_argument("--batch-size", type=int, default=8, help="Images per encoder call (default: 8)")
    return parser.parse_args(argv, namespace=_Args())


class TiffPreprocess:
    """The training pipeline's preprocessing (TIFF decode, area resize, masked z-score) for lists of paths:
    ``loader(paths, batch_size)`` yields device batches ``[b, 1, H, W]``; called with one path it returns ``[1, H, W]``."""

    def __init__(self, patch_size: tuple[int, int], device, num_workers: int = 4) -> None:
        self.patch_size, self.device, self.num_workers = tuple(patch_size), device, num_workers

    def loader(self, paths: list[str], batch_size: int):
        from .data import DeviceImageLoader
        return DeviceImageLoader(paths, batch_size, self.patch_size, self.device, shuffle=False, num_workers=self.num_workers)

    def __call__(self, path: str) -> torch.Tensor:
        return next(iter(self.loader([path], 1)))[0].clone()


def load_and_encode_group_with_cache(analyzer: LatentSpaceAnalyzer, folder_path: str, vae_weights: str, max_images: int,
                                     patch_size: tuple[int, int], group_name: str, cache_dir=Path("cache/latents"),
                                     batch_size: int = 8) -> tuple[np.ndarray, list[str], list[str]]:
    """-> (latents, patient ids, paths) of the folder's images; only images missing from the cache are encoded, all of
    them in batches of ``batch_size``."""
    paths = load_image_paths(folder_path, max_images)
    if not paths:
        raise FileNotFoundError(f"No .tif/.tiff images found in {folder_path}")

    def encode_many(miss_paths):
        return analyzer.encode_images(miss_paths, batch_size=batch_size, show_progress=False)

    def encode_one(path):
        latents, ids = encode_many([path])
        return latents[0], ids[0]

    return LatentCache(cache_root=Path(cache_dir)).get_or_encode_batch(paths, encode_one, vae_weights, tuple(patch_size),
                                                                       group_name, encode_many=encode_many)


def project(analyzer: LatentSpaceAnalyzer, latents: np.ndarray, args: argparse.Namespace) -> tuple[np.ndarray, str]:
    """-> (2-D projection of all rows, the method that produced it).  A missing host library falls back to PCA."""
    n = len(latents)
    if args.method != "pca":
        try:
            if args.method == "umap":
                return analyzer.reduce_dimensionality_umap(latents, n_neighbors=args.n_neighbors, min_dist=args.min_dist,
                                                           random_state=args.seed, pca_components=min(n, 50),
                                                           backend=getattr(args, "umap_backend", "umap-learn"))[0], "umap"
            backend = getattr(args, "tsne_backend", "sklearn")       # a namespace built by hand may not carry it
            if backend == "sklearn":
                print("(This may take a few minutes...)")
            return analyzer.reduce_dimensionality_tsne(latents, perplexity=args.perplexity, random_state=args.seed,
                                                       pca_components=min(n, 50), backend=backend), "tsne"
        except ImportError as e:
            print(f"[WARN] --method {args.method} is not available ({e}); falling back to --method pca")
    if n < 2:
        raise SystemExit("analyze_static: a PCA projection needs at least two images")
    proj, ratio = analyzer.reduce_dimensionality_pca(latents, 2)
    print(f"PCA explained variance ratio: {ratio[0]:.4f}, {ratio[1]:.4f}")
    return proj, "pca"


def project_fit_first(analyzer: LatentSpaceAnalyzer, first: np.ndarray, second: np.ndarray,
                      args: argparse.Namespace) -> tuple[list[np.ndarray], str]:
    """``--umap-fit-group edente``: the device UMAP fitted on ``first`` alone, ``second`` placed into that embedding by
    ``UmapResult.transform`` -> ([projection of first, projection of second], "umap")."""
    fitted, model = analyzer.reduce_dimensionality_umap(first, n_neighbors=args.n_neighbors, min_dist=args.min_dist,
                                                        random_state=args.seed, pca_components=min(len(first), 50), backend="hip")
    return [fitted, model.transform(second)], "umap"


def save_projection_plot(groups: list, output_path: Path, title: str, subtitle: str | None, dpi: int,
                         patient_to_color: dict | None) -> Path:
    """``groups``: ``(points [n, 2], ids, name)``; edente = open circles, dente = filled.  -> the file written: the PNG
    through matplotlib, or an HTML file through plotly when matplotlib cannot be used."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots(figsize=(8, 7))
        for k, (pts, ids, name) in enumerate(groups):
            filled = "dente" in name.lower() and "edente" not in name.lower()
            colors = [patient_to_color[i] for i in ids] if patient_to_color else ("#1f77b4" if k == 0 else "#ff7f0e")
            ax.scatter(pts[:, 0], pts[:, 1], s=36, alpha=0.7, linewidths=1.0, label=name, edgecolors=colors,
                       facecolors=colors if filled else "none")
        ax.set_xlabel("Dimension 1")
        ax.set_ylabel("Dimension 2")
        ax.set_title(title if not subtitle else f"{title}\n{subtitle}")
        ax.grid(True, color="lightgray")
        fig.savefig(output_path, dpi=dpi)
        plt.close(fig)
        return output_path
    except Exception as e:
        try:
            import plotly.graph_objects as go
        except ImportError:
            raise e
        fig = go.Figure()
        for k, (pts, ids, name) in enumerate(groups):
            filled = "dente" in name.lower() and "edente" not in name.lower()
            colors = [patient_to_color[i] for i in ids] if patient_to_color else ("#1f77b4" if k == 0 else "#ff7f0e")
            fig.add_trace(go.Scatter(x=pts[:, 0], y=pts[:, 1], mode="markers", name=name, text=list(ids),
                                     marker={"color": colors, "symbol": "circle" if filled else "circle-open", "size": 10}))
        fig.update_layout(title=title if not subtitle else f"{title}<br><sub>{subtitle}</sub>", xaxis_title="Dimension 1",
                          yaxis_title="Dimension 2", template="plotly_white")
        html_path = output_path.with_suffix(".html")
        fig.write_html(str(html_path))
        print(f"⚠️  Could not export PNG ({e}). Saved HTML instead: {html_path}")
        return html_path


def save_quality_plot(points: np.ndarray, values: np.ndarray, output_path: Path, title: str, dpi: int) -> Path:
    """The projection's scatter coloured by a per-point value, with a colour bar."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(8, 7))
    sc = ax.scatter(points[:, 0], points[:, 1], s=36, c=values, cmap="viridis", vmax=1.0, linewidths=0.0)
    fig.colorbar(sc, ax=ax, label="local trustworthiness")
    ax.set_xlabel("Dimension 1")
    ax.set_ylabel("Dimension 2")
    ax.set_title(title)
    ax.grid(True, color="lightgray")
    fig.savefig(output_path, dpi=dpi)
    plt.close(fig)
    return output_path


def write_projection_quality(analyzer: LatentSpaceAnalyzer, groups: list, projected: list, method: str,
                             args: argparse.Namespace, output_dir: Path) -> dict:
    """``--quality``: rates the projection of all rows (both groups concatenated, also under ``--umap-fit-group edente``) and
    writes ``projection_quality.json`` (byte-identical between two runs), ``projection_quality.npz`` (the per-point arrays,
    ids and paths in the order of the projection) and ``<method>_projection_quality.png``.  -> the report."""
    import json
    latents = np.concatenate([g[0] for g in groups])
    projection = np.concatenate([np.asarray(p) for p in projected])
    ids = [i for g in groups for i in g[1]]
    labels = {}
    if len(groups) > 1:
        labels["group"] = [g[3] for g in groups for _ in g[1]]
    if len(set(ids)) < len(ids):                            # at least one patient with two or more rows
        labels["patient"] = ids
    neighbors = [int(k) for k in getattr(args, "quality_neighbors", _Args.quality_neighbors)]
    try:
        report, points = analyzer.projection_quality(latents, projection, neighbors=neighbors, labels=labels)
    except ValueError as e:
        raise SystemExit(f"analyze_static: --quality: {e}")
    resolved = {k: getattr(args, k) for k in sorted(set(vars(args)) | {"tsne_backend", "umap_backend", "umap_fit_group"})}
    resolved.update(quality=True, quality_neighbors=neighbors)
    doc = {"method": method, "n": report["n"], "high_dims": report["high_dims"], "neighbors": report["neighbors"],
           "excluded": {str(k): v for k, v in report["excluded"].items()}}
    for key in ("trustworthiness", "continuity", "neighborhood_preservation"):
        doc[key] = {str(k): v for k, v in report[key].items()}
    doc["labels"] = {name: {key: ({str(k): v for k, v in val.items()} if isinstance(val, dict) else val)
                            for key, val in entry.items()} for name, entry in report["labels"].items()}
    doc["args"] = resolved
    (output_dir / "projection_quality.json").write_text(json.dumps(doc, indent=2, allow_nan=False) + "\n")
    np.savez(output_dir / "projection_quality.npz", ids=np.array(ids), paths=np.array([p for g in groups for p in g[2]]),
             groups=np.array([g[3] for g in groups for _ in g[1]]), projection=projection,
             neighbors=np.array(report["neighbors"], dtype=np.int64), **points)
    for k in report["neighbors"]:
        print(f"Projection quality k={k}: trustworthiness {report['trustworthiness'][k]:.4f}, continuity "
              f"{report['continuity'][k]:.4f}, neighbourhood preservation {report['neighborhood_preservation'][k]:.4f}")
    for k, reason in report["excluded"].items():
        print(f"Projection quality k={k}: excluded ({reason})")
    if report["neighbors"]:
        k = max(report["neighbors"])
        column = report["neighbors"].index(k)
        title = {"umap": "UMAP", "tsne": "t-SNE", "pca": "PCA"}[method]
        save_quality_plot(projection, points["trustworthiness_local"][:, column], output_dir / f"{method}_projection_quality.png",
                          f"{title}: local trustworthiness (k = {k})", args.dpi)
    else:
        print("[WARN] no admitted neighbour count: the quality picture is not written")
    print(f"✅ Projection quality saved: {output_dir / 'projection_quality.json'}")
    return report


def save_curves_plot(report: dict, arrays: dict, output_path: Path, title: str, dpi: int) -> Path:
    """Three panels: ``Q_NX`` and ``R_NX`` against ``K`` on a log axis with ``K_max`` marked, ``B_NX``, the Shepard heat map."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    n = report["n"]
    k = np.arange(1, n)
    fig, (left, mid, right) = plt.subplots(1, 3, figsize=(18, 5.5))
    left.semilogx(k, arrays["Q_NX"], label="Q_NX")
    left.semilogx(k[:-1], arrays["R_NX"], label=f"R_NX (AUC_logK = {report['auc_logk_rnx']:.3f})")
    left.axvline(report["k_max"], color="gray", linestyle="--", label=f"K_max = {report['k_max']}")
    left.set_xlabel("K")
    left.set_ylim(min(0.0, float(arrays["R_NX"].min())), 1.0)
    left.set_title(title)
    left.legend(loc="best")
    mid.semilogx(k, arrays["B_NX"], color="#d62728")
    mid.axhline(0.0, color="gray", linewidth=0.8)
    mid.set_xlabel("K")
    mid.set_title("B_NX (above 0: extrusive, below 0: intrusive)")
    for ax in (left, mid):
        ax.grid(True, color="lightgray")
    eh, el = arrays["shepard_edges_high"], arrays["shepard_edges_low"]
    if eh[-1] > 0 and el[-1] > 0:
        mesh = right.pcolormesh(eh, el, np.log1p(arrays["shepard_hist"].T.astype(np.float64)), cmap="viridis")
        fig.colorbar(mesh, ax=right, label="log(1 + pairs)")
    right.set_xlabel("latent distance")
    right.set_ylabel("projection distance")
    right.set_title("Shepard diagram" + ("" if report["stress"] is None else f" (stress {report['stress']:.3f})"))
    fig.savefig(output_path, dpi=dpi)
    plt.close(fig)
    return output_path


def write_projection_curves(analyzer: LatentSpaceAnalyzer, groups: list, projected: list, method: str,
                            args: argparse.Namespace, output_dir: Path) -> dict:
    """``--quality-curves``: the co-ranking curves and the Shepard figure of the projection of all rows (both groups
    concatenated, also under ``--umap-fit-group edente``) -> ``projection_curves.json`` (byte-identical between two runs; the
    curves at ``K`` = 1, 2, 5, 10, ... only), ``projection_curves.npz`` (the full curves, histograms and per-point values, ids
    and paths in the order of the projection) and ``<method>_projection_curves.png``.  -> the report."""
    import json

    from .analysis.coranking import curve_samples
    latents = np.concatenate([g[0] for g in groups])
    projection = np.concatenate([np.asarray(p) for p in projected])
    bins = int(getattr(args, "quality_bins", _Args.quality_bins))
    try:
        report, arrays = analyzer.projection_curves(latents, projection, bins=bins)
    except ValueError as e:
        raise SystemExit(f"analyze_static: --quality-curves: {e}")
    ks = curve_samples(report["n"])
    doc = {"method": method}
    doc.update(report)
    doc["K"] = ks
    for key in ("Q_NX", "B_NX", "R_NX"):
        doc[key] = {str(k): float(arrays[key][k - 1]) for k in ks if k - 1 < len(arrays[key])}
    (output_dir / "projection_curves.json").write_text(json.dumps(doc, indent=2, allow_nan=False) + "\n")
    np.savez(output_dir / "projection_curves.npz", ids=np.array([i for g in groups for i in g[1]]),
             paths=np.array([p for g in groups for p in g[2]]), groups=np.array([g[3] for g in groups for _ in g[1]]),
             projection=projection, **arrays)
    title = {"umap": "UMAP", "tsne": "t-SNE", "pca": "PCA"}[method]
    save_curves_plot(report, arrays, output_dir / f"{method}_projection_curves.png", f"{title}: co-ranking curves", args.dpi)
    tail = "" if report["q_global"] is None else f", Q_global {report['q_global']:.4f}"
    stress = "undefined" if report["stress"] is None else f"{report['stress']:.4f}"
    print(f"Projection curves: AUC_logK(R_NX) {report['auc_logk_rnx']:.4f}, K_max {report['k_max']}, Q_local "
          f"{report['q_local']:.4f}{tail}, rank correlation {report['rank_correlation']:.4f}, stress {stress}")
    print(f"✅ Projection curves saved: {output_dir / 'projection_curves.json'}")
    return report


def save_group_test_plot(report: dict, arrays: dict, output_path: Path, dpi: int) -> Path:
    """One panel per test: the null histogram with the observed value marked."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    titles = {"mmd": "unbiased MMD^2", "energy": "energy distance", "knn": "same-label neighbour share"}
    fig, axes = plt.subplots(1, 3, figsize=(18, 5))
    for ax, (name, entry) in zip(axes, report["tests"].items()):
        if entry["statistic"] is None:
            ax.set_title(f"{titles[name]}: undefined")
            continue
        ax.hist(arrays[f"null_{name}"], bins=40, color="#7f7f7f")
        ax.axvline(entry["statistic"], color="#d62728", label=f"observed (p = {entry['p_value']:.4g})")
        ax.set_title(titles[name])
        ax.set_xlabel("statistic")
        ax.legend(loc="best")
        ax.grid(True, color="lightgray")
    fig.savefig(output_path, dpi=dpi)
    plt.close(fig)
    return output_path


def write_group_test(analyzer: LatentSpaceAnalyzer, groups: list, args: argparse.Namespace, output_dir: Path) -> dict:
    """``--group-test``: the permutation tests of the first group's latents against the second's ->
    ``group_test.json`` (byte-identical between two runs), ``group_test.npz`` (null distributions, integer tables, labellings,
    the per-image witness, ids and paths, pooled with the first group first) and ``group_test.png``.  -> the report."""
    import json
    (lat_a, ids_a, paths_a, name_a), (lat_b, ids_b, paths_b, name_b) = groups[0], groups[1]
    lat_a, lat_b = (np.asarray(x).reshape(len(x), -1) for x in (lat_a, lat_b))
    stratify = getattr(args, "group_test_stratify", _Args.group_test_stratify)
    options = dict(permutations=int(getattr(args, "group_test_permutations", _Args.group_test_permutations)),
                   seed=int(getattr(args, "group_test_seed", _Args.group_test_seed)),
                   neighbors=int(getattr(args, "group_test_neighbors", _Args.group_test_neighbors)))
    try:
        report, arrays = analyzer.group_separation_test(lat_a, lat_b, strata_a=ids_a if stratify == "patient" else None,
                                                        strata_b=ids_b if stratify == "patient" else None, **options)
    except ValueError as e:
        raise SystemExit(f"analyze_static: --group-test: {e}")
    doc = {"group_a": name_a, "group_b": name_b, "stratify": stratify}
    doc.update(report)
    (output_dir / "group_test.json").write_text(json.dumps(doc, indent=2, allow_nan=False) + "\n")
    np.savez(output_dir / "group_test.npz", ids=np.array(list(ids_a) + list(ids_b)), paths=np.array(list(paths_a) + list(paths_b)),
             groups=np.array([name_a] * len(ids_a) + [name_b] * len(ids_b)), **arrays)
    save_group_test_plot(report, arrays, output_dir / "group_test.png", args.dpi)
    for name, entry in report["tests"].items():
        if entry["statistic"] is None:
            print(f"Group test {name}: undefined")
        else:
            print(f"Group test {name}: statistic {entry['statistic']:.6g}, p = {entry['p_value']:.4g} "
                  f"({entry['exceed']} of {entry['permutations']} relabellings at least as large)")
    print(f"✅ Group test saved: {output_dir / 'group_test.json'}")
    return report


def main(argv=None) -> None:
    from . import _lib
    from .utils.cli_common import init_device_and_seed, load_config_and_model
    _lib.refuse_wrong_result_env("analyze_static.py")
    args = parse_args(argv)
    fit_first = args.method == "umap" and getattr(args, "umap_fit_group", "all") == "edente" and bool(args.folder_dente)
    if fit_first and getattr(args, "umap_backend", "umap-learn") != "hip":
        raise SystemExit("analyze_static: --umap-fit-group edente places the second group with the device UMAP's transform; "
                         "add --umap-backend hip")
    if getattr(args, "group_test", False) and not args.folder_dente:
        raise SystemExit("analyze_static: --group-test compares two groups; add --folder-dente")
    device = init_device_and_seed(args.seed)
    np.random.seed(args.seed)
    output_dir = Path(args.output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    print("=" * 60)
    print(f"Static Latent Space Analysis - {args.method.upper()}")
    print("=" * 60)
    _, vae = load_config_and_model(args.config_file, args.vae_weights, device)
    print(f"Loaded VAE from {args.vae_weights}")
    patch = (int(args.patch_size[0]), int(args.patch_size[1]))
    analyzer = LatentSpaceAnalyzer(vae, device, TiffPreprocess(patch, device))

    groups = []                                             # (latents, ids, paths, name)
    for folder, name in ((args.folder_edente, "edente"), (args.folder_dente, "dente")):
        if folder:
            latents, ids, paths = load_and_encode_group_with_cache(analyzer, folder, args.vae_weights, args.max_images, patch,
                                                                   name, cache_dir=args.cache_dir, batch_size=args.batch_size)
            groups.append((latents, ids, paths, name))

    print(f"Computing {args.method.upper()} projection...")
    if fit_first:
        projected, method = project_fit_first(analyzer, groups[0][0], groups[1][0], args)
    else:
        combined = np.concatenate([g[0] for g in groups]) if len(groups) > 1 else groups[0][0]
        projection, method = project(analyzer, combined, args)
        split = len(groups[0][0])
        projected = [projection[:split]] + ([projection[split:]] if len(groups) > 1 else [])

    title = {"umap": "UMAP", "tsne": "t-SNE", "pca": "PCA"}[method]
    if len(groups) > 1:
        title = f"{title} (● dente, ○ edente)"
    patient_to_color = None
    if args.color_by_patient:
        patient_to_id, patient_to_color = analyzer.create_patient_colormap([i for g in groups for i in g[1]])
        analyzer.save_color_legend(patient_to_id, patient_to_color, output_dir / "color_legend.txt")
        print(f"✅ Color legend saved: {output_dir / 'color_legend.txt'}")
    written = save_projection_plot([(p, g[1], g[3]) for p, g in zip(projected, groups)], output_dir / f"{method}_projection.png",
                                   title, args.subtitle, args.dpi, patient_to_color)
    print(f"✅ Visualization saved: {written}")

    if len(groups) > 1:
        analyzer.compute_group_statistics([(p, g[1], g[3]) for p, g in zip(projected, groups)],
                                          [(g[0], g[1], g[3]) for g in groups], output_dir)
        arrays = {}
        for p, (latents, ids, paths, name) in zip(projected, groups):
            arrays.update({f"latents_{name}": latents, f"ids_{name}": np.array(ids), f"paths_{name}": np.array(paths),
                           f"projection_{name}": p})
        np.savez(output_dir / "latents.npz", **arrays)
        print(f"✅ Statistics saved to {output_dir}/distance_metrics.txt")
        print(f"✅ Sorted exams saved to {output_dir}/exams_sorted_by_distance.txt")
    if getattr(args, "quality", False):
        write_projection_quality(analyzer, groups, projected, method, args, output_dir)
    if getattr(args, "quality_curves", False):
        write_projection_curves(analyzer, groups, projected, method, args, output_dir)
    if getattr(args, "group_test", False):
        write_group_test(analyzer, groups, args, output_dir)
    print("✅ Analysis complete!")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the device-side UMAP transform of the latent-space analysis, one JSON line:

    python tools/bench_umap_transform.py [--train 6000] [--new 2000] [--n-neighbors 40] [--n-epochs 100] [--repeats 20] [--runs 5]

  Synthetic rows: twelve Gaussian clusters in 50 columns (what ``UmapResult.transform`` sees after the PCA); the fitted
  embedding is the training rows' scaled PCA start -- the layout's cost does not depend on how good the fit is.
  Every stage is timed with device events around ``--repeats`` back-to-back calls after two warm-up calls, ``--runs`` times;
  the line carries the median and the range of the per-call means.
  distances_ms / knn_ms / graph_ms  ``ops.latent_pairwise`` (new x training), ``ops.umap_knn_cross``, ``ops.umap_transform_graph``
  layout_one_launch_ms              ``ops.umap_transform_layout`` over all epochs in one launch
  layout_per_epoch_ms               the same epochs as --n-epochs launches with ``start=e, stop=e + 1`` (bit-identical result)
  fired_per_epoch                   the mean number of slots that fire in an epoch (each costs 1 + negative_sample_rate pairs)
  total_ms                          distances + kNN + graph + the one-launch layout
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--train", type=int, default=6000)
    ap.add_argument("--new", type=int, default=2000)
    ap.add_argument("--n-neighbors", type=int, default=40)
    ap.add_argument("--n-epochs", type=int, default=100)
    ap.add_argument("--min-dist", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    from pti_ldm_vae_amd.analysis.latent_space import find_ab_params
    dev = torch.device("cuda:0")
    a, b = find_ab_params(1.0, args.min_dist)
    n, m, k, n_epochs = args.train, args.new, args.n_neighbors, args.n_epochs

    def timed(fn):
        """-> (median, lowest, highest) over --runs of the mean milliseconds of --repeats calls."""
        means = []
        for _ in range(args.runs):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.repeats):
                fn()
            stop.record()
            torch.cuda.synchronize()
            means.append(start.elapsed_time(stop) / args.repeats)
        return statistics.median(means), min(means), max(means)

    g = torch.Generator().manual_seed(n + m)
    rows = (torch.randn(12, 50, generator=g) * 1.5)[torch.randint(0, 12, (n + m,), generator=g)] + torch.randn(n + m, 50, generator=g)
    train, new = rows[:n].to(dev), rows[n:].to(dev)
    pca = rows[:n].double().numpy()
    pca = (pca - pca.mean(axis=0)) @ np.linalg.svd(pca - pca.mean(axis=0), full_matrices=False)[2][:2].T
    y_train = torch.from_numpy(LatentSpaceAnalyzer.umap_init(pca)).to(dev)
    res = {"train": n, "new": m, "n_neighbors": k, "n_epochs": n_epochs, "repeats": args.repeats, "runs": args.runs}
    spans = {}

    def record(key, fn):
        res[key], lo, hi = timed(fn)
        spans[key] = [round(lo, 4), round(hi, 4)]

    record("distances_ms", lambda: ops.latent_pairwise(new, train))
    dist = ops.latent_pairwise(new, train)
    record("knn_ms", lambda: ops.umap_knn_cross(dist, k))
    idx, kd = ops.umap_knn_cross(dist, k)
    record("graph_ms", lambda: ops.umap_transform_graph(idx, kd, y_train, n_epochs))
    tg = ops.umap_transform_graph(idx, kd, y_train, n_epochs)
    rate = tg.rate.cpu().numpy().astype(np.int64)
    res["dropped"] = int((rate == 0).sum())
    res["fired_per_epoch"] = float(((n_epochs * rate) >> 20).sum() / n_epochs)
    one, many = torch.empty_like(tg.y0), torch.empty_like(tg.y0)
    kw = dict(a=a, b=b, n_epochs=n_epochs, seed=args.seed)

    def per_epoch():
        ops.umap_transform_layout(tg, y_train, tg.y0, many, start=0, stop=1, **kw)
        for e in range(1, n_epochs):
            ops.umap_transform_layout(tg, y_train, many, many, start=e, stop=e + 1, **kw)

    record("layout_one_launch_ms", lambda: ops.umap_transform_layout(tg, y_train, tg.y0, one, **kw))
    record("layout_per_epoch_ms", per_epoch)
    res["same_bits"] = bool(torch.equal(one, many))
    res["finite"] = bool(torch.isfinite(one).all())
    res["total_ms"] = res["distances_ms"] + res["knn_ms"] + res["graph_ms"] + res["layout_one_launch_ms"]
    res["range_ms"] = spans
    print(json.dumps({key: (round(v, 4) if isinstance(v, float) else v) for key, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()

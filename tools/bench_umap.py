#!/usr/bin/env python3
"""Time the device-side UMAP of the latent-space analysis, one JSON line per N:

    python tools/bench_umap.py [--sizes 2000 6000] [--n-neighbors 40] [--n-epochs 500] [--oracle-epochs 50] [--no-oracle]

  Synthetic rows: twelve Gaussian clusters in 50 columns (what ``analyze_static`` hands over after its PCA).
  distances_ms / knn_ms / graph_ms  ``ops.latent_pairwise``, ``ops.umap_knn``, ``ops.umap_graph`` (device events, mean of 5)
  nnz / longest_row / fired_per_epoch  the graph: kept entries, the longest CSR row, and the mean number of edges that fire
                                    in an epoch (each costs 1 + negative_sample_rate pair evaluations)
  epoch_us                          one ``ops.umap_epoch`` (device events over all --n-epochs epochs of the real schedule)
  layout_ms                         ``LatentSpaceAnalyzer.umap_layout``, all epochs (wall clock, ends in a device synchronise)
  total_ms                          distances + kNN + graph + layout
  oracle_epoch_ms / oracle_layout_s the vectorised fp64 numpy statement of the same epochs (``tests/umap_oracle.py``) on this
                                    machine's CPUs: the mean over the first --oracle-epochs epochs, and that mean times
                                    --n-epochs
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000])
    ap.add_argument("--n-neighbors", type=int, default=40)
    ap.add_argument("--n-epochs", type=int, default=500)
    ap.add_argument("--min-dist", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--oracle-epochs", type=int, default=50)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    from pti_ldm_vae_amd.analysis.latent_space import find_ab_params
    dev = torch.device("cuda:0")
    an = LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)
    a, b = find_ab_params(1.0, args.min_dist)

    def timed(fn, iters, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters

    for n in args.sizes:
        g = torch.Generator().manual_seed(n)
        rows = (torch.randn(12, 50, generator=g) * 1.5)[torch.randint(0, 12, (n,), generator=g)] + torch.randn(n, 50, generator=g)
        x = rows.to(dev)
        k, n_epochs = args.n_neighbors, args.n_epochs
        res = {"n": n, "n_neighbors": k, "n_epochs": n_epochs}
        res["distances_ms"] = timed(lambda: ops.latent_pairwise(x), 5)
        dist = ops.latent_pairwise(x)
        res["knn_ms"] = timed(lambda: ops.umap_knn(dist, k), 5)
        idx, kd = ops.umap_knn(dist, k)
        res["graph_ms"] = timed(lambda: ops.umap_graph(idx, kd, n_epochs), 5)
        graph = ops.umap_graph(idx, kd, n_epochs)
        nnz = int(graph.nnz)
        rate = graph.rate[:nnz].cpu().numpy().astype(np.int64)
        res["nnz"], res["longest_row"] = nnz, int(graph.indptr.diff().max())
        res["fired_per_epoch"] = float(((n_epochs * rate) >> 20).sum() / n_epochs)
        y0 = torch.from_numpy(an.umap_init(rows.double().numpy())).to(dev)
        ys = [y0.clone(), torch.empty_like(y0)]
        state = [0, 0]

        def epoch():
            e, cur = state
            ops.umap_epoch(graph, ys[cur], ys[cur ^ 1], a=a, b=b, alpha=1.0 - e / n_epochs, epoch=e, seed=args.seed)
            state[0], state[1] = (e + 1) % n_epochs, cur ^ 1

        res["epoch_us"] = timed(epoch, n_epochs, warm=0) * 1e3
        an.umap_layout(graph, y0, a, b, n_epochs, args.seed, stop=10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = an.umap_layout(graph, y0, a, b, n_epochs, args.seed)
        torch.cuda.synchronize()
        res["layout_ms"] = (time.perf_counter() - t0) * 1e3
        res["finite"] = bool(torch.isfinite(y).all())
        res["total_ms"] = res["distances_ms"] + res["knn_ms"] + res["graph_ms"] + res["layout_ms"]
        if not args.no_oracle:
            import umap_oracle as O
            indptr = graph.indptr.cpu().numpy()
            og = O.Graph(indptr, graph.indices[:nnz].cpu().numpy(), graph.weights[:nnz].cpu().numpy(), graph.rate[:nnz].cpu().numpy(),
                         None, None, 1.0, np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr)))
            stop = min(args.oracle_epochs, n_epochs)
            t0 = time.perf_counter()
            O.layout_jacobi(og, y0.cpu().numpy(), a, b, n_epochs, args.seed, stop=stop)
            res["oracle_epoch_ms"] = (time.perf_counter() - t0) * 1e3 / stop
            res["oracle_layout_s"] = res["oracle_epoch_ms"] * n_epochs * 1e-3
        print(json.dumps({key: (round(v, 4) if isinstance(v, float) else v) for key, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()

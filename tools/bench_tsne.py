#!/usr/bin/env python3
"""Time the exact t-SNE of the latent-space analysis on the device, one JSON line per N:

    python tools/bench_tsne.py [--sizes 500 2000 6000] [--iters 200] [--sklearn-exact-max-n 2000] [--no-sklearn]

  Synthetic rows: six Gaussian clusters in 50 columns (what ``analyze_static`` hands over after its PCA), perplexity 30.
  distances_us / affinities_us      ``ops.latent_pairwise`` + square, ``ops.tsne_affinities`` (device events, mean of 5)
  step_us / step_record_us          one ``ops.tsne_step`` without / with the {KL, |grad|} record (device events, mean of --iters)
  p_gb_per_s / hbm_share            N^2 * 4 bytes of P per step over step_us, and that rate over the 8.0 TB/s HBM peak
                                    (P of 144 MB at N = 6000 can sit in the 256 MB last-level cache: a rate, not a proof of
                                    HBM traffic)
  descend_1000_ms                   ``LatentSpaceAnalyzer.tsne_descend``, 1000 iterations with its 20 record copies (wall clock,
                                    ends in a device synchronise); total_ms adds distances and affinities
  sklearn_barnes_hut_s / _exact_s   ``sklearn.manifold.TSNE(init="pca")`` on the same rows on this machine's CPUs, when
                                    scikit-learn is installed (exact only up to --sklearn-exact-max-n)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s, MI355X spec


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000, 6000])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--sklearn-exact-max-n", type=int, default=2000)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    import torch

    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    dev = torch.device("cuda:0")
    an = LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)

    def timed(fn, iters, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / iters

    for n in args.sizes:
        g = torch.Generator().manual_seed(n)
        rows = (torch.randn(6, 50, generator=g) * 4.0)[torch.randint(0, 6, (n,), generator=g)] + torch.randn(n, 50, generator=g)
        x = rows.to(dev)
        res = {"n": n, "perplexity": args.perplexity, "iters": args.iters}
        res["distances_us"] = timed(lambda: ops.latent_pairwise(x).square_(), 5)
        d2 = ops.latent_pairwise(x).square_()
        p = torch.empty(n, n, device=dev)
        res["affinities_us"] = timed(lambda: ops.tsne_affinities(d2, args.perplexity, out=p), 5)
        _, sums = ops.tsne_affinities(d2, args.perplexity, out=p)
        y0 = torch.from_numpy(an.tsne_init(rows.double().numpy())).to(dev)
        ys = [y0.clone(), torch.empty_like(y0)]
        update, gains = torch.zeros_like(y0), torch.ones_like(y0)
        record = torch.zeros(2, dtype=torch.float64, device=dev)
        lr = max(n / 12.0 / 4.0, 50.0)
        flip = [0]

        def step(with_record):
            ops.tsne_step(p, ys[flip[0]], ys[flip[0] ^ 1], update, gains, record, sums=sums, exaggeration=12.0, momentum=0.5,
                          lr=lr, with_record=with_record)
            flip[0] ^= 1

        res["step_us"] = timed(lambda: step(False), args.iters, warm=10)
        res["step_record_us"] = timed(lambda: step(True), max(args.iters // 4, 1), warm=2)
        res["p_mb"] = n * n * 4 / 1e6
        res["p_gb_per_s"] = n * n * 4 / (res["step_us"] * 1e-6) / 1e9
        res["hbm_share"] = res["p_gb_per_s"] * 1e9 / HBM_PEAK
        an.tsne_descend(p, sums, y0, max_iter=60, exploration_n_iter=30)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, kl = an.tsne_descend(p, sums, y0)
        torch.cuda.synchronize()
        res["descend_1000_ms"] = (time.perf_counter() - t0) * 1e3
        res["kl"] = kl
        res["total_ms"] = res["descend_1000_ms"] + (res["distances_us"] + res["affinities_us"]) * 1e-3
        if not args.no_sklearn:
            try:
                from sklearn.manifold import TSNE
            except ImportError:
                TSNE = None
            if TSNE is not None:
                host = rows.double().numpy()
                for method in ("barnes_hut", "exact"):
                    if method == "exact" and n > args.sklearn_exact_max_n:
                        continue
                    t0 = time.perf_counter()
                    model = TSNE(n_components=2, perplexity=args.perplexity, init="pca", random_state=42, method=method).fit(host)
                    res[f"sklearn_{method}_s"] = time.perf_counter() - t0
                    res[f"sklearn_{method}_kl"] = float(model.kl_divergence_)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()

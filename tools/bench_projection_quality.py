#!/usr/bin/env python3
"""Times the projection-quality report (csrc/projection_quality.hip, analysis/projection_quality.py) at n = 2000, 6000 and
8192 rows of 50 columns with a noisy 2-D projection and k = 40:

* ``ops.neighbor_ranks`` (40 listed neighbours per row) and ``ops.segment_row_sums`` (3 labels), each on its own;
* the whole ``projection_quality`` report (two distance matrices, two neighbour tables, two rank passes, one label set with
  its two segment passes, the folds and the copy to the host);
* a torch restatement of the rank pass on the same device: ``argsort`` of every row of the matrix, the inverse permutation,
  a gather -- what scikit-learn's ``trustworthiness`` does on the host;
* scikit-learn on the host: ``trustworthiness(metric="precomputed")`` in both directions plus ``silhouette_samples`` on the same
  fp64 matrices, host clock, median of 3, with whatever thread count the environment gives its BLAS / OpenMP pools (the
  number is printed); skipped where scikit-learn is not installed.

The ranks of the kernel and of the restatement are compared before a number is printed.  Device-event timings after a warm-up:
five windows of each, alternated, reported as median [min .. max]; a kernel window is sized to about 100 ms.
usage: python tools/bench_projection_quality.py [--json OUT] [--sizes N ...] [--k K]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pti_ldm_vae_amd import ops  # noqa: E402
from pti_ldm_vae_amd.analysis.projection_quality import nearest_others, projection_quality  # noqa: E402

COLS, K, CLASSES = 50, 40, 3


def window(fn, iters):
    """Mean time of ``iters`` back-to-back calls between two device events, in us."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def timed(fn, rounds=5, target_ms=100.0):
    """-> (median, min, max) in us over ``rounds`` windows sized to about ``target_ms`` after a warm-up."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    iters = int(min(2000, max(1, target_ms * 1e3 / max(window(fn, 2), 1e-3))))
    t = sorted(window(fn, iters) for _ in range(rounds))
    return t[len(t) // 2], t[0], t[-1]


def torch_ranks(dist, nbr):
    """The rank pass with torch ops: argsort of every row (the diagonal pushed first), its inverse, a gather."""
    n = dist.shape[0]
    d = dist.clone()
    d.fill_diagonal_(-1.0)
    order = torch.argsort(d, dim=1, stable=True)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(n, device=dist.device)[None, :].expand(n, n))
    return rank.gather(1, nbr.long()).int()


def host_baseline(dh, dl, high, low, codes, k):
    try:
        from sklearn.manifold import trustworthiness
        from sklearn.metrics import silhouette_samples
    except ImportError:
        return None
    t0 = time.perf_counter()
    trustworthiness(dh, low, n_neighbors=k, metric="precomputed")
    trustworthiness(dl, high, n_neighbors=k, metric="precomputed")
    silhouette_samples(dh, codes, metric="precomputed")
    silhouette_samples(dl, codes, metric="precomputed")
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000, 8192])
    ap.add_argument("--k", type=int, default=K, help=f"neighbour count (default: {K})")
    ap.add_argument("--no-host", action="store_true", help="skip the scikit-learn baseline")
    args = ap.parse_args()
    k = args.k
    dev = torch.device("cuda:0")
    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    rows = []
    for n in args.sizes:
        rng = np.random.default_rng(n)
        codes = np.arange(n) % CLASSES
        high = (rng.standard_normal((CLASSES, COLS))[codes] * 1.5 + rng.standard_normal((n, COLS))).astype(np.float32)
        low = (high @ rng.standard_normal((COLS, 2)).astype(np.float32) / np.sqrt(COLS) + 0.35 * rng.standard_normal((n, 2))).astype(np.float32)
        x, y = torch.from_numpy(high).to(dev), torch.from_numpy(low).to(dev)
        dh, dl = ops.latent_pairwise(x), ops.projection_distances(y)
        nbr = nearest_others(dl, k)
        seg = torch.tensor([0] + list(np.cumsum(np.bincount(codes))), dtype=torch.int32, device=dev)
        order = torch.from_numpy(np.argsort(codes, kind="stable")).to(dev)
        grouped = dh.index_select(1, order)
        labels = {"group": codes.tolist()}
        same = bool(torch.equal(ops.neighbor_ranks(dh, nbr), torch_ranks(dh, nbr)))    # random rows: no tied distances
        if not same:
            raise SystemExit(f"n={n}: the kernel and the torch restatement do not agree on every rank")
        t_rank = timed(lambda: ops.neighbor_ranks(dh, nbr))
        t_sums = timed(lambda: ops.segment_row_sums(grouped, seg))
        t_torch = timed(lambda: torch_ranks(dh, nbr), target_ms=1.0)
        t_report = timed(lambda: projection_quality(x, y, neighbors=(k,), labels=labels, device=dev), target_ms=1.0)
        host_us = None
        if not args.no_host:
            d64h, d64l = dh.cpu().double().numpy(), dl.cpu().double().numpy()
            times = sorted(t for t in (host_baseline(d64h, d64l, high.astype(np.float64), low.astype(np.float64), codes, k)
                                       for _ in range(3)) if t is not None)
            host_us = times[len(times) // 2] * 1e6 if times else None
        rows.append(dict(n=n, cols=COLS, k=k, classes=CLASSES, neighbor_ranks_us=t_rank, segment_row_sums_us=t_sums,
                         torch_argsort_ranks_us=t_torch, report_us=t_report, ranks_equal=same, sklearn_host_us=host_us,
                         host_threads=threads))
        fmt = lambda t: f"{t[0]:10.1f} us [{t[0 + 1]:.1f} .. {t[2]:.1f}]"   # noqa: E731
        print(f"n={n} k={k}: neighbor_ranks {fmt(t_rank)} | segment_row_sums {fmt(t_sums)} | torch argsort ranks {fmt(t_torch)} "
              f"(x{t_torch[0] / t_rank[0]:.1f}) | whole report {fmt(t_report)} | sklearn on the host ({threads} threads) "
              + ("n/a" if host_us is None else f"{host_us:.0f} us"), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=2)


if __name__ == "__main__":
    main()

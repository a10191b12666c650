#!/usr/bin/env python3
"""Times ``ops.ksg_counts`` (csrc/ksg.hip: the radii and range counts of the KSG k-nearest-neighbour mutual information) at
N = 2000, 6000 and 12000 images with the AR config's L = 10 channels and na = 6 attributes and k = 3, against two baselines,
and checks that all three agree on every count before a number is printed:

* a torch restatement on the same device, one pair at a time and chunked over the rows to fit memory: broadcast
  differences, ``kthvalue``, two compares and sums;
* scikit-learn on the host (``_compute_mi_cc``'s own steps per pair: a Chebyshev ``NearestNeighbors`` and two ``KDTree`` range
  counts), timed with the host clock on host arrays, median of 3; skipped where sklearn is not installed.

The columns lie on a dyadic grid, so that the host's fp64 differences are the device's fp32 ones and the counts can be
compared exactly.  Device-event timings after a warm-up of every shape: five windows of each, alternated, reported as median
[min .. max]; a kernel window is sized to about 100 ms.  ``ksg_counts`` includes its wrapper's non-finite check, which reads
one flag back (a host synchronisation per call); the restatement makes no such check.
usage: python tools/bench_ksg.py [--json OUT] [--sizes N ...] [--k K]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pti_ldm_vae_amd import ops  # noqa: E402

L_CH, NA, K = 10, 6, 3
GRID = 2.0 ** -20
CHUNK = 2048   # rows of the restatement's [CHUNK, N] tables


def window(fn, iters):
    """Mean time of ``iters`` back-to-back calls between two device events, in us."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def compare(kernel, restatement, rounds=5, target_ms=100.0):
    """``rounds`` timing windows of each, ALTERNATED (kernel, restatement, kernel, ...) after a warm-up of both.  A kernel
    window holds as many calls as fill about ``target_ms`` (sized from a first window of 5), a restatement window 1 call.
    -> ((median, min, max) of the kernel, (median, min, max) of the restatement, calls per kernel window), times in us."""
    for _ in range(2):
        kernel()
    restatement()
    torch.cuda.synchronize()
    iters = int(min(5000, max(5, target_ms * 1e3 / max(window(kernel, 5), 1e-3))))
    tk, tt = [], []
    for _ in range(rounds):
        tk.append(window(kernel, iters))
        tt.append(window(restatement, 1))
    stats = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))   # noqa: E731
    return stats(tk), stats(tt), iters


def torch_ksg(zt, attrs, k):
    """The definition with torch ops: per pair and per chunk of rows, |x_i - x_j| and |y_i - y_j| by broadcasting, the k-th
    value of their maximum with self pushed to +inf, the largest fp32 below it, two compares and sums."""
    l, n = zt.shape
    na = attrs.shape[0]
    eps = torch.empty(na, l, n, device=zt.device)
    nx = torch.empty(na, l, n, dtype=torch.int32, device=zt.device)
    ny = torch.empty_like(nx)
    rows = torch.arange(n, device=zt.device)
    zero = torch.zeros((), device=zt.device)
    for q in range(na):
        for c in range(l):
            x, y = zt[c], attrs[q]
            for i0 in range(0, n, CHUNK):
                i1 = min(n, i0 + CHUNK)
                dx = (x[i0:i1, None] - x[None, :]).abs()
                dy = (y[i0:i1, None] - y[None, :]).abs()
                self_ = rows[i0:i1, None] == rows[None, :]
                e = torch.maximum(dx, dy).masked_fill(self_, float("inf")).kthvalue(k, dim=1).values
                r = torch.where(e > 0, torch.nextafter(e, zero), zero)[:, None]
                eps[q, c, i0:i1] = e
                nx[q, c, i0:i1] = ((dx <= r) & ~self_).sum(1)
                ny[q, c, i0:i1] = ((dy <= r) & ~self_).sum(1)
    return eps, nx, ny


def host_baseline(cols, l, k):
    """-> (seconds, nx, ny) with sklearn's own steps per pair, or None without sklearn."""
    try:
        from sklearn.neighbors import KDTree, NearestNeighbors
    except ImportError:
        return None
    cols = cols.astype(np.float64)
    na, n = cols.shape[0] - l, cols.shape[1]
    nx, ny = np.zeros((na, l, n), np.int32), np.zeros((na, l, n), np.int32)
    t0 = time.perf_counter()
    for q in range(na):
        for c in range(l):
            x, y = cols[c].reshape(-1, 1), cols[l + q].reshape(-1, 1)
            nn = NearestNeighbors(metric="chebyshev", n_neighbors=k).fit(np.hstack((x, y)))
            radius = np.nextafter(nn.kneighbors()[0][:, -1], 0)
            nx[q, c] = KDTree(x, metric="chebyshev").query_radius(x, radius, count_only=True, return_distance=False) - 1
            ny[q, c] = KDTree(y, metric="chebyshev").query_radius(y, radius, count_only=True, return_distance=False) - 1
    return time.perf_counter() - t0, nx, ny


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000, 12000])
    ap.add_argument("--k", type=int, default=K, help=f"neighbour count (default: {K})")
    args = ap.parse_args()
    k = args.k
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    rows = []
    for n in args.sizes:
        z = torch.round(torch.randn(n, L_CH, generator=gen) / GRID) * GRID
        attrs = torch.randint(0, 200, (NA, n), generator=gen).float() / 16.0          # ties as in pixel-count attributes
        cols = torch.cat([z.t(), attrs]).to(dev)                                      # [L + na, N]: used in place
        zv, av = cols[:L_CH].t(), cols[L_CH:]
        kernel = lambda: ops.ksg_counts(zv, av, k)                                    # noqa: E731
        restatement = lambda: torch_ksg(cols[:L_CH], av, k)                           # noqa: E731
        (e_k, nx_k, ny_k), (e_t, nx_t, ny_t) = kernel(), restatement()
        same = bool(torch.equal(e_k.view(torch.int32), e_t.view(torch.int32)) and torch.equal(nx_k, nx_t) and torch.equal(ny_k, ny_t))
        cols_h = cols.cpu().numpy()
        host = [h for h in (host_baseline(cols_h, L_CH, k) for _ in range(3)) if h is not None]
        if host:
            same = same and all(np.array_equal(h[1], nx_k.cpu().numpy()) and np.array_equal(h[2], ny_k.cpu().numpy()) for h in host)
        if not same:
            raise SystemExit(f"N={n}: the kernel, the torch restatement and the host do not agree on every count")
        (t_k, k_lo, k_hi), (t_t, t_lo, t_hi), iters = compare(kernel, restatement)
        times = sorted(h[0] for h in host)
        host_us = times[len(times) // 2] * 1e6 if times else None
        row = dict(n=n, l=L_CH, na=NA, k=k, kernel_us=t_k, kernel_us_min=k_lo, kernel_us_max=k_hi, kernel_calls_per_window=iters,
                   torch_us=t_t, torch_us_min=t_lo, torch_us_max=t_hi, ratio=t_t / t_k, counts_equal=same, host_us=host_us,
                   host_us_min=times[0] * 1e6 if times else None, host_us_max=times[-1] * 1e6 if times else None)
        rows.append(row)
        print(f"N={n} k={k}: ksg_counts {t_k:9.1f} us [{k_lo:.1f} .. {k_hi:.1f}] ({iters} calls x 5 windows) | torch restatement "
              f"{t_t:11.1f} us [{t_lo:.1f} .. {t_hi:.1f}] | x{t_t / t_k:7.2f} | counts equal {same} | sklearn on the host "
              + ("n/a" if host_us is None else f"{host_us:.0f} us [{times[0] * 1e6:.0f} .. {times[-1] * 1e6:.0f}]"), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=2)


if __name__ == "__main__":
    main()

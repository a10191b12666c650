#!/usr/bin/env python3
"""Times the three ops of the disentanglement report (csrc/disentanglement.hip: ``ops.tied_ranks``, ``ops.rank_moments``,
``ops.joint_histogram``) at N = 2000, 6000 and 12000 images with the AR config's L = 10 channels and na = 6 attributes and
20 bins, against two baselines, and checks that all three agree exactly:

* a torch restatement on the same device: sort-based average ranks (``sort`` + two ``searchsorted``), a broadcast Gram matrix,
  ``bucketize`` and one ``bincount``;
* scipy and sklearn on the host (``rankdata``, ``np.digitize``, ``mutual_info_score`` per pair), timed with the host clock on
  host arrays, copies not included; skipped where they are not installed.

Device-event timings after a warm-up of every shape: five windows of each, alternated, reported as median [min .. max]; a
kernel window is sized to about 100 ms.  ``joint_histogram`` includes its wrapper's below-the-first-edge check, which reads
one flag back (a host synchronisation per call); the restatement makes no such check.
usage: python tools/bench_disentanglement.py [--json OUT]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pti_ldm_vae_amd import ops  # noqa: E402
from pti_ldm_vae_amd.utils.disentanglement import edge_tables  # noqa: E402

L_CH, NA, BINS = 10, 6, 20


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
    window holds as many calls as fill about ``target_ms`` (sized from a first window of 5), a restatement window 5 calls.
    -> ((median, min, max) of the kernel, (median, min, max) of the restatement, calls per kernel window), times in us."""
    for _ in range(2):
        kernel()
        restatement()
    torch.cuda.synchronize()
    iters = int(min(5000, max(5, target_ms * 1e3 / max(window(kernel, 5), 1e-3))))
    tk, tt = [], []
    for _ in range(rounds):
        tk.append(window(kernel, iters))
        tt.append(window(restatement, 5))
    stats = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))   # noqa: E731
    return stats(tk), stats(tt), iters


def torch_ranks(cols):
    """2 x the average rank: below + not-above + 1 from the sorted column."""
    ordered = cols.sort(dim=1).values
    below = torch.searchsorted(ordered, cols, right=False)
    not_above = torch.searchsorted(ordered, cols, right=True)
    return (below + not_above + 1).to(torch.int32)


def torch_moments(rank2):
    r = rank2.to(torch.int64)
    return r.sum(1), (r[:, None, :] * r[None, :, :]).sum(-1)


def torch_histogram(cols, edges, l):
    """bucketize per column, then every [B][B] table from ONE bincount over the combined index."""
    bins = torch.stack([torch.bucketize(cols[k].double(), edges[k], right=True) - 1 for k in range(cols.shape[0])])
    b = edges.shape[1]
    na = cols.shape[0] - l
    pair = (torch.arange(na, device=cols.device)[:, None] * l + torch.arange(l, device=cols.device)[None, :])[:, :, None]
    idx = (pair * b + bins[l:, None, :]) * b + bins[None, :l, :]
    counts = torch.bincount(idx.reshape(-1), minlength=na * l * b * b).reshape(na, l, b, b)
    return bins.to(torch.uint8), counts.to(torch.int32)


def host_baseline(cols, l, bins):
    """-> seconds, or None without scipy / sklearn."""
    try:
        from scipy.stats import rankdata
        from sklearn.metrics import mutual_info_score
    except ImportError:
        return None
    t0 = time.perf_counter()
    ranks = np.stack([rankdata(c, method="average") for c in cols])
    np.corrcoef(ranks)
    digit = [np.digitize(c, np.histogram_bin_edges(c, bins)[:-1]) - 1 for c in cols]
    for q in range(l, cols.shape[0]):
        for c in range(l):
            mutual_info_score(digit[q], digit[c])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000, 12000])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    rows = []
    for n in args.sizes:
        z = torch.randn(n, L_CH, generator=gen)
        attrs = torch.randint(0, 200, (NA, n), generator=gen).float()               # ties as in pixel-count attributes
        cols = torch.cat([z.t(), attrs]).to(dev)                                    # [L + na, N]: used in place
        lo, hi = torch.aminmax(cols, dim=1)
        edges = torch.from_numpy(edge_tables(lo.cpu().numpy(), hi.cpu().numpy(), BINS)).to(dev)
        zv, av, ez, ea = cols[:L_CH].t(), cols[L_CH:], edges[:L_CH], edges[L_CH:]

        def kernels():
            rank2 = ops.tied_ranks(cols)
            return rank2, ops.rank_moments(rank2), ops.joint_histogram(zv, av, ez, ea)

        def restatement():
            rank2 = torch_ranks(cols)
            return rank2, torch_moments(rank2), torch_histogram(cols, edges, L_CH)

        (r_k, (s_k, g_k), (bz, ba, c_k)), (r_t, (s_t, g_t), (b_t, c_t)) = kernels(), restatement()
        same = bool(torch.equal(r_k, r_t) and torch.equal(s_k, s_t) and torch.equal(g_k, g_t)
                    and torch.equal(torch.cat([bz, ba]), b_t) and torch.equal(c_k, c_t))
        (t_k, k_lo, k_hi), (t_t, t_lo, t_hi), iters = compare(kernels, restatement)
        parts = {}
        for name, fn, ref in (("tied_ranks", lambda: ops.tied_ranks(cols), lambda: torch_ranks(cols)),
                              ("rank_moments", lambda: ops.rank_moments(r_k), lambda: torch_moments(r_k)),
                              ("joint_histogram", lambda: ops.joint_histogram(zv, av, ez, ea),
                               lambda: torch_histogram(cols, edges, L_CH))):
            (a, a_lo, a_hi), (b, b_lo, b_hi), _ = compare(fn, ref, target_ms=50.0)
            parts[name] = dict(kernel_us=a, kernel_us_min=a_lo, kernel_us_max=a_hi, torch_us=b, torch_us_min=b_lo, torch_us_max=b_hi)
        cols_h = cols.cpu().numpy()
        host = sorted(t for t in (host_baseline(cols_h, L_CH, BINS) for _ in range(3)) if t is not None)
        host_us = host[len(host) // 2] * 1e6 if host else None
        row = dict(n=n, l=L_CH, na=NA, bins=BINS, kernel_us=t_k, kernel_us_min=k_lo, kernel_us_max=k_hi, kernel_calls_per_window=iters,
                   torch_us=t_t, torch_us_min=t_lo, torch_us_max=t_hi, ratio=t_t / t_k, tables_equal=same, host_us=host_us,
                   host_us_min=host[0] * 1e6 if host else None, host_us_max=host[-1] * 1e6 if host else None, parts=parts)
        rows.append(row)
        print(f"N={n}: three ops {t_k:8.1f} us [{k_lo:.1f} .. {k_hi:.1f}] ({iters} calls x 5 windows) | torch restatement "
              f"{t_t:9.1f} us [{t_lo:.1f} .. {t_hi:.1f}] | x{t_t / t_k:6.2f} | tables equal {same} | scipy + sklearn on the host "
              + ("n/a" if host_us is None else f"{host_us:.0f} us [{host[0] * 1e6:.0f} .. {host[-1] * 1e6:.0f}]"), flush=True)
        for name, p in parts.items():
            print(f"    {name:16s} kernel {p['kernel_us']:8.1f} us [{p['kernel_us_min']:.1f} .. {p['kernel_us_max']:.1f}] | torch "
                  f"{p['torch_us']:9.1f} us [{p['torch_us_min']:.1f} .. {p['torch_us_max']:.1f}] | x{p['torch_us'] / p['kernel_us']:6.2f}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=2)


if __name__ == "__main__":
    main()

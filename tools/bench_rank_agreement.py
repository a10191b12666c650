#!/usr/bin/env python3
"""Times ``ops.rank_agreement`` (csrc/rank_agreement.hip) against a torch broadcast restatement on the same device, at
N = 2000, 6000 and 12000 images with the AR config's L = 10 channels and na = 6 attributes, and checks that the two agree
(counts exactly).  Device-event timings after a warm-up of every shape: five windows of each, alternated, reported as median
[min .. max]; a kernel window is sized to about 100 ms.  The restatement materialises N x N temporaries per (attribute,
channel), which is what a host-side or eager implementation has to do.  A third timing runs the kernel with no attribute
mapped (channels = -1): the counts alone, so the difference is what the fp64 loss term costs.
usage: python tools/bench_rank_agreement.py [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pti_ldm_vae_amd import ops  # noqa: E402

L_CH, NA = 10, 6


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
    window holds as many calls as fill about ``target_ms`` (sized from a first window of 5), a restatement window 2 calls.
    -> ((median, min, max) of the kernel, (median, min, max) of the restatement, calls per kernel window), times in us."""
    for _ in range(2):
        kernel()
    restatement()
    torch.cuda.synchronize()
    iters = int(min(5000, max(5, target_ms * 1e3 / max(window(kernel, 5), 1e-3))))
    tk, tt = [], []
    for _ in range(rounds):
        tk.append(window(kernel, iters))
        tt.append(window(restatement, 2))
    stats = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))   # noqa: E731
    return stats(tk), stats(tt), iters


def torch_restatement(z, attrs, channels, deltas):
    """The same five counts and loss sums from N x N broadcasts (int8 sign tables, one boolean reduction per class)."""
    n, l = z.shape
    upper = torch.ones(n, n, dtype=torch.bool, device=z.device).triu(1)
    sz = [torch.sign(z[:, c][None, :] - z[:, c][:, None]).to(torch.int8) for c in range(l)]
    counts = torch.zeros(attrs.shape[0], l, 5, dtype=torch.int64, device=z.device)
    loss = torch.zeros(attrs.shape[0], dtype=torch.float64, device=z.device)
    for q in range(attrs.shape[0]):
        sa = torch.sign(attrs[q][None, :] - attrs[q][:, None]).to(torch.int8)
        a_ne = (sa != 0) & upper
        a_eq = (sa == 0) & upper
        for c in range(l):
            z_ne = sz[c] != 0
            counts[q, c, 0] = (a_ne & (sa == sz[c])).sum()
            counts[q, c, 1] = (a_ne & (sa == -sz[c])).sum()
            counts[q, c, 2] = (a_ne & ~z_ne).sum()
            counts[q, c, 3] = (a_eq & z_ne).sum()
            counts[q, c, 4] = (a_eq & ~z_ne).sum()
        ch = channels[q]
        if ch >= 0:
            d = (z[:, ch][None, :] - z[:, ch][:, None]).double()
            e = torch.tanh(float(deltas[q]) * d) - sa.double()
            loss[q] = ((e * e) * a_ne).sum()
    return counts, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000, 12000])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    channels, deltas = [0, 1, 2, 3, 4, 5], [1.0] * NA
    rows = []
    for n in args.sizes:
        z = torch.randn(n, L_CH, generator=gen).to(dev)
        attrs = torch.randint(0, 200, (NA, n), generator=gen).float().to(dev)      # ties as in pixel-count attributes
        zt = z.t().contiguous().t()                                                 # channel-major: used in place
        got = ops.rank_agreement(zt, attrs, channels, deltas)
        want = torch_restatement(z, attrs, channels, deltas)
        same = bool(torch.equal(got[0], want[0]))
        rel = float(((got[1] - want[1]).abs() / want[1].abs()).max())
        (t_k, k_lo, k_hi), (t_t, t_lo, t_hi), iters = compare(lambda: ops.rank_agreement(zt, attrs, channels, deltas),
                                                              lambda: torch_restatement(z, attrs, channels, deltas))
        none = [-1] * NA                                   # no attribute mapped: the counts alone, without the fp64 loss term
        (t_c, c_lo, c_hi), _, _ = compare(lambda: ops.rank_agreement(zt, attrs, none, deltas), lambda: None, target_ms=50.0)
        pairs = n * (n - 1) // 2
        row = dict(counts_only_us=t_c, counts_only_us_min=c_lo, counts_only_us_max=c_hi, n=n, l=L_CH, na=NA, pairs=pairs, kernel_us=t_k, kernel_us_min=k_lo, kernel_us_max=k_hi,
                   kernel_calls_per_window=iters, torch_us=t_t, torch_us_min=t_lo, torch_us_max=t_hi, ratio=t_t / t_k,
                   counts_equal=same, loss_rel_diff=rel, classifications_per_s=pairs * L_CH * NA / (t_k * 1e-6))
        rows.append(row)
        print(f"N={n}: kernel {t_k:9.1f} us [{k_lo:.1f} .. {k_hi:.1f}] ({iters} calls x 5 windows) | torch restatement "
              f"{t_t:11.1f} us [{t_lo:.1f} .. {t_hi:.1f}] | x{t_t / t_k:7.1f} | counts equal {same} | loss rel diff {rel:.1e} | "
              f"{row['classifications_per_s'] / 1e12:.2f} T pair classes/s | counts only (no channel mapped) {t_c:.1f} us [{c_lo:.1f} .. {c_hi:.1f}]",
              flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=2)


if __name__ == "__main__":
    main()

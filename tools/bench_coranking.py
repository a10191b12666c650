#!/usr/bin/env python3
"""Times the co-ranking curves and the Shepard figure (csrc/coranking.hip, analysis/coranking.py) at n = 2000, 6000 and 8192
rows of 50 columns with a noisy 2-D projection:

* ``ops.full_ranks`` (one matrix), ``ops.coranking_fold`` and ``ops.shepard_fold`` (64 bins), each on its own;
* the whole ``coranking_curves`` report (two distance matrices, two rank tables, the two folds, the copy to the host and
  the curves);
* a torch restatement on the same device, in the same session: ``argsort`` of the 64-bit keyed rows and a scatter to
  ranks (one matrix), and the folds as ``bincount`` calls and fp64 reductions;
* numpy on the host: the ranks as the tests' oracle forms them (``argsort`` of the keyed rows), the histograms by
  ``bincount`` and the fp64 sums, host clock, one run per size (``--no-host`` skips it).

Every integer of the kernels -- both rank tables, the three histograms, the squared rank differences, the Shepard histogram
-- is compared with the torch restatement before a number is printed.  Device-event timings after a warm-up: five windows
of each, reported as median [min .. max]; a kernel window is sized to about 100 ms.  A line says so where a kernel is slower
than its restatement.
usage: python tools/bench_coranking.py [--json OUT] [--sizes N ...] [--bins B] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pti_ldm_vae_amd import ops  # noqa: E402
from pti_ldm_vae_amd.analysis.coranking import coranking_curves  # noqa: E402

COLS, BINS = 50, 64


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


def torch_full_ranks(dist):
    """``ops.full_ranks`` with torch ops: argsort of the keyed rows, the inverse permutation, the own column taken out."""
    n = dist.shape[0]
    cols = torch.arange(n, device=dist.device)
    bits = (dist + 0.0).view(torch.int32).long()            # + 0.0: -0 becomes 0; distances are not negative
    order = torch.argsort((bits << 32) | cols[None, :], dim=1)
    pos = torch.empty_like(order)
    pos.scatter_(1, order, cols[None, :].expand(n, n))
    own = pos.diagonal()[:, None]
    rank = pos + 1 - (pos > own).long()
    rank.diagonal().zero_()
    return rank.short()


def torch_coranking_fold(rank_high, rank_low):
    n = rank_high.shape[1]
    a, b = rank_high.long(), rank_low.long()
    keep = (a >= 1) & (a <= n - 1) & (b >= 1) & (b <= n - 1)
    which = torch.where(a == b, 0, torch.where(b < a, 1, 2))
    hist = torch.bincount((which * n + torch.maximum(a, b))[keep], minlength=3 * n).view(3, n)
    return hist, ((a - b) ** 2 * keep).sum(dim=1)


def torch_shepard_fold(dist_high, dist_low, scale, bins):
    n = dist_high.shape[0]
    a, b = dist_high.double(), dist_low.double()
    off = ~torch.eye(n, dtype=torch.bool, device=dist_high.device)
    sums = torch.stack([(a * a * off).sum(dim=1), (b * b * off).sum(dim=1), (a * b * off).sum(dim=1)], dim=1)
    bh = (dist_high * scale[0]).long().clamp_(0, bins - 1)
    bl = (dist_low * scale[1]).long().clamp_(0, bins - 1)
    return sums, torch.bincount((bh * bins + bl)[off], minlength=bins * bins).view(bins, bins)


def host_baseline(dh, dl, bins):
    """The same report with numpy on the host -> seconds."""
    t0 = time.perf_counter()
    n = dh.shape[0]
    cols = np.arange(n)
    ranks = []
    for d in (dh, dl):
        keys = ((d + np.float32(0)).view(np.uint32).astype(np.uint64) << np.uint64(32)) | cols[None, :].astype(np.uint64)
        order = np.argsort(keys, axis=1, kind="stable")
        pos = np.empty_like(order)
        np.put_along_axis(pos, order, np.broadcast_to(cols, (n, n)), axis=1)
        own = pos[cols, cols][:, None]
        rank = pos + 1 - (pos > own)
        rank[cols, cols] = 0
        ranks.append(rank)
    a, b = ranks
    keep = (a >= 1) & (b >= 1)
    which = np.where(a == b, 0, np.where(b < a, 1, 2))
    np.bincount((which * n + np.maximum(a, b))[keep], minlength=3 * n)
    ((a - b) ** 2 * keep).sum(axis=1)
    off = ~np.eye(n, dtype=bool)
    a64, b64 = dh.astype(np.float64), dl.astype(np.float64)
    (a64 * a64 * off).sum(axis=1), (b64 * b64 * off).sum(axis=1), (a64 * b64 * off).sum(axis=1)
    bh = np.minimum((dh * (np.float32(bins) / dh.max())).astype(np.int64), bins - 1)
    bl = np.minimum((dl * (np.float32(bins) / dl.max())).astype(np.int64), bins - 1)
    np.bincount((bh * bins + bl)[off], minlength=bins * bins)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000, 8192])
    ap.add_argument("--bins", type=int, default=BINS, help=f"bins per axis of the Shepard histogram (default: {BINS})")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
    args = ap.parse_args()
    bins = args.bins
    dev = torch.device("cuda:0")
    rows = []
    for n in args.sizes:
        rng = np.random.default_rng(n)
        codes = np.arange(n) % 3
        high = (rng.standard_normal((3, COLS))[codes] * 1.5 + rng.standard_normal((n, COLS))).astype(np.float32)
        low = (high @ rng.standard_normal((COLS, 2)).astype(np.float32) / np.sqrt(COLS) + 0.35 * rng.standard_normal((n, 2))).astype(np.float32)
        x, y = torch.from_numpy(high).to(dev), torch.from_numpy(low).to(dev)
        dh, dl = ops.latent_pairwise(x), ops.projection_distances(y)
        rh, rl = ops.full_ranks(dh), ops.full_ranks(dl)
        hist, sq = ops.coranking_fold(rh, rl)
        sums, shepard, scale = ops.shepard_fold(dh, dl, bins)
        t_hist, t_sq = torch_coranking_fold(rh, rl)
        t_sums, t_shepard = torch_shepard_fold(dh, dl, scale, bins)
        same = {"rank_high": torch.equal(rh, torch_full_ranks(dh)), "rank_low": torch.equal(rl, torch_full_ranks(dl)),
                "histograms": torch.equal(hist.long(), t_hist), "sqdiff": torch.equal(sq, t_sq),
                "shepard_hist": torch.equal(shepard.long(), t_shepard)}
        if not all(same.values()):
            raise SystemExit(f"n={n}: the kernels and the torch restatement do not agree on every integer: {same}")
        sums_dev = float(((sums - t_sums).abs() / t_sums.abs().clamp_min(1e-300)).max())
        t = {"full_ranks": timed(lambda: ops.full_ranks(dh)),
             "coranking_fold": timed(lambda: ops.coranking_fold(rh, rl)),
             "shepard_fold": timed(lambda: ops.shepard_fold(dh, dl, bins)),
             "report": timed(lambda: coranking_curves(x, y, bins=bins, device=dev), target_ms=1.0),
             "torch_full_ranks": timed(lambda: torch_full_ranks(dh), target_ms=1.0),
             "torch_coranking_fold": timed(lambda: torch_coranking_fold(rh, rl), target_ms=1.0),
             "torch_shepard_fold": timed(lambda: torch_shepard_fold(dh, dl, scale, bins), target_ms=1.0)}
        host_s = None if args.no_host else host_baseline(dh.cpu().numpy(), dl.cpu().numpy(), bins)
        rows.append(dict(n=n, cols=COLS, bins=bins, integers_equal=True, row_sums_rel_dev_vs_torch=sums_dev, numpy_host_s=host_s,
                         **{f"{k}_us": v for k, v in t.items()}))
        fmt = lambda v: f"{v[0]:10.1f} us [{v[1]:.1f} .. {v[2]:.1f}]"   # noqa: E731
        print(f"n={n} bins={bins}: every integer equals the torch restatement; row sums within {sums_dev:.1e} of torch's")
        for name in ("full_ranks", "coranking_fold", "shepard_fold"):
            ratio = t[f"torch_{name}"][0] / t[name][0]
            print(f"  {name:15s} {fmt(t[name])} | torch {fmt(t[f'torch_{name}'])} (x{ratio:.1f})"
                  + ("" if ratio >= 1.0 else "   <-- the kernel is SLOWER than the torch restatement here"))
        torch_whole = 2 * t["torch_full_ranks"][0] + t["torch_coranking_fold"][0] + t["torch_shepard_fold"][0]
        print(f"  whole report    {fmt(t['report'])} | torch ranks + folds alone {torch_whole:10.1f} us | numpy on the host "
              + ("n/a" if host_s is None else f"{host_s:.2f} s"), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=2)


if __name__ == "__main__":
    main()

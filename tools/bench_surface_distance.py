#!/usr/bin/env python3
"""Time the surface-distance kernels against the scipy oracle of the tests on the host.

    python tools/bench_surface_distance.py [--iters 20]                           # device-event timings, one JSON line
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_surface_distance.py --only kernel

Per shape (64 pairs of 256 x 256, 8 pairs of 1024 x 1024; an ellipse against a shifted, dented ellipse with speckle):
``kernel_us`` is ``ops.surface_distance`` alone on the masks ``ops.mask_compare`` wrote; ``compare_us`` / ``compare_surface_us``
are the device work of one ``compare_images`` batch without and with ``--surface`` (``mask_compare`` with and without the mask
output, then the distance launches), ``surface_part_us`` their difference; ``host_1_thread_ms`` / ``host_16_threads_ms`` are the
oracle (``scipy.ndimage.distance_transform_edt`` both ways per pair) over the same masks, pairs spread over a thread pool.
Under rocprofv3 the launches are ``surface_columns_kernel`` / ``surface_rows_kernel`` / ``surface_select_kernel``."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(64, 256, 256), (8, 1024, 1024)]
WARMUP = 3
TOLERANCES, PERCENTILE = (1.0, 2.0), 95.0


def timed(fn, iters):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters, out


def make_pairs(n, h, w):
    rs = np.random.RandomState(n + h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    gts, preds = [], []
    for i in range(n):
        cy, cx = h / 2 + rs.uniform(-0.05, 0.05) * h, w / 2 + rs.uniform(-0.05, 0.05) * w
        g = ((yy - cy) / (0.40 * h)) ** 2 + ((xx - cx) / (0.30 * w)) ** 2 <= 1.0
        p = ((yy - cy - 0.02 * h) / (0.38 * h)) ** 2 + ((xx - cx + 0.015 * w) / (0.31 * w)) ** 2 <= 1.0
        p &= ~(((yy - cy) / (0.06 * h)) ** 2 + ((xx - cx - 0.3 * w) / (0.05 * w)) ** 2 <= 1.0)      # a dent in the wall
        p |= rs.rand(h, w) < 0.002
        gts.append(np.where(g, 0.25 + 0.5 * rs.rand(h, w), 0.0).astype(np.float32))
        preds.append(np.where(p, 0.3 + 0.5 * rs.rand(h, w), 0.0).astype(np.float32))
    return np.stack(gts), np.stack(preds)


def host_oracle(pairs, threads):
    import surface_distance_oracle as O
    t0 = time.perf_counter()
    if threads == 1:
        out = [O.table(a, b, O.GOLDEN_PM, TOLERANCES) for a, b in pairs]
    else:
        with ThreadPoolExecutor(threads) as pool:
            out = list(pool.map(lambda ab: O.table(ab[0], ab[1], O.GOLDEN_PM, TOLERANCES), pairs))
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=("kernel", "host"), default=None)
    args = ap.parse_args()
    from pti_ldm_vae_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    for n, h, w in SHAPES:
        gt_h, pred_h = make_pairs(n, h, w)
        gt, pred = torch.from_numpy(gt_h).to(dev), torch.from_numpy(pred_h).to(dev)
        counts, sums, masks = ops.mask_compare(gt, pred, masks=True)
        row = {}
        if args.only != "host":
            row["kernel_us"], got = timed(lambda: ops.surface_distance(masks, percentile=PERCENTILE, tolerances=TOLERANCES), args.iters)
            row["compare_us"], _ = timed(lambda: ops.mask_compare(gt, pred, out=(counts, sums)), args.iters)

            def with_surface():
                m = ops.mask_compare(gt, pred, out=(counts, sums), masks=masks)[2]
                return ops.surface_distance(m, percentile=PERCENTILE, tolerances=TOLERANCES)

            row["compare_surface_us"], _ = timed(with_surface, args.iters)
            row["surface_part_us"] = row["compare_surface_us"] - row["compare_us"]
            row["edge_pixels"] = int(got[0][:, :, 1].sum())
        if args.only != "kernel":
            m = masks.cpu().numpy()
            pairs = [((a & 1) != 0, (a & 2) != 0) for a in m]
            row["host_1_thread_ms"], want = host_oracle(pairs, 1)
            row["host_16_threads_ms"], _ = host_oracle(pairs, 16)
            if args.only is None:
                row["integers_equal"] = bool(got[0].cpu().numpy().tolist() == [t[0] for t in want])
                row["speedup_vs_16_threads"] = row["host_16_threads_ms"] * 1e3 / row["kernel_us"]
        res[f"{n}x{h}x{w}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

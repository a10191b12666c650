#!/usr/bin/env python3
"""Time the latent-analysis kernels against what a user would otherwise run: ``torch.cdist`` on the device (direct
differences, ``compute_mode="donot_use_mm_for_euclid_dist"``) and the reference-style numpy / scipy loop on the host.

    python tools/bench_latent_stats.py [--iters 10] [--no-host]                 # device-event timings, one JSON line
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_latent_stats.py --no-host

Per shape (rows of group A + rows of group B, D, patients): ``pairwise_us`` (``ops.latent_pairwise``, all rows of A against
all rows of B), ``group_stats_us`` (``ops.latent_group_stats``, all patients), ``statistics_ms`` (the whole
``LatentSpaceAnalyzer.compute_group_statistics`` from host arrays: upload, grouping, two device calls, text files),
``torch_cdist_us`` and ``host_loop_ms`` (per patient: np.mean, np.std, scipy cdist -- scipy missing: a numpy cdist).
Under rocprofv3 the kernels are ``latent_pairwise_tile_kernel`` / ``latent_pairwise_fold_kernel`` and
``latent_group_{cols,cross,finalize}_kernel``."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1000, 1000, 4096, 200), (1000, 1000, 40960, 200), (32, 32, 40960, 1)]
WARMUP = 2


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


def host_loop(a, b, seg):
    try:
        from scipy.spatial.distance import cdist
    except ImportError:
        def cdist(x, y):
            return np.stack([np.sqrt(((y - row) ** 2).sum(axis=1)) for row in x])
    rows = []
    for p in range(len(seg) - 1):
        x, y = a[seg[p]:seg[p + 1]], b[seg[p]:seg[p + 1]]
        rows.append((np.linalg.norm(np.mean(x, axis=0) - np.mean(y, axis=0)), np.mean(np.std(x, axis=0)) if len(x) > 1 else 0.0,
                     np.mean(np.std(y, axis=0)) if len(y) > 1 else 0.0, np.mean(cdist(x, y))))
    return np.array(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host numpy/scipy loop")
    args = ap.parse_args()
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    dev = torch.device("cuda:0")
    analyzer = LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)
    res = {}
    for n1, n2, d, patients in SHAPES:
        g = torch.Generator().manual_seed(n1 + d + patients)
        offset = 3.0 + 2.0 * torch.randn(d, generator=g)
        a = (offset + 0.3 * torch.randn(n1, d, generator=g)).to(dev)
        b = (offset + 0.3 * torch.randn(n2, d, generator=g)).to(dev)
        seg_host = [round(p * n1 / patients) for p in range(patients + 1)]           # both groups: equal patients
        seg = torch.tensor(seg_host, dtype=torch.int32, device=dev)
        ids = [str(p) for p in range(patients) for _ in range(seg_host[p + 1] - seg_host[p])]
        row = {}
        row["pairwise_us"], dist = timed(lambda: ops.latent_pairwise(a, b), args.iters)
        row["group_stats_us"], stats = timed(lambda: ops.latent_group_stats(a, seg, b, seg), args.iters)
        row["torch_cdist_us"], ref = timed(lambda: torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist"), args.iters)
        row["pairwise_vs_cdist_max_rel"] = float(((dist - ref).abs() / ref.clamp(min=1e-30)).max())
        a_host, b_host = a.cpu().numpy(), b.cpu().numpy()
        proj = np.random.default_rng(0).standard_normal((n1 + n2, 2))
        with tempfile.TemporaryDirectory() as tmp:
            def whole():
                analyzer.compute_group_statistics([(proj[:n1], ids, "edente"), (proj[n1:], ids, "dente")],
                                                  [(a_host, ids, "edente"), (b_host, ids, "dente")], tmp)
            whole()
            t0 = time.perf_counter()
            for _ in range(3):
                whole()
            row["statistics_ms"] = (time.perf_counter() - t0) / 3 * 1e3
        if not args.no_host:
            t0 = time.perf_counter()
            want = host_loop(a_host, b_host, seg_host)
            row["host_loop_ms"] = (time.perf_counter() - t0) * 1e3
            row["group_stats_vs_host_max_rel"] = float(np.max(np.abs(stats.cpu().numpy() - want) / np.abs(want)))
        res[f"{n1}+{n2}x{d}p{patients}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

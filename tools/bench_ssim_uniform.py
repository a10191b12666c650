#!/usr/bin/env python3
"""Time the uniform-window SSIM kernel against the same number written with torch ops on the device (what a user would
otherwise write: per-image min / max, five ``avg_pool2d(7, stride=1)`` calls, elementwise, a mean).

    python tools/bench_ssim_uniform.py [--iters 20]                               # device-event timings, one JSON line
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_ssim_uniform.py --iters 20 --only kernel

Under rocprofv3 the launches of the kernel are the rows ``ssim_uniform_minmax_kernel`` / ``ssim_uniform_tile_kernel`` /
``ssim_uniform_finalize_kernel`` (calls = iters + warm-up per shape); ``--only`` restricts the run to one side so that each is
profiled in a run of its own.  ``gbytes_per_s`` is the two-image read (2 * n * h * w * 4 bytes) over the kernel's time."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 256, 256), (8, 1024, 1024)]
WARMUP = 3


def torch_ssim(gt, pred):
    x, y = gt[:, None], pred[:, None]
    rng = (gt.amax(dim=(1, 2)) - gt.amin(dim=(1, 2)))[:, None, None, None]
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2

    def filt(t):
        return F.avg_pool2d(t, 7, stride=1)

    ux, uy = filt(x), filt(y)
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (filt(x * x) - ux * ux), cn * (filt(y * y) - uy * uy), cn * (filt(x * y) - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.mean(dim=(1, 2, 3), dtype=torch.float64)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=("kernel", "torch"), default=None)
    args = ap.parse_args()
    from pti_ldm_vae_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        n, h, w = shape
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        inside = (((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.36 * w)) ** 2 <= 1.0).to(dev)
        t = (0.25 + 0.5 * torch.rand(shape, generator=g).to(dev)) * inside
        p = (t + 0.05 * torch.randn(shape, generator=g).to(dev)) * inside
        row = {"bytes_read": 2 * p.numel() * 4}
        if args.only != "torch":
            row["kernel_us"], a = timed(lambda: ops.ssim_uniform(t, p), args.iters)
            row["gbytes_per_s"] = row["bytes_read"] / row["kernel_us"] * 1e-3
        if args.only != "kernel":
            row["torch_us"], b = timed(lambda: torch_ssim(t, p), args.iters)
        if args.only is None:
            row["max_abs_diff"] = float((a[:, 0] - b).abs().max())
            row["speedup"] = row["torch_us"] / row["kernel_us"]
        res["x".join(map(str, shape))] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

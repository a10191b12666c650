#!/usr/bin/env python3
"""Time the fused metrics kernel against the same four metrics written with torch ops on the device (what a user would
otherwise write: clamp, five conv2d calls with the 11x11 window, elementwise, means).

    python tools/bench_image_metrics.py [--iters 20]                              # device-event timings, one JSON line
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_image_metrics.py --iters 20

Under rocprofv3 the two launches of the kernel are the rows ``image_metrics_tile_kernel`` / ``image_metrics_finalize_kernel``
(calls = iters + warm-up per shape); everything else in the table belongs to the torch formulation.  ``--only`` restricts
the run to one side so that the profiler table of each can be read on its own."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 1, 256, 256), (8, 1, 256, 256)]
WARMUP = 3


def torch_metrics(pred, target, taps):
    x, y = pred.clamp(0.0, 1.0), target.clamp(0.0, 1.0)
    c = x.shape[1]
    k2d = (taps[:, None] @ taps[None, :])[None, None].repeat(c, 1, 1, 1)

    def filt(t):
        return F.conv2d(t, k2d, padding=5, groups=c)

    mu_x, mu_y = filt(x), filt(y)
    mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
    s_xx, s_yy, s_xy = filt(x * x) - mu_xx, filt(y * y) - mu_yy, filt(x * y) - mu_xy
    ssim = (((2 * mu_xy + 1e-4) * (2 * s_xy + 9e-4)) / ((mu_xx + mu_yy + 1e-4) * (s_xx + s_yy + 9e-4))).mean(dim=(1, 2, 3))
    d = x - y
    mse = (d * d).mean(dim=(1, 2, 3))
    return torch.stack([mse, d.abs().mean(dim=(1, 2, 3)), 10 * torch.log10(1.0 / mse.clamp(min=1e-12)), ssim], dim=1)


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
    taps = ops.ssim_taps().to(dev)
    res = {}
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        t = torch.rand(shape, generator=g).to(dev) * 1.2 - 0.1
        p = t + 0.1 * torch.randn(shape, generator=g).to(dev)
        row = {"bytes_read": 2 * p.numel() * 4}
        if args.only != "torch":
            row["kernel_us"], a = timed(lambda: ops.image_metrics(p, t, clamp=(0.0, 1.0)), args.iters)
        if args.only != "kernel":
            row["torch_us"], b = timed(lambda: torch_metrics(p, t, taps), args.iters)
        if args.only is None:
            row["max_abs_diff"] = float((a - b).abs().max())
            row["speedup"] = row["torch_us"] / row["kernel_us"]
        res["x".join(map(str, shape))] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

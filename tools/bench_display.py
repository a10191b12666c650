#!/usr/bin/env python3
"""Time the display triplet from device tensors to a host uint8 array, on the device and on the host.

    python tools/bench_display.py [--iters 20]                                   # wall-clock timings, one JSON line

Per shape, both sides start from the same two fp32 device batches (image, reconstruction) and end with the 8-bit
``[image | reconstruction | |difference|]`` canvas, turned by ``rot90(k=3)``, as a numpy array on the host:
  * ``device_us``: ``ops.display_planes(nsrc=3, rot90=3)`` and one uint8 copy;
  * ``host_us``: what the host path costs today -- ``.cpu()`` of the three planes, ``normalize_batch_for_display`` on each
    (numpy percentiles plane by plane), ``rot90``, concatenation, the cast to 8 bits.
Both end on the host, so the clock is the host's (``time.perf_counter`` after a synchronize); ``kernel_us`` is the launch
alone between two device events."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 256, 256), (8, 256, 256)]
WARMUP = 3


def make_batch(shape, dev):
    """A z-scored ellipse on a zero background and a noisy copy of it."""
    n, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    yy, xx = torch.linspace(-1, 1, h)[:, None], torch.linspace(-1, 1, w)[None, :]
    mask = ((xx / 0.80) ** 2 + (yy / 0.64) ** 2 <= 1.0).float()
    img = torch.randn(shape, generator=g) * mask
    rec = (img + 0.1 * torch.randn(shape, generator=g)) * mask
    return img.to(dev), rec.to(dev)


def device_triplet(img, rec):
    from pti_ldm_vae_amd import ops
    return ops.display_planes(img, rec, nsrc=3, rot90=3, dtype=torch.uint8)[0].cpu().numpy()


def host_triplet(img, rec):
    from pti_ldm_vae_amd.utils.visualization import normalize_batch_for_display
    a, b = img.cpu(), rec.cpu()
    parts = [torch.rot90(normalize_batch_for_display(t[:, None]), k=3, dims=[2, 3])[:, 0] for t in (a, b, torch.abs(a - b))]
    return (torch.cat(parts, dim=2).numpy() * 255).astype(np.uint8)


def wall(fn, iters):
    for _ in range(WARMUP):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters, out


def events(fn, iters):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=("device", "host"), default=None)
    args = ap.parse_args()
    from pti_ldm_vae_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    for shape in SHAPES:
        img, rec = make_batch(shape, dev)
        row = {}
        if args.only != "host":
            row["device_us"], d = wall(lambda: device_triplet(img, rec), args.iters)
            row["kernel_us"] = events(lambda: ops.display_planes(img, rec, nsrc=3, rot90=3), args.iters)
        if args.only != "device":
            row["host_us"], h = wall(lambda: host_triplet(img, rec), args.iters)
        if args.only is None:
            diff = np.abs(d.astype(np.int32) - h.astype(np.int32))
            row["max_level_diff"], row["pixels_differing"] = int(diff.max()), int((diff != 0).sum())
            row["speedup"] = row["host_us"] / row["device_us"]
        res["x".join(map(str, shape))] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

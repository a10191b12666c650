#!/usr/bin/env python3
"""Time the train-time augmentation on the device, no file I/O, one JSON line:

    python tools/bench_augment.py [--batch 32] [--size 256] [--iters 200]

  elastic_field_us / augment_warp_us    device time of one launch for the batch (device events, mean of --iters); every
                                        sample draws the elastic transform
  preprocess_us                         ``pti_preprocess_batch`` alone (raw images of 1.5 x --size, area resize + z-score)
  preprocess_augment_us                 preprocess + elastic_field + augment_warp, what the loader enqueues per batch
  draw_host_us                          host time of the batch's ``draw_params`` calls (wall clock)
  step_ms / ratio                       BENCH_r03's optimiser step (11.79 ms at batch 32, 256 x 256) and
                                        preprocess_augment / step: below 1 the copy stream still hides the input side
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_MS = 11.79   # BENCH_r03.json: config A, batch 32, 256 x 256, one MI355X


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import torch

    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.data.augment import AugmentPolicy, draw_params
    dev = torch.device("cuda:0")
    b, s, raw = args.batch, args.size, args.size * 3 // 2
    pol = AugmentPolicy(hflip_p=0.5, vflip_p=0.5, rot90_p=0.5, ssr_p=1.0, elastic_p=1.0)
    t0 = time.perf_counter()
    drawn = [draw_params(pol, 42, 0, i, s, s) for i in range(b)]
    draw_us = (time.perf_counter() - t0) * 1e6
    mats = torch.from_numpy(np.stack([d[0] for d in drawn])).to(dev)
    keys = torch.from_numpy(np.array([d[1] for d in drawn], np.uint64).view(np.int64)).to(dev)
    alpha = torch.from_numpy(np.array([d[2] for d in drawn], np.float32)).to(dev)

    g = torch.Generator(device=dev).manual_seed(0)
    lin = torch.linspace(-1, 1, raw, device=dev)
    mask = ((lin[None, :] / 0.8) ** 2 + (lin[:, None] / 0.64) ** 2 <= 1.0).float()
    src = ((torch.randn(b, raw, raw, generator=g, device=dev) * 300 + 900) * mask).reshape(-1).contiguous()
    offs = (torch.arange(b, dtype=torch.int64) * raw * raw).to(dev)
    hw = torch.tensor([[raw, raw]] * b, dtype=torch.int32, device=dev)
    pre = torch.empty(b, 1, s, s, device=dev)
    out = torch.empty_like(pre)
    field = torch.empty(b, 2, s, s, device=dev)
    stats = torch.empty(3 * b, dtype=torch.float64, device=dev)

    def preprocess():
        ops.preprocess_batch(src, offs, hw, pre, stats)

    def elastic():
        ops.elastic_field(keys, alpha, pol.elastic_sigma, s, s, out=field)

    def warp():
        ops.augment_warp(pre, mats, field, out=out)

    def both():
        preprocess()
        elastic()
        warp()

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / args.iters

    res = {"batch": b, "size": s, "channels": 1, "elastic_samples": b, "sigma": pol.elastic_sigma, "iters": args.iters}
    preprocess()
    res["elastic_field_us"] = timed(elastic)
    res["augment_warp_us"] = timed(warp)
    res["preprocess_us"] = timed(preprocess)
    res["preprocess_augment_us"] = timed(both)
    res["max_abs_field_px"] = float(field.abs().max())
    res["draw_host_us"] = draw_us
    res["step_ms"] = STEP_MS
    res["ratio_to_step"] = res["preprocess_augment_us"] / (STEP_MS * 1e3)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()

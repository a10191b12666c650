#!/usr/bin/env python3
"""Time the fused regression head against the torch sequence it replaces in an evaluation batch, the head alone
(4096 -> 256 -> 32 -> 6, relu, with the normaliser, targets and MSE) at n = 8 and n = 32.

    python tools/bench_regression_head.py [--iters 200] [--repeats 7]              # one JSON line

fused: ``ops.mlp_head_fwd`` (two launches: first layer, tail).  torch: what ``validate_one_epoch`` runs per batch after the
encoder -- ``normalizer.normalize(targets)``, ``model.regressor(flat)``, ``loss_fn``, ``total += loss``,
``normalizer.denormalize(out)``, the two list appends.  Both run on the same device tensors.  Each repeat times ``iters``
back-to-back calls between two device events after a warm-up; the two sides alternate repeat by repeat.  Reported per
side: the median over the repeats and the spread (min .. max), in microseconds per call, and the number of kernels one
call launches (counted with torch's profiler in a separate, untimed call)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = [4096, 256, 32, 6]
WARMUP = 20


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def kernel_count(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except Exception as exc:                                  # no device tracer in this build: say so, do not guess
        return f"not counted ({type(exc).__name__})"
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.models import LatentRegressor
    from pti_ldm_vae_amd.utils.regression_utils import TargetNormalizer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    head = LatentRegressor(DIMS[0], DIMS[1:-1], DIMS[-1]).to(dev).eval()
    params, dims, act = ops.mlp_head_pack(head)
    norm = TargetNormalizer(torch.linspace(20, 40, DIMS[-1]), torch.linspace(2, 6, DIMS[-1]))
    mean, std = norm.mean.to(dev), norm.std.to(dev)
    loss_fn = torch.nn.MSELoss()
    res = {"dims": DIMS, "iters": args.iters, "repeats": args.repeats}
    for n in (8, 32):
        flat = torch.randn(n, DIMS[0], device=dev)
        targets = (torch.randn(n, DIMS[-1], device=dev) * std + mean).contiguous()
        total = torch.zeros((), device=dev)
        pred, rowloss = torch.empty(n, DIMS[-1], device=dev), torch.empty(n, device=dev)

        def fused():
            ops.mlp_head_fwd(flat, params, dims, act, mean=mean, std=std, targets=targets, loss="mse", pred=pred, rowloss=rowloss)

        def torch_seq():
            nonlocal total
            preds, tgts = [], []
            with torch.no_grad():
                want = norm.normalize(targets)
                out = head(flat)
                total += loss_fn(out, want)
                preds.append(norm.denormalize(out))
                tgts.append(targets)
            return preds

        for fn in (fused, torch_seq):
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        times = {"fused": [], "torch": []}
        for _ in range(args.repeats):                       # alternate the two sides
            times["fused"].append(timed(fused, args.iters))
            times["torch"].append(timed(torch_seq, args.iters))
        row = {}
        for k, v in times.items():
            row[f"{k}_us_median"], row[f"{k}_us_min"], row[f"{k}_us_max"] = statistics.median(v), min(v), max(v)
        row["fused_kernels"], row["torch_kernels"] = kernel_count(fused), kernel_count(torch_seq)
        row["max_abs_diff_pred"] = float((pred - torch_seq()[0]).abs().max())
        res[f"n{n}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the guarded optimiser step (csrc/optim_guard.hip) against the plain ``ops.adam_step`` launch at the
arena size of a config (default: config A, ``config/vae_dente_no_adv.json``), and the whole training step with the guard
off and on.

    python tools/bench_optim_guard.py [--iters 50] [--windows 5] [--step-batch 32] [--no-step]

Device events after a warm-up; the variants alternate inside every window of the same process, and each figure is the
median [min .. max] over the windows.  ``bytes_per_param`` is what the variant must move: 28 B per parameter for Adam
(read p, g, m, v; write p, m, v), + 4 for the norm pass, + 8 for the EMA (read and write), plus two tiny launches.  One
JSON line; no pass or fail threshold."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 5


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters      # us per call


def alternate(variants, iters, windows):
    """{name: fn} -> {name: [median, min, max]} in us, the variants taking turns inside every window."""
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return {k: [statistics.median(v), min(v), max(v)] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config-file", default=os.path.join(ROOT, "config", "vae_dente_no_adv.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=32)
    ap.add_argument("--step-iters", type=int, default=15)
    ap.add_argument("--no-step", action="store_true", help="kernels only, not the whole training step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_guard: needs an MI355X; a CPU run measures nothing")
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.models import VAEModel
    from pti_ldm_vae_amd.trainer import VAETrainer
    from pti_ldm_vae_amd.utils import read_config
    cfg = read_config(args.config_file)
    dev = torch.device("cuda:0")
    n = VAEModel.from_config(cfg["autoencoder_def"]).autoencoder.param_arena.numel()
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=gen).to(dev) * 0.05
    g = torch.randn(n, generator=gen).to(dev) * 1e-3
    lr, betas = 2.5e-5, (0.9, 0.999)

    def state(ema):
        return [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), p0.clone() if ema else None, ops.grad_guard_ctl(dev), [0]]

    s_adam, s_skip, s_clip, s_ema, s_norm = state(False), state(False), state(False), state(True), state(False)

    def adam():
        s_adam[5][0] += 1
        ops.adam_step(s_adam[0], g, s_adam[1], s_adam[2], lr=lr, step=s_adam[5][0])

    def guarded(s, **kw):
        def run():
            ops.grad_guard(g, ctl=s[4], betas=betas, **kw)
            ops.adam_step_guarded(s[0], g, s[1], s[2], ctl=s[4], lr=lr, betas=betas, ema=s[3])
        return run

    variants = {"adam_step": adam,
                "guard (skip only)": guarded(s_skip, skip_nonfinite=True),
                "guard + clip (coef < 1)": guarded(s_clip, skip_nonfinite=True, max_norm=1e-3),
                "guard + clip + ema": guarded(s_ema, skip_nonfinite=True, max_norm=1e-3, ema_decay=0.999),
                "norm pass + decision alone": lambda: ops.grad_guard(g, ctl=s_norm[4], betas=betas, skip_nonfinite=True)}
    bytes_per_param = {"adam_step": 28, "guard (skip only)": 32, "guard + clip (coef < 1)": 32, "guard + clip + ema": 40,
                      "norm pass + decision alone": 4}
    t = alternate(variants, args.iters, args.windows)
    # the variants computed the same thing where they should: clip off and coef 1 is adam_step (checked once, same inputs)
    a, b = state(False), state(False)
    ops.adam_step(a[0], g, a[1], a[2], lr=lr, step=1)
    guarded(b, skip_nonfinite=True)()
    torch.cuda.synchronize()
    res = {"config": os.path.basename(args.config_file), "arena_elements": n, "iters": args.iters, "windows": args.windows,
           "max_abs_diff_guard_vs_adam_step": float((a[0] - b[0]).abs().max()), "kernels": {}}
    for k, (med, lo, hi) in t.items():
        res["kernels"][k] = {"us_median": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
                             "bytes_per_param": bytes_per_param[k],
                             "gbytes_per_s": round(bytes_per_param[k] * n / med * 1e-3, 1),
                             "vs_adam_step": round(med / t["adam_step"][0], 3),
                             "bytes_vs_adam_step": round(bytes_per_param[k] / 28, 3)}
    if not args.no_step:
        tr = cfg["autoencoder_train"]
        size = tuple(tr["patch_size"])
        x = torch.randn(args.step_batch, cfg["autoencoder_def"]["in_channels"], *size, generator=gen).to(dev)
        trainers = {}
        for name, kw in (("guard off", {}), ("guard on (clip 1.0, skip, ema 0.999)",
                                             dict(clip_norm=1.0, skip_nonfinite=True, ema_decay=0.999))):
            torch.manual_seed(0)
            model = VAEModel.from_config(cfg["autoencoder_def"]).to(dev)
            trainers[name] = VAETrainer(model, lr=tr["lr"], kl_weight=tr["kl_weight"], recon_loss=tr.get("recon_loss", "l1"), **kw)
        steps = {k: (lambda v=v: v.step(x)) for k, v in trainers.items()}
        ts = alternate(steps, args.step_iters, args.windows)
        res["step"] = {"batch": args.step_batch, "size": list(size), "iters": args.step_iters,
                       **{k: {"ms_median": round(m / 1e3, 3), "ms_min": round(lo / 1e3, 3), "ms_max": round(hi / 1e3, 3)}
                          for k, (m, lo, hi) in ts.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

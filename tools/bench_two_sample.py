#!/usr/bin/env python3
"""Times the two-sample permutation tests (csrc/two_sample.hip, analysis/two_sample.py) at N = 2000, 6000 and 8192 pooled
rows of 50 columns with P = 9999 relabellings:

* ``ops.permutation_forms`` per matrix (P + 2 labellings: observed, relabellings, all-ones), with the achieved int8
  multiply-add rate of the fold (2 planes x 2 P N^2 operations over the whole call, split and padding included);
* ``ops.distance_median`` and ``ops.two_sample_kernel`` (both kinds);
* the whole ``two_sample_tests`` (host clock, one run: it includes drawing the labellings on the host);
* a torch restatement on the same device, in the same process: ``S.double() @ W.double()`` (exact below 2^53) and the
  three sums from it;
* the numpy oracle's integer product on the host with ``--host-perms`` labellings (default 16), scaled linearly to P --
  the figure is an extrapolation and the row says so.

Every integer of the kernel is compared with the torch restatement before a number is printed.  The measuring runs in ONE
child process under a time limit; this process never touches the device.  Device-event timings after a warm-up: three
windows of each, reported as median [min .. max].  A line says so where the kernel is slower than its restatement.
usage: python tools/bench_two_sample.py [--json OUT] [--sizes N ...] [--perms P] [--host-perms H] [--timeout S]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 50


def window(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def timed(torch, fn, rounds=3, target_ms=50.0):
    """-> (median, min, max) in us over ``rounds`` windows sized to about ``target_ms`` after a warm-up."""
    fn()
    torch.cuda.synchronize()
    iters = int(min(1000, max(1, target_ms * 1e3 / max(window(torch, fn, 1), 1e-3))))
    t = sorted(window(torch, fn, iters) for _ in range(rounds))
    return t[len(t) // 2], t[0], t[-1]


def child(args):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis.two_sample import permutation_masks, two_sample_tests

    def torch_forms(w, s):
        sd, wd = s.double(), w.double()
        t = sd @ wd
        return torch.stack([(t * sd).sum(1), sd @ wd.sum(1), sd @ wd.sum(0)], dim=1).long()

    dev = torch.device("cuda:0")
    rows = []
    for n in args.sizes:
        rng = np.random.default_rng(n)
        n_a = n // 2
        z = rng.standard_normal((n, COLS)).astype(np.float32)
        z[n_a:] += np.float32(0.05)
        x = torch.from_numpy(z).to(dev)
        dist = ops.latent_pairwise(x)
        med = ops.distance_median(dist)
        w = ops.two_sample_kernel(dist, "gaussian", scale=med)
        t0 = time.perf_counter()
        masks = np.concatenate([permutation_masks(n_a, n - n_a, args.perms, 0), np.ones((1, n), np.uint8)])
        masks_s = time.perf_counter() - t0
        s = torch.from_numpy(masks).to(dev)
        p = s.shape[0]
        got = ops.permutation_forms(w, s)
        if not torch.equal(got, torch_forms(w, s)):
            raise SystemExit(f"n={n}: the kernel and the torch restatement do not agree on every integer")
        t = {"permutation_forms": timed(torch, lambda: ops.permutation_forms(w, s)),
             "torch_forms": timed(torch, lambda: torch_forms(w, s)),
             "distance_median": timed(torch, lambda: ops.distance_median(dist)),
             "kernel_gaussian": timed(torch, lambda: ops.two_sample_kernel(dist, "gaussian", scale=med)),
             "kernel_energy": timed(torch, lambda: ops.two_sample_kernel(dist, "energy"))}
        t0 = time.perf_counter()
        report, _ = two_sample_tests(z[:n_a], z[n_a:], permutations=args.perms, device=dev)
        whole_s = time.perf_counter() - t0
        host_s = None
        if args.host_perms > 0:
            w64, s64 = w.cpu().numpy().astype(np.int64), masks[:args.host_perms].astype(np.int64)
            t0 = time.perf_counter()
            tt = s64 @ w64
            (tt * s64).sum(1), s64 @ w64.sum(1), s64 @ w64.sum(0)
            host_s = (time.perf_counter() - t0) * p / args.host_perms
        ops_int8 = 2.0 * 2.0 * p * float(n) * float(n)
        rows.append(dict(n=n, cols=COLS, labellings=p, integers_equal=True, masks_host_s=masks_s, two_sample_tests_s=whole_s,
                         numpy_host_s_extrapolated=host_s, numpy_host_labellings=args.host_perms,
                         int8_tops_achieved=ops_int8 / (t["permutation_forms"][0] * 1e-6) / 1e12,
                         p_values={k: v["p_value"] for k, v in report["tests"].items()},
                         **{f"{k}_us": v for k, v in t.items()}))
        fmt = lambda v: f"{v[0]:10.1f} us [{v[1]:.1f} .. {v[2]:.1f}]"   # noqa: E731
        ratio = t["torch_forms"][0] / t["permutation_forms"][0]
        print(f"n={n} P={p}: every integer equals the torch restatement", file=sys.stderr)
        print(f"  permutation_forms {fmt(t['permutation_forms'])} ({rows[-1]['int8_tops_achieved']:.1f} int8 TOPS) | torch fp64 "
              f"{fmt(t['torch_forms'])} (x{ratio:.2f})"
              + ("" if ratio >= 1.0 else "   <-- the kernel is SLOWER than the torch restatement here"), file=sys.stderr)
        print(f"  median {fmt(t['distance_median'])} | gaussian {fmt(t['kernel_gaussian'])} | energy {fmt(t['kernel_energy'])}",
              file=sys.stderr)
        print(f"  whole two_sample_tests {whole_s:.2f} s (labellings on the host {masks_s:.2f} s) | numpy on the host "
              + ("n/a" if host_s is None else f"{host_s:.1f} s, extrapolated from {args.host_perms} labellings"), file=sys.stderr,
              flush=True)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000, 8192])
    ap.add_argument("--perms", type=int, default=9999)
    ap.add_argument("--host-perms", type=int, default=16, help="labellings of the numpy baseline, scaled to P (0: skip it)")
    ap.add_argument("--timeout", type=float, default=540.0, help="time limit of the measuring process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--perms", str(args.perms), "--host-perms", str(args.host_perms),
           "--sizes"] + [str(n) for n in args.sizes]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_two_sample: the measuring process ran past {args.timeout:.0f} s and was ended")
    if done.returncode != 0:
        raise SystemExit(f"bench_two_sample: the measuring process ended with status {done.returncode}")
    line = done.stdout.strip().splitlines()[-1]
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(json.dumps(json.loads(line), indent=2) + "\n")


if __name__ == "__main__":
    main()

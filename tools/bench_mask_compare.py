#!/usr/bin/env python3
"""Time ``ops.mask_compare`` on what a decoded batch looks like (blob plus speckle, voids inside the blob):

    python tools/bench_mask_compare.py [--images 64] [--size 256] [--iters 200] [--repeats 5]      # one JSON line

  kernel_us            device time of ONE ``pti_mask_compare`` launch over the whole batch: device events round --iters
                       launches after a warm-up, the median of --repeats such windows; kernel_us_min / _max: their spread
  oracle_ms_1thread    wall time of the scipy restatement (``tests/mask_compare_oracle.compare``: label, fill, counts) over
                       the same batch on one host thread; oracle_ms_threads16: on 16 threads
  call_ms              host wall time of upload + launch + the one copy back (``compare_images.compare_batch``)
  workspace_mb         the scratch the call uses

The device result is compared with the oracle's before any number is printed; the host timings run before the device is
touched.  Without a GPU this fails: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import mask_compare_oracle as O
    n, s = args.images, args.size
    pairs = [O.images_from_masks(O.blob_speckle(s, s, 2 * i, speckle=0.005, voids=0.0), O.blob_speckle(s, s, 2 * i + 1), seed=i)
             for i in range(n)]
    gt, pred = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    res = {"images": n, "size": s}

    O.compare(gt[:1], pred[:1])                     # the first call imports scipy.ndimage: not part of the timing
    res["oracle_ms_1thread"], (want_c, want_s, _) = wall_ms(lambda: O.compare(gt, pred))
    with ThreadPoolExecutor(16) as pool:
        res["oracle_ms_threads16"], _ = wall_ms(lambda: list(pool.map(lambda i: O.compare(gt[i:i + 1], pred[i:i + 1]), range(n))))

    import torch
    from pti_ldm_vae_amd import _lib, ops
    from pti_ldm_vae_amd.compare_images import compare_batch
    dev = torch.device("cuda:0")
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    out = ops.mask_compare(d_gt, d_pred)
    for _ in range(10):
        ops.mask_compare(d_gt, d_pred, out=out)
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tolist() == want_c.tolist(), "kernel table differs from the scipy oracle"
    assert np.allclose(out[1].cpu().numpy(), want_s, rtol=1e-12, atol=0), "kernel sums differ from the scipy oracle"
    windows = []
    for _ in range(args.repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            ops.mask_compare(d_gt, d_pred, out=out)
        stop.record()
        torch.cuda.synchronize()
        windows.append(start.elapsed_time(stop) * 1e3 / args.iters)
    res["kernel_us"], res["kernel_us_min"], res["kernel_us_max"] = statistics.median(windows), min(windows), max(windows)
    res["kernel_name"] = ops.last_kernel_name()
    res["workspace_mb"] = _lib.lib().pti_mask_compare_ws_bytes(n, s, s) / 2 ** 20
    res["mpixel_per_s"] = n * s * s / res["kernel_us"]
    compare_batch(list(gt), list(pred), 0.2, dev)
    calls = [wall_ms(lambda: compare_batch(list(gt), list(pred), 0.2, dev))[0] for _ in range(5)]
    res["call_ms"] = statistics.median(calls)
    res["oracle_over_kernel_1thread"] = res["oracle_ms_1thread"] * 1e3 / res["kernel_us"]
    res["oracle_over_kernel_threads16"] = res["oracle_ms_threads16"] * 1e3 / res["kernel_us"]
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()

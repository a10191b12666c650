#!/usr/bin/env python3
"""Time the pair registration of ``compare_images --straighten`` on tilted blob pairs:

    python tools/bench_mask_register.py [--images 8 64 256] [--size 256] [--iters 100] [--repeats 5]    # one JSON line per batch

  moments_us / warp_us / align_us   device time of ONE launch of that kernel over the whole batch: device events round
                                    --iters launches after a warm-up, the median of --repeats such windows, with
                                    ``_min`` / ``_max``: their spread
  register_us                       the same for ``ops.register_pairs`` (the three launches in order)
  compare_us                        the same for the ``ops.mask_compare`` launch that follows on the registered pair
  oracle_ms_per_image               wall time of the numpy restatement (``tests/mask_register_oracle.register``) per image,
                                    one host thread, over the first --oracle-images images of the batch
  call_ms                           host wall time of upload + four launches + the one copy back
                                    (``compare_images.compare_batch(..., straighten=True)``)

The device's moments are compared with the oracle's, and its rotation with the oracle's under the fp32 restatement's own
deviation, before any number is printed; the host timing runs before the device is touched.  Without a GPU this fails:
there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_batch(n, s):
    """Tilted ellipses with voids inside and speckle round them on the prediction side."""
    import mask_compare_oracle as O
    import mask_register_oracle as R
    rs = np.random.RandomState(n)
    gts, preds = [], []
    for i in range(n):
        tilt = rs.uniform(-40, 40)
        g = R.ellipse(s, s, tilt, 0.38 * s, 0.16 * s, cy=0.52 * s)
        r = R.ellipse(s, s, tilt + rs.uniform(-5, 5), 0.36 * s, 0.17 * s, cy=0.52 * s, cx=s / 2 + rs.uniform(-4, 4))
        r = (r & (rs.rand(s, s) >= 0.03)) | (~r & (rs.rand(s, s) < 0.02))
        gt, pred = O.images_from_masks(g, r, seed=i)
        gts.append(gt)
        preds.append(pred)
    return np.stack(gts), np.stack(preds)


def windows(fn, iters, repeats):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop) * 1e3 / iters)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle-images", type=int, default=4)
    args = ap.parse_args()
    import mask_register_oracle as R
    s = args.size
    batches, host = {}, {}
    for n in args.images:                            # every host timing before the device is touched
        gt, pred = batches[n] = make_batch(n, s)
        k = min(n, args.oracle_images)
        R.register(gt[0], pred[0])                   # the first call imports scipy.ndimage: not part of the timing
        t0 = time.perf_counter()
        want = [R.register(gt[i], pred[i]) for i in range(k)]
        host[n] = ((time.perf_counter() - t0) * 1e3 / k, want)

    import torch
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.compare_images import compare_batch
    dev = torch.device("cuda:0")
    for n in args.images:
        gt, pred = batches[n]
        oracle_ms, want = host[n]
        d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        cleaned, moments, coeffs = m_out = ops.mask_moments(d_gt, d_pred)
        w_out = ops.warp_cubic(d_gt, cleaned, coeffs)
        a_out = ops.align_bottom(*w_out)
        r_gt, r_al, info = ops.register_pairs(d_gt, d_pred)
        r_out = (r_gt, r_al, info["moments"], info["coeffs"], info["align"])
        c_out = ops.mask_compare(r_gt, r_al)
        torch.cuda.synchronize()
        got_m, got_g = moments.cpu().numpy(), w_out[0].cpu().numpy()
        for i, res in enumerate(want):
            assert got_m[i].tolist() == res["moments"], f"image {i}: the kernel's moments differ from the oracle's"
            exact = R.rotate(gt[i], res["coeffs"][0][1], res["coeffs"][0][2], np.float64)
            gate = 2.0 * np.abs(res["rot_gt"].astype(np.float64) - exact).max()
            assert np.abs(got_g[i].astype(np.float64) - exact).max() <= gate, f"image {i}: the kernel's rotation differs from the oracle's"
        res = {"images": n, "size": s, "iters": args.iters, "oracle_ms_per_image": oracle_ms, "oracle_images": len(want)}
        for key, fn in (("moments", lambda: ops.mask_moments(d_gt, d_pred, out=m_out)),
                        ("warp", lambda: ops.warp_cubic(d_gt, cleaned, coeffs, out=w_out)),
                        ("align", lambda: ops.align_bottom(*w_out, out=a_out)),
                        ("register", lambda: ops.register_pairs(d_gt, d_pred, out=r_out)),
                        ("compare", lambda: ops.mask_compare(r_gt, r_al, out=c_out))):
            w = windows(fn, args.iters, args.repeats)
            res[f"{key}_us"], res[f"{key}_us_min"], res[f"{key}_us_max"] = statistics.median(w), min(w), max(w)
        compare_batch(list(gt), list(pred), 0.2, dev, straighten=True)
        calls = []
        for _ in range(5):
            t0 = time.perf_counter()
            compare_batch(list(gt), list(pred), 0.2, dev, straighten=True)
            calls.append((time.perf_counter() - t0) * 1e3)
        res["call_ms"] = statistics.median(calls)
        res["oracle_over_register"] = oracle_ms * n * 1e3 / res["register_us"]
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()

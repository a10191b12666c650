#!/usr/bin/env python3
"""Time the mask-geometry path on masks a user would run it on (ellipse-like, ``--size`` x ``--size`` uint8):

    python tools/bench_mask_geometry.py [--masks 256] [--size 512] [--iters 50]          # one JSON line

  kernel_us            device time of ONE ``pti_mask_geometry`` launch over all masks (device events, mean of --iters)
  numpy_ms_threads16   wall time of the numpy restatement (``tests/mask_metrics_oracle.geometry``) over the same masks on
                       16 host threads (numpy releases the GIL in these calls); numpy_ms_1thread: one thread
  decode_ms / decode_deflate_ms   ``read_tiff`` of all masks + as many dente masks from uncompressed / deflate files, one thread
  cli_ms / cli_deflate_ms         ``compute_mask_metrics.process_dataset`` end to end on those folders (decode included)
  attributes_ms        ``data.mask_metrics.mask_attributes`` on the decoded arrays: packing, uploads, two launches, readback

The host timings run before the device is touched."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

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
    ap.add_argument("--masks", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import mask_metrics_oracle as O
    from pti_ldm_vae_amd.data import read_tiff, write_tiff
    n, s = args.masks, args.size
    offsets = O.pixel_offsets([5, 10, 14, 18, 22], 0.15)
    masks = [O.make_mask(O._m(s, s, [["ellipse", s // 2, s // 2, s // 3 - i % 7, s // 4 + i % 11]], seed=i, holes=0.1, speckle=1e-4))
             for i in range(n)]
    res = {"masks": n, "size": s, "dtype": "uint8"}

    want = None
    for threads in (1, 16):
        with ThreadPoolExecutor(threads) as pool:
            res[f"numpy_ms_{'1thread' if threads == 1 else 'threads16'}"], want = wall_ms(
                lambda: list(pool.map(lambda m: O.geometry(m, 5, offsets), masks)))

    with tempfile.TemporaryDirectory() as tmp:
        folders = {}
        for tag, deflate in (("", False), ("_deflate", True)):
            ed, de = Path(tmp) / f"edente{tag}", Path(tmp) / f"dente{tag}"
            ed.mkdir()
            de.mkdir()
            for i, m in enumerate(masks):
                write_tiff(str(ed / f"{i:04d}.tif"), m, deflate=deflate)
                write_tiff(str(de / f"{i:04d}.tif"), masks[(i + 1) % n], deflate=deflate)
            folders[tag] = (ed, de)
            res[f"decode{tag}_ms"], _ = wall_ms(lambda: [read_tiff(str(p)) for d in (ed, de) for p in sorted(d.iterdir())])

        import torch
        from pti_ldm_vae_amd import compute_mask_metrics as cli
        from pti_ldm_vae_amd import ops
        from pti_ldm_vae_amd.data.mask_metrics import mask_attributes, pack_masks, sample_row_table
        dev = torch.device("cuda:0")
        buf, off, hw, elem = pack_masks(masks)
        max_h = s
        t = dict(src=torch.from_numpy(buf).to(dev), offsets=torch.from_numpy(off).to(dev), hw=torch.from_numpy(hw).to(dev))
        kw = dict(elem=elem, max_h=max_h, sample_rows=torch.from_numpy(np.array(sample_row_table(max_h, 5))).to(dev),
                  bottom_offsets=torch.tensor(offsets, dtype=torch.int32, device=dev))
        out = ops.mask_geometry(t["src"], t["offsets"], t["hw"], **kw)
        for _ in range(3):
            ops.mask_geometry(t["src"], t["offsets"], t["hw"], out=out, **kw)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            ops.mask_geometry(t["src"], t["offsets"], t["hw"], out=out, **kw)
        stop.record()
        torch.cuda.synchronize()
        res["kernel_us"] = start.elapsed_time(stop) * 1e3 / args.iters
        res["kernel_gb_per_s"] = buf.nbytes / (res["kernel_us"] * 1e-6) / 1e9
        got = tuple(x.cpu().numpy().tolist() for x in out)
        assert got == tuple([w[k] for w in want] for k in range(3)), "kernel result differs from the numpy restatement"
        res["kernel_name"] = ops.last_kernel_name()

        dente = masks[1:] + masks[:1]
        mask_attributes(masks, dente, samples=5, bottom_offsets=offsets, device=dev)     # warm: tables, allocator
        res["attributes_ms"], _ = wall_ms(lambda: mask_attributes(masks, dente, samples=5, bottom_offsets=offsets, device=dev))
        for tag, (ed, de) in folders.items():
            res[f"cli{tag}_ms"], (a, b) = wall_ms(lambda: cli.process_dataset(
                ed, de, pixel_size_mm=0.15, dente_heights_mm=(5, 10, 14, 18, 22), edente_width_samples=5, batch_size=64, device=dev))
            assert len(a) == len(b) == n
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()

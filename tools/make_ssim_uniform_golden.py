#!/usr/bin/env python3
"""Generates tests/golden/ssim_uniform_golden.npz (TEST INFRASTRUCTURE):

    python tools/make_ssim_uniform_golden.py

Records the cases of ``tests/ssim_uniform_oracle.case_list`` -- every tested shape at noise 0.05, and at 45 x 71 and 64 x 64 the
noise, offset, identical, all-background and constant-ground-truth variants -- as what rebuilds each image (shape, seed, noise,
offset, variant) and the expected ``{ssim, data range}`` of the fp64 valid-window oracle; the images themselves are not stored.
Before anything is written the literal scipy transcription of skimage's function must agree with that oracle to 1e-12 on
every case.  Where ``skimage`` itself can be imported, it is asked too (same bound) and the output says so.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ssim_uniform_golden.npz"))
    args = ap.parse_args()
    import ssim_uniform_oracle as O
    try:
        from skimage.metrics import structural_similarity
    except Exception:
        structural_similarity = None
    cases, expected = O.case_list(), []
    for c in cases:
        x, y = O.case_pair(c)
        want, lit = O.ssim_valid(x, y), O.ssim_scipy(x, y)
        assert abs(want[0] - lit[0]) <= 1e-12 and want[1] == lit[1], f"the two oracles disagree on {c['name']}: {want} / {lit}"
        if structural_similarity is not None and want[1] != 0:
            sk = structural_similarity(y.astype(np.float64), x.astype(np.float64), data_range=want[1])
            assert abs(sk - want[0]) <= 1e-12, f"skimage disagrees on {c['name']}: {sk} / {want[0]}"
        expected.append(want)
    np.savez_compressed(args.out, **O.pack_cases(cases, expected))
    size = os.path.getsize(args.out)
    assert size < 100 * 1024, f"{args.out}: {size} bytes, the fixture must stay under 100 KB"
    print(f"wrote {args.out}: {len(cases)} cases, {size} bytes; skimage " + ("checked too" if structural_similarity else "not importable: not checked"))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/surface_distance_golden.npz (TEST INFRASTRUCTURE):

    python tools/make_surface_distance_golden.py

Records the cases of ``tests/surface_distance_oracle.golden_cases`` -- every hand-built mask of the comparison oracle against
its half turn, and per tested shape blobs, a spiral against a comb, a ring, a full image, a corner pixel against a
checkerboard, identical masks and empty sides -- with the eleven integer columns per side and the fp64 sums the scipy oracle
gives at the 95th percentile and tolerances of 1 and 2 pixels.  Masks are stored as packed bits, names and shapes beside them.
Before anything is written the pure-numpy oracle must give the same table for every case, and the definition itself (all
pairs of edge pixels) for every case of at most 4096 pixels.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "surface_distance_golden.npz"))
    args = ap.parse_args()
    import surface_distance_oracle as O
    cases = O.golden_cases()
    packed = O.pack_cases(cases)
    for (name, a, b), want_c, want_s in zip(cases, packed["counts"], packed["sums"]):
        for impl in ("numpy",) + (("brute",) if a.size <= 4096 else ()):
            got_c, got_s = O.table(a, b, impl=impl)
            assert got_c == want_c.tolist() and got_s == want_s.tolist(), f"the {impl} oracle disagrees with scipy's on {name}"
    np.savez_compressed(args.out, **packed)
    size = os.path.getsize(args.out)
    assert size < 100 * 1024, f"{args.out}: {size} bytes, the fixture must stay under 100 KB"
    print(f"wrote {args.out}: {len(cases)} cases, {size} bytes")


if __name__ == "__main__":
    main()

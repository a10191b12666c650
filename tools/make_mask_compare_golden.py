#!/usr/bin/env python3
"""Generates tests/golden/mask_compare_golden.npz (TEST INFRASTRUCTURE):

    python tools/make_mask_compare_golden.py

Records the cases of ``tests/mask_compare_oracle.golden_cases`` -- the hand-built masks (spiral, U, comb, checkerboard,
rings, equal and late components, empty and full) and one seeded blob-plus-speckle pair per tested shape -- with the 24
integer columns the scipy oracle gives for each.  Masks are stored as packed bits, names and shapes beside them; the float
images the tests run on are derived from the masks by ``mask_compare_oracle.images_from_masks``.  Before anything is written
the pure-numpy oracle must give the same table for every case.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mask_compare_golden.npz"))
    args = ap.parse_args()
    import mask_compare_oracle as O
    cases = O.golden_cases()
    packed = O.pack_cases(cases)
    for (name, g, r), want in zip(cases, packed["expected"]):
        assert O.table_masks(g, r, impl="numpy") == want.tolist(), f"the two oracles disagree on {name}"
    np.savez_compressed(args.out, **packed)
    size = os.path.getsize(args.out)
    assert size < 100 * 1024, f"{args.out}: {size} bytes, the fixture must stay under 100 KB"
    print(f"wrote {args.out}: {len(cases)} cases, {size} bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/mask_register_golden.npz (TEST INFRASTRUCTURE):

    python tools/make_mask_register_golden.py

Records the cases of ``tests/mask_register_oracle.golden_cases`` -- ellipses tilted by 12, -27, 55 and -80 degrees, an
upright one, a disc, a horizontal bar, an object with a hole and an island, one cut by the border, an L-shape and an
odd-sized image -- with what ``mask_register_oracle.register`` gives for each: the six moments and A, B, C per side, both
angles, the six alignment integers, and the non-zero counts and exactly rounded sums of the rotated and aligned images.
Masks are stored as packed bits; the float images are derived from them by ``mask_register_oracle.images``.  Before
anything is written the second restatement of the moments and the pure-numpy labelling must give the same integers.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mask_register_golden.npz"))
    args = ap.parse_args()
    import mask_register_oracle as R
    cases = R.golden_cases()
    packed = R.pack_cases(cases)
    for (name, g, r, _, _), want in zip(cases, packed["expected_moments"]):
        for side, mask in enumerate((g, r)):
            region = R.filled_largest(mask, impl="numpy")
            m = R.raw_moments_profiles(region)
            assert m + list(R.central(m)) == want[side].tolist(), f"the two restatements disagree on {name}, side {side}"
    np.savez_compressed(args.out, **packed)
    size = os.path.getsize(args.out)
    assert size < 100 * 1024, f"{args.out}: {size} bytes, the fixture must stay under 100 KB"
    print(f"wrote {args.out}: {len(cases)} cases, {size} bytes")


if __name__ == "__main__":
    main()

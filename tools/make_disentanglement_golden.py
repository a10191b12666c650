#!/usr/bin/env python3
"""Records tests/golden/disentanglement_golden.npz (TEST INFRASTRUCTURE) from the numpy oracle:

    python tools/make_disentanglement_golden.py

Per case of ``tests/disentanglement_oracle.CASES``: the integer tables (edges as fp64, rank2, sums, gram, bins, counts) and
the fp64 matrices and scores of ``report``.  The GPU tests compare the kernels with these tables cell by cell; the CPU tests
check that the oracle still reproduces the file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import disentanglement_oracle as O
    out = {}
    for case in O.all_cases():
        r = O.report(case.z, case.attrs, case.bins)
        for key in O.TABLES + O.FLOATS:
            out[f"{case.name}/{key}"] = r[key]
        print(f"{case.name}: n {case.n} columns {case.l + case.na} bins {case.bins} scores "
              + " ".join(f"{k} {v:.6f}" for k, v in zip(O.SCORES, r["scores"])))
    os.makedirs(os.path.dirname(O.GOLDEN), exist_ok=True)
    np.savez_compressed(O.GOLDEN, **out)
    print("wrote", O.GOLDEN, os.path.getsize(O.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

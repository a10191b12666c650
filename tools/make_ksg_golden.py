#!/usr/bin/env python3
"""Records tests/golden/ksg_golden.npz (TEST INFRASTRUCTURE) from the numpy oracle:

    python tools/make_ksg_golden.py

Per case of ``tests/ksg_oracle.CASES`` and neighbour count k: ``<case>/k<k>/eps`` (fp32), ``/nx``, ``/ny`` (stored as int16:
no count exceeds n - 1 <= 2499) and ``/mi`` (fp64) over every (attribute, channel), and ``<case>/spec`` = (n, L, na, seed) --
the inputs themselves are regenerated from the seed by ``ksg_oracle.make_case``.  The GPU tests compare the kernel with these
tables cell by cell; the CPU tests check that the oracle still reproduces the file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import ksg_oracle as O
    out = {}
    for spec, case in zip(O.CASES, O.all_cases()):
        out[f"{case.name}/spec"] = np.array([case.n, case.l, case.na, spec[5]], np.int64)
        for k in case.ks:
            t = O.case_tables(case.z, case.attrs, k)
            out[f"{case.name}/k{k}/eps"] = t["eps"]
            out[f"{case.name}/k{k}/nx"] = t["nx"].astype(np.int16)
            out[f"{case.name}/k{k}/ny"] = t["ny"].astype(np.int16)
            out[f"{case.name}/k{k}/mi"] = t["mi"]
            print(f"{case.name}: n {case.n} L {case.l} na {case.na} k {k}: rows with eps = 0: {int((t['eps'] == 0).sum())}, "
                  f"MI {t['mi'].min():.6f} .. {t['mi'].max():.6f}")
    os.makedirs(os.path.dirname(O.GOLDEN), exist_ok=True)
    np.savez_compressed(O.GOLDEN, **out)
    print("wrote", O.GOLDEN, os.path.getsize(O.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

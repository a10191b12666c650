#!/usr/bin/env python3
"""Records tests/golden/projection_quality_golden.npz (TEST INFRASTRUCTURE) with scikit-learn:

    python tools/make_projection_quality_golden.py

Per case of ``CASES``: the seeded fp32 inputs ``<case>/high`` [n, d] and ``<case>/low`` [n, 2] and the label sets
``<case>/labels_group`` / ``<case>/labels_patient`` (``projection_quality_oracle.golden_inputs``), and what scikit-learn makes
of the fp64 distance matrices of those rows (``projection_quality_oracle.pairwise``):
``<case>/trustworthiness`` and ``<case>/continuity`` [K] = ``manifold.trustworthiness(metric="precomputed")`` in the two
directions for the neighbour counts ``<case>/neighbors`` (those below n / 2), and ``<case>/silhouette_<space>_<labels>`` [n] =
``metrics.silhouette_samples(metric="precomputed")``.  A case with two equal off-diagonal distances in a row is refused:
scikit-learn breaks such ties by an unstable sort.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "projection_quality_golden.npz")
CASES = (("main", 11, 240, 32, 0.35), ("small", 12, 61, 7, 0.2))    # name, seed, n, d, noise of the projection
NEIGHBORS = (5, 15, 40)


def main() -> None:
    from sklearn.manifold import trustworthiness
    from sklearn.metrics import silhouette_samples

    import projection_quality_oracle as O
    out = {}
    for name, seed, n, d, noise in CASES:
        high, low, labels = O.golden_inputs(seed, n, d, noise)
        dh, dl = O.pairwise(high), O.pairwise(low)
        if O.has_row_ties(dh) or O.has_row_ties(dl):
            raise SystemExit(f"{name}: tied distances in a row; pick another seed")
        ks, _ = O.admitted(NEIGHBORS, n)
        out[f"{name}/spec"] = np.array([seed, n, d], np.int64)
        out[f"{name}/noise"] = np.float64(noise)
        out[f"{name}/high"], out[f"{name}/low"] = high, low
        out[f"{name}/neighbors"] = np.array(ks, np.int64)
        out[f"{name}/trustworthiness"] = np.array([trustworthiness(dh, low.astype(np.float64), n_neighbors=k, metric="precomputed")
                                                   for k in ks])
        out[f"{name}/continuity"] = np.array([trustworthiness(dl, high.astype(np.float64), n_neighbors=k, metric="precomputed")
                                              for k in ks])
        for label, values in labels.items():
            out[f"{name}/labels_{label}"] = np.array(values)
            _, codes = O.label_codes(values)
            for space, dist in (("latent", dh), ("projection", dl)):
                out[f"{name}/silhouette_{space}_{label}"] = silhouette_samples(dist, codes, metric="precomputed")
        print(f"{name}: n {n} d {d}: trustworthiness {out[f'{name}/trustworthiness']}, continuity {out[f'{name}/continuity']}")
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()

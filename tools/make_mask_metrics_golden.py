#!/usr/bin/env python3
"""Generates tests/golden/mask_metrics_golden.json (TEST INFRASTRUCTURE; run where a checkout of the reference exists):

    python tools/make_mask_metrics_golden.py --reference <checkout of Sukikui/PTI-LDM-VAE>

Loads the reference's ``vae_scripts/compute_mask_metrics.py`` BY FILE PATH -- it imports ``cv2`` and ``tqdm`` at the top,
which ``compute_bbox``, ``compute_edente_widths``, ``compute_dente_width`` and ``pixel_offsets_mm`` never use, so two empty
stand-in modules take those names when the real ones are missing; nothing of the file is copied -- and records what
these four functions return on the masks of ``tests/mask_metrics_oracle.CASES`` (binarised as the reference's loader
does, ``(mask > 0).astype(uint8)``).  The fixture holds the cases' parameters and the expected integers, no masks.
``reference_rows`` are the rows the reference samples for the case's (samples, bbox height), read off a ramp mask whose
row r is r + 1 pixels wide.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_reference(reference: str):
    for name in ("cv2", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            stub = types.ModuleType(name)
            stub.tqdm = stub.error = None
            sys.modules[name] = stub
    path = os.path.join(reference, "vae_scripts", "compute_mask_metrics.py")
    spec = importlib.util.spec_from_file_location("ref_compute_mask_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod   # dataclasses resolves the module of a class through sys.modules
    spec.loader.exec_module(mod)
    return mod


def record(ref, case: dict) -> dict:
    import mask_metrics_oracle as O
    ed = (O.make_mask(case["edente"]) > 0).astype(np.uint8)
    de = (O.make_mask(case["dente"]) > 0).astype(np.uint8)
    offsets = ref.pixel_offsets_mm(case["heights_mm"], case["pixel_size_mm"])
    try:
        x0, y0, w, h = ref.compute_bbox(ed)
    except ValueError as exc:
        return {"error": str(exc), "offsets": [int(o) for o in offsets]}
    height, widths = ref.compute_edente_widths(ed, x0, y0, w, h, case["samples"])
    _, ramp = ref.compute_edente_widths(O.ramp_mask(int(h)), 0, 0, int(h), int(h), case["samples"])
    rows = [max(0, min(de.shape[0] - 1, de.shape[0] - 1 - o)) for o in offsets]
    return {"bbox": [int(x0), int(y0), int(w), int(h)], "height": int(height), "edente_widths": [int(v) for v in widths],
            "reference_rows": [int(v) - 1 for v in ramp], "offsets": [int(o) for o in offsets],
            "dente_widths": [int(ref.compute_dente_width(de, r)) for r in rows]}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mask_metrics_golden.json"))
    args = ap.parse_args()
    import mask_metrics_oracle as O
    ref = load_reference(args.reference)
    cases = [dict(case, expected=record(ref, case)) for case in O.CASES]
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump({"source": "vae_scripts/compute_mask_metrics.py: compute_bbox, compute_edente_widths, "
                             "compute_dente_width, pixel_offsets_mm", "cases": cases}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}: {len(cases)} cases")


if __name__ == "__main__":
    main()

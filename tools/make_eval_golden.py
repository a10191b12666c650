#!/usr/bin/env python3
"""Generates tests/golden/eval_metrics_golden.npz (TEST INFRASTRUCTURE; run where a checkout of the reference exists):

    python tools/make_eval_golden.py --reference <checkout of Sukikui/PTI-LDM-VAE>

Imports the reference's ``src/pti_ldm_vae/utils/eval_metrics.py`` BY FILE PATH (its only import is torch; nothing of it
is copied), runs its ``compute_psnr`` / ``compute_ssim`` on seeded single-channel inputs -- on the images as they are and
clamped to [0, 1] as ``evaluate_vae.py`` does -- and stores the inputs, the outputs and the 11 fp32 window taps.
``tests/test_eval_metrics_cpu.py`` pins the tests' torch restatement (``tests/eval_metrics_oracle.py``) and
``ops.ssim_taps`` to these vectors.  About 90 KB.

The taps are local to ``compute_ssim``, so they are rebuilt here with the same fp32 torch operations and cross-checked
through the function itself: for an 11x11 map holding one unit impulse against an all-zero target, every output pixel
sees the impulse through exactly one tap of the 2-D window, so the SSIM the reference returns is a closed-form function
of the 121 window values.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (samples, height, width, noise): small on purpose; values outside [0, 1] are present in every case
CASES = [(2, 64, 64, 0.05), (1, 100, 76, 0.2), (2, 9, 13, 0.1), (1, 64, 64, 0.0)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference repository")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_eval_metrics",
                                                  os.path.join(args.reference, "src/pti_ldm_vae/utils/eval_metrics.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from eval_metrics_oracle import make_pair

    out = {}
    for i, (n, h, w, noise) in enumerate(CASES):
        pred, target = make_pair((n, 1, h, w), noise, seed=77 + i)
        out[f"pred{i}"], out[f"target{i}"] = pred.numpy(), target.numpy()
        out[f"psnr{i}"] = ref.compute_psnr(pred, target).numpy()
        out[f"ssim{i}"] = ref.compute_ssim(pred, target).numpy()
        pc, tc = pred.clamp(0, 1), target.clamp(0, 1)
        out[f"psnr_clamped{i}"] = ref.compute_psnr(pc, tc).numpy()
        out[f"ssim_clamped{i}"] = ref.compute_ssim(pc, tc).numpy()

    coords = torch.arange(11) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 * 1.5))
    g = g / g.sum()
    assert g.dtype == torch.float32
    impulse = torch.zeros(1, 1, 11, 11)
    impulse[0, 0, 5, 5] = 1.0
    k2d = (g[:, None] @ g[None, :]).double()                 # mu_x = E[x^2] = the window value that pixel sees
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    closed_form = ((c1 * c2) / ((k2d * k2d + c1) * ((k2d - k2d * k2d) + c2))).mean()
    got = float(ref.compute_ssim(impulse, torch.zeros_like(impulse)))
    assert abs(got - float(closed_form)) <= 1e-6, (got, float(closed_form))
    out["taps"] = g.numpy()

    path = os.path.join(ROOT, "tests", "golden", "eval_metrics_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates the latent-analysis fixtures (TEST INFRASTRUCTURE; run where a checkout of the reference exists, with scipy,
scikit-learn and plotly installed):

    python tools/make_latent_golden.py --reference <checkout of Sukikui/PTI-LDM-VAE>

Imports the reference's ``src/pti_ldm_vae/analysis/{latent_space,latent_distance,latent_cache}.py`` BY FILE PATH (the
package ``__init__`` pulls in cv2; nothing of the files is copied) and records what its functions return, in fp64, on
the seeded inputs of ``tests/latent_analysis_oracle.py``:

  tests/golden/latent_analysis_golden.npz          inputs at D = 512 (the D = 40 960 case is regenerated from its seed),
      the four metrics per patient, the full cdist matrix, latent_distance* values, cache keys of fixed non-existent
      paths (mtime 0), patient-id cases, exact PCA projections (``PCA(svd_solver="full")``: the default solver resolves
      to "randomized" here and is not reproducible) -- and beside each expected array the error of the plain fp32 CPU
      restatement, asserted <= 1e-6 (distances, statistics) / <= 1e-4 per component (PCA);
  tests/golden/latent_distance_metrics_golden.txt  ``distance_metrics.txt`` as the reference's own
      ``compute_group_statistics`` writes it (through a dummy model that only has ``.eval()``).
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED_SMALL, D_SMALL = 20251, 512
SEED_LARGE, D_LARGE = 20252, 40960
WEIGHTS = "/nonexistent/weights/autoencoder_epoch73.pth"
IMAGES = ["/nonexistent/data/edente/1000_HA_2021_02_545.tif", "/nonexistent/data/dente/17_HA_2019_11_12.tiff"]
FILENAMES = ["1000_HA_2021_02_545.tif", "a_b.c_d.tiff", "plain", "noext_7", "x.tif", "_.tif", "9_.png", "a.b_c"]


def by_path(reference: str, name: str):
    spec = importlib.util.spec_from_file_location(f"ref_{name}", os.path.join(reference, "src/pti_ldm_vae/analysis", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class DummyModel:
    def eval(self):
        return self


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference repository")
    args = ap.parse_args()
    import latent_analysis_oracle as O
    from scipy.spatial.distance import cdist
    from sklearn.decomposition import PCA
    space, dist, cache = (by_path(args.reference, n) for n in ("latent_space", "latent_distance", "latent_cache"))

    out = {"seed_small": SEED_SMALL, "d_small": D_SMALL, "seed_large": SEED_LARGE, "d_large": D_LARGE,
           "patients": np.array(O.PATIENTS)}
    for tag, seed, d in (("small", SEED_SMALL, D_SMALL), ("large", SEED_LARGE, D_LARGE)):
        a, ids_a, b, ids_b = O.make_latents(seed, d)
        if tag == "small":
            out.update(a=a, b=b, ids_a=np.array(ids_a), ids_b=np.array(ids_b))
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        want = np.full((len(O.PATIENTS), 4), np.nan)
        got32 = np.full((len(O.PATIENTS), 4), np.nan)
        for p, patient in enumerate(O.PATIENTS):
            ra = a64[[i for i, q in enumerate(ids_a) if q == patient]]
            rb = b64[[i for i, q in enumerate(ids_b) if q == patient]]
            m = space.compute_distance_metrics(ra, rb)
            if m is not None:
                want[p] = [float(v) for v in m]
            got32[p] = O.fp32_metrics(ra.astype(np.float32), rb.astype(np.float32))
        full = cdist(a64, b64)
        out[f"metrics_{tag}"], out[f"cdist_{tag}"] = want, full
        out[f"metrics_{tag}_fp32_err"] = O.rel_err(got32, want)
        out[f"cdist_{tag}_fp32_err"] = O.rel_err(O.fp32_cdist(a, b), full)
        print(tag, "fp32 restatement error: metrics", out[f"metrics_{tag}_fp32_err"], "cdist", out[f"cdist_{tag}_fp32_err"])
        assert out[f"metrics_{tag}_fp32_err"] <= 1e-6 and out[f"cdist_{tag}_fp32_err"] <= 1e-6
        x64 = np.concatenate([a64, b64])
        pca = PCA(n_components=O.PCA_COMPONENTS, svd_solver="full")
        proj = pca.fit_transform(x64)
        assert pca.singular_values_[-1] >= 1e-2 * pca.singular_values_[0]
        p32, r32 = O.fp32_pca(np.concatenate([a, b]), O.PCA_COMPONENTS)
        out[f"pca_{tag}"], out[f"pca_ratio_{tag}"] = proj, pca.explained_variance_ratio_
        out[f"pca_{tag}_fp32_err"] = O.component_err(p32, O.sign_rule(proj))
        print(tag, "fp32 restatement error: pca", out[f"pca_{tag}_fp32_err"], "ratio", np.abs(r32 - pca.explained_variance_ratio_).max())
        assert out[f"pca_{tag}_fp32_err"] <= 1e-4

    # single-vector distances and their error cases' inputs are in the tests; values here
    a, b = out["a"], out["b"]
    out["latent_distance"] = np.array([dist.latent_distance(a[0], b[0]), dist.latent_distance(a[3], a[3]),
                                       dist.latent_distance_from_indices(a, 0, 47), dist.latent_distance_from_indices(a, 5, 6),
                                       dist.latent_distance_cross(a, 47, b, 39), dist.latent_distance_cross(a, 1, b, 0)])

    with tempfile.TemporaryDirectory() as tmp:
        c = cache.LatentCache(cache_root=Path(tmp) / "c")
        out["model_signature"] = np.array(c._get_model_signature(WEIGHTS, (256, 256)))
        out["model_signature_64"] = np.array(c._get_model_signature(WEIGHTS, (64, 64)))
        out["image_keys"] = np.array([c._get_image_cache_key(p) for p in IMAGES])
        out["weights_path"], out["image_paths"] = np.array(WEIGHTS), np.array(IMAGES)
        out["filenames"] = np.array(FILENAMES)
        out["filename_ids"] = np.array([space.extract_patient_id_from_filename(f) for f in FILENAMES])

        ids_a, ids_b = list(out["ids_a"]), list(out["ids_b"])
        proj = out["pca_small"][:, :2]
        analyzer = space.LatentSpaceAnalyzer(DummyModel(), "cpu", None)
        analyzer.compute_group_statistics([(proj[:len(a)], ids_a, "edente"), (proj[len(a):], ids_b, "dente")],
                                          [(a, ids_a, "edente"), (b, ids_b, "dente")], Path(tmp))
        text = (Path(tmp) / "distance_metrics.txt").read_text()
        out["sorted_text"] = np.array((Path(tmp) / "exams_sorted_by_distance.txt").read_text())

    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "latent_distance_metrics_golden.txt"), "w") as f:
        f.write(text)
    path = os.path.join(golden, "latent_analysis_golden.npz")
    np.savez_compressed(path, **out)
    total = os.path.getsize(path) + len(text.encode())
    print(f"wrote {path} and latent_distance_metrics_golden.txt: {total} bytes")
    assert total <= 512 * 1024


if __name__ == "__main__":
    main()

"""CPU tests of the latent-space analysis: everything of ``pti_ldm_vae_amd.analysis`` and ``analyze_static`` that runs on
the host, pinned to what the reference's own functions returned (``tests/golden/latent_analysis_golden.npz`` and
``latent_distance_metrics_golden.txt``, written by ``tools/make_latent_golden.py``), and the validation paths of the two
C entry points that return before any launch."""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import latent_analysis_oracle as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "latent_analysis_golden.npz"))


def test_fixture_inputs_are_the_seeded_ones(gold):
    a, ids_a, b, ids_b = O.make_latents(int(gold["seed_small"]), int(gold["d_small"]))
    assert np.array_equal(a, gold["a"]) and np.array_equal(b, gold["b"])
    assert ids_a == list(gold["ids_a"]) and ids_b == list(gold["ids_b"]) and list(gold["patients"]) == O.PATIENTS
    assert a.shape == (48, 512) and b.shape == (40, 512) and a.dtype == np.float32
    counts = [(ids_a.count(p), ids_b.count(p)) for p in O.PATIENTS]
    assert max(c[0] for c in counts) == 12 and (1, 6) in counts and any(c[0] == 0 for c in counts) and any(c[1] == 0 for c in counts)
    for tag in ("small", "large"):
        assert float(gold[f"metrics_{tag}_fp32_err"]) <= 1e-6 and float(gold[f"cdist_{tag}_fp32_err"]) <= 1e-6
        assert float(gold[f"pca_{tag}_fp32_err"]) <= 1e-4


def test_patient_id_parsing_equals_the_reference(gold):
    from pti_ldm_vae_amd.analysis import extract_patient_id_from_filename
    assert extract_patient_id_from_filename("1000_HA_2021_02_545.tif") == "545"
    for name, want in zip(gold["filenames"], gold["filename_ids"]):
        assert extract_patient_id_from_filename(str(name)) == str(want), name


def test_load_image_paths(tmp_path):
    from pti_ldm_vae_amd.analysis import load_image_paths
    for name in ("b.tif", "a.tiff", "c.tif", "d.png", "notes.txt", "e.TIF"):
        (tmp_path / name).write_bytes(b"")
    names = lambda paths: [os.path.basename(p) for p in paths]
    assert names(load_image_paths(str(tmp_path))) == ["a.tiff", "b.tif", "c.tif"]
    assert names(load_image_paths(str(tmp_path), max_images=2)) == ["a.tiff", "b.tif"]
    assert names(load_image_paths(str(tmp_path), extensions=["png", ".tif"])) == ["b.tif", "c.tif", "d.png"]
    assert load_image_paths(str(tmp_path), extensions=[".jpg"]) == [] and load_image_paths(str(tmp_path), max_images=0) == []


def test_latent_distance_values_and_errors(gold):
    from pti_ldm_vae_amd.analysis import latent_distance, latent_distance_cross, latent_distance_from_indices
    a, b = gold["a"], gold["b"]
    got = [latent_distance(a[0], b[0]), latent_distance(a[3], a[3]), latent_distance_from_indices(a, 0, 47),
           latent_distance_from_indices(a, 5, 6), latent_distance_cross(a, 47, b, 39), latent_distance_cross(a, 1, b, 0)]
    assert all(isinstance(g, float) for g in got) and got[1] == 0.0
    assert np.allclose(got, gold["latent_distance"], rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="Expected 1D latent vectors"):
        latent_distance(a, b[0])
    with pytest.raises(ValueError, match="must have the same shape"):
        latent_distance(a[0], b[0][:10])
    with pytest.raises(ValueError, match=r"Expected latents of shape \[N, D\]"):
        latent_distance_from_indices(a[0], 0, 1)
    for i, j in ((-1, 0), (0, 48), (48, 48)):
        with pytest.raises(ValueError, match=r"indices must be in \[0, 47\]"):
            latent_distance_from_indices(a, i, j)
    with pytest.raises(ValueError, match="Expected 2D latents for both groups"):
        latent_distance_cross(a[0], 0, b, 0)
    with pytest.raises(ValueError, match="Latent dimensions must match"):
        latent_distance_cross(a, 0, b[:, :100], 0)
    with pytest.raises(ValueError, match=r"idx_a must be in \[0, 47\], got 48"):
        latent_distance_cross(a, 48, b, 0)
    with pytest.raises(ValueError, match=r"idx_b must be in \[0, 39\], got -1"):
        latent_distance_cross(a, 0, b, -1)


class _FakeEncoder:
    def __init__(self):
        self.single, self.many = [], []

    def vector(self, path):
        seed = int.from_bytes(os.path.basename(path).encode()[:4], "little")
        return np.random.default_rng(seed).standard_normal(12).astype(np.float32)

    def one(self, path):
        self.single.append(path)
        return self.vector(path), os.path.basename(path).rsplit(".", 1)[0].split("_")[-1]

    def batch(self, paths):
        self.many.append(list(paths))
        return np.stack([self.vector(p) for p in paths]), [os.path.basename(p).rsplit(".", 1)[0].split("_")[-1] for p in paths]


def test_latent_cache_names_equal_the_reference(gold, tmp_path):
    from pti_ldm_vae_amd.analysis import LatentCache
    cache = LatentCache(tmp_path / "root")
    weights = str(gold["weights_path"])
    assert cache._get_model_signature(weights, (256, 256)) == str(gold["model_signature"])
    assert cache._get_model_signature(weights, (64, 64)) == str(gold["model_signature_64"])
    assert [cache._get_image_cache_key(str(p)) for p in gold["image_paths"]] == [str(k) for k in gold["image_keys"]]
    sig = str(gold["model_signature"])
    assert cache._get_cache_file_path(str(gold["image_paths"][0]), sig) == tmp_path / "root" / sig / f"{gold['image_keys'][0]}.npz"
    assert cache._get_metadata_path(sig) == tmp_path / "root" / sig / "_metadata.json"


def test_latent_cache_hits_misses_and_invalidation(tmp_path):
    from pti_ldm_vae_amd.analysis import LatentCache
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    paths = [str(imgs / f"{i}_HA_2020_01_{7 + i % 2}.tif") for i in range(5)]
    for p in paths:
        Path(p).write_bytes(b"x")
    weights = str(tmp_path / "w.pth")
    cache, enc = LatentCache(tmp_path / "cache"), _FakeEncoder()
    lat, ids, out_paths = cache.get_or_encode_batch(paths, enc.one, weights, (64, 64), "edente")
    assert enc.single == paths and lat.shape == (5, 12) and ids == ["7", "8", "7", "8", "7"] and out_paths == paths
    sig = cache._get_model_signature(weights, (64, 64))
    folder = tmp_path / "cache" / sig
    assert sorted(f.name for f in folder.iterdir()) == sorted([f"{cache._get_image_cache_key(p)}.npz" for p in paths] + ["_metadata.json"])
    meta = json.load(open(folder / "_metadata.json"))
    assert meta["model"] == "w.pth" and meta["patch_size"] == [64, 64] and set(meta["images"]) == {str(Path(p).resolve()) for p in paths}
    assert meta["images"][str(Path(paths[1]).resolve())] == {"cache_key": cache._get_image_cache_key(paths[1]), "patient_id": "8"}
    stored = np.load(folder / f"{cache._get_image_cache_key(paths[2])}.npz")
    assert set(stored.files) == {"latent", "patient_id"} and np.array_equal(stored["latent"], enc.vector(paths[2]))
    assert str(stored["patient_id"]) == "7"

    # second call: nothing is encoded, same values
    enc2 = _FakeEncoder()
    lat2, ids2, _ = cache.get_or_encode_batch(paths, enc2.one, weights, (64, 64), "edente", encode_many=enc2.batch)
    assert enc2.single == [] and enc2.many == [] and np.array_equal(lat2, lat) and ids2 == ids

    # a touched file (new mtime) and a corrupted cache file are encoded again -- through encode_many, misses only, and
    # the results come back in input order
    st = os.stat(paths[3])
    os.utime(paths[3], (st.st_atime, st.st_mtime + 10))
    (folder / f"{cache._get_image_cache_key(paths[0])}.npz").write_bytes(b"not a zip file")
    new = str(imgs / "9_HA_2020_01_55.tif")
    Path(new).write_bytes(b"x")
    order = [paths[4], new, paths[3], paths[0], paths[1]]
    enc3 = _FakeEncoder()
    lat3, ids3, p3 = cache.get_or_encode_batch(order, enc3.one, weights, (64, 64), "edente", encode_many=enc3.batch)
    assert enc3.single == [] and enc3.many == [[new, paths[3], paths[0]]]
    assert p3 == order and ids3 == ["7", "55", "8", "7", "8"]
    assert np.array_equal(lat3, np.stack([enc.vector(p) for p in order]))
    enc4 = _FakeEncoder()
    cache.get_or_encode_batch(order, enc4.one, weights, (64, 64), "edente")
    assert enc4.single == []                                                  # the repaired entries are hits now
    with pytest.raises(ValueError, match="encode_many returned"):
        Path(paths[2]).write_bytes(b"changed")
        os.utime(paths[2], (st.st_atime, st.st_mtime + 20))
        cache.get_or_encode_batch([paths[2]], enc4.one, weights, (64, 64), "edente", encode_many=lambda ps: (np.zeros((0, 12)), []))

    # another patch size is another model directory; stats and clearing
    cache.get_or_encode_batch(paths[:2], enc.one, weights, (32, 32), "edente")
    stats = cache.get_cache_stats()
    sig32 = cache._get_model_signature(weights, (32, 32))
    assert set(stats) == {sig, sig32} and stats[sig32]["num_images"] == 2 and stats[sig32]["patch_size"] == [32, 32]
    assert stats[sig]["model"] == "w.pth" and stats[sig]["num_images"] == 6 and stats[sig]["cache_size_mb"] > 0
    cache.clear_cache(sig32)
    assert set(cache.get_cache_stats()) == {sig}
    cache.clear_cache()
    assert cache.get_cache_stats() == {} and (tmp_path / "cache").is_dir()


def test_host_distance_metrics_equal_the_reference(gold):
    from pti_ldm_vae_amd.analysis import compute_distance_metrics
    from pti_ldm_vae_amd.analysis.latent_space import segmented_distance_metrics_host
    a, b, ids_a, ids_b = gold["a"], gold["b"], list(gold["ids_a"]), list(gold["ids_b"])
    assert compute_distance_metrics([], b) is None and compute_distance_metrics(a, np.zeros((0, 512))) is None
    for p, patient in enumerate(O.PATIENTS):
        ra, rb = a[[i for i, q in enumerate(ids_a) if q == patient]], b[[i for i, q in enumerate(ids_b) if q == patient]]
        got = compute_distance_metrics(list(ra), list(rb))                  # lists of rows, as the reference is called
        if got is None:
            assert np.isnan(gold["metrics_small"][p]).all()
        else:
            assert O.rel_err(np.array(got), gold["metrics_small"][p]) <= 1e-12
    (oa, sa), (ob, sb) = O.segments(ids_a), O.segments(ids_b)
    assert O.rel_err(segmented_distance_metrics_host(a[oa], sa, b[ob], sb), gold["metrics_small"]) <= 1e-12
    cpu = compute_distance_metrics(torch.from_numpy(a[:5]), torch.from_numpy(b[:4]))   # host tensors: the numpy path
    assert O.rel_err(np.array(cpu), np.array(compute_distance_metrics(a[:5], b[:4]))) == 0.0


def test_statistics_files_equal_the_reference_text(gold, tmp_path, monkeypatch):
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    from pti_ldm_vae_amd.analysis.latent_space import group_rows_by_patient, segmented_distance_metrics_host
    monkeypatch.setattr(LatentSpaceAnalyzer, "_segmented_metrics",
                        lambda self, p1, s1, p2, s2: segmented_distance_metrics_host(p1, s1, p2, s2))
    a, b, ids_a, ids_b = gold["a"], gold["b"], list(gold["ids_a"]), list(gold["ids_b"])
    proj = gold["pca_small"][:, :2]
    analyzer = LatentSpaceAnalyzer(torch.nn.Identity(), torch.device("cpu"), None)
    analyzer.compute_group_statistics([(proj[:48], ids_a, "edente"), (proj[48:], ids_b, "dente")],
                                      [(a, ids_a, "edente"), (b, ids_b, "dente")], tmp_path)
    want = open(os.path.join(GOLDEN_DIR, "latent_distance_metrics_golden.txt"), "rb").read()
    assert (tmp_path / "distance_metrics.txt").read_bytes() == want
    assert (tmp_path / "exams_sorted_by_distance.txt").read_bytes() == str(gold["sorted_text"]).encode()
    assert want.count(b"[Latent]") == 7                                      # two patients have rows in one group only
    # one group only: nothing is written
    analyzer.compute_group_statistics([(proj[:48], ids_a, "edente")], [(a, ids_a, "edente")], tmp_path / "none")
    assert not (tmp_path / "none").exists()
    patients, o1, s1, o2, s2 = group_rows_by_patient(["b", "a", "b"], ["c", "a"])
    assert (patients, o1, s1, o2, s2) == (["a", "b", "c"], [1, 0, 2], [0, 1, 3, 3], [1, 0], [0, 1, 1, 2])


def test_reduction_validation_errors_and_colormap(tmp_path):
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    from pti_ldm_vae_amd.analysis.latent_space import PATIENT_PALETTE
    an = LatentSpaceAnalyzer(torch.nn.Identity(), torch.device("cpu"), None)
    x = np.zeros((20, 8), dtype=np.float32)
    for fn in (an.reduce_dimensionality_tsne, an.reduce_dimensionality_umap, an.reduce_dimensionality_pca):
        with pytest.raises(ValueError, match="Expected 2D array, got 1D array"):
            fn(x[0])
    for fn in (an.reduce_dimensionality_tsne, an.reduce_dimensionality_umap):
        with pytest.raises(ValueError, match="Need at least 50 samples for PCA with 50 components, got 20 samples"):
            fn(x)
    with pytest.raises(ValueError, match=r"perplexity \(30\) must be < n_samples \(20\)"):
        an.reduce_dimensionality_tsne(x, pca_components=5)
    with pytest.raises(ValueError, match=r"n_neighbors \(40\) must be < n_samples \(20\)"):
        an.reduce_dimensionality_umap(x, pca_components=5)
    with pytest.raises(ValueError, match="n_components=9"):
        an.reduce_dimensionality_pca(x, 9)
    with pytest.raises(ValueError, match="image_paths cannot be empty"):
        an.encode_images([])
    to_id, to_color = an.create_patient_colormap(["9", "10", "9", "2"])
    assert to_id == {"10": 0, "2": 1, "9": 2} and to_color == {"10": "#636EFA", "2": "#EF553B", "9": "#00CC96"}
    many = an.create_patient_colormap([str(i) for i in range(40)])[1]
    assert len(PATIENT_PALETTE) == 34 and many["0"] == many[sorted(map(str, range(40)))[34]]
    try:
        import plotly.express as px
        assert list(PATIENT_PALETTE) == px.colors.qualitative.Plotly + px.colors.qualitative.Dark24
    except ImportError:
        pass
    an.save_color_legend(to_id, to_color, tmp_path / "legend.txt")
    assert (tmp_path / "legend.txt").read_text().splitlines()[3:] == ["0: 10 — #636EFA", "1: 2 — #EF553B", "2: 9 — #00CC96"]


def test_c_entry_points_validate_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    ws = h.pti_latent_pairwise_ws_floats
    assert ws(1000, 1000, 4096) == 1 and ws(2000, 2000, 40960) == 1           # many tiles: one pass, no scratch
    assert ws(32, 32, 40960) == 80 * 32 * 32 and ws(48, 40, 4096) == 8 * 48 * 40   # few tiles: D split in 512-column slabs
    assert ws(256, 256, 513) == 2 * 256 * 256 and ws(257, 256, 513) == 1      # 16 tiles is the last split shape
    assert ws(64, 64, 512) == 1 and ws(1, 1, 1) == 1                          # a single slab is never split
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 22, 4, 4), (4, 4, (1 << 24) + 1)):
        assert ws(*bad) == 0, bad
    gws = h.pti_latent_group_stats_ws_floats
    assert gws(48, 40, 9, 512) == 2 * 9 * (2 * 3 + 1) and gws(1000, 1000, 200, 40960) == 2 * 200 * (160 * 3 + 256)
    assert gws(5, 5, 1, 2) == 2 * (3 + 1)
    for bad in ((0, 4, 1, 4), (4, 0, 1, 4), (4, 4, 0, 4), (4, 4, 1, 0), (4, 4, 70000, 4), (1 << 21, 1 << 21, 2, 4)):
        assert gws(*bad) == 0, bad
    p, q = C.c_void_p(256), C.c_void_p(512)                                   # never dereferenced: refused first
    pair = h.pti_latent_pairwise
    for bad in (0, 3, 9, 11):
        args = [p, 8, 4, p, 8, 4, 8, None, 0, q, 4, q, None]
        args[bad] = None
        assert pair(*args) == -1 and b"null" in h.pti_last_error_string()
    for n1, n2, d in ((0, 4, 8), (4, -1, 8), (4, 4, 0)):
        assert pair(p, 8, n1, p, 8, n2, d, None, 0, q, 4, q, None) == -1 and b"dimension" in h.pti_last_error_string()
    for lda, ldb, ldo in ((7, 8, 4), (8, 7, 4), (8, 8, 3)):
        assert pair(p, lda, 4, p, ldb, 4, 8, None, 0, q, ldo, q, None) == -1 and b"stride" in h.pti_last_error_string()
    for mode in (2, -1):
        assert pair(p, 8, 4, p, 8, 4, 8, None, mode, q, 4, q, None) == -2 and b"mode" in h.pti_last_error_string()
    assert pair(p, 8, 1 << 22, p, 8, 4, 8, None, 0, q, 4, q, None) == -2 and b"shape" in h.pti_last_error_string()
    group = h.pti_latent_group_stats
    for bad in (0, 3, 4, 7, 10, 11):
        args = [p, 8, 4, q, p, 8, 4, q, 2, 8, q, q, None]
        args[bad] = None
        assert group(*args) == -1 and b"null" in h.pti_last_error_string()
    for n1, n2, e, d in ((0, 4, 2, 8), (4, 0, 2, 8), (4, 4, 0, 8), (4, 4, 2, -8)):
        assert group(p, 8, n1, q, p, 8, n2, q, e, d, q, q, None) == -1 and b"dimension" in h.pti_last_error_string()
    assert group(p, 7, 4, q, p, 8, 4, q, 2, 8, q, q, None) == -1 and b"stride" in h.pti_last_error_string()
    assert group(p, 8, 4, q, p, 8, 4, q, 2, 8, q, C.c_void_p(516), None) == -1 and b"aligned" in h.pti_last_error_string()
    rc = group(p, 8, 4, q, p, 8, 4, q, 70000, 8, q, q, None)
    assert rc == -2 and b"shape" in h.pti_last_error_string()
    with pytest.raises(_lib.PtiError):
        _lib.check(rc, "latent_group_stats")


def test_ops_refuse_cpu_tensors():
    from pti_ldm_vae_amd import ops
    x, seg = torch.rand(4, 8), torch.tensor([0, 2, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        ops.latent_pairwise(x)
    with pytest.raises(ValueError, match="CUDA"):
        ops.latent_pairwise(x, x, mode="dot")
    with pytest.raises(ValueError, match="mode"):
        ops.latent_pairwise(x, mode="cosine")
    with pytest.raises(ValueError, match="CUDA"):
        ops.latent_group_stats(x, seg, x, seg)
    with pytest.raises(ValueError, match="CUDA"):
        ops.latent_pairwise(x.numpy())


def test_analyze_static_defaults():
    from pti_ldm_vae_amd import analyze_static
    a = analyze_static.parse_args(["--vae-weights", "w.pth", "--config-file", "c.json", "--folder-edente", "e"])
    assert vars(a) == dict(vae_weights="w.pth", config_file="c.json", folder_edente="e", folder_dente=None,
                           output_dir="projections", max_images=1000, patch_size=[256, 256], color_by_patient=False,
                           method="umap", n_neighbors=40, min_dist=0.5, perplexity=30, seed=42, subtitle=None, dpi=300,
                           cache_dir="cache/latents", batch_size=8)
    a = analyze_static.parse_args(["--vae-weights", "w", "--config-file", "c", "--folder-edente", "e", "--folder-dente", "d",
                                   "--method", "pca", "--patch-size", "64", "32", "--color-by-patient", "--batch-size", "3"])
    assert (a.method, a.patch_size, a.color_by_patient, a.folder_dente, a.batch_size) == ("pca", [64, 32], True, "d", 3)
    for missing in (["--config-file", "c", "--folder-edente", "e"], ["--vae-weights", "w", "--folder-edente", "e"],
                    ["--vae-weights", "w", "--config-file", "c"], ["--vae-weights", "w", "--config-file", "c", "--folder-edente", "e",
                                                                  "--method", "isomap"]):
        with pytest.raises(SystemExit):
            analyze_static.parse_args(missing)

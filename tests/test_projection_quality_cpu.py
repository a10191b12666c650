"""CPU tests of the projection-quality report: the numpy oracle (tests/projection_quality_oracle.py) against scikit-learn's
recorded values (tests/golden/projection_quality_golden.npz) and against scikit-learn itself where it is installed, the
oracle's identities, and the command line of ``analyze_static --quality``.

Gate of the scikit-learn comparison: 1e-12 absolute.  Both sides are given the SAME fp64 distance matrix and only tie-free
cases are compared, so the integers under trustworthiness and continuity are equal and only the order in which a few hundred
fp64 terms are added differs (a silhouette term: sums of <= 240 distances, relative error <= 240 x 2^-53 = 2.7e-14)."""
import os

import numpy as np
import pytest

import projection_quality_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "projection_quality_golden.npz")
CASES = ("main", "small")
ARGV = ["--vae-weights", "w.pth", "--config-file", "c.json", "--folder-edente", "e"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def reports(gold):
    """case -> (dist_high, dist_low, labels, report, points) of the oracle on the fp64 distances of the stored rows."""
    out = {}
    for case in CASES:
        high, low = gold[f"{case}/high"], gold[f"{case}/low"]
        labels = {name: list(gold[f"{case}/labels_{name}"]) for name in ("group", "patient")}
        dh, dl = O.pairwise(high), O.pairwise(low)
        out[case] = (dh, dl, labels) + O.report_from_distances(dh, dl, high.shape[1], (5, 15, 40), labels)
    return out


@pytest.mark.parametrize("case", CASES)
def test_golden_inputs_are_the_seeded_ones_and_tie_free(gold, reports, case):
    seed, n, d = (int(v) for v in gold[f"{case}/spec"])
    high, low, labels = O.golden_inputs(seed, n, d, float(gold[f"{case}/noise"]))
    assert np.array_equal(high, gold[f"{case}/high"]) and np.array_equal(low, gold[f"{case}/low"])
    assert labels["patient"] == list(gold[f"{case}/labels_patient"]) and labels["group"] == list(gold[f"{case}/labels_group"])
    assert not O.has_row_ties(reports[case][0]) and not O.has_row_ties(reports[case][1])
    assert O.has_row_ties(np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 2.0], [1.0, 2.0, 0.0]]))


@pytest.mark.parametrize("case", CASES)
def test_oracle_equals_the_recorded_sklearn_values(gold, reports, case):
    dh, dl, labels, report, points = reports[case]
    assert not O.has_row_ties(dh) and not O.has_row_ties(dl)         # sklearn's unstable argsort: tie-free cases only
    ks = [int(k) for k in gold[f"{case}/neighbors"]]
    assert report["neighbors"] == ks and ks == ([5, 15, 40] if case == "main" else [5, 15])
    for c, k in enumerate(ks):
        for key in ("trustworthiness", "continuity"):
            dev = abs(report[key][k] - float(gold[f"{case}/{key}"][c]))
            print(f"{case} {key}[{k}]: oracle {report[key][k]!r}, sklearn {float(gold[f'{case}/{key}'][c])!r}, |dev| {dev:.1e}")
            assert dev <= 1e-12
    for name in ("group", "patient"):
        for space in ("latent", "projection"):
            want = gold[f"{case}/silhouette_{space}_{name}"]
            got = points[f"silhouette_{space}_{name}"]
            assert np.abs(got - want).max() <= 1e-12
            assert abs(report["labels"][name][f"silhouette_{space}"] - want.mean()) <= 1e-12
    single = np.bincount(O.label_codes(labels["patient"])[1])[O.label_codes(labels["patient"])[1]] == 1
    assert single.sum() >= 3 and (points["silhouette_latent_patient"][single] == 0.0).all()  # labels with one row are covered


@pytest.mark.parametrize("case", CASES)
def test_oracle_equals_sklearn_itself(gold, reports, case):
    manifold = pytest.importorskip("sklearn.manifold")
    metrics = pytest.importorskip("sklearn.metrics")
    dh, dl, labels, report, points = reports[case]
    assert not O.has_row_ties(dh) and not O.has_row_ties(dl)
    high, low = gold[f"{case}/high"].astype(np.float64), gold[f"{case}/low"].astype(np.float64)
    for k in report["neighbors"]:
        assert abs(report["trustworthiness"][k] - manifold.trustworthiness(dh, low, n_neighbors=k, metric="precomputed")) <= 1e-12
        assert abs(report["continuity"][k] - manifold.trustworthiness(dl, high, n_neighbors=k, metric="precomputed")) <= 1e-12
    for name, values in labels.items():
        codes = O.label_codes(values)[1]
        for space, dist in (("latent", dh), ("projection", dl)):
            want = metrics.silhouette_samples(dist, codes, metric="precomputed")
            assert np.abs(points[f"silhouette_{space}_{name}"] - want).max() <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_local_values_average_to_the_global_ones(reports, case):
    _, _, _, report, points = reports[case]
    for c, k in enumerate(report["neighbors"]):
        assert abs(points["trustworthiness_local"][:, c].mean() - report["trustworthiness"][k]) <= 1e-13
        assert abs(points["continuity_local"][:, c].mean() - report["continuity"][k]) <= 1e-13
        assert 0.0 < report["neighborhood_preservation"][k] <= 1.0
        for name in ("group", "patient"):
            for space in ("latent", "projection"):
                assert 0.0 <= report["labels"][name][f"knn_agreement_{space}"][k] <= 1.0


def test_identity_projection_is_perfect_and_excluded_bookkeeping():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((31, 2)).astype(np.float32)
    report, points = O.report(x, x, neighbors=(3, 15, 16, 40, 0, 3), labels={"one": ["a"] * 31})
    assert report["neighbors"] == [3, 15] and sorted(report["excluded"]) == [0, 16, 40]      # 15 < 15.5 <= 16
    assert "n / 2" in report["excluded"][16] and "at least 1" in report["excluded"][0]
    for k in (3, 15):
        assert report["trustworthiness"][k] == 1.0 and report["continuity"][k] == 1.0
        assert report["neighborhood_preservation"][k] == 1.0
        assert report["labels"]["one"]["knn_agreement_latent"][k] == 1.0
    assert (points["trustworthiness_local"] == 1.0).all() and points["trustworthiness_local"].shape == (31, 2)
    assert report["labels"]["one"]["silhouette_latent"] is None and report["labels"]["one"]["classes"] == ["a"]
    nothing, pts = O.report(x[:5], x[:5], neighbors=(5, 40))
    assert nothing["neighbors"] == [] and nothing["trustworthiness"] == {} and sorted(nothing["excluded"]) == [5, 40]
    assert pts["trustworthiness_local"].shape == (5, 0)


def test_oracle_ops_follow_the_key_rule():
    """Ties go to the lower column, -0 is 0, +inf sorts last, the row's own index ranks 0, a foreign index -1."""
    d = np.array([[0.0, 2.0, 2.0, -0.0, np.inf],
                  [1.0, 0.0, 1.0, 1.0, 1.0],
                  [3.0, 1.0, 0.0, 2.0, 0.0],
                  [5.0, 5.0, 5.0, 0.0, 5.0],
                  [np.inf, np.inf, 1.0, 2.0, 0.0]], dtype=np.float32)
    nbr = np.array([[1, 2, 3, 4, 0, 7], [0, 2, 3, 4, 1, -1], [4, 1, 3, 0, 2, 5], [0, 1, 2, 4, 3, 3], [2, 3, 0, 1, 4, 2]])
    want = np.array([[2, 3, 1, 4, 0, -1], [1, 2, 3, 4, 0, -1], [1, 2, 3, 4, 0, -1], [1, 2, 3, 4, 0, 0], [1, 2, 3, 4, 0, 1]])
    assert np.array_equal(O.neighbor_ranks(d, nbr), want)
    assert np.array_equal(O.neighbor_ranks(d.astype(np.float64), nbr), want)                 # the value route agrees
    assert np.array_equal(O.nearest_others(d, 4), np.array([[3, 1, 2, 4], [0, 2, 3, 4], [4, 1, 3, 0], [0, 1, 2, 4], [2, 3, 0, 1]]))
    sums = O.segment_row_sums(d[:, :4], [0, 0, 2, 2, 4])
    assert sums.shape == (5, 4) and np.array_equal(sums[2], [0.0, 4.0, 0.0, 2.0])


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_parse_args_without_quality_is_unchanged():
    from pti_ldm_vae_amd import analyze_static
    plain = analyze_static.parse_args(ARGV)
    assert vars(plain) == dict(vae_weights="w.pth", config_file="c.json", folder_edente="e", folder_dente=None,
                               output_dir="projections", max_images=1000, patch_size=[256, 256], color_by_patient=False,
                               method="umap", n_neighbors=40, min_dist=0.5, perplexity=30, seed=42, subtitle=None, dpi=300,
                               cache_dir="cache/latents", batch_size=8)
    assert plain.quality is False and tuple(plain.quality_neighbors) == (5, 15, 40)
    a = analyze_static.parse_args(ARGV + ["--quality"])
    assert vars(a)["quality"] is True and "quality_neighbors" not in vars(a) and tuple(a.quality_neighbors) == (5, 15, 40)
    b = analyze_static.parse_args(ARGV + ["--quality", "--quality-neighbors", "3", "7"])
    assert b.quality_neighbors == [3, 7] and "tsne_backend" not in vars(b)
    with pytest.raises(SystemExit):
        analyze_static.parse_args(ARGV + ["--quality-neighbors"])


def test_new_symbols_are_declared_bound_and_exported():
    import test_abi
    from pti_ldm_vae_amd import _lib, analysis
    from pti_ldm_vae_amd.analysis.projection_quality import projection_quality
    assert {"pti_neighbor_ranks", "pti_segment_row_sums", "pti_projection_distances"} <= set(test_abi._declared())
    test_abi.test_header_symbols_are_bound_and_exported()
    assert analysis.projection_quality is projection_quality and "projection_quality" in analysis.__all__
    h = _lib.lib()
    import ctypes as C
    p = C.c_void_p(16)
    ranks, sums = h.pti_neighbor_ranks, h.pti_segment_row_sums      # every call below returns before any launch
    for fn, call, rc, text in ((ranks, (None, 8, 8, p, 2, p, None), -1, b"null"),
                               (ranks, (p, 8, 2, p, 1, p, None), -1, b"at least 3"),
                               (ranks, (p, 8193, 8193, p, 1, p, None), -2, b"at most 8192"),
                               (ranks, (p, 300, 300, p, 257, p, None), -2, b"256"),
                               (ranks, (p, 7, 8, p, 2, p, None), -1, b"stride"),
                               (sums, (p, 8, 8, p, 2049, p, None), -2, b"2048"),
                               (sums, (p, 8, 8, p, 0, p, None), -1, b"at least 1"),
                               (sums, (p, 8, 8, p, 2, C.c_void_p(20), None), -1, b"misaligned"),
                               (h.pti_projection_distances, (p, 2, 5, 9, p, 5, None), -2, b"8 columns"),
                               (h.pti_projection_distances, (p, 2, 0, 2, p, 5, None), -1, b"at least 1 row"),
                               (h.pti_projection_distances, (p, 2, 5, 2, p, 4, None), -1, b"stride")):
        assert fn(*call) == rc and text in h.pti_last_error_string(), (call, h.pti_last_error_string())


def test_report_refusals_come_before_the_device():
    import torch

    from pti_ldm_vae_amd.analysis.projection_quality import admitted_neighbors, label_codes, projection_quality
    cpu = torch.device("cpu")
    x = np.zeros((6, 3), np.float32)
    with pytest.raises(ValueError, match="255"):
        projection_quality(x, x[:, :2], neighbors=(5, 256), device=cpu)
    with pytest.raises(ValueError, match="8192"):
        projection_quality(np.zeros((8193, 1), np.float32), np.zeros((8193, 2), np.float32), device=cpu)
    with pytest.raises(ValueError, match="at least 4"):
        projection_quality(x[:3], x[:3, :2], device=cpu)
    bad = x.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        projection_quality(bad, x[:, :2], device=cpu)
    with pytest.raises(ValueError, match="non-finite"):
        projection_quality(x, torch.full((6, 2), float("nan")), device=cpu)
    with pytest.raises(ValueError, match="at most 8"):
        projection_quality(np.zeros((6, 9), np.float32), np.zeros((6, 9), np.float32), device=cpu)
    with pytest.raises(ValueError, match="label set"):
        projection_quality(x, x[:, :2], labels={"g": [1, 2]}, device=cpu)
    assert admitted_neighbors((5, 15, 40, 5), 31) == O.admitted((5, 15, 40, 5), 31) == ([5, 15], {40: "k = 40 is not below n / 2 = 15.5"})
    assert label_codes(["b", "a", "b"])[0] == ["a", "b"] and list(label_codes([2, "a", 2])[1]) == [0, 1, 0]

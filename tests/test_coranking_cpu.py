"""CPU tests of the co-ranking curves and the Shepard figure: the numpy oracle (tests/coranking_oracle.py) against scipy and
against scipy's recorded values (tests/golden/coranking_golden.npz), the host half of ``analysis.coranking`` against the
oracle and on hand-made histograms, the identities of the curves, the refusals of the three new entry points (each returns
before any launch) and the command line of ``analyze_static --quality-curves``.

Gates.  Ranks, histograms, S_i, K_max: equality.  The row Spearman coefficient against ``scipy.stats.spearmanr``: 1e-12 (both
are a ratio of sums over at most 239 ranks; observed 2.2e-16 on the 61-row case).  That comparison uses fp64 DISTANCES
only: rounded to fp32 the 240-row case has tied distances within a row, where scipy's average ranks and the keyed order
differ (4.9e-5 in the coefficient).  Curves and scalars formed in fp64 from equal integers: 1e-13."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from scipy import stats

import coranking_oracle as CO
import projection_quality_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "coranking_golden.npz")
CASES = ("main", "small")
ARGV = ["--vae-weights", "w.pth", "--config-file", "c.json", "--folder-edente", "e"]
CURVES = ("Q_NX", "B_NX", "R_NX", "LCMC")
SCALARS = ("auc_logk_rnx", "q_local", "q_global", "rank_correlation", "stress")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cases(gold):
    """case -> (n, dist_high, dist_low in fp64, rank tables of the oracle, its report and arrays); computed once, read only."""
    out = {}
    for case in CASES:
        seed, n, d = (int(v) for v in gold[f"{case}/spec"])
        high, low, _ = O.golden_inputs(seed, n, d, float(gold[f"{case}/noise"]))
        dh, dl = O.pairwise(high), O.pairwise(low)
        out[case] = (n, dh, dl, O.rank_table(dh), O.rank_table(dl)) + CO.report_from_distances(dh, dl)
    return out


def _others(a):
    n = a.shape[0]
    return a[~np.eye(n, dtype=bool)].reshape(n, n - 1)


@pytest.mark.parametrize("case", CASES)
def test_oracle_ranks_equal_scipy_ordinal_ranks(gold, cases, case):
    n, dh, dl, rho, r, _, _ = cases[case]
    assert (n, dh.dtype) == ((240, np.float64) if case == "main" else (61, np.float64))
    assert not O.has_row_ties(dh) and not O.has_row_ties(dl)
    for dist, rank in ((dh, rho), (dl, r)):
        want = np.stack([stats.rankdata(row, method="ordinal") for row in _others(dist)])
        assert np.array_equal(_others(rank), want) and (np.diagonal(rank) == 0).all()
        assert np.array_equal(CO.full_ranks(dist[3:9], 3), rank[3:9].astype(np.int16))      # a slice of rows, offset


@pytest.mark.parametrize("case", CASES)
def test_row_spearman_equals_scipy(gold, cases, case):
    """fp64 distances only: see the module's docstring."""
    n, dh, dl, _, _, report, arrays = cases[case]
    assert not O.has_row_ties(dh) and not O.has_row_ties(dl)
    want = np.array([stats.spearmanr(a, b)[0] for a, b in zip(_others(dh), _others(dl))])
    worst = np.abs(arrays["spearman"] - want).max()
    print(f"{case}: row Spearman against scipy.stats.spearmanr: largest deviation {worst:.1e}")
    assert worst <= 1e-12 and abs(report["rank_correlation"] - want.mean()) <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_oracle_and_host_functions_equal_the_recorded_values(gold, cases, case):
    from pti_ldm_vae_amd.analysis import coranking
    n, _, _, _, _, report, arrays = cases[case]
    assert np.array_equal(arrays["histograms"], gold[f"{case}/histograms"]) and np.array_equal(arrays["sqdiff"], gold[f"{case}/sqdiff"])
    assert np.abs(arrays["spearman"] - gold[f"{case}/spearman"]).max() <= 1e-12
    assert np.abs(coranking.row_spearman(gold[f"{case}/sqdiff"], n) - gold[f"{case}/spearman"]).max() <= 1e-12
    host = coranking.curves_from_histograms(gold[f"{case}/histograms"], n)
    for got in (dict(arrays, **report), host):
        for key in CURVES:
            assert got[key].shape == gold[f"{case}/{key}"].shape and np.abs(got[key] - gold[f"{case}/{key}"]).max() <= 1e-13, key
        assert got["k_max"] == int(gold[f"{case}/k_max"])
        for key in ("auc_logk_rnx", "q_local", "q_global"):
            assert abs(got[key] - float(gold[f"{case}/{key}"])) <= 1e-13, key
    assert abs(report["stress"] - float(gold[f"{case}/stress"])) <= 1e-13
    assert abs(coranking.stress_from_sums(arrays["shepard_sums"]) - float(gold[f"{case}/stress"])) <= 1e-13
    assert os.path.getsize(GOLDEN) < 200 * 1024 and not any("rank" in key.split("/")[1] for key in gold.files)


@pytest.mark.parametrize("case", CASES)
def test_identities(cases, case):
    n, dh, dl, rho, r, report, arrays = cases[case]
    hist = arrays["histograms"]
    assert int(hist.sum()) == n * (n - 1) and not hist[:, 0].any() and int(hist.max()) <= 2 * n
    assert arrays["Q_NX"][-1] == 1.0 and arrays["LCMC"][-1] == 0.0 and arrays["B_NX"][-1] == (hist[2].sum() - hist[1].sum()) / (n * (n - 1))
    ks = [k for k in (5, 15, 40) if 2 * k < n]
    shared = O.rank_sums(dh, dl, ks)["shared"]
    for c, k in enumerate(ks):
        assert arrays["Q_NX"][k - 1] == float(shared[:, c].sum()) / (n * k)
    assert len(ks) == (3 if case == "main" else 2)
    # identical spaces
    same, same_arrays = CO.report_from_distances(dh, dh)
    assert (same_arrays["Q_NX"] == 1.0).all() and (same_arrays["B_NX"] == 0.0).all() and (same_arrays["R_NX"] == 1.0).all()
    assert (same_arrays["spearman"] == 1.0).all() and same["rank_correlation"] == 1.0 and same["stress"] == 0.0
    assert same["auc_logk_rnx"] == 1.0 and same["k_max"] == 1 and same["q_local"] == 1.0 and same["q_global"] == 1.0
    # one row in reversed order: that row's coefficient is -1, the others stay 1
    back = rho.copy()
    back[7] = np.where(rho[7] > 0, n - rho[7], 0)
    _, sq = CO.coranking_fold(rho, back)
    coeff = CO.row_spearman(sq, n)
    assert coeff[7] == -1.0 and (np.delete(coeff, 7) == 1.0).all()


def test_curves_from_hand_made_histograms():
    from pti_ldm_vae_amd.analysis.coranking import curve_samples, curves_from_histograms, stress_from_sums
    perfect = curves_from_histograms([[0, 4, 4, 4], [0, 0, 0, 0], [0, 0, 0, 0]], 4)
    assert list(perfect["Q_NX"]) == [1.0, 1.0, 1.0] and list(perfect["R_NX"]) == [1.0, 1.0] and list(perfect["B_NX"]) == [0.0] * 3
    assert (perfect["k_max"], perfect["q_local"], perfect["q_global"], perfect["auc_logk_rnx"]) == (1, 1.0, 1.0, 1.0)
    # nothing shared before the last K: LCMC is negative up to n - 2, its maximum 0 sits at n - 1, the global range is empty
    worst = curves_from_histograms([[0, 0, 0, 0], [0, 0, 2, 4], [0, 0, 2, 4]], 4)
    assert list(worst["Q_NX"]) == [0.0, 0.5, 1.0] and list(worst["R_NX"]) == [-0.5, -0.5] and list(worst["B_NX"]) == [0.0] * 3
    assert np.abs(worst["LCMC"] - [-1 / 3, -1 / 6, 0.0]).max() <= 1e-16
    assert (worst["k_max"], worst["q_local"], worst["q_global"], worst["auc_logk_rnx"]) == (3, 0.5, None, -0.5)
    mixed = curves_from_histograms(np.array([[0, 2, 0, 0], [0, 0, 3, 1], [0, 0, 1, 5]], dtype=np.int32), 4)
    assert list(mixed["Q_NX"]) == [0.5, 0.75, 1.0] and list(mixed["B_NX"]) == [0.0, -0.25, 2 / 12] and list(mixed["R_NX"]) == [0.25, 0.25]
    assert (mixed["k_max"], mixed["q_local"], mixed["q_global"], mixed["auc_logk_rnx"]) == (1, 0.5, 0.875, 0.25)
    for key, want in CO.curves([[0, 2, 0, 0], [0, 0, 3, 1], [0, 0, 1, 5]], 4).items():
        assert np.array_equal(mixed[key], want), key
    for bad, n in (([[0, 4, 4, 4]] * 3, 4), ([[1, 3, 4, 4], [0] * 4, [0] * 4], 4), ([[0, 4, 4, 4], [0] * 4], 4), ([[0, 3, 3], [0] * 3, [0] * 3], 3)):
        with pytest.raises(ValueError):
            curves_from_histograms(bad, n)
    assert stress_from_sums([[4.0, 1.0, 2.0], [4.0, 1.0, 2.0]]) == 0.0                      # low = high / 2: no stress at the best scale
    assert stress_from_sums([[1.0, 1.0, 0.0]]) == 1.0 and stress_from_sums([[2.0, 2.0, 1.0], [0.0, 0.0, 1.0]]) == 0.0
    assert stress_from_sums([[1.0, 4.0, 1.0]]) == math.sqrt(0.75)
    assert stress_from_sums([[0.0, 1.0, 0.0]]) is None and stress_from_sums([[1.0, 0.0, 0.0]]) is None
    assert stress_from_sums([[np.inf, 1.0, 1.0]]) is None and stress_from_sums([[1.0, 1.0, np.nan]]) is None
    assert curve_samples(4) == [1, 2] and curve_samples(61) == [1, 2, 5, 10, 20, 50] and curve_samples(101) == [1, 2, 5, 10, 20, 50, 100]
    assert curve_samples(8192)[-3:] == [1000, 2000, 5000]


def test_oracle_shepard_bins_follow_the_rule():
    d = np.array([[0.0, 1.0, 2.0, np.inf], [1.0, 0.0, 4.0, -0.0], [2.0, 4.0, 0.0, 3.999], [np.inf, 0.0, 3.999, 0.0]], dtype=np.float32)
    scale = CO.shepard_scale(d, 4)
    assert scale == np.float32(1.0) and CO.shepard_scale(np.zeros((4, 4), np.float32), 4) == 0.0
    assert np.array_equal(CO.shepard_bins(d, scale, 4), [[0, 1, 2, 3], [1, 0, 3, 0], [2, 3, 0, 3], [3, 0, 3, 0]])
    assert np.array_equal(CO.shepard_bins(d, np.float32(0), 4)[0], [0, 0, 0, 3])            # inf * 0 is NaN: the last bin
    sums, mags, hist, scales = CO.shepard_fold(d, d, 4)
    assert int(hist.sum()) == 12 and int(np.trace(hist)) == 12 and list(scales) == [1.0, 1.0] and sums[1, 0] == 17.0


def test_new_symbols_are_declared_bound_and_refuse_before_any_launch():
    import test_abi
    from pti_ldm_vae_amd import _lib, analysis
    from pti_ldm_vae_amd.analysis.coranking import coranking_curves
    assert {"pti_full_ranks", "pti_coranking_fold", "pti_shepard_fold"} <= set(test_abi._declared())
    test_abi.test_header_symbols_are_bound_and_exported()
    assert analysis.coranking_curves is coranking_curves and "coranking_curves" in analysis.__all__
    h = _lib.lib()
    p, odd = C.c_void_p(16), C.c_void_p(17)
    ranks, fold, shepard = h.pti_full_ranks, h.pti_coranking_fold, h.pti_shepard_fold
    for fn, call, rc, text in ((ranks, (None, 8, 8, 8, 0, p, 8, None), -1, b"null"),
                               (ranks, (p, 8, 8, 8, 0, None, 8, None), -1, b"null"),
                               (ranks, (p, 8, 3, 3, 0, p, 8, None), -1, b"at least 4"),
                               (ranks, (p, 8193, 1, 8193, 0, p, 8193, None), -2, b"at most 8192"),
                               (ranks, (p, 8, 0, 8, 0, p, 8, None), -1, b"at least 1 row"),
                               (ranks, (p, 8, 4, 8, 5, p, 8, None), -1, b"outside"),
                               (ranks, (p, 8, 4, 8, -1, p, 8, None), -1, b"outside"),
                               (ranks, (p, 8, 9, 8, 0, p, 8, None), -1, b"outside"),
                               (ranks, (p, 8, 1, 8, 2 ** 31 - 1, p, 8, None), -1, b"outside"),
                               (ranks, (p, 7, 8, 8, 0, p, 8, None), -1, b"stride"),
                               (ranks, (p, 8, 8, 8, 0, p, 7, None), -1, b"stride"),
                               (ranks, (p, 8, 8, 8, 0, odd, 8, None), -1, b"misaligned"),
                               (fold, (None, 8, p, 8, 8, 8, p, p, None), -1, b"null"),
                               (fold, (p, 8, p, 8, 8, 8, None, p, None), -1, b"null"),
                               (fold, (p, 8, p, 8, 8, 8, p, None, None), -1, b"null"),
                               (fold, (p, 8, p, 8, 3, 3, p, p, None), -1, b"at least 4"),
                               (fold, (p, 8193, p, 8193, 1, 8193, p, p, None), -2, b"at most 8192"),
                               (fold, (p, 8, p, 8, 0, 8, p, p, None), -1, b"at least 1 row"),
                               (fold, (p, 8, p, 8, 9, 8, p, p, None), -1, b"outside"),
                               (fold, (p, 8, p, 7, 8, 8, p, p, None), -1, b"stride"),
                               (fold, (p, 8, p, 8, 8, 8, C.c_void_p(20), C.c_void_p(20), None), -1, b"misaligned"),
                               (shepard, (p, 8, p, 8, 8, None, 64, p, p, None), -1, b"null"),
                               (shepard, (p, 8, None, 8, 8, p, 64, p, p, None), -1, b"null"),
                               (shepard, (p, 8, p, 8, 3, p, 64, p, p, None), -1, b"at least 4"),
                               (shepard, (p, 8193, p, 8193, 8193, p, 64, p, p, None), -2, b"at most 8192"),
                               (shepard, (p, 8, p, 8, 8, p, 1, p, p, None), -1, b"at least 2"),
                               (shepard, (p, 8, p, 8, 8, p, 129, p, p, None), -2, b"at most 128"),
                               (shepard, (p, 7, p, 8, 8, p, 64, p, p, None), -1, b"stride"),
                               (shepard, (p, 8, p, 8, 8, p, 64, C.c_void_p(20), p, None), -1, b"misaligned")):
        assert fn(*call) == rc and text in h.pti_last_error_string(), (call, h.pti_last_error_string())


def test_report_refusals_come_before_the_device():
    import torch

    from pti_ldm_vae_amd.analysis.coranking import coranking_curves
    cpu = torch.device("cpu")
    x = np.zeros((6, 3), np.float32)
    for bins in (1, 129):
        with pytest.raises(ValueError, match="2 .. 128"):
            coranking_curves(x, x[:, :2], bins=bins, device=cpu)
    with pytest.raises(ValueError, match="8192"):
        coranking_curves(np.zeros((8193, 1), np.float32), np.zeros((8193, 2), np.float32), device=cpu)
    with pytest.raises(ValueError, match="at least 4"):
        coranking_curves(x[:3], x[:3, :2], device=cpu)
    with pytest.raises(ValueError, match="6 rows, low 5"):
        coranking_curves(x, x[:5, :2], device=cpu)
    bad = x.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError, match="coranking_curves: high holds a non-finite value"):
        coranking_curves(bad, x[:, :2], device=cpu)
    with pytest.raises(ValueError, match="at most 8"):
        coranking_curves(np.zeros((6, 9), np.float32), np.zeros((6, 9), np.float32), device=cpu)


def test_curves_plot_is_written_with_and_without_a_shepard_extent(tmp_path):
    import matplotlib.image

    from pti_ldm_vae_amd import analyze_static
    from pti_ldm_vae_amd.analysis.coranking import bin_edges, curves_from_histograms
    arrays = curves_from_histograms([[0, 2, 0, 0], [0, 0, 3, 1], [0, 0, 1, 5]], 4)
    report = {"n": 4, "stress": 0.25, **{key: arrays[key] for key in ("auc_logk_rnx", "k_max")}}
    arrays.update(shepard_hist=np.array([[5, 1], [0, 6]]), shepard_edges_high=bin_edges(0.5, 2), shepard_edges_low=bin_edges(4.0, 2))
    assert list(bin_edges(0.5, 2)) == [0.0, 2.0, 4.0] and list(bin_edges(0.0, 2)) == [0.0, 0.0, 0.0]
    analyze_static.save_curves_plot(report, arrays, tmp_path / "a.png", "PCA: co-ranking curves", 40)
    arrays.update(shepard_edges_low=bin_edges(0.0, 2))      # a projection without extent: no heat map, no stress
    analyze_static.save_curves_plot(dict(report, stress=None), arrays, tmp_path / "b.png", "PCA: co-ranking curves", 40)
    for name in ("a.png", "b.png"):
        assert matplotlib.image.imread(str(tmp_path / name)).ndim == 3


def test_parse_args_without_the_curve_flags_is_unchanged():
    from pti_ldm_vae_amd import analyze_static
    plain = analyze_static.parse_args(ARGV)
    assert vars(plain) == dict(vae_weights="w.pth", config_file="c.json", folder_edente="e", folder_dente=None,
                               output_dir="projections", max_images=1000, patch_size=[256, 256], color_by_patient=False,
                               method="umap", n_neighbors=40, min_dist=0.5, perplexity=30, seed=42, subtitle=None, dpi=300,
                               cache_dir="cache/latents", batch_size=8)
    assert plain.quality_curves is False and plain.quality_bins == 64 and plain.quality is False
    a = analyze_static.parse_args(ARGV + ["--quality-curves"])
    assert vars(a)["quality_curves"] is True and "quality_bins" not in vars(a) and "quality" not in vars(a) and a.quality_bins == 64
    b = analyze_static.parse_args(ARGV + ["--quality", "--quality-curves", "--quality-bins", "32", "--method", "tsne"])
    assert b.quality is True and b.quality_curves is True and b.quality_bins == 32 and "quality_neighbors" not in vars(b)
    with pytest.raises(SystemExit):
        analyze_static.parse_args(ARGV + ["--quality-bins"])

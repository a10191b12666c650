"""GPU tests of the co-ranking curves and the Shepard figure: ``ops.full_ranks`` / ``ops.coranking_fold`` /
``ops.shepard_fold`` (csrc/coranking.hip) against the numpy oracle (tests/coranking_oracle.py), ``analysis.coranking_curves``
on the golden cases, and ``analyze_static --quality-curves`` end to end.

Gates.  Ranks, histograms, squared rank differences and every other integer: equality.  A Shepard row sum: |got - fsum| <=
(n - 2) 2^-53 sum |term| -- the products are exact in fp64, a row has n - 1 terms and so n - 2 adds in whatever order.  The
report against the oracle on the device's OWN distance matrices: every ratio formed in fp64 from equal integers 1e-13
relative (DESIGN 5r's figure); the stress, sqrt(1 - c^2 / (a b)) of three sums of n (n - 1) positive terms that each carry at
most (n - 2) 2^-53 relative error, 4 (n - 2) 2^-53 / (2 stress^2) relative -- first-order propagation through the quotient
and the root."""
import json
import math
import os

import numpy as np
import pytest
import torch

import coranking_oracle as CO
import projection_quality_oracle as O
from test_gpu_projection_quality import _planted_ties, _true_distances, _write_group

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "coranking_golden.npz")
RANK_SIZES = (4, 5, 63, 64, 65, 256, 257, 300, 1000)      # padding, the 256-thread stride and the power-of-two boundary


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("n", RANK_SIZES)
@pytest.mark.parametrize("kind", ["true", "ties"])
def test_full_ranks_equal_the_oracle(dev, n, kind):
    from pti_ldm_vae_amd import ops
    d = (_true_distances if kind == "true" else _planted_ties)(n, 31 * n + 1)
    assert kind == "true" or O.has_row_ties(d)
    want = CO.full_ranks(d)
    dist = torch.from_numpy(d).to(dev)
    got = ops.full_ranks(dist)
    assert got.dtype == torch.int16 and tuple(got.shape) == (n, n)
    g = got.cpu().numpy()
    assert np.array_equal(g, want)
    assert np.array_equal(np.sort(g, axis=1), np.tile(np.arange(n, dtype=np.int16), (n, 1)))     # every row a permutation
    assert torch.equal(ops.full_ranks(dist), got)                                              # two calls, equal bits
    # a row-strided view of the matrix is used in place; out with ldo > n at an odd element offset, between canaries
    pad = torch.full((n, n + 5), 9.0, device=dev)
    pad[:, 2:n + 2] = dist
    buf = torch.full((n * (n + 3) + 64,), -77, dtype=torch.int16, device=dev)
    out = buf[1:1 + n * (n + 3)].view(n, n + 3)[:, :n]
    assert ops.full_ranks(pad[:, 2:n + 2], out=out) is out and torch.equal(out, got)
    out.fill_(-77)
    assert bool((buf == -77).all())                         # nothing outside the view was written
    # gathered at umap_knn's indices: neighbor_ranks
    k = min(n - 1, 41)
    idx, _ = ops.umap_knn(dist, k)
    idx = idx.contiguous()
    assert torch.equal(got.long().gather(1, idx.long()), ops.neighbor_ranks(dist, idx).long())


def test_full_ranks_of_a_slice_of_rows(dev):
    from pti_ldm_vae_amd import ops
    d = _planted_ties(300, 17)
    dist = torch.from_numpy(d).to(dev)
    whole = ops.full_ranks(dist)
    for lo, hi in ((37, 45), (0, 1), (299, 300), (150, 300)):
        part = ops.full_ranks(dist[lo:hi], lo)
        assert tuple(part.shape) == (hi - lo, 300) and torch.equal(part, whole[lo:hi])
        assert np.array_equal(part.cpu().numpy(), CO.full_ranks(d[lo:hi], lo))
    with pytest.raises(ValueError, match="outside"):
        ops.full_ranks(dist[:8], 293)
    with pytest.raises(ValueError, match="outside"):
        ops.full_ranks(dist[:8], -1)
    with pytest.raises(TypeError):
        ops.full_ranks(dist.double())
    with pytest.raises(TypeError):
        ops.full_ranks(dist, out=torch.zeros(300, 300, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="columns"):
        ops.full_ranks(dist[:3, :3])
    with pytest.raises(ValueError, match="8192"):
        ops.full_ranks(torch.empty(2, 8193, device=dev))


@pytest.mark.parametrize("n,row0", [(8192, 0), (8192, 8184), (4097, 2050), (2048, 100), (2049, 2041)])
def test_full_ranks_at_the_cap_on_a_few_rows(dev, n, row0):
    """8 rows of an 8192-column matrix (the cap: 64 KB of keys), of a 4097-column one (the worst padding) and of 2048- and
    2049-column ones (the last size of the 256-thread sort and the first of the 1024-thread one)."""
    from pti_ldm_vae_amd import ops
    gen = torch.Generator(device=dev).manual_seed(n + row0)
    rows = torch.rand(8, n, generator=gen, device=dev)
    rows[0, 5:9] = 0.25                                     # ties, a -0 and an inf on top of those rand itself repeats
    rows[1, n - 1] = float("inf")
    rows[2, 0] = -0.0
    got = ops.full_ranks(rows, row0).cpu().numpy()
    assert np.array_equal(got, CO.full_ranks(rows.cpu().numpy(), row0))
    assert (got[np.arange(8), row0 + np.arange(8)] == 0).all() and got.max() == n - 1
    # the fold of the same rows against a second table: three n-bin histograms in LDS (96 KB at the cap)
    other = ops.full_ranks(torch.rand(8, n, generator=gen, device=dev), row0)
    hist, sq = ops.coranking_fold(torch.from_numpy(got).to(dev), other)
    want_hist, want_sq = CO.coranking_fold(got, other.cpu().numpy())
    assert np.array_equal(hist.cpu().numpy(), want_hist) and np.array_equal(sq.cpu().numpy(), want_sq) and int(want_hist.sum()) == 8 * (n - 1)


def _rank_pair(n, seed):
    """Two int16 rank tables of n rows: true distances of seeded rows and of a noisy 2-D projection of them."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 5)).astype(np.float32)
    y = (x[:, :2] + 0.7 * rng.standard_normal((n, 2))).astype(np.float32)
    return CO.full_ranks(O.pairwise(x, np.float32)), CO.full_ranks(O.pairwise(y, np.float32))


@pytest.mark.parametrize("n", [4, 65, 300])
def test_coranking_fold_equals_the_oracle(dev, n):
    from pti_ldm_vae_amd import ops
    rho, r = _rank_pair(n, n)
    want_hist, want_sq = CO.coranking_fold(rho, r)
    assert int(want_hist.sum()) == n * (n - 1) and (n == 4 or (want_hist[1:] > 0).any())
    th, tl = torch.from_numpy(rho).to(dev), torch.from_numpy(r).to(dev)
    hist, sq = ops.coranking_fold(th, tl)
    assert hist.dtype == torch.int32 and tuple(hist.shape) == (3, n) and sq.dtype == torch.int64 and tuple(sq.shape) == (n,)
    assert np.array_equal(hist.cpu().numpy(), want_hist) and np.array_equal(sq.cpu().numpy(), want_sq)
    # two half-row calls that accumulate, on row-strided views, into a table between canaries
    pad_h = torch.full((n, n + 7), 3, dtype=torch.int16, device=dev)
    pad_l = torch.full((n, n + 2), 5, dtype=torch.int16, device=dev)
    pad_h[:, 3:n + 3], pad_l[:, 1:n + 1] = th, tl
    buf = torch.full((3 * n + 64,), -5, dtype=torch.int32, device=dev)
    acc = buf[:3 * n].view(3, n)
    acc.zero_()
    half = n // 2
    first, sq_a = ops.coranking_fold(pad_h[:half, 3:n + 3], pad_l[:half, 1:n + 1], acc)
    again, sq_b = ops.coranking_fold(pad_h[half:, 3:n + 3], pad_l[half:, 1:n + 1], acc)
    assert first is acc and again is acc and torch.equal(acc, hist) and torch.equal(torch.cat([sq_a, sq_b]), sq)
    assert bool((buf[3 * n:] == -5).all())
    part, _ = CO.coranking_fold(rho[:half], r[:half])
    assert np.array_equal(ops.coranking_fold(th[:half], tl[:half])[0].cpu().numpy(), part)


def test_coranking_fold_skips_foreign_rank_values(dev):
    from pti_ldm_vae_amd import ops
    n = 65
    rho, r = (a.copy() for a in _rank_pair(n, 9))
    rho[3, 10], rho[3, 11], rho[4, 12], r[5, 13], r[6, 14], r[7, 7] = -1, n, 32767, -32768, n, 5
    rho[8, 20], r[8, 20] = 32767, 32767
    want_hist, want_sq = CO.coranking_fold(rho, r)
    assert int(want_hist.sum()) == n * (n - 1) - 6
    buf = torch.full((3 * n + 128,), -9, dtype=torch.int32, device=dev)
    acc = buf[64:64 + 3 * n].view(3, n)
    acc.zero_()
    hist, sq = ops.coranking_fold(torch.from_numpy(rho).to(dev), torch.from_numpy(r).to(dev), acc)
    assert np.array_equal(hist.cpu().numpy(), want_hist) and np.array_equal(sq.cpu().numpy(), want_sq)
    assert bool((buf[:64] == -9).all()) and bool((buf[64 + 3 * n:] == -9).all()) and not bool(hist[:, 0].any())
    with pytest.raises(TypeError):
        ops.coranking_fold(torch.from_numpy(rho).to(dev).int(), torch.from_numpy(r).to(dev))
    with pytest.raises(ValueError):
        ops.coranking_fold(torch.from_numpy(rho).to(dev), torch.from_numpy(r[:, :64].copy()).to(dev))
    with pytest.raises(TypeError):
        ops.coranking_fold(torch.from_numpy(rho).to(dev), torch.from_numpy(r).to(dev), torch.zeros(3, n, device=dev))


def _shepard_inputs(kind, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 5)).astype(np.float32)
    dh = O.pairwise(x, np.float32) * np.float32(3.0)
    dl = O.pairwise((x[:, :2] + 0.5 * rng.standard_normal((n, 2))).astype(np.float32), np.float32)
    if kind == "zero":
        dl = np.zeros_like(dl)
    if kind == "inf":
        dh[1, 3] = dh[3, 1] = np.inf
        dl[0, 2] = np.inf
        dl[4, 4] = 7.5                                      # the own column takes no part, whatever it holds
    return dh, dl


@pytest.mark.parametrize("bins", [2, 64, 128])
@pytest.mark.parametrize("kind,n", [("true", 65), ("true", 300), ("zero", 65), ("inf", 65)])
def test_shepard_fold_equals_the_restatement(dev, kind, n, bins):
    from pti_ldm_vae_amd import ops
    dh, dl = _shepard_inputs(kind, n)
    want_sums, mags, want_hist, want_scale = CO.shepard_fold(dh, dl, bins)
    th, tl = torch.from_numpy(dh).to(dev), torch.from_numpy(dl).to(dev)
    sums, hist, scale = ops.shepard_fold(th, tl, bins)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (n, 3) and tuple(hist.shape) == (bins, bins)
    assert np.array_equal(scale.cpu().numpy(), want_scale) and (kind != "zero" or float(scale[1]) == 0.0)
    assert np.array_equal(hist.cpu().numpy(), want_hist) and int(want_hist.sum()) == n * (n - 1)
    if kind == "zero":
        assert int(want_hist[:, 0].sum()) == n * (n - 1)
    if kind == "inf":
        assert want_hist[bins - 1, :].sum() >= 2 and want_hist[:, bins - 1].sum() >= 1
    got = sums.cpu().numpy()
    finite = np.isfinite(want_sums)
    assert np.array_equal(np.isfinite(got), finite) and (kind == "inf") == (not finite.all())
    assert np.array_equal(got[~finite], want_sums[~finite])                                   # +inf where a term is
    off, bound = np.abs(got[finite] - want_sums[finite]), (n - 2) * 2.0 ** -53 * mags[finite]
    print(f"{kind} n={n} bins={bins}: largest deviation of a row sum from fsum, relative to sum |term|: "
          f"{(off / np.maximum(mags[finite], 1e-300)).max():.2e}")
    assert (off <= bound).all()
    # the same rows, at the same indices of another call with the rest of the matrices changed, a row stride and an
    # accumulating histogram: the same bits
    keep = [0, 7, 64]
    oh, ol = torch.full((n, n + 3), 2.0, device=dev), torch.full((n, n + 1), 0.5, device=dev)
    oh[:, 1:n + 1], ol[:, :n] = th * 0.5, tl * 2.0
    oh[keep, 1:n + 1], ol[keep, :n] = th[keep], tl[keep]
    acc = hist.clone()
    other, twice, _ = ops.shepard_fold(oh[:, 1:n + 1], ol[:, :n], bins, hist=acc)
    assert twice is acc and int(acc.sum()) == 2 * n * (n - 1)
    assert torch.equal(other[keep].view(torch.int64), sums[keep].view(torch.int64))
    assert torch.equal(ops.shepard_fold(th, tl, bins)[0].view(torch.int64), sums.view(torch.int64))


def test_shepard_fold_refusals(dev):
    from pti_ldm_vae_amd import ops
    d = torch.rand(8, 8, device=dev)
    for bins in (1, 129):
        with pytest.raises(ValueError, match="2 <= bins <= 128"):
            ops.shepard_fold(d, d, bins)
    with pytest.raises(ValueError, match="4 <= n"):
        ops.shepard_fold(d[:3, :3], d[:3, :3])
    with pytest.raises(ValueError):
        ops.shepard_fold(d, d[:7, :7])
    with pytest.raises(TypeError):
        ops.shepard_fold(d, d.double())
    with pytest.raises(ValueError):
        ops.shepard_fold(d, d, 8, hist=torch.zeros(8, 9, dtype=torch.int32, device=dev))


# ---- the report ----------------------------------------------------------------------------------------------------------------
def _assert_reports_agree(got, want, got_arrays, want_arrays):
    n = want["n"]
    assert list(got) == ["n", "auc_logk_rnx", "k_max", "q_local", "q_global", "rank_correlation", "stress", "bins"]
    assert (got["n"], got["k_max"], got["bins"]) == (want["n"], want["k_max"], want["bins"])
    for key in ("histograms", "sqdiff", "shepard_hist"):
        assert np.array_equal(got_arrays[key], want_arrays[key]), key
    for key in ("auc_logk_rnx", "q_local", "q_global", "rank_correlation"):
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            assert not math.isnan(got[key]) and abs(got[key] - want[key]) <= 1e-13 * abs(want[key]), (key, got[key], want[key])
    for key in ("Q_NX", "B_NX", "R_NX", "LCMC", "spearman"):
        assert got_arrays[key].shape == want_arrays[key].shape
        assert (np.abs(got_arrays[key] - want_arrays[key]) <= 1e-13 * np.abs(want_arrays[key])).all(), key
    assert (got["stress"] is None) == (want["stress"] is None)
    if want["stress"] is not None:
        assert abs(got["stress"] - want["stress"]) <= 4 * (n - 2) * 2.0 ** -53 / (2 * want["stress"] ** 2) * want["stress"]


@pytest.mark.parametrize("case", ["main", "small"])
def test_coranking_curves_on_the_golden_cases(gold, dev, case):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import coranking_curves, projection_quality
    seed, n, d = (int(v) for v in gold[f"{case}/spec"])
    high, low, _ = O.golden_inputs(seed, n, d, float(gold[f"{case}/noise"]))
    got, got_arrays = coranking_curves(high, low, device=dev)
    again, again_arrays = coranking_curves(torch.from_numpy(high).to(dev), torch.from_numpy(low).to(dev), bins=64, device=dev)
    assert json.dumps(got, allow_nan=False) == json.dumps(again, allow_nan=False)
    assert sorted(got_arrays) == sorted(again_arrays) and all(np.array_equal(got_arrays[k], again_arrays[k]) for k in got_arrays)
    # against the oracle on the device's own distance matrices
    dh = ops.latent_pairwise(torch.from_numpy(high).to(dev)).cpu().numpy()
    dl = ops.projection_distances(torch.from_numpy(low).to(dev)).cpu().numpy()
    want, want_arrays = CO.report_from_distances(dh, dl, 64)
    _assert_reports_agree(got, want, got_arrays, want_arrays)
    assert np.array_equal(got_arrays["shepard_edges_high"], np.arange(65) / float(CO.shepard_scale(dh, 64)))
    assert np.array_equal(got_arrays["shepard_edges_low"], np.arange(65) / float(CO.shepard_scale(dl, 64)))
    # the same integer over n k as projection_quality's neighbourhood preservation
    quality, _ = projection_quality(high, low, neighbors=(5, 15, 40), device=dev)
    assert quality["neighbors"] == ([5, 15, 40] if case == "main" else [5, 15])
    for k in quality["neighbors"]:
        assert got_arrays["Q_NX"][k - 1] == quality["neighborhood_preservation"][k]
    print(f"{case}: against scipy's recorded fp64 values: rank correlation {got['rank_correlation'] - gold[f'{case}/spearman'].mean():+.2e}, "
          f"stress {got['stress'] - float(gold[f'{case}/stress']):+.2e}, AUC {got['auc_logk_rnx'] - float(gold[f'{case}/auc_logk_rnx']):+.2e}")


def test_coranking_curves_edge_inputs(dev):
    from pti_ldm_vae_amd.analysis import coranking_curves
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 2)).astype(np.float32)
    x[7] = x[3]                                             # duplicate rows: ties, the own column not first
    # identical spaces, stated on ONE matrix (the report forms the two matrices by two routes that differ in the last bits)
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis.coranking import curves_from_histograms, stress_from_sums
    dist = ops.latent_pairwise(torch.from_numpy(x).to(dev))
    ranks = ops.full_ranks(dist)
    hist, sq = ops.coranking_fold(ranks, ranks)
    curves = curves_from_histograms(hist.cpu().numpy(), 40)
    assert not bool(hist[1:].any()) and not bool(sq.any()) and (curves["Q_NX"] == 1.0).all() and (curves["B_NX"] == 0.0).all()
    assert (curves["k_max"], curves["q_local"], curves["q_global"], curves["auc_logk_rnx"]) == (1, 1.0, 1.0, 1.0)
    sums, shepard, _ = ops.shepard_fold(dist, dist, 2)
    assert stress_from_sums(sums.cpu().numpy()) == 0.0 and int(shepard.diagonal().sum()) == 40 * 39
    # a projection without extent: no stress, and nothing that JSON cannot hold
    flat, _ = coranking_curves(x, np.zeros((40, 2), np.float32), device=dev)
    assert flat["stress"] is None and flat["n"] == 40 and flat["bins"] == 64
    json.dumps(flat, allow_nan=False)
    tiny, tiny_arrays = coranking_curves(x[:4], x[:4, ::-1].copy(), bins=2, device=dev)
    assert tiny["n"] == 4 and tiny["bins"] == 2 and tiny_arrays["Q_NX"].shape == (3,) and tiny_arrays["R_NX"].shape == (2,)
    assert tiny_arrays["Q_NX"][-1] == 1.0 and int(tiny_arrays["histograms"].sum()) == 12 and tiny_arrays["shepard_hist"].shape == (2, 2)
    with pytest.raises(ValueError, match="non-finite"):
        coranking_curves(torch.full((6, 2), float("inf"), device=dev), x[:6], device=dev)


# ---- analyze_static --quality-curves end to end ------------------------------------------------------------------------------
def test_analyze_static_quality_curves_end_to_end(dev, tmp_path, capsys):
    import matplotlib.image

    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import analyze_static, ops
    _write_group(tmp_path / "edente", ["11", "12", "13", "14", "15", "16"], 4, seed=1)     # 24 + 24 images, six patients
    _write_group(tmp_path / "dente", ["12", "13", "11", "16", "15", "14"], 4, seed=2)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64])
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)
    base = ["--vae-weights", str(ck), "--config-file", str(tmp_path / "cfg.json"), "--folder-edente", str(tmp_path / "edente"),
            "--folder-dente", str(tmp_path / "dente"), "--patch-size", "64", "64", "--cache-dir", str(tmp_path / "cache"),
            "--batch-size", "8", "--dpi", "40"]
    curve_files = ["projection_curves.json", "projection_curves.npz"]
    runs = (("pca", ["--method", "pca", "--quality-curves", "--quality-bins", "16"], 16, False),
            ("umap", ["--method", "umap", "--umap-backend", "hip", "--umap-fit-group", "edente", "--n-neighbors", "5", "--quality",
                      "--quality-curves"], 64, True))
    for method, extra, bins, with_quality in runs:
        out = tmp_path / f"out_{method}"
        analyze_static.main(base + extra + ["--output-dir", str(out)])
        assert "Projection curves: AUC_logK(R_NX) " in capsys.readouterr().out
        for name in curve_files + [f"{method}_projection_curves.png", "latents.npz"]:
            assert (out / name).is_file() and (out / name).stat().st_size > 0, name
        assert (out / "projection_quality.json").is_file() == with_quality
        assert matplotlib.image.imread(str(out / f"{method}_projection_curves.png")).ndim == 3
        raw = (out / "projection_curves.json").read_bytes()
        assert b"NaN" not in raw and b"Infinity" not in raw
        doc = json.loads(raw)
        assert list(doc) == ["method", "n", "auc_logk_rnx", "k_max", "q_local", "q_global", "rank_correlation", "stress", "bins",
                             "K", "Q_NX", "B_NX", "R_NX"]
        assert doc["method"] == method and doc["n"] == 48 and doc["bins"] == bins and doc["K"] == [1, 2, 5, 10, 20]
        assert list(doc["Q_NX"]) == list(doc["B_NX"]) == list(doc["R_NX"]) == ["1", "2", "5", "10", "20"]
        # the oracle's report on latents.npz, from the distances the device makes of those rows
        z = np.load(out / "latents.npz")
        high = np.concatenate([z["latents_edente"], z["latents_dente"]])
        low = np.concatenate([z["projection_edente"], z["projection_dente"]]).astype(np.float32)
        dh = ops.latent_pairwise(torch.from_numpy(high).to(dev)).cpu().numpy()
        dl = ops.projection_distances(torch.from_numpy(low).to(dev)).cpu().numpy()
        want, want_arrays = CO.report_from_distances(dh, dl, bins)
        pts = np.load(out / "projection_curves.npz")
        _assert_reports_agree({k: doc[k] for k in list(doc)[1:9]}, want, pts, want_arrays)
        for key in ("Q_NX", "B_NX", "R_NX"):
            assert [doc[key][str(k)] for k in doc["K"]] == [float(pts[key][k - 1]) for k in doc["K"]]
        assert list(pts["ids"]) == list(z["ids_edente"]) + list(z["ids_dente"])
        assert list(pts["paths"]) == list(z["paths_edente"]) + list(z["paths_dente"])
        assert pts["shepard_hist"].shape == (bins, bins) and pts["shepard_edges_high"].shape == (bins + 1,) and pts["histograms"].shape == (3, 48)
        if method == "pca":                                 # a second run writes the same bytes
            analyze_static.main(base + extra + ["--output-dir", str(out)])
            assert (out / "projection_curves.json").read_bytes() == raw
    # without the flag the file set is what it has always been
    plain = tmp_path / "plain"
    analyze_static.main(base + ["--method", "pca", "--output-dir", str(plain)])
    assert sorted(os.listdir(plain)) == ["distance_metrics.txt", "exams_sorted_by_distance.txt", "latents.npz", "pca_projection.png"]
    assert sorted(os.listdir(tmp_path / "out_pca")) == sorted(os.listdir(plain) + curve_files + ["pca_projection_curves.png"])
    for name in ("distance_metrics.txt", "exams_sorted_by_distance.txt"):
        assert (plain / name).read_bytes() == (tmp_path / "out_pca" / name).read_bytes()

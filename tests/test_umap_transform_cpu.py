"""CPU tests of the device-side UMAP transform's host half: the fp64 oracle (``tests/umap_transform_oracle.py``) against
numpy / scikit-learn and against ``tests/golden/umap_transform_golden.npz``, the validation paths of ``pti_umap_knn_cross`` /
``pti_umap_transform_graph`` / ``pti_umap_transform_layout`` that return before any launch, and the ``UmapResult`` /
``--umap-fit-group`` plumbing of ``LatentSpaceAnalyzer`` and ``analyze_static``."""
import ctypes as C

import numpy as np
import pytest
import torch

import umap_transform_oracle as T

O = T.O


@pytest.fixture(scope="module")
def gold():
    return np.load(T.GOLDEN)


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def test_oracle_pca_model_equals_sklearn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    train, new = (v.astype(np.float64) for v in T.split("t300k40"))
    emb, mean, axes = T.pca_fit(train, 50)
    model = decomposition.PCA(n_components=50, svd_solver="full").fit(train)
    want_train, want_new = model.transform(train), model.transform(new)
    flip = np.sign((emb * want_train).sum(axis=0))                       # sklearn >= 1.5 fixes signs by the components, not by U
    scale = np.abs(want_new).max()
    assert np.allclose(mean, model.mean_, rtol=0, atol=1e-12)
    assert np.abs(emb * flip - want_train).max() <= 1e-9 * scale
    assert np.abs(T.pca_transform(new, train, mean, axes) * flip - want_new).max() <= 1e-9 * scale
    assert np.abs(T.pca_transform(train, train, mean, axes) - emb).max() <= 1e-9 * scale


def test_oracle_pca_zeroes_columns_without_variance():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(8, 3)) @ rng.normal(size=(3, 20))               # rank 3
    emb, mean, axes = T.pca_fit(x, 6)
    out = T.pca_transform(rng.normal(size=(4, 20)), x, mean, axes)
    assert np.abs(out[:, :3]).min() > 0 and not out[:, 3:].any() and np.isfinite(out).all()


@pytest.mark.parametrize("name", list(T.CASES))
def test_oracle_cross_knn_equals_a_stable_argsort(gold, name):
    train, new = T.split(name)
    dist, k = T.cross_distances(new, train), T.CASES[name][2]
    idx, kd = T.knn(dist, k)
    want = np.argsort(dist, axis=1, kind="stable")[:, :k]
    assert dist.shape == (len(new), len(train)) and idx.shape == kd.shape == (len(new), k)
    assert np.array_equal(idx, want) and np.array_equal(kd, np.take_along_axis(dist, want, axis=1))
    assert int((kd == 0).sum()) == int(gold[f"zeros_{name}"])
    if name == "t97":
        assert len(new) == 30 and np.array_equal(idx[27, :3], [0, 1, 2]) and idx[28, 0] == idx[29, 0] == 45 and (kd == 0).sum() == 5
        ties = (kd[:, 1:] == kd[:, :-1]) & (kd[:, 1:] > 0)
        assert ties.any(axis=1).sum() >= 20 and (idx[:, 1:][ties] > idx[:, :-1][ties]).all()
    if name == "thub":
        assert (idx[:, 0] == 0).all()                                     # the origin is every new row's nearest training row


def test_oracle_transform_graph_is_what_it_says():
    _, idx, kd, yt, g = T.case_graph("t97")
    k = idx.shape[1]
    psum = np.where(kd[:, 1:] > 0, np.exp(-kd[:, 1:].astype(np.float64) / g.sigma[:, None]), 1.0).sum(axis=1)
    floored = g.sigma <= 1e-3 * kd.astype(np.float64).mean() * (1 + 1e-12)
    assert (np.abs(psum - np.log2(k)) < 1e-5)[~floored].all() and (~floored).sum() > len(idx) // 2
    assert g.wmax == 1.0 and np.array_equal(g.weights == 1.0, kd == 0) and (g.rate > 0).all() and g.rate.max() == 1 << 20
    short = T.transform_graph(idx, kd, yt, T.T_SHORT["t97"])
    dropped = short.rate == 0
    assert dropped.sum() == 4 and (short.w32[dropped] * 10.0 < 1.0).all() and (short.w32[~dropped] * 10.0 >= 1.0).all()
    assert np.array_equal(short.rate[~dropped], T.rates(short.w32, np.float32(1.0))[~dropped])
    assert np.array_equal(short.y0, g.y0)                                 # the start is normalised before the threshold
    lo, hi = yt[idx].min(axis=1), yt[idx].max(axis=1)
    assert ((g.y0 >= lo - 1e-5) & (g.y0 <= hi + 1e-5)).all()              # a convex combination of the neighbours' points
    assert np.array_equal(g.y0[28], g.y0[29])


def test_oracle_layout_splits_and_skips():
    _, idx, _, yt, g = T.case_graph("t97")
    a, b = O.find_ab_params(1.0, O.MIN_DIST)
    whole = T.layout(g.indices, g.rate, g.y0, yt, a, b, 100, T.SEED, stop=6)
    parts = g.y0
    for e in range(6):
        parts = T.layout(g.indices, g.rate, parts, yt, a, b, 100, T.SEED, start=e, stop=e + 1)
    assert whole.dtype == np.float32 and np.array_equal(whole, parts) and not np.array_equal(whole, g.y0)
    bad = idx.copy()
    bad[3], bad[4, ::2] = len(yt), -1
    moved = T.layout(bad, g.rate, g.y0, yt, a, b, 100, T.SEED, stop=20)
    assert np.array_equal(moved[3], g.y0[3]) and not np.array_equal(moved[4], g.y0[4])
    keep = np.ones(len(idx), bool)
    keep[[3, 4]] = False
    assert np.array_equal(moved[keep], T.layout(g.indices, g.rate, g.y0, yt, a, b, 100, T.SEED, stop=20)[keep])


def test_oracle_reproduces_the_golden_file(gold):
    a, b = O.find_ab_params(1.0, O.MIN_DIST)
    assert np.allclose(gold["ab"], [a, b], rtol=1e-12, atol=0)
    for name in T.CASES:
        again = T.graph_bounds(name)
        for key, value in again.items():
            assert np.allclose(value, gold[key], rtol=1e-6, atol=1e-12), key
        for key in ("sigma", "w", "y0"):
            tol, f32, bound = (float(gold[f"{key}_{kind}_{name}"]) for kind in ("dev_tol", "dev_fp32", "bound"))
            assert bound == 2.0 * max(tol, f32) and 0 < bound < 1e-5
        for t in (T.CASES[name][3],) + ((T.T_SHORT[name],) if name in T.T_SHORT else ()):
            assert float(gold[f"thr_gap_{t}_{name}"]) > 100.0 * float(gold[f"w_bound_{name}"])   # the dropped slots are decidable
    assert int(gold["dropped_10_t97"]) == 4 and all(int(gold[f"dropped_100_{name}"]) == 0 for name in T.CASES)
    assert 0.05 < float(gold["thr_gap_10_t97"]) * 10.0 < 0.1              # the nearest weight: 8 % from the threshold 1 / 10
    name = "t97"
    again = T.epoch_bounds(name, a, b)
    for key, value in again.items():
        assert np.allclose(value, gold[key], rtol=1e-3 if "dev" in key or "bound" in key else 1e-9, atol=1e-12), key
    for name in T.EPOCH_CASES:
        store = float(gold[f"store_dev_{name}"])
        assert float(gold[f"restart_bound_{name}"]) == 2.0 * max(float(gold[f"restart_fp32_dev_{name}"]), store)
        for stop in (1, 10):
            assert float(gold[f"epoch_bound_{stop}_{name}"]) >= 2.0 * float(gold[f"epoch_fp32_dev_{stop}_{name}"]) > 0
            assert gold[f"y{stop}_{name}"].dtype == np.float64
    # the quality gate: the fit, the start and one seed are recomputed here
    train, new, yt = T.quality_fit(a, b)
    idx, kd = T.knn(T.cross_distances(new, train), T.QUALITY_FIT[0])
    g = T.transform_graph(idx, kd, yt, T.QUALITY_T)
    shares = gold["share_seeds"]
    assert np.isclose(T.neighbour_share(new, train, g.y0, yt), float(gold["share_start"]), rtol=1e-9)
    one = T.neighbour_share(new, train, T.layout(g.indices, g.rate, g.y0, yt, a, b, T.QUALITY_T, T.QUALITY_SEEDS[0]), yt)
    assert abs(one - shares[0]) <= np.ptp(shares)
    assert len(shares) == 6 and float(gold["share_gate"]) == shares.min() - np.ptp(shares) > float(gold["share_start"])
    default = gold["share_seeds_default"]
    assert T.QUALITY_T_DEFAULT == 66 and len(default) == 6
    assert float(gold["share_gate_default"]) == default.min() - np.ptp(default) > float(gold["share_start"])
    again = T.pca_bounds()
    assert np.isclose(again["pca_bound"], float(gold["pca_bound"]), rtol=1e-2) and float(gold["pca_bound"]) < 1e-4


def test_neighbour_share_counts_what_it_says():
    train = np.arange(40.0)[:, None] * np.ones((1, 3))
    new = np.array([[10.2, 10.2, 10.2]])
    line = np.stack([np.arange(40.0), np.zeros(40)], axis=1)
    assert T.neighbour_share(new, train, np.array([[10.2, 0.0]]), line, k=5) == 1.0
    assert T.neighbour_share(new, train, np.array([[12.2, 0.0]]), line, k=5) == 3 / 5
    assert T.neighbour_share(new, train, np.array([[30.0, 0.0]]), line, k=5) == 0.0


# ---- the C entry points ----------------------------------------------------------------------------------------------------
def test_c_entry_points_validate_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    ws = h.pti_umap_transform_graph_ws_floats
    assert ws(30, 70, 15) == 2 * 31 + 31 and ws(8192, 8192, 256) == 2 * 8193 + 8193 and ws(1, 3, 2) == 6
    for bad in ((0, 70, 15), (8193, 70, 15), (30, 2, 2), (30, 70, 70), (30, 70, 1), (30, 300, 257), (30, 8193, 40), (-1, 70, 15)):
        assert ws(*bad) == 0, bad
    p, q, r, t = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024), C.c_void_p(1 << 20)   # never dereferenced: refused first
    err = h.pti_last_error_string
    cross = h.pti_umap_knn_cross
    for bad in (0, 5, 6):
        args = [p, 8, 5, 8, 3, q, r, None]
        args[bad] = None
        assert cross(*args) == -1 and b"null" in err()
    for m, n, k in ((0, 8, 3), (-2, 8, 3), (5, 2, 2), (5, 0, 2), (5, 8, 8), (5, 8, 1), (5, 300, 300)):
        assert cross(p, 300, m, n, k, q, r, None) == -1 and b"dimension" in err(), (m, n, k)
    for m, n, k in ((8193, 300, 40), (5, 8193, 40), (5, 300, 257)):
        assert cross(p, 9000, m, n, k, q, r, None) == -2 and b"shape" in err()
    assert cross(p, 7, 5, 8, 3, q, r, None) == -1 and b"stride" in err()

    graph = h.pti_umap_transform_graph
    good = [p, q, 5, 3, t, 8, 100, r, r, r, r, r, None]
    for bad in (0, 1, 4, 7, 8, 9, 10, 11):
        args = list(good)
        args[bad] = None
        assert graph(*args) == -1 and b"null" in err()
    for pos, value, rc, text in ((2, 0, -1, b"dimension"), (2, 8193, -2, b"shape"), (5, 2, -1, b"dimension"), (5, 8193, -2, b"shape"),
                                 (3, 1, -1, b"dimension"), (3, 8, -1, b"dimension"), (6, 0, -1, b"n_epochs"), (6, -4, -1, b"n_epochs"),
                                 (6, 2001, -2, b"n_epochs"), (11, C.c_void_p(1028), -1, b"aligned")):
        args = list(good)
        args[pos] = value
        assert graph(*args) == rc and text in err(), (pos, value)
    args = list(good)
    args[3], args[5] = 257, 300
    assert graph(*args) == -2 and b"shape" in err()

    layout = h.pti_umap_transform_layout
    good = [p, q, 5, 3, t, 8, r, r, 0.58, 1.33, 0.25, 100, 0, 100, 42, 5, None]
    for bad in (0, 1, 4, 6, 7):
        args = list(good)
        args[bad] = None
        assert layout(*args) == -1 and b"null" in err()
    for pos, value, rc, text in ((2, 0, -1, b"dimension"), (2, 8193, -2, b"shape"), (5, 2, -1, b"dimension"), (5, 8193, -2, b"shape"),
                                 (3, 1, -1, b"dimension"), (3, 8, -1, b"dimension"), (11, 0, -1, b"n_epochs"), (11, 2001, -2, b"n_epochs"),
                                 (12, -1, -1, b"epoch range"), (12, 101, -1, b"epoch range"), (13, 101, -1, b"epoch range"),
                                 (15, -1, -1, b"negative_sample_rate"), (15, 65, -1, b"negative_sample_rate"),
                                 (8, 0.0, -1, b"positive"), (9, float("nan"), -1, b"positive"), (10, 0.0, -1, b"initial_alpha"),
                                 (10, float("inf"), -1, b"initial_alpha")):
        args = list(good)
        args[pos] = value
        assert layout(*args) == rc and text in err(), (pos, value)
    args = list(good)
    args[7] = t                                                           # y_out is y_train
    assert layout(*args) == -1 and b"y_train" in err()
    for at in ((1 << 20) + 8 * 8 - 4, (1 << 20) - 8 * 5 + 4):            # y_out begins in y_train's last float / ends in its first
        args[7] = C.c_void_p(at)
        assert layout(*args) == -1 and b"y_train" in err()
    args = list(good)
    args[7] = C.c_void_p(1024 + 8)                                        # overlaps y_in without being it
    rc = layout(*args)
    assert rc == -1 and b"y_in itself" in err()
    with pytest.raises(_lib.PtiError):
        _lib.check(rc, "umap_transform_layout")


def test_ops_refuse_cpu_tensors():
    from pti_ldm_vae_amd import ops
    d, idx, kd, y = torch.rand(5, 8), torch.zeros(5, 3, dtype=torch.int32), torch.rand(5, 3), torch.rand(5, 2)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_knn_cross(d, 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_knn_cross(d.numpy(), 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_transform_graph(idx, kd, torch.rand(8, 2), 100)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_transform_graph(idx.numpy(), kd, torch.rand(8, 2), 100)
    tg = ops.UmapTransformGraph(idx, kd, idx, None, y)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_transform_layout(tg, torch.rand(8, 2), y, y, a=0.58, b=1.33, n_epochs=100, seed=1)


def test_umap_knn_cross_refuses_an_out_tuple_of_the_wrong_length():
    """The length of ``out=(knn_idx, knn_dist)`` is checked before anything else, so no device is needed."""
    from pti_ldm_vae_amd import ops
    for out in ((None,), (None, None, None)):
        with pytest.raises(ValueError, match=r"umap_knn_cross: out must be \(knn_idx, knn_dist\)"):
            ops.umap_knn_cross(torch.rand(5, 8), 3, out=out)


# ---- API and CLI -------------------------------------------------------------------------------------------------------------
ARGV = ["--vae-weights", "w.pth", "--config-file", "c.json", "--folder-edente", "e"]


def test_parse_args_umap_fit_group():
    from pti_ldm_vae_amd import analyze_static
    plain = analyze_static.parse_args(ARGV)
    assert "umap_fit_group" not in vars(plain) and plain.umap_fit_group == "all"
    assert sorted(vars(plain)) == sorted(["vae_weights", "config_file", "folder_edente", "folder_dente", "output_dir", "max_images",
                                          "patch_size", "color_by_patient", "method", "n_neighbors", "min_dist", "perplexity", "seed",
                                          "subtitle", "dpi", "cache_dir", "batch_size"])
    a = analyze_static.parse_args(ARGV + ["--umap-fit-group", "edente"])
    assert vars(a)["umap_fit_group"] == "edente" and "umap_backend" not in vars(a) and a.umap_backend == "umap-learn"
    assert analyze_static.parse_args(ARGV + ["--umap-fit-group", "all"]).umap_fit_group == "all"
    with pytest.raises(SystemExit):
        analyze_static.parse_args(ARGV + ["--umap-fit-group", "dente"])


@pytest.mark.parametrize("backend", [[], ["--umap-backend", "umap-learn"]])
def test_fit_group_edente_needs_the_device_backend(backend, monkeypatch):
    """The exit comes before the device, the model or any image is touched."""
    from pti_ldm_vae_amd import analyze_static
    from pti_ldm_vae_amd.utils import cli_common
    monkeypatch.setattr(cli_common, "init_device_and_seed", lambda *a: pytest.fail("went on to the device"))
    with pytest.raises(SystemExit, match="--umap-fit-group edente.*--umap-backend hip"):
        analyze_static.main(ARGV + ["--folder-dente", "d", "--umap-fit-group", "edente"] + backend)


def test_project_fit_first_fits_on_the_first_group_only():
    from pti_ldm_vae_amd import analyze_static
    seen = []

    class Model:
        def transform(self, rows):
            seen.append(("transform", len(rows)))
            return np.ones((len(rows), 2))

    class Fake:
        def reduce_dimensionality_umap(self, latents, **kw):
            seen.append(("fit", len(latents), kw))
            return np.zeros((len(latents), 2)), Model()

    args = analyze_static.parse_args(ARGV + ["--umap-backend", "hip", "--umap-fit-group", "edente", "--n-neighbors", "9", "--seed", "3"])
    (first, second), method = analyze_static.project_fit_first(Fake(), np.zeros((30, 8)), np.zeros((12, 8)), args)
    assert method == "umap" and first.shape == (30, 2) and not first.any() and second.shape == (12, 2) and second.all()
    assert seen == [("fit", 30, dict(n_neighbors=9, min_dist=0.5, random_state=3, pca_components=30, backend="hip")), ("transform", 12)]


def test_umap_result_without_state_constructs_and_refuses_to_transform():
    from pti_ldm_vae_amd.analysis.latent_space import UmapResult
    y = np.zeros((5, 2))
    r = UmapResult(y, 0.58, 1.33, 200, None)
    assert r.embedding_ is y and (r.a_, r.b_, r.n_epochs_, r.graph_) == (0.58, 1.33, 200, None)
    with pytest.raises(RuntimeError, match="carries no fitted state"):
        r.transform(np.zeros((3, 8), dtype=np.float32))
    with pytest.raises(TypeError):
        UmapResult(y, 0.58, 1.33, 200, None, object())                    # the state is keyword-only


def test_umap_result_transform_checks_its_arguments_first():
    from pti_ldm_vae_amd.analysis.latent_space import UmapResult
    state = dict(pca=object(), train_pca=torch.zeros(60, 50), train_embedding=torch.zeros(60, 2), n_neighbors=15, seed=42)
    r = UmapResult(np.zeros((60, 2)), 0.58, 1.33, 200, None, n_epochs_defaulted=False, **state)
    with pytest.raises(ValueError, match="Expected 2D array"):
        r.transform(np.zeros(8, dtype=np.float32))
    for rows in (0, 8193):
        with pytest.raises(ValueError, match=f"1 to 8192 new rows at once, got {rows}"):
            r.transform(np.zeros((rows, 8), dtype=np.float32))
    for n_epochs in (0, 2001):
        with pytest.raises(ValueError, match=f"1 <= n_epochs <= 2000, got {n_epochs}"):
            r.transform(np.zeros((3, 8), dtype=np.float32), n_epochs=n_epochs)


def test_transform_epochs_follow_umap_learns_rule(monkeypatch):
    """100 when the fit's n_epochs was defaulted, else a third of the fit's, at least 1."""
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis.latent_space import UmapResult
    seen = []

    class Stop(Exception):
        pass

    class Pca:
        def transform(self, rows):
            return np.zeros((len(rows), 50))

    def graph(knn_idx, knn_dist, y_train, n_epochs):
        seen.append(n_epochs)
        raise Stop

    monkeypatch.setattr(ops, "latent_pairwise", lambda a, b: None)
    monkeypatch.setattr(ops, "umap_knn_cross", lambda dist, k: (None, None))
    monkeypatch.setattr(ops, "umap_transform_graph", graph)
    state = dict(pca=Pca(), train_pca=torch.zeros(60, 50), train_embedding=torch.zeros(60, 2), n_neighbors=15, seed=42)
    for fit_epochs, defaulted, given, want in ((500, True, None, 100), (200, False, None, 66), (2, False, None, 1), (500, True, 7, 7)):
        with pytest.raises(Stop):
            UmapResult(None, 0.58, 1.33, fit_epochs, None, n_epochs_defaulted=defaulted, **state).transform(np.zeros((3, 8)), n_epochs=given)
        assert seen[-1] == want

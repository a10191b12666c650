"""CPU tests of the device-side UMAP's host half: the fp64 oracle (``tests/umap_oracle.py``) against numpy / scipy /
scikit-learn and against ``tests/golden/umap_golden.npz``, the numpy ``find_ab_params``, the validation paths of
``pti_umap_knn`` / ``pti_umap_graph`` / ``pti_umap_epoch`` that return before any launch, and the ``backend`` /
``--umap-backend`` plumbing of ``LatentSpaceAnalyzer`` and ``analyze_static``."""
import argparse
import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch

import umap_oracle as O


@pytest.fixture(scope="module")
def gold():
    return np.load(O.GOLDEN)


@pytest.fixture(scope="module")
def inputs():
    """name -> fp32 distances; computed once, never written to."""
    out = {}
    for name in O.CASES:
        out[name] = O.distances(O.make_rows(name))
        out[name].setflags(write=False)
    return out


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CASES))
def test_oracle_knn_equals_a_stable_argsort(inputs, name):
    dist, k = inputs[name], O.CASES[name][1]
    idx, kd = O.knn(dist, k)
    want = np.argsort(dist, axis=1, kind="stable")[:, :k]
    assert idx.dtype == np.int32 and kd.dtype == np.float32 and idx.shape == kd.shape == (len(dist), k)
    assert np.array_equal(idx, want) and np.array_equal(kd, np.take_along_axis(dist, want, axis=1))
    if name == "n97dup":                                    # zero distances and exact ties, decided by the column
        assert np.array_equal(idx[:3, :3], [[0, 1, 2]] * 3) and not kd[:3, :3].any()
        ties = (kd[:, 1:] == kd[:, :-1]) & (kd[:, 1:] > 0)
        assert ties.any() and (idx[:, 1:][ties] > idx[:, :-1][ties]).all()
    if name in ("n700hub", "n1030k40"):                     # the origin is every other row's nearest neighbour
        assert (idx[1:, 1] == 0).all()


@pytest.mark.parametrize("min_dist,want", [(0.5, (0.58303, 1.33417)), (0.1, (1.57694, 0.89506))])
def test_find_ab_params(min_dist, want):
    from pti_ldm_vae_amd.analysis.latent_space import find_ab_params
    assert O.find_ab_params is find_ab_params
    a, b = find_ab_params(1.0, min_dist)
    assert (round(a, 5), round(b, 5)) == want
    optimize = pytest.importorskip("scipy.optimize")
    x = np.linspace(0.0, 3.0, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist)))
    (sa, sb), _ = optimize.curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
    print(f"min_dist {min_dist}: a {a:.9f} (scipy {sa:.9f}), b {b:.9f} (scipy {sb:.9f})")
    assert abs(a - sa) <= 1e-6 * sa and abs(b - sb) <= 1e-6 * sb


def test_find_ab_params_needs_no_scipy(monkeypatch):
    from pti_ldm_vae_amd.analysis.latent_space import find_ab_params
    for name in [m for m in sys.modules if m == "scipy" or m.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "scipy", None)
    assert round(find_ab_params(1.0, 0.5)[0], 5) == 0.58303


def test_oracle_trustworthiness_equals_sklearn():
    manifold = pytest.importorskip("sklearn.manifold")
    rows = O.make_rows("n300k40").astype(np.float64)        # fp64 on both sides: no ties made by rounding
    rng = np.random.default_rng(3)
    for y in (O.pca_init(rows).astype(np.float64), rng.normal(size=(300, 2)), rows[:, :2]):
        for k in (5, 15):
            assert abs(O.trustworthiness(rows, y, k) - manifold.trustworthiness(rows, y, n_neighbors=k)) <= 1e-12


@pytest.mark.parametrize("name", ["n97dup", "n300k40", "n700hub"])
def test_schedule_fires_each_edge_in_proportion_to_its_weight(name):
    n_epochs = O.CASES[name][2]
    g = O.case_graph(name)[3]
    fired = sum(O.fires(g.rate, e).astype(np.int64) for e in range(n_epochs))
    assert np.array_equal(fired, (n_epochs * g.rate.astype(np.int64)) >> 20)           # the schedule telescopes
    want = np.floor(n_epochs * g.weights.astype(np.float64) / g.wmax)
    assert np.abs(fired - want).max() <= 1 and fired.min() >= 1 and fired.max() == n_epochs
    assert g.rate.max() == 1 << 20 and g.rate.min() >= (1 << 20) // n_epochs


def test_oracle_graph_is_what_it_says(inputs):
    name = "n97dup"
    _, k, n_epochs, _ = O.CASES[name]
    idx, kd = O.knn(inputs[name], k)
    g = O.fuzzy_graph(idx, kd, n_epochs)
    n = len(idx)
    assert g.rho[0] > 0 and g.rho[0] == kd[0][kd[0] > 0][0] and kd[0, 2] == 0            # rho skips the zero distances
    dd = kd[:, 1:].astype(np.float64) - g.rho[:, None]
    psum = np.where(dd > 0, np.exp(-dd / g.sigma[:, None]), 1.0).sum(axis=1)
    floored = g.sigma <= 1e-3 * kd.astype(np.float64).mean(axis=1) * (1 + 1e-12)
    assert (np.abs(psum - np.log2(k)) < 1e-5)[~floored].all() and (~floored).sum() > n // 2
    w = np.zeros((n, n))
    w[g.row, g.indices] = g.weights
    assert np.array_equal(w, w.T) and not w.diagonal().any() and g.wmax == 1.0
    assert (np.diff(g.indptr) > 0).all() and all((np.diff(g.indices[s:e]) > 0).all() for s, e in zip(g.indptr[:-1], g.indptr[1:]))
    assert g.weights.min() >= 1.0 / n_epochs and np.array_equal(g.rate, O.rates(g.weights, np.float32(g.wmax)))


def test_oracle_hub_rows_are_long():
    for name, length in (("n700hub", 699), ("n1030k40", 1029)):
        g = O.case_graph(name)[3]
        assert g.indptr[1] - g.indptr[0] == length and np.array_equal(g.indices[:length], np.arange(1, length + 1))


def test_oracle_reproduces_the_golden_file(gold):
    a, b = O.find_ab_params(1.0, O.MIN_DIST)
    assert np.allclose(gold["ab"], [a, b], rtol=1e-12, atol=0) and np.array_equal(O.make_rows("n97dup"), gold["rows_n97dup"])
    for name in O.CASES:
        for key in ("sigma", "w"):
            tol, f32, bound = (float(gold[f"{key}_{kind}_{name}"]) for kind in ("dev_tol", "dev_fp32", "bound"))
            assert bound == 2.0 * max(tol, f32) and bound < 1e-5
        assert float(gold[f"thr_gap_{name}"]) > float(gold[f"w_bound_{name}"])            # the sparsity pattern is decidable
    for name in ("n3k2", "n97dup", "n300k40"):
        again = O.graph_bounds(name)
        for key, value in again.items():
            assert np.allclose(value, gold[key], rtol=1e-6, atol=1e-12), key
    name = "n97dup"
    again = O.epoch_bounds(name, a, b)
    assert np.array_equal(again[f"y0_{name}"], gold[f"y0_{name}"])
    assert O.span_dev(again[f"y1_{name}"], gold[f"y1_{name}"]) <= 1e-12 and O.span_dev(again[f"y10_{name}"], gold[f"y10_{name}"]) <= 1e-6
    for stop in (1, 10):
        for name in O.EPOCH_CASES:
            assert float(gold[f"epoch_bound_{stop}_{name}"]) == 2.0 * float(gold[f"epoch_fp32_dev_{stop}_{name}"]) > 0
    assert np.isclose(again["restart_bound_n97dup"], float(gold["restart_bound_n97dup"]), rtol=1e-3)
    # the quality gate: the start and the Jacobi layout are recomputed here, the sequential sweeps (minutes) are not
    rows, n_epochs = O.make_rows("n300k40"), O.CASES["n300k40"][2]
    y0 = O.pca_init(rows)
    assert np.isclose(O.trustworthiness(rows, y0), float(gold["trust_start"]), rtol=1e-9)
    t_jacobi = O.trustworthiness(rows, O.layout_jacobi(O.case_graph("n300k40")[3], y0, a, b, n_epochs, O.SEED))
    assert abs(t_jacobi - float(gold["trust_jacobi"])) <= float(gold["trust_margin"])
    assert float(gold["trust_margin"]) == 3.0 * np.ptp(gold["trust_seq_seeds"]) and 0 < float(gold["trust_margin"]) < 0.01
    gate = min(float(gold["trust_seq"]), float(gold["trust_jacobi"])) - float(gold["trust_margin"])
    assert gate > float(gold["trust_start"]) + 0.05                                        # the gate tells a layout from its start


def test_sequential_reference_moves_like_the_jacobi_epoch_on_one_edge():
    """Two vertices, one mirrored edge of weight 1, no negative samples: both sweeps attract; the in-place sweep sees the
    first move when it handles the mirrored edge, the buffered one does not."""
    g = O.Graph(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.ones(2, np.float32), np.full(2, 1 << 20, np.int32),
                None, None, 1.0, np.array([0, 1], np.int32))
    y0 = np.array([[0.0, 0.0], [3.0, 4.0]])
    a, b = 0.583, 1.334
    jac = O.epoch_jacobi(g, y0, a, b, 1.0, 0, 1, nsr=0)
    seq = O.layout_sequential(g, y0, a, b, 1, 1, nsr=0)
    pw = 25.0 ** b
    move = -2 * a * b * (pw / 25.0) / (a * pw + 1.0) * np.array([-3.0, -4.0])
    assert np.allclose(jac, y0 + 2 * np.array([move, -move]), rtol=1e-12)
    assert np.allclose(seq[0] - y0[0], -(seq[1] - y0[1]), rtol=1e-12) and 0 < seq[0, 0] < 1.5 and np.all(jac[0] > y0[0])


# ---- the C entry points ----------------------------------------------------------------------------------------------------
def test_c_entry_points_validate_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    cap, ws = h.pti_umap_graph_capacity, h.pti_umap_graph_ws_floats
    assert cap(300, 40) == 2 * 300 * 40 and cap(300, 200) == 300 * 300 and cap(3, 2) == 9 and cap(8192, 256) == 2 * 8192 * 256
    assert ws(97, 15) == 2 * 98 + 97 * 97 + 4 * 4 + 1 + 97 and ws(8192, 256) == 2 * 8193 + 8192 * 8192 + 256 * 256 + 1 + 8192
    for bad in ((2, 2), (3, 3), (300, 1), (300, 257), (8193, 40), (0, 0), (-5, 2)):
        assert cap(*bad) == 0 and ws(*bad) == 0, bad
    p, q, r = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)              # never dereferenced: refused first
    err = h.pti_last_error_string
    knn = h.pti_umap_knn
    for bad in (0, 4, 5):
        args = [p, 8, 8, 3, q, r, None]
        args[bad] = None
        assert knn(*args) == -1 and b"null" in err()
    for n, k in ((2, 2), (0, 2), (8, 8), (8, 1), (300, 300)):
        assert knn(p, 300, n, k, q, r, None) == -1 and b"dimension" in err(), (n, k)
    for n, k in ((8193, 40), (300, 257)):
        assert knn(p, 9000, n, k, q, r, None) == -2 and b"shape" in err()
    assert knn(p, 7, 8, 3, q, r, None) == -1 and b"stride" in err()
    graph = h.pti_umap_graph
    good = [p, q, 8, 3, 200, r, r, r, r, 48, r, r, r, None]
    for bad in (0, 1, 5, 6, 7, 8, 10, 11, 12):
        args = list(good)
        args[bad] = None
        assert graph(*args) == -1 and b"null" in err()
    for n, k in ((2, 2), (8, 8), (8, 1)):
        args = list(good)
        args[2], args[3] = n, k
        assert graph(*args) == -1 and b"dimension" in err()
    for n, k, cap_ in ((8193, 40, 1 << 30), (300, 257, 1 << 30)):
        args = list(good)
        args[2], args[3], args[9] = n, k, cap_
        assert graph(*args) == -2 and b"shape" in err()
    for n_epochs, rc in ((0, -1), (-3, -1), (2001, -2)):
        args = list(good)
        args[4] = n_epochs
        assert graph(*args) == rc and b"n_epochs" in err()
    args = list(good)
    args[9] = 47
    assert graph(*args) == -1 and b"capacity" in err()
    args = list(good)
    args[12] = C.c_void_p(1028)
    assert graph(*args) == -1 and b"aligned" in err()
    epoch = h.pti_umap_epoch
    good = [p, q, r, 48, 8, 2, q, r, 0.58, 1.33, 1.0, 0, 42, 5, None]
    for bad in (0, 1, 2, 6, 7):
        args = list(good)
        args[bad] = None
        assert epoch(*args) == -1 and b"null" in err()
    for pos, value, rc, text in ((4, 2, -1, b"dimension"), (4, 8193, -2, b"shape"), (5, 3, -2, b"n_components"), (3, 65, -1, b"capacity"),
                                 (3, -1, -1, b"capacity"), (11, -1, -1, b"epoch"), (11, 2000, -2, b"epoch"), (13, -1, -1, b"negative_sample_rate"),
                                 (13, 65, -1, b"negative_sample_rate"), (8, 0.0, -1, b"positive"), (9, float("nan"), -1, b"positive")):
        args = list(good)
        args[pos] = value
        assert epoch(*args) == rc and text in err(), (pos, value)
    args = list(good)
    args[7] = q
    rc = epoch(*args)
    assert rc == -1 and b"double buffered" in err()
    with pytest.raises(_lib.PtiError):
        _lib.check(rc, "umap_epoch")


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from pti_ldm_vae_amd import ops
    d, idx, kd, y = torch.rand(8, 8), torch.zeros(8, 3, dtype=torch.int32), torch.rand(8, 3), torch.rand(8, 2)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_knn(d, 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_knn(d.numpy(), 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_graph(idx, kd, 200)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_graph(idx.numpy(), kd, 200)
    g = ops.UmapGraph(torch.zeros(9, dtype=torch.int32), idx.flatten(), kd.flatten(), idx.flatten(), None, None, None)
    with pytest.raises(ValueError, match="CUDA"):
        ops.umap_epoch(g, y, y.clone(), a=0.58, b=1.33, alpha=1.0, epoch=0, seed=1)


def test_umap_knn_refuses_an_out_tuple_of_the_wrong_length():
    """The length of ``out=(knn_idx, knn_dist)`` is checked before anything else, so no device is needed."""
    from pti_ldm_vae_amd import ops
    for out in ((None,), (None, None, None)):
        with pytest.raises(ValueError, match=r"umap_knn: out must be \(knn_idx, knn_dist\)"):
            ops.umap_knn(torch.rand(8, 8), 3, out=out)


# ---- API and CLI -------------------------------------------------------------------------------------------------------------
ARGV = ["--vae-weights", "w.pth", "--config-file", "c.json", "--folder-edente", "e"]


def test_parse_args_umap_backend():
    from pti_ldm_vae_amd import analyze_static
    plain = analyze_static.parse_args(ARGV)
    assert "umap_backend" not in vars(plain) and plain.umap_backend == "umap-learn"
    a = analyze_static.parse_args(ARGV + ["--umap-backend", "hip"])
    assert (a.method, a.umap_backend) == ("umap", "hip") and vars(a)["umap_backend"] == "hip" and "tsne_backend" not in vars(a)
    assert analyze_static.parse_args(ARGV + ["--umap-backend", "umap-learn"]).umap_backend == "umap-learn"
    with pytest.raises(SystemExit):
        analyze_static.parse_args(ARGV + ["--umap-backend", "cuml"])


def _analyzer():
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    return LatentSpaceAnalyzer(torch.nn.Identity(), torch.device("cpu"), None)


def test_backend_is_validated():
    an, x = _analyzer(), np.zeros((60, 64), dtype=np.float32)
    with pytest.raises(ValueError, match="backend must be 'umap-learn' or 'hip', got 'nope'"):
        an.reduce_dimensionality_umap(x, backend="nope")
    with pytest.raises(ValueError, match="n_components=2 only"):
        an.reduce_dimensionality_umap(x, n_components=3, backend="hip")
    with pytest.raises(ValueError, match=r"n_neighbors \(40\) must be < n_samples \(20\)"):     # today's checks come first
        an.reduce_dimensionality_umap(x[:20], pca_components=5, backend="hip")
    with pytest.raises(ValueError, match="Need at least 50 samples"):
        an.reduce_dimensionality_umap(x[:20], backend="hip")
    for kw in (dict(n_neighbors=1), dict(n_epochs=2001), dict(n_epochs=0)):
        with pytest.raises(ValueError, match="backend='hip' needs 2 <= n_neighbors <= 256"):
            an.reduce_dimensionality_umap(x, backend="hip", **kw)
    with pytest.raises(ValueError, match="backend='hip' needs"):
        an.reduce_dimensionality_umap(np.zeros((300, 64), dtype=np.float32), n_neighbors=257, backend="hip")


def test_umap_learn_backend_is_reached_as_before(monkeypatch):
    calls = []

    class UMAP:
        def __init__(self, **kw):
            calls.append(kw)

        def fit_transform(self, x):
            calls.append(x)
            return x[:, :2] * 2.0

    module = types.ModuleType("umap")
    module.UMAP = UMAP
    an = _analyzer()
    pca = np.arange(60.0 * 50).reshape(60, 50)
    monkeypatch.setattr(an, "reduce_dimensionality_pca", lambda x, k: (pca[:, :k], None))
    monkeypatch.setattr(an, "_umap_device", lambda *a: pytest.fail("the device path was taken"))
    x = np.zeros((60, 64), dtype=np.float32)
    monkeypatch.setitem(sys.modules, "umap", None)                             # the default keeps its ImportError
    with pytest.raises(ImportError, match="Please install umap-learn: pip install umap-learn"):
        an.reduce_dimensionality_umap(x)
    monkeypatch.setitem(sys.modules, "umap", module)
    for kw in ({}, {"backend": "umap-learn", "n_epochs": 7}):
        calls.clear()
        out, model = an.reduce_dimensionality_umap(x, n_neighbors=11, min_dist=0.3, random_state=5, **kw)
        assert calls[0] == dict(n_components=2, random_state=5, n_neighbors=11, min_dist=0.3) and isinstance(model, UMAP)
        assert np.array_equal(calls[1], pca) and np.array_equal(out, pca[:, :2] * 2.0)


def test_umap_init_is_the_leading_pair_scaled_to_ten():
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    pca = np.random.default_rng(0).standard_normal((40, 7)) * np.array([9, 5, 3, 2, 1, 1, 1.0])
    y = LatentSpaceAnalyzer.umap_init(pca)
    assert y.dtype == np.float32 and y.shape == (40, 2) and np.array_equal(y, O.scale_init(pca[:, :2]))
    assert (y.min(axis=0) == 0).all() and (y.max(axis=0) == 10).all()
    assert np.array_equal(np.argsort(y[:, 1]), np.argsort(pca[:, 1].astype(np.float32)))
    flat = LatentSpaceAnalyzer.umap_init(np.ones((5, 1)))
    assert flat.shape == (5, 2) and not flat.any()


def test_project_passes_the_backend_and_keeps_the_fallback(capsys):
    from pti_ldm_vae_amd import analyze_static
    seen = []

    class Fake:
        def reduce_dimensionality_umap(self, latents, **kw):
            seen.append(kw)
            if kw["backend"] == "umap-learn":
                raise ImportError("Please install umap-learn: pip install umap-learn")
            return np.zeros((len(latents), 2)), None

        def reduce_dimensionality_pca(self, latents, k):
            return np.ones((len(latents), k)), np.array([0.5, 0.25])

    latents = np.zeros((70, 8), dtype=np.float32)
    args = analyze_static.parse_args(ARGV + ["--umap-backend", "hip", "--n-neighbors", "9", "--min-dist", "0.2", "--seed", "3"])
    assert analyze_static.project(Fake(), latents, args)[1] == "umap"
    assert seen[-1] == dict(n_neighbors=9, min_dist=0.2, random_state=3, pca_components=50, backend="hip")
    assert "[WARN]" not in capsys.readouterr().out
    for args in (analyze_static.parse_args(ARGV), argparse.Namespace(method="umap", n_neighbors=40, min_dist=0.5, seed=42)):
        assert analyze_static.project(Fake(), latents, args)[1] == "pca" and seen[-1]["backend"] == "umap-learn"
        assert ("[WARN] --method umap is not available (Please install umap-learn: pip install umap-learn); falling back to "
                "--method pca") in capsys.readouterr().out

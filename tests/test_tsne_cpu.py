"""CPU tests of the exact t-SNE: the fp64 oracle (``tests/tsne_oracle.py``) against scikit-learn's own functions and against
``tests/golden/tsne_golden.npz``, the validation paths of ``pti_tsne_affinities`` / ``pti_tsne_step`` that return before any
launch, and the ``backend`` / ``--tsne-backend`` plumbing of ``LatentSpaceAnalyzer`` and ``analyze_static``."""
import argparse
import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch

import tsne_oracle as O


@pytest.fixture(scope="module")
def gold():
    return np.load(O.GOLDEN)


@pytest.fixture(scope="module")
def inputs():
    """name -> (fp32 squared distances, perplexity)."""
    return {name: (O.squared_distances(O.make_rows(name)), case[1]) for name, case in O.CASES.items()}


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CASES))
def test_oracle_joint_probabilities_equal_sklearn(inputs, name):
    pytest.importorskip("sklearn")
    from sklearn.manifold import _t_sne
    d2, perplexity = inputs[name]
    want = _t_sne._joint_probabilities(d2, perplexity, 0)
    got = O.condensed(O.joint_probabilities(d2, perplexity))
    err = O.rel_dev(got, want)
    print(f"[{name}] oracle P vs sklearn: {err:.2e} of max P")
    assert got.shape == want.shape and err <= 1e-12
    if name == "n97dup":                                    # zero distances, the outlier's underflowing row
        assert d2[0, 1] == 0 and d2[1, 2] == 0 and np.delete(d2[3], 3).min() > 1e7
        assert np.exp(-np.float64(d2[3, 0])) == 0.0         # beta = 1 gives a row sum of 0: the 1e-8 branch is taken


@pytest.mark.parametrize("name,scale,exag", [c for c in O.STEP_CASES if c[0] == "n97"] + [("n300", 10.0, 12.0)])
def test_oracle_kl_and_gradient_equal_sklearn(inputs, name, scale, exag):
    pytest.importorskip("sklearn")
    from sklearn.manifold import _t_sne
    d2, perplexity = inputs[name]
    p = O.joint_probabilities(d2, perplexity)
    y = O.step_embedding(name, scale).astype(np.float64)
    want_kl, want_grad = _t_sne._kl_divergence(y.ravel(), O.condensed(p) * exag, 1, len(y), 2)
    kl, grad = O.kl_and_grad(p, y, exag)
    print(f"[{name} {scale:g} {exag:g}] KL {kl:.12g} vs {want_kl:.12g}, gradient {O.rel_dev(grad.ravel(), want_grad):.2e}")
    assert abs(kl - want_kl) <= 1e-12 * abs(want_kl) and O.rel_dev(grad.ravel(), want_grad) <= 1e-12


def test_oracle_reproduces_the_golden_file(gold, inputs):
    assert np.array_equal(O.make_rows("n97"), gold["rows_n97"])
    for name, (d2, perplexity) in inputs.items():
        p = O.joint_probabilities(d2, perplexity)
        n = len(p)
        assert np.array_equal(p, p.T) and not p.diagonal().any() and abs(p.sum() - 1.0) <= 1e-12 + n * n * O.EPS   # the clamp adds
        assert np.allclose([p.sum(), (p * np.arange(n)[:, None]).sum(), p.max()], gold[f"p_checksum_{name}"], rtol=1e-10, atol=0)
        if f"p_{name}" in gold.files:
            assert O.rel_dev(p, gold[f"p_{name}"]) <= 1e-12
        tol, f32, bound = (float(gold[f"aff_{k}_{name}"]) for k in ("dev_tol", "dev_fp32", "bound"))
        assert bound == 2.0 * max(tol, f32) and 0 < tol < 1e-4
    d2, perplexity = inputs["n97"]
    p = O.joint_probabilities(d2, perplexity)
    assert np.isclose(O.rel_dev(p, O.joint_probabilities(d2, perplexity, tol=1e-10)), float(gold["aff_dev_tol_n97"]), rtol=1e-6)
    for name, scale, exag in O.STEP_CASES:
        tag = f"{name}_{scale:g}_{exag:g}"
        assert float(gold[f"step_bound_{tag}"]) == 2.0 * gold[f"step_fp32_dev_{tag}"].max()
        if name != "n97":
            continue
        n = O.CASES[name][0]
        kl, norm, y1, upd, gains = O.one_step(p.astype(np.float32), O.step_embedding(name, scale), np.zeros((n, 2)), np.ones((n, 2)),
                                              exag, 0.5, O.learning_rate(n))
        assert np.isclose(kl, float(gold[f"step_kl_{tag}"]), rtol=1e-10) and np.isclose(norm, float(gold[f"step_norm_{tag}"]), rtol=1e-10)
        assert O.rel_dev(upd, gold[f"step_update_{tag}"]) <= 1e-10 and (gains == 0.8).all()
    # the short trajectory across the switch of momentum and exaggeration
    d2, perplexity = inputs["n300"]
    p = O.joint_probabilities(d2, perplexity)
    assert O.rel_dev(O.pca_init(O.make_rows("n300")), gold["y0_n300"]) <= 1e-5
    y10, kl10, iters = O.descend(p, gold["y0_n300"], max_iter=10, exploration_n_iter=5)
    assert iters == 10 and O.rel_dev(y10, gold["y10_n300"]) <= 1e-9
    assert np.isclose(kl10, O.kl_and_grad(p, y10)[0], rtol=1e-12)
    assert 0 < float(gold["kl_spread_n300"]) < 0.05 and int(gold["iters_full_n300"]) == 1000
    assert np.isclose(float(gold["kl_spread_n300"]), np.ptp(gold["kl_perturbed_n300"]) / float(gold["kl_full_n300"]), rtol=1e-12)


def test_oracle_stopping_rule():
    """Every 50 iterations: stop when KL has not improved for more than the patience."""
    d2 = O.squared_distances(O.make_rows("n97"))
    p = O.joint_probabilities(d2, 30.0)
    y0 = O.pca_init(O.make_rows("n97"))
    assert O.descend(p, y0, max_iter=120, exploration_n_iter=20)[2] == 120
    assert O.learning_rate(97) == 50.0 and O.learning_rate(6000) == 125.0


# ---- the C entry points ----------------------------------------------------------------------------------------------------
def test_c_entry_points_validate_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    aws, sws = h.pti_tsne_affinities_ws_floats, h.pti_tsne_step_ws_floats
    assert aws(97) == 2 * (97 + 2 * 4 * 4) and aws(2) == 2 * (2 + 2) and aws(8192) == 2 * (8192 + 2 * 256 * 256)
    assert sws(97, 2) == 2 * (97 * 4 + 25 * 2 + 2)                           # 25 row blocks, one chunk, two update blocks
    assert sws(6000, 2) == 2 * (3 * 6000 * 4 + 3 * 1500 * 2 + 94)            # the columns split into 3 chunks
    assert sws(200, 2) == 2 * (200 * 4 + 50 * 2 + 4) and sws(8192, 2) == 2 * (2 * 8192 * 4 + 2 * 2048 * 2 + 128)
    for bad in (1, 0, -5, 8193):
        assert aws(bad) == 0 and sws(bad, 2) == 0, bad
    for comps in (1, 3, 0):
        assert sws(100, comps) == 0
    p, q, r = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)              # never dereferenced: refused first
    aff = h.pti_tsne_affinities
    for bad in (0, 4, 6, 7):
        args = [p, 8, 8, 3.0, q, 8, r, r, None]
        args[bad] = None
        assert aff(*args) == -1 and b"null" in h.pti_last_error_string()
    for n in (1, 0, -3):
        assert aff(p, 8, n, 0.5, q, 8, r, r, None) == -1 and b"dimension" in h.pti_last_error_string()
    assert aff(p, 9000, 8193, 30.0, q, 9000, r, r, None) == -2 and b"shape" in h.pti_last_error_string()
    for perplexity in (8.0, 30.0, 0.0, -1.0, float("nan")):
        assert aff(p, 8, 8, perplexity, q, 8, r, r, None) == -1 and b"perplexity" in h.pti_last_error_string()
    for ldd, ldp in ((7, 8), (8, 7)):
        assert aff(p, ldd, 8, 3.0, q, ldp, r, r, None) == -1 and b"stride" in h.pti_last_error_string()
    assert aff(p, 8, 8, 3.0, q, 8, C.c_void_p(1028), r, None) == -1 and b"aligned" in h.pti_last_error_string()
    assert aff(p, 8, 8, 3.0, p, 8, r, r, None) == -1 and b"must not be d2" in h.pti_last_error_string()
    step = h.pti_tsne_step
    good = [p, 8, 8, 2, q, r, q, q, r, 12.0, 0.5, 50.0, r, 1, r, None]
    for bad in (0, 4, 5, 6, 7, 8, 12, 14):
        args = list(good)
        args[bad] = None
        assert step(*args) == -1 and b"null" in h.pti_last_error_string()
    for n in (1, 0):
        args = list(good)
        args[2] = n
        assert step(*args) == -1 and b"dimension" in h.pti_last_error_string()
    for comps in (1, 3):
        args = list(good)
        args[3] = comps
        assert step(*args) == -2 and b"n_components" in h.pti_last_error_string()
    args = list(good)
    args[1], args[2] = 9000, 8193
    assert step(*args) == -2 and b"shape" in h.pti_last_error_string()
    args = list(good)
    args[1] = 7
    assert step(*args) == -1 and b"stride" in h.pti_last_error_string()
    args = list(good)
    args[9] = 0.0
    assert step(*args) == -1 and b"exaggeration" in h.pti_last_error_string()
    args = list(good)
    args[12] = C.c_void_p(1028)
    assert step(*args) == -1 and b"aligned" in h.pti_last_error_string()
    args = list(good)
    args[5] = q
    rc = step(*args)
    assert rc == -1 and b"double buffered" in h.pti_last_error_string()
    with pytest.raises(_lib.PtiError):
        _lib.check(rc, "tsne_step")


def test_ops_refuse_cpu_tensors():
    from pti_ldm_vae_amd import ops
    d2, y, rec = torch.rand(8, 8), torch.rand(8, 2), torch.zeros(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        ops.tsne_affinities(d2, 3.0)
    with pytest.raises(ValueError, match="CUDA"):
        ops.tsne_affinities(d2.numpy(), 3.0)
    with pytest.raises(ValueError, match="CUDA"):
        ops.tsne_step(d2, y, y.clone(), y.clone(), y.clone(), rec, sums=rec.clone(), exaggeration=12.0, momentum=0.5, lr=50.0)


# ---- API and CLI -------------------------------------------------------------------------------------------------------------
ARGV = ["--vae-weights", "w.pth", "--config-file", "c.json", "--folder-edente", "e"]


def test_parse_args_tsne_backend():
    from pti_ldm_vae_amd import analyze_static
    assert analyze_static.parse_args(ARGV).tsne_backend == "sklearn"
    a = analyze_static.parse_args(ARGV + ["--method", "tsne", "--tsne-backend", "hip"])
    assert (a.method, a.tsne_backend) == ("tsne", "hip") and vars(a)["tsne_backend"] == "hip"
    assert analyze_static.parse_args(ARGV + ["--tsne-backend", "sklearn"]).tsne_backend == "sklearn"
    with pytest.raises(SystemExit):
        analyze_static.parse_args(ARGV + ["--tsne-backend", "cuda"])


def _analyzer():
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    return LatentSpaceAnalyzer(torch.nn.Identity(), torch.device("cpu"), None)


def test_backend_is_validated():
    an, x = _analyzer(), np.zeros((60, 64), dtype=np.float32)
    with pytest.raises(ValueError, match="backend must be 'sklearn' or 'hip', got 'nope'"):
        an.reduce_dimensionality_tsne(x, backend="nope")
    with pytest.raises(ValueError, match="n_components=2 only"):
        an.reduce_dimensionality_tsne(x, n_components=3, backend="hip")
    with pytest.raises(ValueError, match=r"perplexity \(30\) must be < n_samples \(20\)"):     # today's checks come first
        an.reduce_dimensionality_tsne(x[:20], pca_components=5, backend="hip")
    with pytest.raises(ValueError, match="Need at least 50 samples"):
        an.reduce_dimensionality_tsne(x[:20], backend="hip")


def test_sklearn_backend_reaches_tsne_as_before(monkeypatch):
    calls = []

    class TSNE:
        def __init__(self, **kw):
            calls.append(kw)

        def fit_transform(self, x):
            calls.append(x)
            return x[:, :2] * 2.0

    manifold = types.ModuleType("sklearn.manifold")
    manifold.TSNE = TSNE
    package = types.ModuleType("sklearn")
    package.manifold = manifold
    monkeypatch.setitem(sys.modules, "sklearn", package)
    monkeypatch.setitem(sys.modules, "sklearn.manifold", manifold)
    an = _analyzer()
    pca = np.arange(60.0 * 50).reshape(60, 50)
    monkeypatch.setattr(an, "reduce_dimensionality_pca", lambda x, k: (pca[:, :k], None))
    monkeypatch.setattr(an, "_tsne_device", lambda *a: pytest.fail("the device path was taken"))
    x = np.zeros((60, 64), dtype=np.float32)
    for kw in ({}, {"backend": "sklearn", "max_iter": 7, "exploration_n_iter": 3, "early_exaggeration": 4.0}):
        calls.clear()
        out = an.reduce_dimensionality_tsne(x, perplexity=11, random_state=5, **kw)
        assert calls[0] == dict(n_components=2, perplexity=11, init="pca", random_state=5)
        assert calls[1] is not None and np.array_equal(calls[1], pca) and np.array_equal(out, pca[:, :2] * 2.0)


def test_tsne_init_is_the_scaled_leading_pair():
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    pca = np.random.default_rng(0).standard_normal((40, 7)) * np.array([9, 5, 3, 2, 1, 1, 1.0])
    y = LatentSpaceAnalyzer.tsne_init(pca)
    assert y.dtype == np.float32 and y.shape == (40, 2)
    assert np.array_equal(y, (pca[:, :2] / pca[:, 0].std() * 1e-4).astype(np.float32))
    assert abs(float(y[:, 0].astype(np.float64).std()) - 1e-4) <= 1e-10


def test_project_passes_the_backend_and_prints_the_warning_for_sklearn_only(capsys):
    from pti_ldm_vae_amd import analyze_static
    seen = []

    class Fake:
        def reduce_dimensionality_tsne(self, latents, **kw):
            seen.append(kw)
            return np.zeros((len(latents), 2))

    latents = np.zeros((70, 8), dtype=np.float32)
    args = analyze_static.parse_args(ARGV + ["--method", "tsne", "--tsne-backend", "hip", "--perplexity", "9", "--seed", "3"])
    assert analyze_static.project(Fake(), latents, args)[1] == "tsne"
    assert seen[-1] == dict(perplexity=9, random_state=3, pca_components=50, backend="hip")
    assert "few minutes" not in capsys.readouterr().out
    args = analyze_static.parse_args(ARGV + ["--method", "tsne"])
    analyze_static.project(Fake(), latents, args)
    assert seen[-1]["backend"] == "sklearn" and "(This may take a few minutes...)" in capsys.readouterr().out
    bare = argparse.Namespace(method="tsne", perplexity=30, seed=42)          # a namespace built before the option existed
    analyze_static.project(Fake(), latents, bare)
    assert seen[-1]["backend"] == "sklearn"

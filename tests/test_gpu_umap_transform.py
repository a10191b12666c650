"""GPU tests of the device-side UMAP transform (csrc/umap.hip): ``ops.umap_knn_cross`` /
``ops.umap_transform_graph`` / ``ops.umap_transform_layout`` against the fp64 oracle of ``tests/umap_transform_oracle.py``,
``PcaModel`` against scikit-learn, ``UmapResult.transform`` against the quality gate, its reproducibility, and
``analyze_static --umap-fit-group edente`` end to end.

Every bound comes from ``tests/golden/umap_transform_golden.npz`` and was measured on the CPU by
``umap_transform_oracle.__main__``: twice the deviation of the oracle's own stopping slack or of the plain fp32 numpy
restatement from the fp64 oracle (for a layout at least the half ulp of its fp32 result) -- never from what the kernels
give.  What the kernels gave on MI355X: DESIGN.md 5m."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import umap_transform_oracle as T

pytestmark = pytest.mark.gpu

O = T.O
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(T.GOLDEN)


@pytest.fixture(scope="module")
def oracle():
    """name -> (fp32 cross distances, kNN indices, kNN distances, the frozen embedding, the oracle's transform graph);
    computed once, never written to."""
    out = {}
    for name in T.CASES:
        out[name] = T.case_graph(name)
        for arr in out[name][:4] + tuple(v for v in out[name][4] if isinstance(v, np.ndarray)):
            arr.setflags(write=False)
    return out


def _analyzer(dev):
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    return LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)


def _upload(g, dev):
    """The oracle's transform graph as the device slab ``ops.umap_transform_layout`` reads."""
    from pti_ldm_vae_amd import ops
    return ops.UmapTransformGraph(torch.tensor(g.indices, device=dev), torch.tensor(g.w32, device=dev), torch.tensor(g.rate, device=dev),
                                  torch.tensor(g.sigma.astype(np.float32), device=dev), torch.tensor(g.y0, device=dev))


def _layout(tg, yt, y_in, ab, n_epochs, seed=T.SEED, **kw):
    from pti_ldm_vae_amd import ops
    y_out = torch.empty_like(y_in)
    ops.umap_transform_layout(tg, yt, y_in, y_out, a=ab[0], b=ab[1], n_epochs=n_epochs, seed=seed, **kw)
    return y_out


# ---- 1. neighbours -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CASES))
def test_knn_cross_equals_the_oracle(oracle, dev, name):
    from pti_ldm_vae_amd import ops
    dist, want_idx, want_kd = oracle[name][:3]
    idx, kd = ops.umap_knn_cross(torch.tensor(dist, device=dev), T.CASES[name][2])
    assert idx.dtype == torch.int32 and kd.dtype == torch.float32 and tuple(idx.shape) == tuple(kd.shape) == want_idx.shape
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kd.cpu().numpy(), want_kd)


def test_knn_cross_strided_out_and_few_rows(oracle, dev):
    from pti_ldm_vae_amd import ops
    dist, want_idx, want_kd = oracle["t97"][:3]
    buf = torch.full((30, 128), -1.0, device=dev)
    buf[:, :70] = torch.tensor(dist, device=dev)
    out = (torch.empty(30, 15, dtype=torch.int32, device=dev), torch.empty(30, 15, device=dev))
    idx, kd = ops.umap_knn_cross(buf[:, :70], 15, out=out)
    assert idx.data_ptr() == out[0].data_ptr() and kd.data_ptr() == out[1].data_ptr()
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kd.cpu().numpy(), want_kd)
    for m in (1, 5):                                                           # fewer rows than a workgroup of the later stages holds
        idx, kd = ops.umap_knn_cross(buf[:m, :70], 15)
        assert np.array_equal(idx.cpu().numpy(), want_idx[:m]) and np.array_equal(kd.cpu().numpy(), want_kd[:m])


# ---- 2. graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_epochs", [(name, T.CASES[name][3]) for name in T.CASES] + [("t97", T.T_SHORT["t97"])])
def test_transform_graph_against_the_oracle(gold, oracle, dev, name, n_epochs):
    from pti_ldm_vae_amd import ops
    _, idx, kd, yt, g = oracle[name]
    if n_epochs != T.CASES[name][3]:
        g = T.transform_graph(idx, kd, yt, n_epochs)
    knn_idx = torch.tensor(idx, device=dev)
    got = ops.umap_transform_graph(knn_idx, torch.tensor(kd, device=dev), torch.tensor(yt, device=dev), n_epochs)
    assert got.indices is knn_idx and tuple(got.weights.shape) == tuple(got.rate.shape) == idx.shape
    sigma, weights, rate, y0 = (t.cpu().numpy() for t in (got.sigma, got.weights, got.rate, got.y0))
    sigma_err, sigma_bound = T.rel_dev(sigma, g.sigma), float(gold[f"sigma_bound_{name}"])
    print(f"[{name} T={n_epochs}] sigma vs fp64 oracle: {sigma_err:.3e} of max sigma (bound {sigma_bound:.3e})")
    assert sigma_err <= sigma_bound
    w_err, w_bound = T.rel_dev(weights, g.weights), float(gold[f"w_bound_{name}"])
    print(f"[{name} T={n_epochs}] weights vs fp64 oracle: {w_err:.3e} of max w (bound {w_bound:.3e}); dropped {(rate == 0).sum()}")
    assert w_err <= w_bound and np.array_equal(weights == 1.0, kd == 0)
    own = np.where(weights.astype(np.float64) * n_epochs >= weights.max(), T.rates(weights, weights.max()), 0)
    assert np.array_equal(rate, own)                                           # from the device's own stored weights
    assert np.array_equal(rate == 0, g.rate == 0) and int((rate == 0).sum()) == int(gold[f"dropped_{n_epochs}_{name}"])
    y0_err, y0_bound = T.tspan_dev(y0, g.y0, yt), float(gold[f"y0_bound_{name}"])
    print(f"[{name} T={n_epochs}] start points vs fp64 oracle: {y0_err:.3e} of the training span (bound {y0_bound:.3e})")
    assert y0_err <= y0_bound and np.array_equal(g.y0, gold[f"y0_{name}"])


# ---- 3. layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.EPOCH_CASES)
def test_layout_against_the_oracle(gold, oracle, dev, name):
    _, _, _, yt, g = oracle[name]
    n_epochs, ab = T.CASES[name][3], gold["ab"]
    tg, yt_dev = _upload(g, dev), torch.tensor(yt, device=dev)
    for stop in (1, 10):
        y = _layout(tg, yt_dev, tg.y0, ab, n_epochs, stop=stop).cpu().numpy()
        err, bound = T.tspan_dev(y, gold[f"y{stop}_{name}"], yt), float(gold[f"epoch_bound_{stop}_{name}"])
        print(f"[{name}] {stop} epoch(s) vs fp64 oracle: {err:.3e} of the training span (bound {bound:.3e})")
        assert np.isfinite(y).all() and err <= bound

    # the same ten epochs one at a time, each from the oracle's trajectory: no dynamics between the comparisons
    def device_epoch(e, y32):
        return _layout(tg, yt_dev, torch.tensor(y32, device=dev), ab, n_epochs, start=e, stop=e + 1).cpu().numpy()

    err, bound = T.restarted_epochs(g, yt, ab[0], ab[1], n_epochs, device_epoch), float(gold[f"restart_bound_{name}"])
    print(f"[{name}] epochs 0-9 one at a time vs fp64 oracle: {err:.3e} of the training span (bound {bound:.3e})")
    assert err <= bound


# ---- 4. bitwise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t97", "t300k200"])
def test_one_launch_is_many_and_in_place_is_out_of_place(gold, oracle, dev, name):
    from pti_ldm_vae_amd import ops
    _, _, _, yt, g = oracle[name]
    n_epochs, ab = 25, gold["ab"]
    tg, yt_dev = _upload(g, dev), torch.tensor(yt, device=dev)
    whole = _layout(tg, yt_dev, tg.y0, ab, n_epochs)
    step = tg.y0
    for e in range(n_epochs):
        step = _layout(tg, yt_dev, step, ab, n_epochs, start=e, stop=e + 1)
    assert torch.equal(step, whole) and not torch.equal(whole, tg.y0)
    y = tg.y0.clone()
    ops.umap_transform_layout(tg, yt_dev, y, y, a=ab[0], b=ab[1], n_epochs=n_epochs, seed=T.SEED)
    assert torch.equal(y, whole)
    head = tg._replace(indices=tg.indices[:5], rate=tg.rate[:5])
    assert torch.equal(_layout(head, yt_dev, tg.y0[:5], ab, n_epochs), whole[:5])
    assert torch.equal(_layout(tg, yt_dev, tg.y0, ab, n_epochs, start=7, stop=7), tg.y0)     # an empty range copies


# ---- 5. indices outside the training rows ----------------------------------------------------------------------------------
def test_layout_skips_indices_outside_the_training_rows(gold, oracle, dev):
    """A slot whose index is no training row never fires: the row moves as if that slot's rate were 0, bit for bit, and a
    row without a valid slot stays where it was."""
    _, idx, _, yt, g = oracle["t97"]
    ab = gold["ab"]
    good, yt_dev = _upload(g, dev), torch.tensor(yt, device=dev)
    bad, rate = idx.copy(), g.rate.copy()
    bad[3], bad[4, ::2], bad[5, 1] = len(yt), -1, 1 << 30
    rate[3], rate[4, ::2], rate[5, 1] = 0, 0, 0
    got = _layout(good._replace(indices=torch.tensor(bad, device=dev)), yt_dev, good.y0, ab, 100, stop=20)
    want = _layout(good._replace(rate=torch.tensor(rate, device=dev)), yt_dev, good.y0, ab, 100, stop=20)
    plain = _layout(good, yt_dev, good.y0, ab, 100, stop=20)
    keep = torch.ones(len(idx), dtype=torch.bool, device=dev)
    keep[[3, 4, 5]] = False
    assert torch.equal(got, want) and torch.equal(got[3], good.y0[3]) and torch.equal(got[keep], plain[keep])
    assert not torch.equal(got[4], plain[4]) and not torch.equal(got[4], good.y0[4])
    oracle_rows = T.layout(bad, g.rate, g.y0, yt, ab[0], ab[1], 100, T.SEED, stop=20)
    assert np.array_equal(oracle_rows[3], g.y0[3]) and np.isfinite(got.cpu().numpy()).all()


# ---- 6. the public path and its quality gate ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(dev):
    train, new = T.split("t300k40")
    y, result = _analyzer(dev).reduce_dimensionality_umap(train, n_neighbors=T.QUALITY_FIT[0], min_dist=O.MIN_DIST,
                                                          n_epochs=T.QUALITY_FIT[1], random_state=T.SEED, backend="hip")
    return train, new, y, result


def test_transform_passes_the_quality_gate(gold, fitted):
    """The share of a new row's 15 nearest training rows that are among its 15 nearest training points in the plane, on
    t300k40 with T = 100 (the case's epoch count; the fit ran 200 epochs, so the default would be 66).  Measured on the CPU
    with the oracle's own fit: 0.750 at the start points, 0.790 .. 0.804 over six seeds, so the gate is 0.790 - 0.014."""
    train, new, y_train, result = fitted
    y = result.transform(new, n_epochs=T.QUALITY_T)
    assert isinstance(y, np.ndarray) and y.shape == (len(new), 2) and y.dtype == np.float64 and np.isfinite(y).all()
    assert np.array_equal(result.embedding_, y_train)                          # the fit is untouched
    share, gate, start = T.neighbour_share(new, train, y, y_train), float(gold["share_gate"]), float(gold["share_start"])
    print(f"neighbour share {share:.4f} (gate {gate:.4f}: oracle seeds {np.round(gold['share_seeds'], 4).tolist()}; start {start:.4f})")
    assert share >= gate and share > start
    # the default: transform(new) runs 200 // 3 = 66 epochs after a fit of 200; its own gate, measured in the same way
    y = result.transform(new)
    share, gate = T.neighbour_share(new, train, y, y_train), float(gold["share_gate_default"])
    print(f"default T = {T.QUALITY_T_DEFAULT}: neighbour share {share:.4f} (gate {gate:.4f}: oracle seeds "
          f"{np.round(gold['share_seeds_default'], 4).tolist()})")
    assert share >= gate and share > start


def test_transform_is_reproducible_and_seeded(fitted, dev):
    _, new, _, result = fitted
    first = result.transform(new)
    second = result.transform(new)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        third = result.transform(new)
        side.synchronize()
    assert np.array_equal(first, second) and np.array_equal(first, third)
    assert np.array_equal(first, result.transform(new, n_epochs=66, random_state=T.SEED))    # the defaults: 200 // 3, the fit's seed
    other = result.transform(new, random_state=7)
    assert not np.array_equal(other, first) and np.isfinite(other).all()
    assert not np.array_equal(result.transform(new, n_epochs=65), first)
    with pytest.raises(ValueError, match="columns of the fit"):
        result.transform(new[:, :49])


# ---- 7. PCA model ------------------------------------------------------------------------------------------------------------
def test_pca_model(gold, dev):
    decomposition = pytest.importorskip("sklearn.decomposition")
    train, new = T.split("t300k40")
    an = _analyzer(dev)
    model = an.fit_pca(train, 50)
    emb, ratio = an.reduce_dimensionality_pca(train, 50)
    assert np.array_equal(model.embedding_, emb) and np.array_equal(model.explained_variance_ratio_, ratio)
    assert model.mean_.shape == (50,) and np.allclose(model.mean_, train.astype(np.float64).mean(axis=0), atol=1e-5)
    ref = decomposition.PCA(n_components=50, svd_solver="full").fit(train.astype(np.float64))
    want_train, want_new = ref.transform(train.astype(np.float64)), ref.transform(new.astype(np.float64))
    flip = np.sign((emb * want_train).sum(axis=0))
    got = model.transform(new)
    bound = float(gold["pca_bound"])
    err_new, err_self = T.rel_dev(got * flip, want_new), T.rel_dev(model.transform(train), emb)
    print(f"PcaModel.transform vs sklearn fp64: {err_new:.3e} of the largest projection; transform(train) vs embedding_: "
          f"{err_self:.3e} (bound {bound:.3e}, fp32 restatement {float(gold['pca_fp32_dev']):.3e})")
    assert got.dtype == np.float64 and got.shape == (len(new), 50) and err_new <= bound and err_self <= bound
    assert np.array_equal(model.transform(torch.tensor(new, device=dev)), got)
    with pytest.raises(ValueError, match="columns of the fit"):
        model.transform(new[:, :10])


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static_runs(dev, tmp_path_factory):
    """The folders, config and checkpoint of the runs below, and ``run(tag, *extra)`` -> (latents.npz of that run, its
    standard output is the caller's to capture)."""
    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import analyze_static
    from test_gpu_latent_analysis import _write_group
    tmp = tmp_path_factory.mktemp("fit_group")
    _write_group(tmp / "edente", ["11", "12", "13"], 4, seed=1)
    _write_group(tmp / "dente", ["12", "13", "11"], 4, seed=2)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64])
    (tmp / "cfg.json").write_text(json.dumps(cfg))
    ck = tmp / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)

    def run(tag, *extra, dente=True):
        out = tmp / tag
        argv = ["--vae-weights", str(ck), "--config-file", str(tmp / "cfg.json"), "--folder-edente", str(tmp / "edente"), "--method",
                "umap", "--umap-backend", "hip", "--n-neighbors", "5", "--patch-size", "64", "64", "--cache-dir", str(tmp / "cache"),
                "--batch-size", "6", "--dpi", "40", "--output-dir", str(out)] + list(extra)
        analyze_static.main(argv + (["--folder-dente", str(tmp / "dente")] if dente else []))
        return out
    return run


def test_analyze_static_fits_on_the_first_group(static_runs, monkeypatch, capsys):
    monkeypatch.setitem(sys.modules, "umap", None)                             # `import umap` raises ImportError
    out = static_runs("edente_fit", "--umap-fit-group", "edente")
    text = capsys.readouterr().out
    assert (out / "umap_projection.png").stat().st_size > 0 and not (out / "pca_projection.png").exists() and "[WARN]" not in text
    assert (out / "distance_metrics.txt").is_file() and (out / "exams_sorted_by_distance.txt").is_file()
    z = np.load(out / "latents.npz")
    assert sorted(z.files) == sorted(f"{key}_{name}" for key in ("latents", "ids", "paths", "projection") for name in ("edente", "dente"))
    assert z["projection_dente"].shape == (12, 2) and np.isfinite(z["projection_dente"]).all()
    # the first group's map is the one it gets alone: the second group did not shape it
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    alone, _ = LatentSpaceAnalyzer(torch.nn.Identity(), torch.device("cuda:0"), None).reduce_dimensionality_umap(
        z["latents_edente"], n_neighbors=5, min_dist=0.5, random_state=42, pca_components=12, backend="hip")
    assert np.array_equal(z["projection_edente"], alone)
    solo = static_runs("edente_alone", "--umap-fit-group", "edente", dente=False)         # one group: the flag changes nothing
    assert (solo / "umap_projection.png").stat().st_size > 0 and not (solo / "latents.npz").exists()
    assert "[WARN]" not in capsys.readouterr().out


def test_analyze_static_without_the_flag_fits_on_all(static_runs, capsys):
    plain, flagged = static_runs("plain"), static_runs("all", "--umap-fit-group", "all")
    assert "[WARN]" not in capsys.readouterr().out
    a, b = np.load(plain / "latents.npz"), np.load(flagged / "latents.npz")
    assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[key], b[key]) for key in a.files)
    for name in ("distance_metrics.txt", "exams_sorted_by_distance.txt"):
        assert (plain / name).read_text() == (flagged / name).read_text()
    fit_first = np.load(static_runs("edente_fit_again", "--umap-fit-group", "edente") / "latents.npz")
    assert not np.array_equal(fit_first["projection_edente"], a["projection_edente"])        # the two fits differ
    assert np.array_equal(fit_first["latents_dente"], a["latents_dente"])


# ---- 9. limits -----------------------------------------------------------------------------------------------------------
def test_shapes_outside_the_limits_raise_before_any_launch(dev):
    from pti_ldm_vae_amd import ops
    for m, n, k in ((0, 300, 40), (8193, 300, 40), (5, 300, 300), (5, 300, 301), (5, 300, 257), (5, 300, 1), (5, 2, 2), (5, 8193, 40)):
        with pytest.raises(ValueError, match="umap_knn_cross: unsupported shape"):
            ops.umap_knn_cross(torch.empty(m, n, device=dev), k)
    for m, n, k in ((0, 300, 40), (8193, 300, 40), (5, 40, 40), (5, 300, 257), (5, 300, 1)):
        with pytest.raises(ValueError, match="umap_transform_graph: unsupported shape"):
            ops.umap_transform_graph(torch.empty(m, k, dtype=torch.int32, device=dev), torch.empty(m, k, device=dev),
                                     torch.empty(n, 2, device=dev), 100)
    idx, kd, yt = torch.zeros(5, 40, dtype=torch.int32, device=dev), torch.zeros(5, 40, device=dev), torch.zeros(300, 2, device=dev)
    for n_epochs in (0, 2001):
        with pytest.raises(ValueError, match=f"n_epochs={n_epochs}"):
            ops.umap_transform_graph(idx, kd, yt, n_epochs)
        with pytest.raises(ValueError, match=f"n_epochs={n_epochs}"):
            ops.umap_transform_layout(ops.UmapTransformGraph(idx, kd, idx, None, None), yt, kd[:, :2].contiguous(),
                                      torch.empty(5, 2, device=dev), a=0.58, b=1.33, n_epochs=n_epochs, seed=1)
    with pytest.raises(TypeError, match="dist"):
        ops.umap_knn_cross(torch.empty(5, 300, dtype=torch.float64, device=dev), 40)
    with pytest.raises(TypeError, match="knn_idx"):
        ops.umap_transform_graph(idx.long(), kd, yt, 100)
    with pytest.raises(TypeError, match="knn_dist"):
        ops.umap_transform_graph(idx, kd.double(), yt, 100)
    with pytest.raises(TypeError, match="y_train"):
        ops.umap_transform_graph(idx, kd, yt.double(), 100)
    with pytest.raises(ValueError, match="only n_components = 2"):
        ops.umap_transform_graph(idx, kd, torch.zeros(300, 3, device=dev), 100)
    tg, y = ops.UmapTransformGraph(idx, kd, idx, None, None), torch.zeros(5, 2, device=dev)
    with pytest.raises(TypeError, match="rate"):
        ops.umap_transform_layout(tg._replace(rate=kd), yt, y, y, a=0.58, b=1.33, n_epochs=100, seed=1)
    with pytest.raises(ValueError, match="y_out must not overlap y_train"):
        ops.umap_transform_layout(tg, yt, y, yt[:5], a=0.58, b=1.33, n_epochs=100, seed=1)
    with pytest.raises(ValueError, match="y_out must not overlap y_train"):
        ops.umap_transform_layout(tg, yt, y, yt[295:], a=0.58, b=1.33, n_epochs=100, seed=1)
    both = torch.zeros(6, 2, device=dev)
    with pytest.raises(ValueError, match="y_in itself or apart"):
        ops.umap_transform_layout(tg, yt, both[:5], both[1:], a=0.58, b=1.33, n_epochs=100, seed=1)
    with pytest.raises(ValueError, match="epochs \\[3, 2\\)"):
        ops.umap_transform_layout(tg, yt, y, y, a=0.58, b=1.33, n_epochs=100, seed=1, start=3, stop=2)
    an = _analyzer(dev)
    _, result = an.reduce_dimensionality_umap(np.random.default_rng(0).normal(size=(60, 64)).astype(np.float32), n_neighbors=10,
                                              n_epochs=3, backend="hip")
    for rows in (0, 8193):
        with pytest.raises(ValueError, match="new rows at once"):
            result.transform(np.zeros((rows, 64), dtype=np.float32))
    for n_epochs in (0, 2001):
        with pytest.raises(ValueError, match="n_epochs"):
            result.transform(np.zeros((4, 64), dtype=np.float32), n_epochs=n_epochs)
    assert result.transform(np.zeros((1, 64), dtype=np.float32)).shape == (1, 2)             # T = max(1, 3 // 3)

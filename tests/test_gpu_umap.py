"""GPU tests of the device-side UMAP (csrc/umap.hip): ``ops.umap_knn`` / ``ops.umap_graph`` / ``ops.umap_epoch`` against the
fp64 oracle of ``tests/umap_oracle.py``, the full run of ``LatentSpaceAnalyzer.reduce_dimensionality_umap(backend="hip")``
against the quality gate, its reproducibility, and ``analyze_static --umap-backend hip`` end to end.

Every bound comes from ``tests/golden/umap_golden.npz`` and was measured on the CPU by ``umap_oracle.__main__``: twice the
deviation of the oracle's own stopping slack or of the plain fp32 numpy restatement from the fp64 oracle -- never from
what the kernels give.  What the kernels gave on MI355X: DESIGN.md 5l."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import umap_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(O.GOLDEN)


@pytest.fixture(scope="module")
def oracle():
    """name -> (fp32 distances, kNN indices, kNN distances, the oracle's graph, its fp64 weights); computed once, never
    written to."""
    out = {}
    for name in O.CASES:
        dist, idx, kd, g = O.case_graph(name)
        w64 = O.dense_weights(idx, kd, g.rho, g.sigma)[g.row, g.indices]
        for arr in (dist, idx, kd, w64) + tuple(v for v in g if isinstance(v, np.ndarray)):
            arr.setflags(write=False)
        out[name] = (dist, idx, kd, g, w64)
    return out


def _analyzer(dev):
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    return LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)


def _upload(g, dev):
    """The oracle's graph as the device CSR ``ops.umap_epoch`` reads."""
    from pti_ldm_vae_amd import ops
    t = [torch.tensor(v, device=dev) for v in (g.indptr, g.indices, g.weights, g.rate, g.rho, g.sigma.astype(np.float32))]
    return ops.UmapGraph(*t, t[0][-1])


def _gate(gold):
    return min(float(gold["trust_seq"]), float(gold["trust_jacobi"])) - float(gold["trust_margin"])


# ---- 1. neighbours -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CASES))
def test_knn_equals_the_oracle(oracle, dev, name):
    from pti_ldm_vae_amd import ops
    dist, want_idx, want_kd = oracle[name][:3]
    idx, kd = ops.umap_knn(torch.tensor(dist, device=dev), O.CASES[name][1])
    assert idx.dtype == torch.int32 and kd.dtype == torch.float32 and tuple(idx.shape) == tuple(kd.shape) == want_idx.shape
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kd.cpu().numpy(), want_kd)


def test_knn_reads_a_strided_matrix_and_writes_out(oracle, dev):
    from pti_ldm_vae_amd import ops
    dist, want_idx, want_kd = oracle["n97dup"][:3]
    buf = torch.full((97, 128), -1.0, device=dev)
    buf[:, :97] = torch.tensor(dist, device=dev)
    out = (torch.empty(97, 15, dtype=torch.int32, device=dev), torch.empty(97, 15, device=dev))
    idx, kd = ops.umap_knn(buf[:, :97], 15, out=out)
    assert idx.data_ptr() == out[0].data_ptr() and kd.data_ptr() == out[1].data_ptr()
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kd.cpu().numpy(), want_kd)


# ---- 2. graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CASES))
def test_graph_against_the_oracle(gold, oracle, dev, name):
    from pti_ldm_vae_amd import ops
    _, idx, kd, g, w64 = oracle[name]
    n, n_epochs = len(idx), O.CASES[name][2]
    got = ops.umap_graph(torch.tensor(idx, device=dev), torch.tensor(kd, device=dev), n_epochs)
    nnz = int(got.nnz)
    indptr, rho, sigma = got.indptr.cpu().numpy(), got.rho.cpu().numpy(), got.sigma.cpu().numpy()
    indices, weights, rate = (t[:nnz].cpu().numpy() for t in (got.indices, got.weights, got.rate))
    assert got.indices.numel() == got.weights.numel() == got.rate.numel() == min(2 * n * idx.shape[1], n * n) >= nnz
    assert np.array_equal(rho, g.rho)
    sigma_err, sigma_bound = O.rel_dev(sigma, g.sigma), float(gold[f"sigma_bound_{name}"])
    print(f"[{name}] sigma vs fp64 oracle: {sigma_err:.3e} of max sigma (bound {sigma_bound:.3e}: stopping slack "
          f"{float(gold[f'sigma_dev_tol_{name}']):.2e}, fp32 restatement {float(gold[f'sigma_dev_fp32_{name}']):.2e})")
    assert sigma_err <= sigma_bound
    assert nnz == g.indptr[-1] and np.array_equal(indptr, g.indptr) and np.array_equal(indices, g.indices)
    w_err, w_bound = O.rel_dev(weights, w64), float(gold[f"w_bound_{name}"])
    print(f"[{name}] weights vs fp64 oracle: {w_err:.3e} of max w (bound {w_bound:.3e}: stopping slack "
          f"{float(gold[f'w_dev_tol_{name}']):.2e}, fp32 restatement {float(gold[f'w_dev_fp32_{name}']):.2e}); nnz {nnz}, "
          f"longest row {np.diff(indptr).max()}")
    assert w_err <= w_bound
    assert np.array_equal(rate, O.rates(weights, weights.max()))              # from the device's own stored weights
    dense = np.zeros((n, n), np.float32)
    dense[g.row, indices] = weights
    assert np.array_equal(dense, dense.T) and not dense.diagonal().any()      # symmetric bit for bit


# ---- 3. epochs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.EPOCH_CASES)
def test_epochs_against_the_oracle(gold, oracle, dev, name):
    from pti_ldm_vae_amd import ops
    g, n_epochs = oracle[name][3], O.CASES[name][2]
    a, b = gold["ab"]
    graph = _upload(g, dev)
    y0 = torch.from_numpy(gold[f"y0_{name}"]).to(dev)
    an = _analyzer(dev)
    for stop in (1, 10):
        y = an.umap_layout(graph, y0, a, b, n_epochs, O.SEED, stop=stop).cpu().numpy()
        err, bound = O.span_dev(y, gold[f"y{stop}_{name}"]), float(gold[f"epoch_bound_{stop}_{name}"])
        print(f"[{name}] {stop} epoch(s) vs fp64 oracle: {err:.3e} of the span (bound {bound:.3e})")
        assert np.isfinite(y).all() and err <= bound

    # the same ten epochs one at a time, each from the oracle's trajectory: no dynamics between the comparisons
    def device_epoch(e, y32):
        y_in = torch.from_numpy(y32).to(dev)
        y_out = torch.empty_like(y_in)
        ops.umap_epoch(graph, y_in, y_out, a=a, b=b, alpha=1.0 - e / n_epochs, epoch=e, seed=O.SEED)
        return y_out.cpu().numpy()

    err, bound = O.restarted_epochs(g, gold[f"y0_{name}"], a, b, n_epochs, device_epoch), float(gold[f"restart_bound_{name}"])
    print(f"[{name}] epochs 0-9 one at a time vs fp64 oracle: {err:.3e} of the span (bound {bound:.3e})")
    assert err <= bound


def test_epoch_skips_what_lies_outside_the_graph(oracle, dev):
    """Column indices outside [0, n) and positions beyond the arrays are skipped, not read."""
    from pti_ldm_vae_amd import ops
    g = oracle["n97dup"][3]
    good = _upload(g, dev)
    y0 = torch.from_numpy(O.pca_init(O.make_rows("n97dup"))).to(dev)
    want, got = torch.empty_like(y0), torch.empty_like(y0)
    ops.umap_epoch(good, y0, want, a=0.58, b=1.33, alpha=1.0, epoch=0, seed=1, negative_sample_rate=0)
    indices = good.indices.clone()
    last = int(g.indptr[-2])                                                   # the last row's entries point nowhere
    indices[last:] = 97
    ops.umap_epoch(good._replace(indices=indices), y0, got, a=0.58, b=1.33, alpha=1.0, epoch=0, seed=1, negative_sample_rate=0)
    assert torch.equal(got[:96], want[:96]) and torch.equal(got[96], y0[96])


# ---- 4. full run and quality gate ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_run(dev):
    rows = O.make_rows("n300k40")
    an = _analyzer(dev)

    def run(seed):
        return an.reduce_dimensionality_umap(rows, n_neighbors=40, min_dist=O.MIN_DIST, n_epochs=O.CASES["n300k40"][2],
                                             random_state=seed, backend="hip")
    return rows, run, run(O.SEED)


def test_full_run_passes_the_quality_gate(gold, full_run):
    """Trustworthiness (15 neighbours) on n300k40 after 200 epochs, measured on the CPU: sequential sweep 0.99348, Jacobi
    0.99338, start 0.87285; spread of the sequential sweep over five seeds 0.00040, so the gate is 0.99338 - 0.00121."""
    rows, _, (y, result) = full_run
    assert isinstance(y, np.ndarray) and y.shape == (300, 2) and y.dtype == np.float64 and np.isfinite(y).all()
    assert result.embedding_ is y and result.n_epochs_ == 200 and np.allclose([result.a_, result.b_], gold["ab"], rtol=1e-12)
    assert int(result.graph_.nnz) == result.graph_.indptr[-1].item() > 300 * 20
    trust, gate = O.trustworthiness(rows, y), _gate(gold)
    print(f"trustworthiness {trust:.5f} (gate {gate:.5f}: sequential {float(gold['trust_seq']):.5f}, Jacobi "
          f"{float(gold['trust_jacobi']):.5f}, margin {float(gold['trust_margin']):.5f}; start {float(gold['trust_start']):.5f})")
    assert trust >= gate and trust > float(gold["trust_start"])


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_give_the_same_bits(gold, full_run, dev):
    rows, run, (first, result) = full_run
    second = run(O.SEED)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        third = run(O.SEED)
        side.synchronize()
    nnz = int(result.graph_.nnz)
    for y, other in (second, third):
        assert np.array_equal(y, first)
        for key in ("indptr", "rho", "sigma"):
            assert torch.equal(getattr(other.graph_, key), getattr(result.graph_, key)), key
        for key in ("indices", "weights", "rate"):
            assert torch.equal(getattr(other.graph_, key)[:nnz], getattr(result.graph_, key)[:nnz]), key
    y, _ = run(7)
    trust = O.trustworthiness(rows, y)
    print(f"seed 7: trustworthiness {trust:.5f}, largest move from seed {O.SEED} {np.abs(y - first).max():.3f}")
    assert not np.array_equal(y, first) and np.isfinite(y).all() and trust >= _gate(gold) and trust > float(gold["trust_start"])


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def test_analyze_static_umap_backend_hip_needs_no_umap_learn(dev, tmp_path, monkeypatch, capsys):
    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import analyze_static
    from test_gpu_latent_analysis import _write_group
    _write_group(tmp_path / "edente", ["11", "12", "13"], 4, seed=1)
    _write_group(tmp_path / "dente", ["12", "13", "11"], 4, seed=2)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64])
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)
    monkeypatch.setitem(sys.modules, "umap", None)                             # `import umap` raises ImportError
    with pytest.raises(ImportError):
        import umap  # noqa: F401
    out = tmp_path / "out"
    analyze_static.main(["--vae-weights", str(ck), "--config-file", str(tmp_path / "cfg.json"), "--folder-edente",
                         str(tmp_path / "edente"), "--folder-dente", str(tmp_path / "dente"), "--method", "umap",
                         "--umap-backend", "hip", "--n-neighbors", "5", "--patch-size", "64", "64", "--cache-dir",
                         str(tmp_path / "cache"), "--batch-size", "6", "--dpi", "40", "--output-dir", str(out)])
    assert (out / "umap_projection.png").is_file() and (out / "umap_projection.png").stat().st_size > 0
    assert not (out / "pca_projection.png").exists() and "[WARN]" not in capsys.readouterr().out   # no fall-back to PCA
    z = np.load(out / "latents.npz")
    assert z["projection_edente"].shape == (12, 2) and np.isfinite(z["projection_dente"]).all()


# ---- 7. limits -------------------------------------------------------------------------------------------------------------
def test_shapes_outside_the_limits_raise_before_any_launch(dev):
    from pti_ldm_vae_amd import ops
    for n, k in ((2, 2), (300, 300), (300, 301), (300, 257), (300, 1), (8193, 40)):
        with pytest.raises(ValueError, match="umap_knn: unsupported shape"):
            ops.umap_knn(torch.empty(n, n, device=dev), k)
        with pytest.raises(ValueError, match="umap_graph: unsupported shape"):
            ops.umap_graph(torch.empty(n, k, dtype=torch.int32, device=dev), torch.empty(n, k, device=dev), 200)
    idx, kd = torch.zeros(300, 40, dtype=torch.int32, device=dev), torch.zeros(300, 40, device=dev)
    for n_epochs in (2001, 0):
        with pytest.raises(ValueError, match=f"n_epochs={n_epochs}"):
            ops.umap_graph(idx, kd, n_epochs)
    with pytest.raises(TypeError, match="knn_idx"):
        ops.umap_graph(idx.long(), kd, 200)
    graph = ops.UmapGraph(torch.zeros(301, dtype=torch.int32, device=dev), idx.flatten(), kd.flatten(), idx.flatten(), None, None, None)
    y = torch.zeros(300, 2, device=dev)
    with pytest.raises(ValueError, match="y_out must not be y_in"):
        ops.umap_epoch(graph, y, y, a=0.58, b=1.33, alpha=1.0, epoch=0, seed=1)
    with pytest.raises(ValueError, match="only n_components = 2"):
        ops.umap_epoch(graph, torch.zeros(300, 3, device=dev), torch.zeros(300, 3, device=dev), a=0.58, b=1.33, alpha=1.0, epoch=0, seed=1)
    from pti_ldm_vae_amd._lib import PtiError
    with pytest.raises(PtiError, match="epoch 2000"):
        ops.umap_epoch(graph, y, torch.empty_like(y), a=0.58, b=1.33, alpha=1.0, epoch=2000, seed=1)
    an = _analyzer(dev)
    x = torch.zeros(300, 64, device=dev)
    for kw in (dict(n_epochs=2001), dict(n_neighbors=257), dict(n_components=3)):
        with pytest.raises(ValueError, match="backend='hip'"):
            an.reduce_dimensionality_umap(x, backend="hip", **kw)

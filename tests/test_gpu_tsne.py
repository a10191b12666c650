"""GPU tests of the exact t-SNE (csrc/tsne.hip): ``ops.tsne_affinities`` and ``ops.tsne_step`` against the fp64 oracle of
``tests/tsne_oracle.py``, the descent loop of ``LatentSpaceAnalyzer``, its reproducibility, and ``analyze_static
--tsne-backend hip`` end to end.

Every bound comes from ``tests/golden/tsne_golden.npz`` and was measured on the CPU by ``tsne_oracle.__main__``: twice the
deviation of the oracle's own stopping slack or of the plain fp32 numpy restatement from the fp64 oracle -- never from
what the kernels give.  What the kernels gave on MI355X: DESIGN.md 5k."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import tsne_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(O.GOLDEN)


@pytest.fixture(scope="module")
def oracle():
    """name -> (fp32 squared distances, perplexity, the oracle's fp64 P); computed once, never written to."""
    out = {}
    for name, case in O.CASES.items():
        d2 = O.squared_distances(O.make_rows(name))
        p = O.joint_probabilities(d2, case[1])
        p.setflags(write=False)
        out[name] = (d2, case[1], p)
    return out


def _analyzer(dev):
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    return LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)


def _upload(p64, dev):
    """The oracle's P rounded to fp32 on the device, with its {sum P log P, sum P}."""
    p32 = p64.astype(np.float32)
    return torch.from_numpy(p32).to(dev), torch.from_numpy(O.host_sums(p32)).to(dev), p32


# ---- 1. affinities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CASES))
def test_affinities_against_the_oracle(gold, oracle, dev, name):
    from pti_ldm_vae_amd import ops
    d2, perplexity, want = oracle[name]
    if f"p_{name}" in gold.files:
        assert O.rel_dev(want, gold[f"p_{name}"]) <= 1e-12
    p, sums = ops.tsne_affinities(torch.from_numpy(d2).to(dev), perplexity)
    assert p.dtype == torch.float32 and tuple(p.shape) == d2.shape and sums.dtype == torch.float64 and tuple(sums.shape) == (2,)
    assert torch.equal(p, p.t().contiguous()) and not p.diagonal().any()      # symmetric bit for bit, zero diagonal
    got, s = p.cpu().numpy(), sums.cpu().numpy()
    assert np.isfinite(got).all() and got[~np.eye(len(got), dtype=bool)].min() >= np.float32(O.EPS)
    assert np.allclose(s, O.host_sums(got), rtol=1e-12, atol=0)               # the two fp64 scalars are those of the stored P
    assert abs(s[1] - 1.0) <= 2.0 ** -23                                      # sum P = 1 within the fp32 rounding of its entries
    err, bound = O.rel_dev(got, want), float(gold[f"aff_bound_{name}"])
    print(f"[{name}] P vs fp64 oracle: {err:.3e} of max P (bound {bound:.3e}: stopping slack "
          f"{float(gold[f'aff_dev_tol_{name}']):.2e}, fp32 restatement {float(gold[f'aff_dev_fp32_{name}']):.2e})")
    assert err <= bound
    if name == "n97dup":
        # The outlier's own search (row 3) runs where exp(-beta d) is an fp64 SUBNORMAL: its row sum is about twenty quanta
        # of 4.9e-324, the search never converges and its 20 non-zero p_j|3 = 0.05 are the quantisation of those few bits
        # (also in sklearn).  Any exp that differs in the last subnormal bit gives another row, which is why the fp32
        # restatement -- and with it the bound above -- is of order 1 here.  Everything outside that row and column does
        # not see it (p_3|j underflows to exactly 0 for every j), so there the widest bound of the regular cases holds.
        keep = np.arange(len(got)) != 3
        rest = O.rel_dev(got[keep][:, keep], want[keep][:, keep])
        print(f"[{name}] without the outlier's row and column: {rest:.3e}")
        assert rest <= max(float(gold[f"aff_bound_{k}"]) for k in O.CASES if k != "n97dup")


def test_affinities_write_a_strided_out_in_place(oracle, dev):
    from pti_ldm_vae_amd import ops
    d2, perplexity, _ = oracle["n97"]
    d2 = torch.from_numpy(d2).to(dev)
    dense, sums = ops.tsne_affinities(d2, perplexity)
    buf = torch.full((97, 128), -1.0, device=dev)
    p, sums2 = ops.tsne_affinities(d2, perplexity, out=buf[:, :97])
    assert p.data_ptr() == buf.data_ptr() and torch.equal(p, dense) and torch.equal(sums, sums2) and (buf[:, 97:] == -1.0).all()


# ---- 2. one step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale,exag", O.STEP_CASES)
def test_one_step_against_the_oracle(gold, oracle, dev, name, scale, exag):
    from pti_ldm_vae_amd import ops
    tag = f"{name}_{scale:g}_{exag:g}"
    p, sums, _ = _upload(oracle[name][2], dev)
    n = p.shape[0]
    y = torch.from_numpy(O.step_embedding(name, scale)).to(dev)
    y_out, update, gains = torch.empty_like(y), torch.zeros_like(y), torch.ones_like(y)
    record = torch.zeros(2, dtype=torch.float64, device=dev)
    lr = O.learning_rate(n)
    ops.tsne_step(p, y, y_out, update, gains, record, sums=sums, exaggeration=exag, momentum=0.5, lr=lr)
    kl, norm = record.cpu().tolist()
    assert torch.equal(y_out, y + update) and (gains == 0.8).all()            # update 0: no sign is opposite, every gain * 0.8
    bound = float(gold[f"step_bound_{tag}"])
    errs = (O.rel_dev(update.cpu().numpy(), gold[f"step_update_{tag}"]), abs(kl - float(gold[f"step_kl_{tag}"])) / float(gold[f"step_kl_{tag}"]),
            abs(norm - float(gold[f"step_norm_{tag}"])) / float(gold[f"step_norm_{tag}"]))
    print(f"[{tag}] update {errs[0]:.3e}, KL {errs[1]:.3e}, |grad| {errs[2]:.3e} (bound {bound:.3e}; fp32 restatement "
          f"{gold[f'step_fp32_dev_{tag}']})")
    assert max(errs) <= bound
    # without a record the same update, and the record is left alone
    y2, update2, gains2 = torch.empty_like(y), torch.zeros_like(y), torch.ones_like(y)
    record2 = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    ops.tsne_step(p, y, y2, update2, gains2, record2, sums=sums, exaggeration=exag, momentum=0.5, lr=lr, with_record=False)
    assert torch.equal(y2, y_out) and torch.equal(update2, update) and (record2 == -7.0).all()


# ---- 3. short trajectory -----------------------------------------------------------------------------------------------
def test_short_trajectory_across_the_stage_switch(gold, oracle, dev):
    p, sums, _ = _upload(oracle["n300"][2], dev)
    y0 = torch.from_numpy(gold["y0_n300"]).to(dev)
    y, kl = _analyzer(dev).tsne_descend(p, sums, y0, max_iter=10, exploration_n_iter=5)
    err, bound = O.rel_dev(y.cpu().numpy(), gold["y10_n300"]), float(gold["traj_bound_n300"])
    print(f"Y after 10 iterations vs fp64 oracle: {err:.3e} of max |Y| (bound {bound:.3e})")
    assert err <= bound and np.isfinite(kl)


# ---- 4. full run ---------------------------------------------------------------------------------------------------------
def test_full_run_reaches_the_oracles_kl(gold, oracle, dev):
    """KL_oracle = 0.308247 (descend, 1000 iterations, same init); spread over five inits perturbed by 1e-6: 0.67 %, so the
    margin is 2.0 %."""
    p64 = oracle["n300"][2]
    p, sums, p32 = _upload(p64, dev)
    an = _analyzer(dev)
    y, kl = an.tsne_descend(p, sums, torch.from_numpy(gold["y0_n300"]).to(dev))
    y = y.cpu().double().numpy()
    assert y.shape == (300, 2) and np.isfinite(y).all() and np.isfinite(kl) and an.tsne_kl_divergence_ == kl
    recomputed = float(O.kl_and_grad(p64, y)[0])
    want, margin = float(gold["kl_full_n300"]), 3.0 * float(gold["kl_spread_n300"])
    print(f"final KL {recomputed:.6f} (oracle {want:.6f}, margin {margin:.2%}); reported {kl:.9f}")
    assert recomputed <= want * (1.0 + margin)
    same_p = float(O.kl_and_grad(p32.astype(np.float64), y)[0])               # the P the device was given
    bound = max(float(gold[f"step_bound_n300_{scale:g}_1"]) for scale in (1e-4, 10.0))
    print(f"reported vs recomputed KL: {abs(kl - same_p) / same_p:.3e} (bound {bound:.3e})")
    assert abs(kl - same_p) <= bound * same_p


# ---- 5. reproducibility --------------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_give_the_same_bits(oracle, gold, dev):
    from pti_ldm_vae_amd import ops
    d2, perplexity, _ = oracle["n300"]
    d2 = torch.from_numpy(d2).to(dev)
    y0 = torch.from_numpy(gold["y0_n300"]).to(dev)
    an = _analyzer(dev)

    def run():
        p, sums = ops.tsne_affinities(d2, perplexity)
        y, kl = an.tsne_descend(p, sums, y0)
        return p.clone(), sums.clone(), y.clone(), kl

    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        third = run()
        side.synchronize()
    for other in (second, third):
        assert all(torch.equal(a, b) for a, b in zip(first[:3], other[:3])) and first[3] == other[3]


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def test_reduce_dimensionality_tsne_hip_backend(dev, capsys):
    an = _analyzer(dev)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(120, 4096, generator=g) + 3.0 * torch.randint(0, 4, (120, 1), generator=g)).to(dev)
    a = an.reduce_dimensionality_tsne(x, backend="hip")
    kl = an.tsne_kl_divergence_
    b = an.reduce_dimensionality_tsne(x.cpu().numpy(), backend="hip", random_state=7)      # random_state changes nothing
    for out in (a, b):
        assert isinstance(out, np.ndarray) and out.shape == (120, 2) and out.dtype == np.float64 and np.isfinite(out).all()
    assert np.array_equal(a, b) and np.isfinite(kl) and kl == an.tsne_kl_divergence_ and np.ptp(a[:, 0]) > 1.0
    an.reduce_dimensionality_tsne(x, backend="hip", perplexity=4, max_iter=20, exploration_n_iter=10)
    assert "perplexity=4 is very low" in capsys.readouterr().out


def test_analyze_static_tsne_backend_hip_needs_no_sklearn(dev, tmp_path, monkeypatch):
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
    for name in [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "sklearn", None)                          # `import sklearn` raises ImportError
    with pytest.raises(ImportError):
        import sklearn.manifold  # noqa: F401
    out = tmp_path / "out"
    analyze_static.main(["--vae-weights", str(ck), "--config-file", str(tmp_path / "cfg.json"), "--folder-edente",
                         str(tmp_path / "edente"), "--folder-dente", str(tmp_path / "dente"), "--method", "tsne",
                         "--tsne-backend", "hip", "--perplexity", "5", "--patch-size", "64", "64", "--cache-dir",
                         str(tmp_path / "cache"), "--batch-size", "6", "--dpi", "40", "--output-dir", str(out)])
    assert (out / "tsne_projection.png").is_file() and (out / "tsne_projection.png").stat().st_size > 0
    assert not (out / "pca_projection.png").exists()                          # no fall-back to PCA
    z = np.load(out / "latents.npz")
    assert z["projection_edente"].shape == (12, 2) and np.isfinite(z["projection_dente"]).all()

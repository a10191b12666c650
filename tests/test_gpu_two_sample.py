"""GPU tests of the two-sample permutation tests (csrc/two_sample.hip, analysis/two_sample.py) against the numpy oracle
(tests/two_sample_oracle.py) on the same inputs.

Gates.  Every integer of ``permutation_forms``, ``knn_indicator`` and the median's bits: equality.  ``two_sample_kernel``:
equality, except at the entries the oracle lists as lying within 1e-9 of a half-integer before rounding (under 0.1 % of the
entries; they may differ by 1).  The report: integer tables, ``exceed`` and p-values equal to the oracle's."""
import json
import os

import numpy as np
import pytest
import torch

import bounds_util as B
import two_sample_oracle as O
from test_gpu_projection_quality import _write_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(n, seed):
    """Random ASYMMETRIC int32 in [0, 65535] with forced 0 and 65535 entries and a non-zero diagonal."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 65536, size=(n, n)).astype(np.int32)
    w[np.arange(n), np.arange(n)] = rng.integers(1, 65536, size=n)
    w[0, n - 1], w[n - 1, 0], w[1, 2], w[2, 1] = 0, 65535, 65535, 0
    w[n // 2, n // 2] = 65535
    assert not np.array_equal(w, w.T)
    return w


def _masks(p, n, seed):
    """Mixed density, with an all-zero and an all-one row where there is room."""
    rng = np.random.default_rng(seed)
    density = rng.random((p, 1))
    m = (rng.random((p, n)) < density).astype(np.uint8)
    if p >= 3:
        m[1], m[p - 1] = 0, 1
    return m


def _forms(dev, w, masks):
    from pti_ldm_vae_amd import ops
    return ops.permutation_forms(torch.from_numpy(w).to(dev), torch.from_numpy(masks).to(dev)).cpu().numpy()


# ---- permutation_forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 129, 300])
def test_permutation_forms_equal_the_oracle(dev, n):
    w = _weights(n, n)
    for p in (1, 17, 100):
        masks = _masks(p, n, 1000 * n + p)
        got = _forms(dev, w, masks)
        assert got.dtype == np.int64 and got.shape == (p, 3)
        assert np.array_equal(got, O.forms(w, masks)), (n, p)


def test_one_hot_masks_pin_every_position(dev):
    n = 65
    w = _weights(n, 7)
    got = _forms(dev, w, np.eye(n, dtype=np.uint8))
    assert np.array_equal(got[:, 0], np.diag(w).astype(np.int64))
    assert np.array_equal(got[:, 1], w.astype(np.int64).sum(1)) and np.array_equal(got[:, 2], w.astype(np.int64).sum(0))


def test_pair_masks_across_tile_and_k_step_boundaries(dev):
    """e_i + e_j with i, j either side of every fragment (16), wave (32), tile / k-step (64) and 128 boundary: the fragment-layout
    check.  A = w_ii + w_jj + w_ij + w_ji separates w_ij from w_ji only together with R and C, which the one-hot test pins."""
    n = 200
    w = _weights(n, 9)
    at = [0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 65, 79, 80, 127, 128, 129, 191, 192, 199]
    pairs = [(i, j) for i in at for j in at if i < j]
    masks = np.zeros((len(pairs), n), dtype=np.uint8)
    for row, (i, j) in enumerate(pairs):
        masks[row, i] = masks[row, j] = 1
    got = _forms(dev, w, masks)
    w64 = w.astype(np.int64)
    want = np.array([w64[i, i] + w64[j, j] + w64[i, j] + w64[j, i] for i, j in pairs])
    assert np.array_equal(got[:, 0], want)
    assert np.array_equal(got, O.forms(w, masks))
    # directed: rows {i} x columns {i, j} through an asymmetric matrix that is zero but for one entry
    one = np.zeros((n, n), dtype=np.int32)
    one[63, 64] = 40000                                      # w_ij without w_ji
    got = _forms(dev, one, masks)
    assert np.array_equal(got, O.forms(one, masks))
    assert got[pairs.index((63, 64)), 0] == 40000 and got[:, 0].sum() == 40000


def test_bound_case_has_no_overflow(dev):
    """n = 8192, every entry 65535: the largest sums the kernel can meet, against the closed form."""
    from pti_ldm_vae_amd import ops
    n = 8192
    w = torch.full((n, n), 65535, dtype=torch.int32, device=dev)
    masks = torch.ones(2, n, dtype=torch.uint8, device=dev)
    masks[1, 1::2] = 0
    got = ops.permutation_forms(w, masks).cpu().tolist()
    assert got[0] == [n * n * 65535] * 3
    assert got[1] == [(n // 2) ** 2 * 65535, (n // 2) * n * 65535, (n // 2) * n * 65535]


def test_results_are_reproducible_and_independent_of_the_batch(dev):
    from pti_ldm_vae_amd import ops
    n = 129
    w = torch.from_numpy(_weights(n, 21)).to(dev)
    masks = torch.from_numpy(_masks(100, n, 22)).to(dev)
    first = ops.permutation_forms(w, masks)
    again = ops.permutation_forms(w, masks)
    halves = torch.cat([ops.permutation_forms(w, masks[:50]).clone(), ops.permutation_forms(w, masks[50:]).clone()])
    assert torch.equal(first, again) and torch.equal(first, halves)
    view = torch.zeros(n, n + 7, dtype=torch.int32, device=dev)[:, :n]      # a row-strided view is used in place
    view.copy_(w)
    assert torch.equal(first, ops.permutation_forms(view, masks))


# ---- distance_median --------------------------------------------------------------------------------------------------------
def _tied(n):
    x = np.round(np.random.default_rng(n).standard_normal((n, 3)) * 2) / 2      # a coarse grid: many equal distances
    x[1] = x[0]                                                                 # zeros off the diagonal
    x[n - 1] = x[n // 2]
    return O.pairwise(x)


@pytest.mark.parametrize("n", [4, 5, 64, 301])
def test_distance_median_equals_partition(dev, n):
    from pti_ldm_vae_amd import ops
    smooth = O.pairwise(np.random.default_rng(n).standard_normal((n, 6)))
    for dist in (smooth, _tied(n), np.zeros((n, n), np.float32)):
        got = ops.distance_median(torch.from_numpy(dist).to(dev))
        assert got.dtype == torch.float32 and got.shape == ()
        assert got.cpu().numpy().tobytes() == np.float32(O.lower_median(dist)).tobytes(), n


# ---- two_sample_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(4, 0), (5, 1), (64, 2), (301, 3)])          # the CPU test shows their half zone is (nearly) empty
def test_two_sample_kernel_equals_the_oracle(dev, n, seed):
    from pti_ldm_vae_amd import ops
    dist = O.pairwise(np.random.default_rng(seed).standard_normal((n, 6)))
    d = torch.from_numpy(dist).to(dev)
    med = ops.distance_median(d)
    used = torch.zeros(2, device=dev)
    got = {"gaussian": ops.two_sample_kernel(d, "gaussian", scale=med, scale_out=used[0]),
           "energy": ops.two_sample_kernel(d, "energy", scale_out=used[1])}
    assert used.cpu().numpy().tobytes() == np.array([O.lower_median(dist), dist.max()], np.float32).tobytes()
    for kind, w in got.items():
        w = w.cpu().numpy()
        want, near = O.kernel_matrix(dist, kind, O.lower_median(dist) if kind == "gaussian" else dist.max())
        assert near.sum() < 0.001 * n * n
        assert w.dtype == np.int32 and w.min() >= 0 and w.max() <= 65535 and not np.diag(w).any()
        diff = np.abs(w.astype(np.int64) - want)
        assert not diff[~near].any() and diff.max(initial=0) <= 1, (kind, int(diff.max()))
    assert got["energy"].max().item() == 65535
    zero = torch.zeros((), device=dev)
    assert not ops.two_sample_kernel(d, "gaussian", scale=zero).any()
    assert not ops.two_sample_kernel(torch.zeros(n, n, device=dev), "energy").any()
    one = ops.two_sample_kernel(d, "gaussian", scale=med, bandwidths=(1.5,)).cpu().numpy()
    assert np.abs(one - O.kernel_matrix(dist, "gaussian", O.lower_median(dist), (1.5,))[0]).max() <= 1


# ---- knn_indicator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(5, 2), (64, 5), (301, 15)])
def test_knn_indicator_equals_the_oracle(dev, n, k):
    from pti_ldm_vae_amd import ops
    dist = O.pairwise(np.random.default_rng(n).standard_normal((n, 6)))
    idx, _ = ops.umap_knn(torch.from_numpy(dist).to(dev), k + 1)
    assert np.array_equal(idx.cpu().numpy(), O.knn_table(dist, k + 1))
    got = ops.knn_indicator(idx, n).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, O.knn_indicator(O.knn_table(dist, k + 1), n))
    assert (got.sum(1) == k).all() and not np.diag(got).any()
    wild = idx.clone()
    wild[0, 0], wild[1, 1] = -1, n                           # skipped, never dereferenced
    assert np.array_equal(ops.knn_indicator(wild, n).cpu().numpy(), O.knn_indicator(wild.cpu().numpy(), n))


# ---- two_sample_tests -------------------------------------------------------------------------------------------------------
def _case(name):
    from test_two_sample_cpu import PERM_SEED, ROWS, groups
    if name == "stratified":
        rng = np.random.default_rng(17)
        a, b = rng.standard_normal((60, 16)).astype(np.float32), rng.standard_normal((60, 16)).astype(np.float32) + np.float32(0.4)
        return a, b, [f"p{i % 9}" for i in range(60)], [f"p{i % 10}" for i in range(60)], 3      # p9: rows of B only
    a, b = groups(0.0 if name == "same" else 2.0)
    assert len(a) == ROWS
    return a, b, None, None, PERM_SEED


@pytest.mark.parametrize("name", ["same", "shifted", "stratified"])
def test_two_sample_tests_equal_the_oracle(dev, name):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import two_sample_tests
    a, b, strata_a, strata_b, seed = _case(name)
    n_a, n_b = len(a), len(b)
    run = lambda: two_sample_tests(a, b, permutations=199, seed=seed, strata_a=strata_a, strata_b=strata_b, device=dev)
    report, arrays = run()
    dist = ops.latent_pairwise(torch.from_numpy(np.concatenate([a, b])).to(dev)).cpu().numpy()
    want = O.two_sample(dist, n_a, n_b, permutations=199, seed=seed, strata=None if strata_a is None else strata_a + strata_b)
    assert np.array_equal(arrays["masks"], want["masks"])
    assert (report["n_a"], report["n_b"], report["stratified"], report["seed"]) == (n_a, n_b, strata_a is not None, seed)
    assert (report["fixed_strata"], report["fixed_rows"]) == want["fixed"] == ((1, 6) if name == "stratified" else (0, 0))
    for kind in ("mmd", "energy", "knn"):
        entry = report["tests"][kind]
        assert np.array_equal(arrays[f"forms_{kind}"], want[kind]["forms"]), kind
        assert entry["exceed"] == want[kind]["exceed"] and entry["p_value"] == want[kind]["p_value"], kind
        assert entry["permutations"] == 199 and entry["levels"] == (2 if kind == "knn" else 65536)
        assert np.array_equal(arrays[f"null_{kind}"], want[kind]["null"]) and entry["statistic"] == want[kind]["statistic"]
    assert report["tests"]["mmd"]["scale"] == want["median"] and report["tests"]["energy"]["scale"] == want["max"]
    if name == "shifted":
        assert all(report["tests"][k]["p_value"] == 1 / 200 for k in report["tests"])
    if name == "same":
        assert all(report["tests"][k]["p_value"] > 0.05 for k in report["tests"])
    w = want["mmd"]["w"].astype(np.float64)
    witness = (w[:, :n_a].sum(1) / n_a - w[:, n_a:].sum(1) / n_b) / 65535.0
    assert np.array_equal(arrays["witness"], witness)
    again, _ = run()
    text = json.dumps(report, indent=2, allow_nan=False)
    assert text == json.dumps(again, indent=2, allow_nan=False) and "NaN" not in text


def test_equal_rows_are_reported_as_undefined(dev):
    from pti_ldm_vae_amd.analysis import two_sample_tests
    report, arrays = two_sample_tests(np.ones((6, 4), np.float32), np.ones((7, 4), np.float32), permutations=20, neighbors=2,
                                      device=dev)
    for kind in ("mmd", "energy"):
        entry = report["tests"][kind]
        assert entry["statistic"] is None and entry["p_value"] is None and entry["scale"] == 0.0 and not arrays[f"forms_{kind}"].any()
    json.dumps(report, allow_nan=False)


def test_analyze_static_group_test_end_to_end(dev, tmp_path, capsys):
    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import analyze_static
    _write_group(tmp_path / "edente", ["11", "12", "13", "14"], 3, seed=1)          # 12 + 12 images, four patients
    _write_group(tmp_path / "dente", ["12", "13", "11", "14"], 3, seed=2)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64])
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)
    base = ["--vae-weights", str(ck), "--config-file", str(tmp_path / "cfg.json"), "--folder-edente", str(tmp_path / "edente"),
            "--folder-dente", str(tmp_path / "dente"), "--patch-size", "64", "64", "--cache-dir", str(tmp_path / "cache"),
            "--batch-size", "8", "--dpi", "40", "--method", "pca"]
    flags = ["--group-test", "--group-test-permutations", "99", "--group-test-stratify", "patient", "--group-test-neighbors", "3",
             "--group-test-seed", "5"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    analyze_static.main(base + flags + ["--output-dir", str(out)])
    assert "Group test mmd: " in capsys.readouterr().out
    files = ["group_test.json", "group_test.npz", "group_test.png"]
    for name in files:
        assert (out / name).is_file() and (out / name).stat().st_size > 0, name
    raw = (out / "group_test.json").read_bytes()
    doc = json.loads(raw)
    assert (doc["group_a"], doc["group_b"], doc["stratify"], doc["n_a"], doc["n_b"], doc["stratified"], doc["seed"]) == \
        ("edente", "dente", "patient", 12, 12, True, 5)
    assert list(doc["tests"]) == ["mmd", "energy", "knn"] and all(t["permutations"] == 99 for t in doc["tests"].values())
    npz = np.load(out / "group_test.npz")
    assert npz["masks"].shape == (100, 24) and npz["witness"].shape == (24,) and len(npz["ids"]) == len(npz["paths"]) == 24
    analyze_static.main(base + flags + ["--output-dir", str(out)])
    assert (out / "group_test.json").read_bytes() == raw
    analyze_static.main(base + ["--output-dir", str(plain)])
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + files)
    for name in os.listdir(plain):
        if name.endswith(".npz"):
            x, y = np.load(plain / name), np.load(out / name)
            assert sorted(x.files) == sorted(y.files) and all(np.array_equal(x[k], y[k]) for k in x.files), name
        else:
            assert (plain / name).read_bytes() == (out / name).read_bytes(), name


# ---- memory -----------------------------------------------------------------------------------------------------------------
def _guarded_bytes(dev, t):
    """A uint8 tensor inside a buffer of 0xFF bytes."""
    flat = torch.full((2 * B.PAD_BYTES + t.numel(),), 255, dtype=torch.uint8, device=dev)
    view = flat[B.PAD_BYTES:B.PAD_BYTES + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("n,p", [(5, 3), (65, 17), (130, 129)])
def test_permutation_forms_stays_inside_its_buffers(dev, n, p):
    """Inputs inside poison, output and workspace inside canaries, the workspace exactly as large as the library asks."""
    import ctypes as C

    from pti_ldm_vae_amd import _lib as L
    from pti_ldm_vae_amd import ops
    w_host, m_host = _weights(n, n + p), _masks(p, n, p)
    want = O.forms(w_host, m_host)
    w = B.guarded(dev, torch.from_numpy(w_host).to(dev), B.POISON_BIG)
    masks = _guarded_bytes(dev, torch.from_numpy(m_host).to(dev))
    nbytes = L.lib().pti_permutation_forms_ws_bytes(n, p)
    assert nbytes > 0 and nbytes % 4 == 0
    out = B.with_canary(dev, (p, 3), torch.int64, -7)
    for fill in (0, -1):                                     # whatever the workspace held before
        ws = B.with_canary(dev, (nbytes // 4,), torch.int32, fill)
        L.check(L.lib().pti_permutation_forms(C.c_void_p(w.data_ptr()), n, n, C.c_void_p(masks.data_ptr()), p,
                                              C.c_void_p(out.view.data_ptr()), C.c_void_p(ws.view.data_ptr()), nbytes,
                                              torch.cuda.current_stream().cuda_stream), "pti_permutation_forms")
        torch.cuda.synchronize()
        assert B.intact(ws) and B.intact(out)
        assert np.array_equal(out.view.cpu().numpy(), want)
    assert np.array_equal(ops.permutation_forms(w, masks).cpu().numpy(), want)


@pytest.mark.parametrize("poison", B.POISONS)
def test_matrix_launchers_stay_inside_their_buffers(dev, poison):
    from pti_ldm_vae_amd import ops
    n, k = 67, 4
    dist = O.pairwise(np.random.default_rng(5).standard_normal((n, 6)))
    plain = torch.from_numpy(dist).to(dev)
    d = B.guarded(dev, plain, poison)
    med = B.with_canary(dev, (), torch.float32, 0.0)
    ops.distance_median(d, out=med.view)
    assert B.intact(med) and torch.equal(med.view, ops.distance_median(plain))
    for kind in ("gaussian", "energy"):
        out = B.with_canary(dev, (n, n), torch.int32, -3)
        used = B.with_canary(dev, (), torch.float32, 0.0)
        ops.two_sample_kernel(d, kind, scale=med.view if kind == "gaussian" else None, out=out.view, scale_out=used.view)
        assert B.intact(out) and B.intact(used)
        assert torch.equal(out.view, ops.two_sample_kernel(plain, kind, scale=med.view if kind == "gaussian" else None))
    idx, _ = ops.umap_knn(plain, k + 1)
    out = B.with_canary(dev, (n, n), torch.int32, -3)
    ops.knn_indicator(B.guarded(dev, idx, B.POISON_BIG), n, out=out.view)
    assert B.intact(out) and torch.equal(out.view, ops.knn_indicator(idx, n))

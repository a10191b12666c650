"""GPU tests of the latent-space analysis: ``ops.latent_pairwise`` / ``ops.latent_group_stats`` (csrc/latent_stats.hip)
against the reference's recorded fp64 outputs (``tests/golden/latent_analysis_golden.npz``), their shape, stride and
reproducibility contracts, the Gram-matrix PCA, and ``analyze_static`` end to end on two folders of TIF files.

Gate: relative error against the fp64 reference <= max(1e-5, 20 x the error of the plain fp32 CPU restatement recorded in
the fixture) -- the reference's arithmetic in fp32 plus a margin for a different summation order; PCA projections per
component <= max(1e-3, 20 x recorded).  Measured on MI355X: see DESIGN.md 5g."""
import json
import os

import numpy as np
import pytest
import torch

import latent_analysis_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "latent_analysis_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cases(gold, dev):
    """tag -> (a, ids_a, b, ids_b) on the device; the D = 40 960 inputs are regenerated from the stored seed."""
    out = {}
    for tag in ("small", "large"):
        a, ids_a, b, ids_b = O.make_latents(int(gold[f"seed_{tag}"]), int(gold[f"d_{tag}"]))
        out[tag] = (torch.from_numpy(a).to(dev), ids_a, torch.from_numpy(b).to(dev), ids_b)
    assert np.array_equal(out["small"][0].cpu().numpy(), gold["a"])
    return out


def _bound(gold, key, floor=1e-5):
    return max(floor, 20.0 * float(gold[key]))


def _grouped(a, ids_a, b, ids_b, dev):
    (oa, sa), (ob, sb) = O.segments(ids_a), O.segments(ids_b)
    ga, gb = a[torch.tensor(oa, device=dev)], b[torch.tensor(ob, device=dev)]
    return ga, torch.tensor(sa, dtype=torch.int32, device=dev), gb, torch.tensor(sb, dtype=torch.int32, device=dev), sa, sb


# ---- accuracy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["small", "large"])
def test_pairwise_distance_against_the_reference(gold, cases, tag):
    from pti_ldm_vae_amd import ops
    a, _, b, _ = cases[tag]
    got = ops.latent_pairwise(a, b).cpu().numpy()
    err, bound = O.rel_err(got, gold[f"cdist_{tag}"]), _bound(gold, f"cdist_{tag}_fp32_err")
    print(f"[{tag}] pairwise distance: relative error {err:.3e} (bound {bound:.1e}, fp32 CPU {float(gold[f'cdist_{tag}_fp32_err']):.1e})")
    assert err <= bound


@pytest.mark.parametrize("tag", ["small", "large"])
def test_group_stats_against_the_reference(gold, cases, dev, tag):
    from pti_ldm_vae_amd import ops
    a, ids_a, b, ids_b = cases[tag]
    ga, sa, gb, sb, ha, hb = _grouped(a, ids_a, b, ids_b, dev)
    got = ops.latent_group_stats(ga, sa, gb, sb).cpu().numpy()
    want = gold[f"metrics_{tag}"]
    assert got.shape == (9, 4) and np.isnan(want).all(axis=1).sum() == 2
    err, bound = O.rel_err(got, want), _bound(gold, f"metrics_{tag}_fp32_err")
    print(f"[{tag}] group statistics: relative error {err:.3e} (bound {bound:.1e}, fp32 CPU {float(gold[f'metrics_{tag}_fp32_err']):.1e})")
    assert err <= bound
    # the mean-cross-distance column is the mean of the matching block of the pairwise output
    full = ops.latent_pairwise(ga, gb).cpu().double().numpy()
    for p in range(9):
        if ha[p + 1] > ha[p] and hb[p + 1] > hb[p]:
            block = full[ha[p]:ha[p + 1], hb[p]:hb[p + 1]].mean()
            assert abs(got[p, 3] - block) <= 1e-6 * block, (p, got[p, 3], block)
    single = [p for p in range(9) if ha[p + 1] - ha[p] == 1][0]
    assert got[single, 1] == 0.0                                              # one row: std 0.0


# ---- shapes ------------------------------------------------------------------------------------------------------------
def _host_cdist(a, b):
    a, b = a.cpu().double(), b.cpu().double()
    return torch.stack([((b - row) ** 2).sum(dim=1).sqrt() for row in a]).numpy()


@pytest.mark.parametrize("n1,n2,d", [(1, 1, 2), (1, 70, 3), (65, 1, 63), (130, 67, 4096), (5, 7, 40960), (64, 64, 512), (33, 129, 515)])
def test_pairwise_shapes(dev, n1, n2, d):
    from pti_ldm_vae_amd import ops
    g = torch.Generator().manual_seed(n1 * 1000 + n2 + d)
    a = (3.0 + torch.randn(n1, d, generator=g)).to(dev)
    b = (3.0 + torch.randn(n2, d, generator=g)).to(dev)
    got = ops.latent_pairwise(a, b)
    assert got.shape == (n1, n2) and got.dtype == torch.float32
    assert O.rel_err(got.cpu().numpy(), _host_cdist(a, b)) <= 1e-5
    dot = ops.latent_pairwise(a, b, mode="dot").cpu().double().numpy()
    want = (a.cpu().double() @ b.cpu().double().t()).numpy()
    assert np.abs(dot - want).max() <= 1e-5 * np.abs(want).max()
    c = a.mean(dim=0)
    cdot = ops.latent_pairwise(a, b, mode="dot", center=c).cpu().double().numpy()
    cwant = ((a - c).cpu().double() @ (b - c).cpu().double().t()).numpy()
    assert np.abs(cdot - cwant).max() <= 1e-5 * max(np.abs(cwant).max(), 1.0)


def test_strided_inputs_same_operand_and_offset_out(dev):
    from pti_ldm_vae_amd import ops
    g = torch.Generator().manual_seed(5)
    big_a = torch.randn(70, 300, generator=g).to(dev) + 2.0
    big_b = torch.randn(90, 301, generator=g).to(dev) + 2.0
    a, b = big_a[3:, 8:264], big_b[:77, 1:257]                                # row-strided views, one of them unaligned
    assert not a.is_contiguous() and not b.is_contiguous()
    want = ops.latent_pairwise(a.contiguous(), b.contiguous())
    assert torch.equal(ops.latent_pairwise(a, b), want)
    assert O.rel_err(want.cpu().numpy(), _host_cdist(a, b)) <= 1e-5
    every_other = big_a[::2, :256]                                            # row stride 600
    assert torch.equal(ops.latent_pairwise(every_other, b), ops.latent_pairwise(every_other.contiguous(), b.contiguous()))
    same = ops.latent_pairwise(a)                                             # A is B
    assert torch.equal(same, ops.latent_pairwise(a, a)) and torch.equal(same, same.t()) and float(same.diagonal().abs().max()) == 0.0
    pad = torch.full((80, 100), -7.0, device=dev)
    view = pad[5:72, 11:88]
    assert ops.latent_pairwise(a, b, out=view) is view and torch.equal(view, want)
    pad[5:72, 11:88] = -7.0
    assert float((pad + 7.0).abs().max()) == 0.0                              # nothing outside the view was written
    for bad in (lambda: ops.latent_pairwise(a, b[:, :10]), lambda: ops.latent_pairwise(a[0]),
                lambda: ops.latent_pairwise(a, b, out=torch.zeros(3, 4, device=dev)),
                lambda: ops.latent_pairwise(a, b, center=torch.zeros(5, device=dev)),
                lambda: ops.latent_pairwise(a, b, out=torch.zeros(67, 77, device=dev).t().contiguous().t())):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.latent_pairwise(a.long(), b.long())


@pytest.mark.parametrize("d", [2, 3, 63, 4096])
def test_group_stats_shapes_and_empty_segments(dev, d):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis.latent_space import segmented_distance_metrics_host
    g = torch.Generator().manual_seed(d)
    big_a, big_b = torch.randn(150, d + 3, generator=g) + 1.5, torch.randn(90, d + 5, generator=g) + 1.5
    a, b = big_a[:, 1:d + 1].to(dev), big_b.to(dev)[:, 2:d + 2]               # a: copied dense; b: a row-strided view
    sa, sb = [0, 70, 70, 71, 150], [0, 3, 10, 10, 90]                         # 70x3, empty A, empty B, 79x80 (two tiles each way)
    dsa, dsb = (torch.tensor(s, dtype=torch.int32, device=dev) for s in (sa, sb))
    got = ops.latent_group_stats(a, dsa, b, dsb)
    want = segmented_distance_metrics_host(a.cpu().numpy(), sa, b.cpu().numpy(), sb)
    assert torch.isnan(got[1]).all() and torch.isnan(got[2]).all()
    assert O.rel_err(got.cpu().numpy(), want) <= 1e-5
    # every other row unchanged when the empty patients are taken out
    keep = ops.latent_group_stats(torch.cat([a[:70], a[71:]]), torch.tensor([0, 70, 149], dtype=torch.int32, device=dev),
                                  torch.cat([b[:3], b[10:]]), torch.tensor([0, 3, 83], dtype=torch.int32, device=dev))
    assert torch.equal(keep, got[[0, 3]])
    out = torch.zeros(6, 4, device=dev)
    assert ops.latent_group_stats(a, dsa, b, dsb, out=out[1:5]).data_ptr() == out[1:5].data_ptr()
    assert torch.equal(out[1:5][[0, 3]], got[[0, 3]]) and float(out[0].abs().max()) == 0.0 and float(out[5].abs().max()) == 0.0
    with pytest.raises(TypeError):
        ops.latent_group_stats(a, dsa.long(), b, dsb)
    with pytest.raises(ValueError):
        ops.latent_group_stats(a, dsa, b, dsb[:-1])
    with pytest.raises(ValueError):
        ops.latent_group_stats(a, dsa, b[:, :-1], dsb)


def test_compute_distance_metrics_on_device_tensors(gold, cases):
    from pti_ldm_vae_amd.analysis import compute_distance_metrics
    a, ids_a, b, ids_b = cases["small"]
    p = 0
    ra = a[[i for i, q in enumerate(ids_a) if q == O.PATIENTS[p]]]
    rb = b[[i for i, q in enumerate(ids_b) if q == O.PATIENTS[p]]]
    got = compute_distance_metrics(ra, rb)
    assert O.rel_err(np.array(got), gold["metrics_small"][p]) <= _bound(gold, "metrics_small_fp32_err")
    assert compute_distance_metrics(ra[:0], rb) is None


# ---- reproducibility -----------------------------------------------------------------------------------------------------
def _same(x, y):
    """Bitwise equality where NaN rows (patients present in one group only) count as equal."""
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))


def test_results_are_bitwise_reproducible_and_local(cases, dev):
    from pti_ldm_vae_amd import ops
    for tag in ("small", "large"):
        a, ids_a, b, ids_b = cases[tag]
        full = ops.latent_pairwise(a, b)
        assert torch.equal(ops.latent_pairwise(a, b), full)
        # any sub-block alone = the same block of the full result: whether D is split over workgroups (few tiles) or
        # not, and wherever the rows fall in a tile, an entry's bits depend on its two rows only
        for r0, r1, c0, c1 in ((0, 48, 0, 40), (5, 6, 7, 8), (13, 45, 2, 39), (47, 48, 0, 40)):
            assert torch.equal(ops.latent_pairwise(a[r0:r1], b[c0:c1]), full[r0:r1, c0:c1]), (tag, r0, r1, c0, c1)
        big = ops.latent_pairwise(torch.cat([a] * 7), torch.cat([b] * 8))    # 336 x 320: 30 tiles, the one-pass route
        assert torch.equal(big[48:96, 280:320], full) and torch.equal(big[:48, :40], full)
        dot = ops.latent_pairwise(a, b, mode="dot", center=a[0])
        assert torch.equal(ops.latent_pairwise(a[9:20], b[30:], mode="dot", center=a[0]), dot[9:20, 30:])
        ga, sa, gb, sb, ha, hb = _grouped(a, ids_a, b, ids_b, dev)
        stats = ops.latent_group_stats(ga, sa, gb, sb)
        assert _same(ops.latent_group_stats(ga, sa, gb, sb), stats)
        # permuting the patients permutes the rows
        perm = [4, 0, 8, 2, 6, 1, 7, 5, 3]
        pa = torch.cat([ga[ha[p]:ha[p + 1]] for p in perm])
        pb = torch.cat([gb[hb[p]:hb[p + 1]] for p in perm])
        psa = torch.tensor([0] + list(np.cumsum([ha[p + 1] - ha[p] for p in perm])), dtype=torch.int32, device=dev)
        psb = torch.tensor([0] + list(np.cumsum([hb[p + 1] - hb[p] for p in perm])), dtype=torch.int32, device=dev)
        moved = ops.latent_group_stats(pa, psa, pb, psb)
        assert _same(moved, stats[perm])
        one = ops.latent_group_stats(ga[ha[3]:ha[4]], torch.tensor([0, ha[4] - ha[3]], dtype=torch.int32, device=dev),
                                     gb[hb[3]:hb[4]], torch.tensor([0, hb[4] - hb[3]], dtype=torch.int32, device=dev))
        assert torch.equal(one[0], stats[3])


# ---- PCA -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["small", "large"])
def test_pca_against_the_reference(gold, cases, dev, tag):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import LatentSpaceAnalyzer
    a, _, b, _ = cases[tag]
    x = torch.cat([a, b])
    gram = ops.latent_pairwise(x, mode="dot", center=x.mean(dim=0))
    assert torch.equal(gram, gram.t())                                        # symmetric bit for bit
    analyzer = LatentSpaceAnalyzer(torch.nn.Identity(), dev, None)
    proj, ratio = analyzer.reduce_dimensionality_pca(x, O.PCA_COMPONENTS)
    proj_np, _ = analyzer.reduce_dimensionality_pca(x.cpu().numpy(), O.PCA_COMPONENTS)
    assert np.array_equal(proj, proj_np) and proj.shape == (88, O.PCA_COMPONENTS) and proj.dtype == np.float64
    assert np.array_equal(proj, O.sign_rule(proj))                            # already in the deterministic sign convention
    err, bound = O.component_err(proj, O.sign_rule(gold[f"pca_{tag}"])), _bound(gold, f"pca_{tag}_fp32_err", floor=1e-3)
    print(f"[{tag}] PCA: per-component relative L2 error {err:.3e} (bound {bound:.1e}, fp32 CPU {float(gold[f'pca_{tag}_fp32_err']):.1e})")
    assert err <= bound
    assert np.abs(ratio - gold[f"pca_ratio_{tag}"]).max() <= 1e-4


# ---- analyze_static end to end ---------------------------------------------------------------------------------------------
def _write_group(folder, patients, per_patient, seed):
    from pti_ldm_vae_amd.data import write_tiff
    rng = np.random.default_rng(seed)
    folder.mkdir(parents=True)
    k = 0
    for patient in patients:
        for _ in range(per_patient):
            h, w = 96 + 8 * (k % 3), 120 - 4 * (k % 5)
            img = rng.standard_normal((h, w)).astype(np.float32) * 300 + 900 + 40 * int(patient)
            yy, xx = np.mgrid[0:h, 0:w]
            img[((xx - w / 2) / (0.4 * w)) ** 2 + ((yy - h / 2) / (0.32 * h)) ** 2 > 1.0] = 0.0
            write_tiff(str(folder / f"{k:03d}_HA_2021_02_{patient}.tif"), img)
            k += 1


def test_analyze_static_end_to_end(dev, tmp_path, monkeypatch):
    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import analyze_static
    from pti_ldm_vae_amd.analysis.latent_space import segmented_distance_metrics_host
    from pti_ldm_vae_amd.models.autoencoder import VAEModel
    from pti_ldm_vae_amd.utils.cli_common import load_config_and_model
    _write_group(tmp_path / "edente", ["11", "12", "13"], 4, seed=1)          # 12 + 12 images, three patients
    _write_group(tmp_path / "dente", ["12", "13", "11"], 4, seed=2)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64])
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)

    calls = []
    encode = VAEModel.encode_deterministic
    monkeypatch.setattr(VAEModel, "encode_deterministic", lambda self, x: (calls.append(x.shape[0]), encode(self, x))[1])
    argv = ["--vae-weights", str(ck), "--config-file", str(tmp_path / "cfg.json"), "--folder-edente", str(tmp_path / "edente"),
            "--folder-dente", str(tmp_path / "dente"), "--method", "pca", "--patch-size", "64", "64", "--color-by-patient",
            "--cache-dir", str(tmp_path / "cache"), "--batch-size", "5", "--dpi", "40"]
    out = tmp_path / "out"
    analyze_static.main(argv + ["--output-dir", str(out)])
    assert calls == [5, 5, 2, 5, 5, 2]                                        # batched encodes of all misses
    for name in ("pca_projection.png", "color_legend.txt", "distance_metrics.txt", "exams_sorted_by_distance.txt", "latents.npz"):
        assert (out / name).is_file() and (out / name).stat().st_size > 0, name
    z = np.load(out / "latents.npz")
    assert z["latents_edente"].shape == (12, 4 * 8 * 8) and z["projection_dente"].shape == (12, 2)
    assert list(z["ids_edente"]) == ["11"] * 4 + ["12"] * 4 + ["13"] * 4 and list(z["ids_dente"]) == ["12"] * 4 + ["13"] * 4 + ["11"] * 4
    assert [os.path.basename(p) for p in z["paths_edente"]] == sorted(os.listdir(tmp_path / "edente"))

    # the statistics equal the fp64 numpy values computed from latents.npz at the printed precision
    lines = (out / "distance_metrics.txt").read_text().splitlines()
    assert lines[0] == "Distance Metrics per Exam (Latent Space and Projection)" and lines[1] == "=" * 60
    blocks = [lines[i:i + 4] for i in range(3, len(lines), 5)]
    assert [b[0] for b in blocks] == ["11", "12", "13"]
    for patient, block in zip(["11", "12", "13"], blocks):
        assert block[1] == "  - n_edente: 4, n_dente: 4"
        for line, key in ((block[2], "latents"), (block[3], "projection")):
            ra = z[f"{key}_edente"][z["ids_edente"] == patient]
            rb = z[f"{key}_dente"][z["ids_dente"] == patient]
            want = segmented_distance_metrics_host(ra, [0, 4], rb, [0, 4])[0]
            got = [float(part.split(": ")[1]) for part in line.split("] ")[1].split(", ")]
            print(patient, key, got, want)
            assert np.abs(np.array(got) - want).max() <= 0.0005 + 1e-5 * np.abs(want).max()

    # the cached latents equal encode_deterministic of the same image encoded alone
    _, model = load_config_and_model(str(tmp_path / "cfg.json"), str(ck), dev)
    pre = analyze_static.TiffPreprocess((64, 64), dev)
    with torch.no_grad():
        for k in (0, 7):
            alone = encode(model, pre(str(z["paths_dente"][k]))[None]).flatten().cpu().numpy()
            assert np.array_equal(alone, z["latents_dente"][k])

    # a second run encodes nothing and writes the same statistics
    calls.clear()
    out2 = tmp_path / "out2"
    analyze_static.main(argv + ["--output-dir", str(out2)])
    assert calls == []
    for name in ("distance_metrics.txt", "exams_sorted_by_distance.txt", "color_legend.txt"):
        assert (out2 / name).read_bytes() == (out / name).read_bytes(), name

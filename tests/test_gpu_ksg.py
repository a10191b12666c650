"""GPU tests of the k-nearest-neighbour (KSG) mutual information: ``pti_ksg_counts`` against ``tests/ksg_oracle.py`` through
``tests/golden/ksg_golden.npz`` -- the radius is one of the fp32 distances and the counts are integers, so the check is
EQUALITY in every cell, bitwise for the radius, no tolerance --, its bitwise properties, the wrapper's refusals, and
``evaluate_disentanglement --mi-estimator ksg`` end to end on a TIFF directory.

Measured on an MI355X: no cell of any table differs in any case (``tiny``, whose differences are subnormal, included); end to
end MI deviates from the oracle by 1.4e-15 and the four scores by at most 5.6e-16.
The first test prints, per case, how many cells of each table differ before it asserts.  Bounds of the end-to-end run: MI
1e-12 against the oracle on the same scaled bits (the oracle's digammas are a compensated sum, the command's a running one:
they differ by about 1e-15 at these n); the scores as in tests/test_gpu_disentanglement.py, 1e-12 for the two that come from
MI and the entropies, 1e-9 for the two that go through r^2."""
import json
import os

import numpy as np
import pytest
import torch

import ksg_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 64


@pytest.fixture(scope="module")
def cases():
    """(spec, seeded inputs) of every oracle case and the golden file: built once and shared."""
    return [(spec, O.make_case(*spec[:7])) for spec in O.CASES], O.load_golden()


def _buffers(case, dev, pads):
    """Channel-major z [L, n + pads[0]] and attrs [na, n + pads[1]] with junk behind every row."""
    zbuf = torch.full((case.l, case.n + pads[0]), 9.0, device=dev)
    zbuf[:, :case.n] = torch.from_numpy(case.z).to(dev).t()
    abuf = torch.full((case.na, case.n + pads[1]), -3.0, device=dev)
    abuf[:, :case.n] = torch.from_numpy(case.attrs).to(dev)
    return zbuf, abuf


def _run(case, k, dev, pads=(0, 0), out=None):
    from pti_ldm_vae_amd import ops
    zbuf, abuf = _buffers(case, dev, pads)
    return ops.ksg_counts(zbuf[:, :case.n].t(), abuf[:, :case.n], k, out=out)


def _same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def _poisoned(case, dev):
    """Three output buffers filled with a poison value, each with CANARY more poisoned elements behind it."""
    size = case.na * case.l * case.n
    flat = (torch.full((size + CANARY,), float("nan"), device=dev), torch.full((size + CANARY,), -7, dtype=torch.int32, device=dev),
            torch.full((size + CANARY,), -7, dtype=torch.int32, device=dev))
    return flat, tuple(f[:size].view(case.na, case.l, case.n) for f in flat)


def test_every_table_equals_the_oracle_in_every_cell(dev, cases):
    specs, gold = cases
    bad = []
    for spec, case in specs:
        for k in case.ks:
            flat, out = _poisoned(case, dev)
            eps, nx, ny = _run(case, k, dev, pads=spec[7], out=out)
            assert eps is out[0] and nx is out[1] and ny is out[2]
            assert eps.dtype == torch.float32 and nx.dtype == torch.int32 and ny.dtype == torch.int32
            size = case.na * case.l * case.n
            if not (bool(torch.isnan(flat[0][size:]).all()) and bool((flat[1][size:] == -7).all()) and bool((flat[2][size:] == -7).all())):
                bad.append(f"{case.name} k {k}: a canary behind an output was overwritten")
            host = dict(eps=eps.cpu().numpy(), nx=nx.cpu().numpy(), ny=ny.cpu().numpy())
            want = {key: gold[f"{case.name}/k{k}/{key}"] for key in O.TABLES}
            diff = dict(eps=int((host["eps"].view(np.int32) != want["eps"].view(np.int32)).sum()),           # bitwise
                        nx=int((host["nx"] != want["nx"].astype(np.int32)).sum()), ny=int((host["ny"] != want["ny"].astype(np.int32)).sum()))
            print(f"{case.name} k {k}: cells that differ: " + ", ".join(f"{key} {v} of {host[key].size}" for key, v in diff.items()))
            bad += [f"{case.name} k {k}: {key} differs in {v} cells" for key, v in diff.items() if v]
            if np.isnan(host["eps"]).any() or (host["nx"] < 0).any() or (host["ny"] < 0).any():
                bad.append(f"{case.name} k {k}: a cell of an output was not written")
    assert bad == [], bad


def test_mutual_information_from_the_device_counts(dev, cases):
    from pti_ldm_vae_amd.utils.disentanglement import ksg_mutual_information
    specs, gold = cases
    for spec, case in specs:
        for k in case.ks:
            _, nx, ny = _run(case, k, dev, pads=spec[7])
            mi = ksg_mutual_information(nx.cpu().numpy(), ny.cpu().numpy(), case.n, k)
            assert np.max(np.abs(mi - gold[f"{case.name}/k{k}/mi"])) <= 1e-12, (case.name, k)
            if case.name == "const":
                assert mi[1].tolist() == [0.0, 0.0] and mi[0, 1] == 0.0


def test_second_call_strides_layouts_and_out_buffers(dev, cases):
    from pti_ldm_vae_amd import ops
    specs, _ = cases
    for idx, k in ((4, 3), (6, 16), (10, 3)):                        # n257 (10 x 6), n2500 (padded strides), tiny (subnormals)
        spec, case = specs[idx]
        a, b = _run(case, k, dev, pads=spec[7]), _run(case, k, dev, pads=spec[7])
        assert _same(a, b), case.name                                                      # bit for bit
        for pads in ((0, 0), (4, 0) if spec[7] == (0, 0) else (1, 7), (3, 129)):
            assert _same(_run(case, k, dev, pads=pads), a), (case.name, pads)
        z_rows = torch.from_numpy(case.z).to(dev)                                           # [N, L] rows: copied once
        attrs = torch.from_numpy(case.attrs).to(dev)
        assert _same(ops.ksg_counts(z_rows, attrs, k), a), case.name
        assert _same(ops.ksg_counts(z_rows.double(), attrs.double(), k), a), case.name
        attrs_t = attrs.t().contiguous().t()                                                # column stride != 1: copied once
        assert _same(ops.ksg_counts(z_rows.t().contiguous().t(), attrs_t, k), a), case.name
        _, out = _poisoned(case, dev)
        got = _run(case, k, dev, pads=spec[7], out=out)
        assert all(x is y for x, y in zip(got, out)) and _same(got, a), case.name
        only_eps = ops.ksg_counts(z_rows, attrs, k, out=(out[0], None, None))
        assert only_eps[0] is out[0] and _same(only_eps, a)


def test_a_pair_does_not_depend_on_the_other_columns(dev, cases):
    from pti_ldm_vae_amd import ops
    specs, _ = cases
    spec, case = specs[4]                                                                   # n257, 10 x 6
    z, attrs = torch.from_numpy(case.z).to(dev), torch.from_numpy(case.attrs).to(dev)
    full = ops.ksg_counts(z, attrs, 3)
    for q, c in ((0, 0), (5, 9), (2, 7)):
        alone = ops.ksg_counts(z[:, c:c + 1], attrs[q:q + 1], 3)
        assert _same(alone, tuple(t[q:q + 1, c:c + 1] for t in full)), (q, c)
    gen = torch.Generator().manual_seed(1)
    z2, a2 = torch.randn(case.n, case.l, generator=gen).to(dev), torch.randn(case.na, case.n, generator=gen).to(dev)
    z2[:, 7], a2[2] = z[:, 7], attrs[2]                                                     # every other column replaced
    other = ops.ksg_counts(z2, a2, 3)
    assert _same(tuple(t[2:3, 7:8] for t in other), tuple(t[2:3, 7:8] for t in full))
    moved = ops.ksg_counts(z2[:, [7, 0, 1]], a2[[4, 2]], 3)                                 # ... and the pair moved in the launch
    assert _same(tuple(t[1:2, 0:1] for t in moved), tuple(t[2:3, 7:8] for t in full))


def test_wrapper_refusals(dev):
    from pti_ldm_vae_amd import ops
    z, a = torch.rand(10, 3, device=dev), torch.rand(2, 10, device=dev)
    eps, nx, ny = ops.ksg_counts(z, a, 3)                                                   # the accepted call
    assert tuple(eps.shape) == (2, 3, 10) and tuple(nx.shape) == (2, 3, 10) and tuple(ny.shape) == (2, 3, 10)
    ops.ksg_counts(z, a, 9)                                                                 # n = k + 1
    bad = z.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="channel 1 holds a non-finite value"):
        ops.ksg_counts(bad, a, 3)
    bad = a.clone()
    bad[1, 7] = float("-inf")
    with pytest.raises(ValueError, match="attribute 1 holds a non-finite value"):
        ops.ksg_counts(z, bad, 3)
    with pytest.raises(TypeError, match="ksg_counts: attrs"):
        ops.ksg_counts(z, a.long(), 3)
    with pytest.raises(TypeError, match="ksg_counts: z"):
        ops.ksg_counts(z.int(), a, 3)
    with pytest.raises(TypeError, match="ksg_counts: k"):
        ops.ksg_counts(z, a, 3.0)
    with pytest.raises(ValueError, match="expected a matrix"):
        ops.ksg_counts(z[:, 0], a, 3)
    with pytest.raises(ValueError, match="attrs"):
        ops.ksg_counts(z, torch.rand(2, 9, device=dev), 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.ksg_counts(z.cpu(), a, 3)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="ksg_counts: k = "):
            ops.ksg_counts(z, a, k)
    with pytest.raises(TypeError):
        ops.ksg_counts(z, a, 3, out=(None, torch.zeros(2, 3, 10, device=dev), None))
    with pytest.raises(ValueError):
        ops.ksg_counts(z, a, 3, out=(torch.zeros(2, 3, 9, device=dev), None, None))
    for zz, aa, k in ((torch.rand(10, 17, device=dev), a, 3),                                              # L past the limit
                      (z, torch.rand(17, 10, device=dev), 3),                                              # na
                      (z, a, 10),                                                                          # n < k + 1
                      (torch.rand(1, 3, device=dev), torch.rand(2, 1, device=dev), 1),
                      (torch.rand(32769, 1, device=dev), torch.rand(1, 32769, device=dev), 3)):
        with pytest.raises(ValueError, match="ksg_counts: unsupported shape"):
            ops.ksg_counts(zz, aa, k)


# ---- end to end ---------------------------------------------------------------------------------------------------------
N_IMAGES = 21
TODAYS_KEYS = {"scores", "attributes", "spearman_rho", "mutual_information", "pearson_r", "entropy", "bins", "n_images",
               "excluded", "args", "files"}
SCORES = ("mig", "modularity", "sap", "interpretability")


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """21 synthetic 64 x 64 TIFFs, an attribute file with ties, the AR config at 64 x 64 with a [32, 64]-channel VAE."""
    from pti_ldm_vae_amd.data import write_tiff
    tmp = tmp_path_factory.mktemp("ksg")
    rng = np.random.default_rng(6)
    d = tmp / "data" / "dente"
    d.mkdir(parents=True)
    cfg = json.load(open(os.path.join(ROOT, "config", "ar_vae_dente_kl1e3.json")))
    names = list(cfg["regularized_attributes"]["attribute_latent_mapping"])
    table = {}
    for i in range(N_IMAGES):
        img = np.zeros((64, 64), np.float32)
        hh, ww = 12 + 2 * (i % 9), 10 + 3 * (i % 7)
        img[6:6 + hh, 8:8 + ww] = 1.0 + rng.random((hh, ww), dtype=np.float32)
        write_tiff(str(d / f"img_{i:03d}.tif"), img)
        table[f"img_{i:03d}.tif"] = {"height_0": float(hh), "other": 1.0,
                                     **{f"width_{k}": float(ww // (k + 1)) for k in range(5)}}     # plenty of ties
    af = tmp / "attrs.json"
    af.write_text(json.dumps(table))
    cfg["autoencoder_def"].update(channels=[32, 64], attention_levels=[False, False], num_res_blocks=1, norm_num_groups=16)
    cfg["autoencoder_train"]["patch_size"] = [64, 64]
    cfg["run_dir"] = str(tmp / "run")
    cfg["regularized_attributes"]["attribute_file"] = str(af)
    cf = tmp / "ar.json"
    cf.write_text(json.dumps(cfg))
    return dict(tmp=tmp, cfg=str(cf), data=str(tmp / "data"), attrs=str(af), names=names, table=table)


def _reference_scores(mi, h, pearson):
    """The four scores and the per-attribute MIG from an MI matrix, entropies and Pearson's r (NaN where undefined): the
    definitions of tests/disentanglement_oracle.report."""
    import disentanglement_oracle as DO
    na, l = mi.shape
    r2 = pearson ** 2
    mig = np.array([DO._nan_gap(mi[q]) / h[q] if h[q] > 0 else np.nan for q in range(na)])
    sap = np.array([DO._nan_gap(r2[q]) for q in range(na)])
    interp = np.array([r2[q, int(np.argmax(mi[q]))] if h[q] > 0 else np.nan for q in range(na)])
    sq = mi ** 2
    modularity = np.array([1.0 - (sq[:, c].sum() - sq[:, c].max()) / (sq[:, c].max() * (na - 1)) if na >= 2 and sq[:, c].max() > 0
                           else np.nan for c in range(l)])
    return np.array([DO._nan_mean(mig), DO._nan_mean(modularity), DO._nan_mean(sap), DO._nan_mean(interp)]), mig


def test_evaluate_disentanglement_ksg_end_to_end(dev, run):
    import disentanglement_oracle as DO
    from pti_ldm_vae_amd import evaluate_ar_vae as A
    from pti_ldm_vae_amd import evaluate_disentanglement as E
    from pti_ldm_vae_amd.data import create_regression_eval_dataloader
    from pti_ldm_vae_amd.utils.config import load_vae_config
    from pti_ldm_vae_amd.utils.disentanglement import ksg_scale
    base = ["-c", run["cfg"], "--checkpoint", str(run["tmp"] / "nope.pth"), "--input-dir", run["data"], "--random-init-vae",
            "--batch-size", "5", "--num-workers", "2"]
    E.main(base + ["--mi-estimator", "ksg"])
    out = run["tmp"] / "run" / "ar_eval"
    first = (out / "disentanglement.json").read_bytes()
    doc = json.loads(first)
    assert set(doc) == TODAYS_KEYS | {"mutual_information_binned", "mi_estimator", "ksg_neighbors"}
    assert doc["mi_estimator"] == "ksg" and doc["ksg_neighbors"] == 3 and doc["n_images"] == N_IMAGES
    assert doc["args"]["mi_estimator"] == "ksg" and doc["args"]["ksg_neighbors"] == 3 and doc["args"]["batch_size"] == 5
    names = run["names"]
    # z = the public encode_deterministic on the same batches, reduced the documented way
    torch.manual_seed(42)
    model = A.load_model(load_vae_config(run["cfg"]), "", dev, True)
    loader, _ = create_regression_eval_dataloader(run["data"], run["attrs"], names, (64, 64), 5, num_workers=2,
                                                  data_source="dente", device=dev)
    with torch.no_grad():
        z = torch.cat([model.encode_deterministic(images).double().mean((2, 3)).float() for images, _ in loader]).cpu().numpy()
    attrs = np.array([[run["table"][f][k] for f in doc["files"]] for k in names], np.float32)
    l = z.shape[1]
    scaled = ksg_scale(np.concatenate([z.T, attrs]))                 # the oracle is fed the bits the kernel is fed
    want = O.case_tables(scaled[:l].T, scaled[l:], 3)["mi"]
    got = np.array(doc["mutual_information"])
    dev_mi = float(np.max(np.abs(got - want)))
    print(f"evaluate_disentanglement --mi-estimator ksg: MI deviates by at most {dev_mi:.3e}; MI {want.min():.4f} .. {want.max():.4f}")
    assert got.shape == (len(names), l) and dev_mi <= 1e-12
    r = DO.report(z, attrs, 20)                                      # everything else is the histogram report's
    assert float(np.max(np.abs(np.array(doc["mutual_information_binned"]) - r["mutual_information"]))) <= 1e-12
    assert float(np.max(np.abs(np.array(doc["entropy"]) - r["entropy"]))) <= 1e-12
    ref, mig = _reference_scores(want, r["entropy"], r["pearson_r"])
    scores = np.array([np.nan if doc["scores"][k] is None else doc["scores"][k] for k in SCORES])
    print("evaluate_disentanglement --mi-estimator ksg: scores deviate by "
          + ", ".join(f"{k} {abs(g - w):.3e}" for k, g, w in zip(SCORES, scores, ref)))
    assert not np.isnan(scores).any() and np.all(np.abs(scores - ref)[:2] <= 1e-12)            # MIG, modularity: from MI and H
    assert np.all(np.abs(scores - ref)[2:] <= 1e-9)                                            # SAP, interpretability: from r^2
    for q, k in enumerate(names):
        assert abs(doc["attributes"][k]["mig"] - mig[q]) <= 1e-12
    from PIL import Image
    with Image.open(out / "disentanglement.png") as im:
        assert im.format == "PNG"
    E.main(base + ["--mi-estimator", "ksg"])                                        # a second run: the same bytes
    assert (out / "disentanglement.json").read_bytes() == first
    # --from-npz on the channel_means.npz of an evaluate_ar_vae run over the same directory: the same report
    A.main(base)
    other = run["tmp"] / "from_npz"
    E.main(["-c", run["cfg"], "--from-npz", str(out / "channel_means.npz"), "--output-dir", str(other), "--mi-estimator", "ksg"])
    again = json.loads((other / "disentanglement.json").read_text())
    for key in ("scores", "attributes", "spearman_rho", "mutual_information", "mutual_information_binned", "pearson_r", "entropy",
                "excluded", "files", "mi_estimator", "ksg_neighbors"):
        assert again[key] == doc[key], key
    # without the flag: no new key, in the report or in its args; the histogram MI is where it was
    plain = run["tmp"] / "binned"
    E.main(base + ["--output-dir", str(plain)])
    default = json.loads((plain / "disentanglement.json").read_text())
    assert set(default) == TODAYS_KEYS and "mi_estimator" not in default["args"] and "ksg_neighbors" not in default["args"]
    assert default["mutual_information"] == doc["mutual_information_binned"] and default["spearman_rho"] == doc["spearman_rho"]
    with pytest.raises(SystemExit, match="3 images"):
        E.main(base + ["--mi-estimator", "ksg", "--num-samples", "3", "--output-dir", str(run["tmp"] / "few")])

"""GPU tests of the disentanglement report: ``pti_tied_ranks`` / ``pti_rank_moments`` / ``pti_joint_histogram`` against
``tests/disentanglement_oracle.py`` through ``tests/golden/disentanglement_golden.npz`` -- every table is an integer table, so
the check is EQUALITY in every cell, no tolerance --, their bitwise properties, the wrappers' refusals, and the command end
to end on a TIFF directory.

Measured on an MI355X: no cell of any table differs in any case; end to end Spearman's rho deviates from the oracle by at most
1.1e-16, MI by 2.2e-16 and the four scores by 5.6e-17 (bounds: 1e-12, and 1e-9 for the two scores that go through r^2).  The
first test prints, per case, how many cells of each table differ before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import disentanglement_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    """(spec, seeded inputs) of every oracle case and the golden file: built once and shared."""
    return [(spec, O.make_case(*spec[:7])) for spec in O.CASES], O.load_golden()


def _buffers(case, dev, pads):
    """Channel-major z [L, n + pads[0]] and attrs [na, n + pads[1]] with junk behind every row, and the column table
    [L + na, n + max(pads)] of the same values."""
    zbuf = torch.full((case.l, case.n + pads[0]), 9.0, device=dev)
    zbuf[:, :case.n] = torch.from_numpy(case.z).to(dev).t()
    abuf = torch.full((case.na, case.n + pads[1]), -3.0, device=dev)
    abuf[:, :case.n] = torch.from_numpy(case.attrs).to(dev)
    cbuf = torch.full((case.l + case.na, case.n + max(pads)), 5.0, device=dev)
    cbuf[:, :case.n] = torch.cat([zbuf[:, :case.n], abuf[:, :case.n]])
    return zbuf, abuf, cbuf


def _run(case, gold, dev, pads=(0, 0), out=(None, None, None)):
    """The three ops on ``case`` -> {table name: device tensor}; the edges are the golden file's."""
    from pti_ldm_vae_amd import ops
    zbuf, abuf, cbuf = _buffers(case, dev, pads)
    edges = gold[f"{case.name}/edges"]
    rank2 = ops.tied_ranks(cbuf[:, :case.n], out=out[0])
    sums, gram = ops.rank_moments(rank2, out=out[1])
    bins_z, bins_a, counts = ops.joint_histogram(zbuf[:, :case.n].t(), abuf[:, :case.n], edges[:case.l], torch.from_numpy(edges[case.l:]),
                                                 out=out[2])
    return dict(rank2=rank2, sums=sums, gram=gram, bins=torch.cat([bins_z, bins_a]), counts=counts,
                parts=(rank2, (sums, gram), (bins_z, bins_a, counts)))


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("rank2", "sums", "gram", "bins", "counts"))


def test_every_table_equals_the_oracle_in_every_cell(dev, cases):
    specs, gold = cases
    bad = []
    for spec, case in specs:
        got = _run(case, gold, dev, pads=spec[7])
        m = case.l + case.na
        assert got["rank2"].dtype == torch.int32 and tuple(got["rank2"].shape) == (m, case.n) and got["rank2"].is_cuda
        assert got["sums"].dtype == torch.int64 and tuple(got["sums"].shape) == (m,)
        assert got["gram"].dtype == torch.int64 and tuple(got["gram"].shape) == (m, m)
        assert got["bins"].dtype == torch.uint8 and tuple(got["bins"].shape) == (m, case.n)
        assert got["counts"].dtype == torch.int32 and tuple(got["counts"].shape) == (case.na, case.l, case.bins, case.bins)
        host = {k: got[k].cpu().numpy() for k in ("rank2", "sums", "gram", "bins", "counts")}
        diff = {k: int((host[k] != gold[f"{case.name}/{k}"]).sum()) for k in host}
        print(f"{case.name}: cells that differ: " + ", ".join(f"{k} {v} of {host[k].size}" for k, v in diff.items()))
        bad += [f"{case.name}: {k} differs in {v} cells" for k, v in diff.items() if v]
        if not np.all(host["rank2"].astype(np.int64).sum(1) == case.n * (case.n + 1)):
            bad.append(f"{case.name}: a row of rank2 does not sum to n (n + 1)")
        if not np.all(host["counts"].astype(np.int64).sum((2, 3)) == case.n):
            bad.append(f"{case.name}: a [B][B] table does not sum to n")
    assert bad == [], bad


def test_second_call_strides_layouts_and_out_buffers(dev, cases):
    from pti_ldm_vae_amd import ops
    specs, gold = cases
    for idx in (3, 5):                                              # n257 (10 x 6) and n2500 (padded strides, two chunks)
        spec, case = specs[idx]
        a, b = _run(case, gold, dev, pads=spec[7]), _run(case, gold, dev, pads=spec[7])
        assert _same(a, b), case.name                                                      # bit for bit
        for pads in ((0, 0), (4, 0) if spec[7] == (0, 0) else (1, 7)):
            assert _same(_run(case, gold, dev, pads=pads), a), (case.name, pads)
        edges = torch.from_numpy(gold[f"{case.name}/edges"]).to(dev)
        z_rows = torch.from_numpy(case.z).to(dev)                                           # [N, L] rows: copied once
        attrs = torch.from_numpy(case.attrs).to(dev)
        bz, ba, counts = ops.joint_histogram(z_rows, attrs.double(), edges[:case.l], edges[case.l:])
        assert torch.equal(torch.cat([bz, ba]), a["bins"]) and torch.equal(counts, a["counts"]), case.name
        cols_t = torch.cat([z_rows.t(), attrs]).t().contiguous().t()                        # column stride != 1: copied once
        assert torch.equal(ops.tied_ranks(cols_t), a["rank2"]) and torch.equal(ops.tied_ranks(cols_t.double()), a["rank2"])
        m = case.l + case.na
        out = (torch.full((m, case.n), -1, dtype=torch.int32, device=dev),
               (torch.full((m,), -1, dtype=torch.int64, device=dev), torch.full((m, m), -1, dtype=torch.int64, device=dev)),
               (torch.full((case.l, case.n), 77, dtype=torch.uint8, device=dev),
                torch.full((case.na, case.n), 77, dtype=torch.uint8, device=dev),
                torch.full((case.na, case.l, case.bins, case.bins), -1, dtype=torch.int32, device=dev)))
        got = _run(case, gold, dev, pads=spec[7], out=out)
        assert got["parts"][0] is out[0] and got["parts"][1][0] is out[1][0] and got["parts"][1][1] is out[1][1]
        assert all(x is y for x, y in zip(got["parts"][2], out[2])) and _same(got, a), case.name


def test_wrapper_refusals(dev):
    from pti_ldm_vae_amd import ops
    z, a = torch.rand(10, 3, device=dev), torch.rand(2, 10, device=dev)
    ez, ea = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64)
    ops.joint_histogram(z, a, ez, ea)                                                        # the accepted call
    low = z.clone()
    low[4, 1] = -0.5
    with pytest.raises(ValueError, match="channel 1 holds a value below its first edge"):
        ops.joint_histogram(low, a, ez, ea)
    low = a.clone()
    low[1, 7] = -1e-30
    with pytest.raises(ValueError, match="attribute 1 holds a value below its first edge"):
        ops.joint_histogram(z, low, ez, ea)
    with pytest.raises(TypeError, match="joint_histogram: attrs"):
        ops.joint_histogram(z, a.long(), ez, ea)
    with pytest.raises(TypeError, match="joint_histogram: edges_z"):
        ops.joint_histogram(z, a, ez.long(), ea)
    with pytest.raises(ValueError, match="joint_histogram: edges_a"):
        ops.joint_histogram(z, a, ez, ea[:, :3])
    with pytest.raises(ValueError, match="attrs"):
        ops.joint_histogram(z, torch.rand(2, 9, device=dev), ez, ea)
    with pytest.raises(ValueError, match="CUDA"):
        ops.joint_histogram(z.cpu(), a, ez, ea)
    with pytest.raises(TypeError):
        ops.joint_histogram(z, a, ez, ea, out=(None, None, torch.zeros(2, 3, 4, 4, device=dev)))
    for zz, aa, e1, e2 in ((torch.rand(10, 17, device=dev), a, torch.zeros(17, 4), ea),                       # L past the limit
                           (z, torch.rand(17, 10, device=dev), ez, torch.zeros(17, 4)),                       # na
                           (z, a, torch.zeros(3, 33), torch.zeros(2, 33)),                                    # B
                           (z, a, torch.zeros(3, 1), torch.zeros(2, 1)),
                           (torch.rand(1, 3, device=dev), torch.rand(2, 1, device=dev), ez, ea),              # N
                           (torch.rand(32769, 1, device=dev), torch.rand(1, 32769, device=dev), ez[:1], ea[:1])):
        with pytest.raises(ValueError, match="joint_histogram: unsupported shape"):
            ops.joint_histogram(zz, aa, e1, e2)
    for cols in (torch.rand(33, 10, device=dev), torch.rand(2, 32769, device=dev), torch.rand(2, 1, device=dev)):
        with pytest.raises(ValueError, match="tied_ranks: unsupported shape"):
            ops.tied_ranks(cols)
        with pytest.raises(ValueError, match="rank_moments: unsupported shape"):
            ops.rank_moments(torch.ones(cols.shape, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError, match="tied_ranks: cols"):
        ops.tied_ranks(torch.ones(2, 10, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="CUDA"):
        ops.tied_ranks(torch.rand(2, 10))
    with pytest.raises(TypeError):
        ops.tied_ranks(torch.rand(2, 10, device=dev), out=torch.zeros(2, 10, device=dev))
    with pytest.raises(TypeError, match="rank_moments: rank2"):
        ops.rank_moments(torch.rand(2, 10, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        ops.rank_moments(torch.ones(2, 20, dtype=torch.int32, device=dev)[:, :10])
    with pytest.raises(TypeError):
        ops.rank_moments(torch.ones(2, 10, dtype=torch.int32, device=dev), out=(torch.zeros(2, device=dev), None))


# ---- end to end ---------------------------------------------------------------------------------------------------------
N_IMAGES = 23


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """23 synthetic 64 x 64 TIFFs, an attribute file with ties, the AR config at 64 x 64 with a [32, 64]-channel VAE."""
    from pti_ldm_vae_amd.data import write_tiff
    tmp = tmp_path_factory.mktemp("disentanglement")
    rng = np.random.default_rng(4)
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
    cfg["regularized_attributes"]["attribute_latent_mapping"]["width_4"] = {"latent_channel": 7, "delta": 2.5}
    cf = tmp / "ar.json"
    cf.write_text(json.dumps(cfg))
    return dict(tmp=tmp, cfg=str(cf), data=str(tmp / "data"), attrs=str(af), names=names, table=table)


def _nan(rows):
    return np.array([[np.nan if v is None else v for v in row] for row in rows], dtype=np.float64)


def test_evaluate_disentanglement_end_to_end(dev, run):
    from pti_ldm_vae_amd import evaluate_ar_vae as A
    from pti_ldm_vae_amd import evaluate_disentanglement as E
    from pti_ldm_vae_amd.data import create_regression_eval_dataloader
    from pti_ldm_vae_amd.utils.config import load_vae_config
    base = ["-c", run["cfg"], "--checkpoint", str(run["tmp"] / "nope.pth"), "--input-dir", run["data"], "--random-init-vae",
            "--batch-size", "5", "--num-workers", "2"]
    E.main(base)                                                                    # default output dir, attribute file, bins
    out = run["tmp"] / "run" / "ar_eval"
    first = (out / "disentanglement.json").read_bytes()
    doc = json.loads(first)
    assert set(doc) == {"scores", "attributes", "spearman_rho", "mutual_information", "pearson_r", "entropy", "bins", "n_images",
                        "excluded", "args", "files"}
    names = run["names"]
    assert list(doc["attributes"]) == names and doc["n_images"] == N_IMAGES and doc["bins"] == 20
    assert doc["files"] == [f"img_{i:03d}.tif" for i in range(N_IMAGES)]
    assert doc["args"]["batch_size"] == 5 and doc["args"]["resolved_attributes_path"] == run["attrs"]
    # z = the public encode_deterministic on the same batches, reduced the documented way
    torch.manual_seed(42)
    model = A.load_model(load_vae_config(run["cfg"]), "", dev, True)
    loader, _ = create_regression_eval_dataloader(run["data"], run["attrs"], names, (64, 64), 5, num_workers=2,
                                                  data_source="dente", device=dev)
    with torch.no_grad():
        z = torch.cat([model.encode_deterministic(images).double().mean((2, 3)).float() for images, _ in loader]).cpu().numpy()
    attrs = np.array([[run["table"][f][k] for f in doc["files"]] for k in names], np.float32)
    # the JSON = the oracle applied to that z: the integer-derived quantities to 1e-12
    r = O.report(z, attrs, 20)
    for key in ("spearman_rho", "mutual_information"):
        got = _nan(doc[key])
        assert np.array_equal(np.isnan(got), np.isnan(r[key])), key
        dev_k = float(np.max(np.abs(got - r[key])[~np.isnan(got)]))
        print(f"evaluate_disentanglement: {key} deviates by at most {dev_k:.3e}")
        assert dev_k <= 1e-12, key
    assert float(np.max(np.abs(np.array(doc["entropy"]) - r["entropy"]))) <= 1e-12
    pearson = _nan(doc["pearson_r"])
    assert np.array_equal(np.isnan(pearson), np.isnan(r["pearson_r"]))
    np.testing.assert_allclose(pearson[~np.isnan(pearson)], r["pearson_r"][~np.isnan(pearson)], rtol=1e-10, atol=0)
    got = np.array([np.nan if doc["scores"][k] is None else doc["scores"][k] for k in O.SCORES])
    print("evaluate_disentanglement: scores deviate by " + ", ".join(f"{k} {abs(g - w):.3e}" for k, g, w in zip(O.SCORES, got, r["scores"])))
    assert not np.isnan(got).any() and np.all(np.abs(got - r["scores"])[:2] <= 1e-12)          # MIG, modularity: from the counts
    assert np.all(np.abs(got - r["scores"])[2:] <= 1e-9)                                       # SAP, interpretability: from r^2
    channels = [0, 1, 2, 3, 4, 7]
    for q, k in enumerate(names):
        entry = doc["attributes"][k]
        assert entry["latent_channel"] == channels[q] and entry["spearman_rho"] == doc["spearman_rho"][q][channels[q]]
        assert entry["best_channel_spearman"] == int(np.nanargmax(np.abs(r["spearman_rho"][q])))
        assert entry["mapped_channel_is_best"] == (entry["best_channel_spearman"] == channels[q])
        assert abs(entry["mig"] - r["mig"][q]) <= 1e-12 and abs(entry["sap"] - r["sap"][q]) <= 1e-9
    assert doc["excluded"] == {k: [] for k in O.SCORES}
    from PIL import Image
    with Image.open(out / "disentanglement.png") as im:
        assert im.format == "PNG"
    E.main(base)                                                                    # a second run: the same bytes
    assert (out / "disentanglement.json").read_bytes() == first
    # --from-npz on the channel_means.npz of an evaluate_ar_vae run over the same directory: the same report
    A.main(base)
    with np.load(out / "channel_means.npz") as f:
        assert np.array_equal(f["z"], z)
    other = run["tmp"] / "from_npz"
    E.main(["-c", run["cfg"], "--from-npz", str(out / "channel_means.npz"), "--output-dir", str(other)])
    again = json.loads((other / "disentanglement.json").read_text())
    for key in ("scores", "attributes", "spearman_rho", "mutual_information", "pearson_r", "entropy", "excluded", "files"):
        assert again[key] == doc[key], key
    assert (out / "disentanglement.json").read_bytes() == first                     # the other run wrote elsewhere

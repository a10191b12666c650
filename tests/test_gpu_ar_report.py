"""GPU tests of the attribute-ordering report: ``pti_rank_agreement`` against ``tests/ar_report_oracle.py`` (counts exact,
``ar_loss`` within the gate recorded in ``tests/golden/ar_report_golden.npz``: 2 x the deviation of the fp32 CPU
restatement from fp64), its bitwise properties, and both commands end to end on a TIFF directory.

The kernel forms the summand in fp64; the gates are 5.7e-8 .. 8.3e-7 (0 for the case without a qualifying pair, where
both sides are exactly 0).  Measured on an MI355X: counts equal in every cell of every case, ``ar_loss`` deviation at most
1.2e-15 (n = 2500).  The first test prints every case's deviation before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import ar_report_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    """(spec, seeded inputs) of every oracle case and the golden file: built once and shared."""
    return [(spec, O.make_case(*spec[:6])) for spec in O.CASES], O.load_golden()


def _run(case, dev, pads=(0, 0), out=None):
    """The kernel on ``case`` with ``pads`` extra columns behind every channel-major row of z / row of attrs."""
    from pti_ldm_vae_amd import ops
    zbuf = torch.full((case.l, case.n + pads[0]), 9.0, device=dev)
    zbuf[:, :case.n] = torch.from_numpy(case.z).to(dev).t()
    abuf = torch.full((case.na, case.n + pads[1]), -3.0, device=dev)
    abuf[:, :case.n] = torch.from_numpy(case.attrs).to(dev)
    return ops.rank_agreement(zbuf[:, :case.n].t(), abuf[:, :case.n], case.channels.tolist(), case.deltas.tolist(), out=out)


def test_counts_are_exact_and_the_loss_is_inside_the_gate(dev, cases):
    specs, gold = cases
    bad = []
    for spec, case in specs:
        counts, loss_sum = _run(case, dev, pads=spec[6])
        assert counts.dtype == torch.int64 and tuple(counts.shape) == (case.na, case.l, 5) and counts.is_cuda
        assert loss_sum.dtype == torch.float64 and tuple(loss_sum.shape) == (case.na,)
        counts, loss_sum = counts.cpu().numpy(), loss_sum.cpu().numpy()
        want = gold[f"{case.name}/counts"]
        pairs = counts[:, 0, :3].sum(-1)
        ar_loss = np.where(pairs > 0, loss_sum / np.maximum(pairs, 1), 0.0)
        dev_k, gate = O.loss_deviation(ar_loss, gold[f"{case.name}/ar_loss"]), float(gold[f"{case.name}/gate"])
        print(f"{case.name}: counts differ in {int((counts != want).sum())} cells, ar_loss deviation {dev_k:.3e} (gate {gate:.3e})")
        if not np.array_equal(counts, want):
            bad.append(f"{case.name}: counts")
        if not np.all(counts.sum(-1) == case.n * (case.n - 1) // 2):
            bad.append(f"{case.name}: the classes do not sum to n (n - 1) / 2")
        if not dev_k <= gate:
            bad.append(f"{case.name}: ar_loss deviation {dev_k:.3e} > gate {gate:.3e}")
    assert bad == [], bad


def test_second_call_strides_and_out_buffers(dev, cases):
    from pti_ldm_vae_amd import ops
    specs, _ = cases
    for idx in (3, 5):                                              # n257 (10 x 6) and n2500 (padded strides)
        spec, case = specs[idx]
        a, b = _run(case, dev, pads=spec[6]), _run(case, dev, pads=spec[6])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), case.name            # bit for bit
        packed = _run(case, dev, pads=(0, 0))
        other = _run(case, dev, pads=(4, 0) if spec[6] == (0, 0) else (1, 7))
        for got in (packed, other):
            assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1]), case.name
        rows = ops.rank_agreement(torch.from_numpy(case.z).to(dev), torch.from_numpy(case.attrs).to(dev).double(),
                                  torch.from_numpy(case.channels), torch.from_numpy(case.deltas))   # [N, L] rows: copied once
        assert torch.equal(rows[0], a[0]) and torch.equal(rows[1], a[1]), case.name
        counts = torch.full((case.na, case.l, 5), -1, dtype=torch.int64, device=dev)
        loss = torch.full((case.na,), -1.0, dtype=torch.float64, device=dev)
        got = _run(case, dev, pads=spec[6], out=(counts, loss))
        assert got[0] is counts and got[1] is loss and torch.equal(counts, a[0]) and torch.equal(loss, a[1])


def test_wrapper_refusals(dev):
    from pti_ldm_vae_amd import ops
    z, a = torch.zeros(10, 3, device=dev), torch.zeros(2, 10, device=dev)
    with pytest.raises(ValueError, match="attrs"):
        ops.rank_agreement(z, torch.zeros(2, 9, device=dev), [0, 1], [1.0, 1.0])
    with pytest.raises(ValueError, match="one value per attribute"):
        ops.rank_agreement(z, a, [0], [1.0, 1.0])
    with pytest.raises(ValueError, match="below the 3 latent channels"):
        ops.rank_agreement(z, a, [0, 3], [1.0, 1.0])
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.rank_agreement(torch.zeros(10, 17, device=dev), a, [0, 1], [1.0, 1.0])
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.rank_agreement(torch.zeros(1, 3, device=dev), torch.zeros(2, 1, device=dev), [0, 1], [1.0, 1.0])
    with pytest.raises(TypeError):
        ops.rank_agreement(z, a.long(), [0, 1], [1.0, 1.0])
    with pytest.raises(ValueError, match="CUDA"):
        ops.rank_agreement(z.cpu(), a, [0, 1], [1.0, 1.0])
    with pytest.raises(TypeError):
        ops.rank_agreement(z, a, [0, 1], [1.0, 1.0], out=(torch.zeros(2, 3, 5, device=dev), None))


# ---- end to end ---------------------------------------------------------------------------------------------------------
N_IMAGES = 23


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """23 synthetic 64 x 64 TIFFs, an attribute file with ties, the AR config at 64 x 64 with a [32, 64]-channel VAE."""
    from pti_ldm_vae_amd.data import write_tiff
    tmp = tmp_path_factory.mktemp("ar_report")
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


def test_evaluate_ar_vae_end_to_end(dev, run, cases):
    from pti_ldm_vae_amd import evaluate_ar_vae as E
    from pti_ldm_vae_amd.data import create_regression_eval_dataloader
    from pti_ldm_vae_amd.utils.config import load_vae_config
    base = ["-c", run["cfg"], "--checkpoint", str(run["tmp"] / "nope.pth"), "--input-dir", run["data"], "--random-init-vae",
            "--batch-size", "5", "--num-workers", "2"]
    E.main(base)                                                                    # default output dir and attribute file
    out = run["tmp"] / "run" / "ar_eval"
    first = (out / "ar_metrics.json").read_bytes()
    doc = json.loads(first)
    assert set(doc) == {"attributes", "kendall_tau_b", "concordance", "pearson_r", "counts", "n_images", "args", "files"}
    names = run["names"]
    assert list(doc["attributes"]) == names and doc["n_images"] == N_IMAGES
    assert doc["files"] == [f"img_{i:03d}.tif" for i in range(N_IMAGES)]
    assert doc["args"]["batch_size"] == 5 and doc["args"]["resolved_attributes_path"] == run["attrs"]
    npz = np.load(out / "channel_means.npz")
    z, attrs = npz["z"], npz["attrs"]
    assert z.shape == (N_IMAGES, 10) and z.dtype == np.float32 and list(npz["names"]) == names and list(npz["files"]) == doc["files"]
    want_attrs = np.array([[run["table"][f][k] for f in doc["files"]] for k in names], np.float32)
    assert np.array_equal(attrs, want_attrs)
    # z = the public encode_deterministic on the same batches, reduced the documented way
    torch.manual_seed(42)
    config = load_vae_config(run["cfg"])
    model = E.load_model(config, "", dev, True)
    loader, _ = create_regression_eval_dataloader(run["data"], run["attrs"], names, (64, 64), 5, num_workers=2,
                                                  data_source="dente", device=dev)
    with torch.no_grad():
        want_z = torch.cat([model.encode_deterministic(images).double().mean((2, 3)).float() for images, _ in loader])
    assert np.array_equal(z, want_z.cpu().numpy())
    # the JSON = the oracle applied to that z
    channels, deltas = [0, 1, 2, 3, 4, 7], [1.0] * 5 + [2.5]
    r = O.report(z, attrs, channels, deltas)
    assert np.array_equal(np.array(doc["counts"], dtype=np.int64), r["counts"])
    gate = O.gate_of(r["ar_loss"], O.ar_loss_fp32(z, attrs, channels, deltas))
    got = np.array([doc["attributes"][k]["ar_loss"] for k in names])
    print(f"evaluate_ar_vae: ar_loss deviation {O.loss_deviation(got, r['ar_loss']):.3e} (gate {gate:.3e})")
    assert O.loss_deviation(got, r["ar_loss"]) <= gate
    tau = np.array([[np.nan if v is None else v for v in row] for row in doc["kendall_tau_b"]], dtype=np.float64)
    assert np.array_equal(np.isnan(tau), np.isnan(r["kendall_tau_b"]))
    np.testing.assert_allclose(tau[~np.isnan(tau)], r["kendall_tau_b"][~np.isnan(tau)], rtol=1e-13, atol=0)
    for q, k in enumerate(names):
        entry = doc["attributes"][k]
        assert entry["latent_channel"] == channels[q] and entry["delta"] == deltas[q] and entry["pairs"] == int(r["pairs"][q, 0])
        assert entry["kendall_tau_b"] == doc["kendall_tau_b"][q][channels[q]]
        assert entry["best_channel"] == int(np.nanargmax(np.abs(r["kendall_tau_b"][q])))
        assert entry["mapped_channel_is_best"] == (entry["best_channel"] == channels[q])
    from PIL import Image
    with Image.open(out / "ar_matrix.png") as im:
        assert im.format == "PNG"
    E.main(base)                                                                    # a second run: the same bytes
    assert (out / "ar_metrics.json").read_bytes() == first


def test_analyze_ar_channels_end_to_end(dev, run):
    from PIL import Image
    from pti_ldm_vae_amd import analyze_ar_channels as A
    from pti_ldm_vae_amd import evaluate_ar_vae as E
    from pti_ldm_vae_amd.data import DeviceImageLoader
    from pti_ldm_vae_amd.utils.config import load_vae_config
    img = os.path.join(run["data"], "dente", "img_004.tif")
    out = run["tmp"] / "panel"
    A.main(["-c", run["cfg"], "--checkpoint", "nope.pth", "--image-path", img, "--output-dir", str(out), "--random-init-vae"])
    npz = np.load(out / "ar_channels_img_004.npz")
    assert npz["latents"].shape == (10, 32, 32) and npz["input"].shape == (1, 64, 64) and npz["reconstruction"].shape == (1, 64, 64)
    assert npz["original"].shape == (64, 64)
    torch.manual_seed(42)
    model = E.load_model(load_vae_config(run["cfg"]), "", dev, True)
    batch = next(iter(DeviceImageLoader([img], 1, (64, 64), dev, shuffle=False, num_workers=1)))
    with torch.no_grad():
        want = model.encode_deterministic(batch)[0]
    assert np.array_equal(npz["input"], batch[0].cpu().numpy()) and np.array_equal(npz["latents"], want.cpu().numpy())
    with Image.open(out / "ar_channels_img_004.png") as im:                        # 12 tiles in rows of 4: 3 rows
        assert im.format == "PNG" and abs(im.size[0] - 3.4 * 4 * 110) <= 2 and abs(im.size[1] - 3.4 * 3 * 110) <= 2

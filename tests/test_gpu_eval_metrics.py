"""GPU tests of the evaluation side: the fused metrics kernel (``pti_image_metrics``, csrc/image_metrics.hip) against the
fp64 torch restatement of the reference's ``compute_psnr`` / ``compute_ssim`` (``tests/eval_metrics_oracle.py``, pinned
to the reference's recorded outputs by ``tests/test_eval_metrics_cpu.py``), and ``evaluate_vae`` / ``inference_vae`` end
to end on a folder of TIF files.

Gate: per metric, ``D_ref`` = the largest deviation of the fp32 CPU restatement from the fp64 one over the case list
below (absolute for SSIM and PSNR in dB, relative for MSE and MAE), computed here; the kernel's deviation from fp64 must
be at most ``8 * D_ref`` on EVERY case.  The yardstick is the reference's own fp32 arithmetic; the factor 8 allows for
the separable two-pass summation order and fast-math instruction selection.  Measured on MI355X: see DESIGN.md 5f."""
import json
import os

import numpy as np
import pytest
import torch

import eval_metrics_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gate_and_ref():
    gate, ref = O.reference_deviation()
    print("D_ref", gate.d_ref, "-> bound", gate.bound)
    return gate, ref


def _kernel(p, t, clamp, dev, **kw):
    from pti_ldm_vae_amd import ops
    out = ops.image_metrics(p.to(dev), t.to(dev), clamp=clamp, **kw)
    torch.cuda.synchronize()
    return out


def _as_dict(out):
    out = out.detach().cpu()
    return {k: out[:, i] for i, k in enumerate(O.METRICS)}


@pytest.fixture(scope="module")
def kernel_results(dev, gate_and_ref):
    """case id -> the kernel's [n, 4] output (on the host) for every (shape, noise, clamp) case."""
    return {cid: _kernel(p, t, clamp, dev).cpu() for cid, p, t, clamp in O.cases()}


def test_kernel_within_eight_d_ref_of_fp64_on_every_case(gate_and_ref, kernel_results):
    gate, ref = gate_and_ref
    assert len(kernel_results) == len(O.SHAPES) * len(O.NOISES) * len(O.CLAMPS) == len(ref)
    worst = {k: 0.0 for k in O.METRICS}
    failures = []
    for cid, out in kernel_results.items():
        assert torch.isfinite(out).all(), cid
        d = O.deviation(_as_dict(out), ref[cid])
        for k in O.METRICS:
            worst[k] = max(worst[k], d[k])
        bad = gate.violations(d)
        print(f"[{cid}] " + " ".join(f"{k} {d[k]:.2e}" for k in O.METRICS) + (" VIOLATES " + "; ".join(bad) if bad else ""))
        if bad:
            failures.append((cid, bad))
    print("kernel worst deviation from fp64:", worst, "| D_ref:", gate.d_ref, "| bound:", gate.bound)
    assert not failures, failures


def test_gate_rejects_every_mutation_against_kernel_outputs(gate_and_ref, kernel_results):
    """The mutated fp64 restatements (9-tap window, sigma 1.4, reflect padding, border renormalisation, k2 = 0.02,
    missing clamp) are all rejected by the gate, as coded, when they are compared with what the kernel returned."""
    gate, _ = gate_and_ref

    def base_of(cid, p, t, clamp):
        return _as_dict(kernel_results[cid + "/clamp01"])

    survivors = O.mutation_survivors(gate, base_of)
    assert survivors == [], survivors


def test_identical_and_all_zero_inputs(dev, gate_and_ref):
    gate, _ = gate_and_ref
    p, _t = O.make_pair((3, 1, 100, 76), 0.1, seed=5)
    for x in (p, torch.zeros(2, 1, 64, 64), torch.zeros(1, 3, 9, 13)):
        for clamp in O.CLAMPS:
            out = _kernel(x, x.clone(), clamp, dev).cpu().double()
            assert float(out[:, 0].abs().max()) == 0.0 and float(out[:, 1].abs().max()) == 0.0
            assert float((out[:, 2] - 120.0).abs().max()) <= gate.bound["psnr"]
            assert float((out[:, 3] - 1.0).abs().max()) <= gate.bound["ssim"]


def test_bitwise_reproducible_and_batch_invariant(dev):
    from pti_ldm_vae_amd import ops
    p, t = O.make_pair((8, 1, 256, 256), 0.1, seed=11)
    p, t = p.to(dev), t.to(dev)
    a = ops.image_metrics(p, t, clamp=(0.0, 1.0))
    b = ops.image_metrics(p, t, clamp=(0.0, 1.0))
    assert torch.equal(a, b)
    # sample i alone, in the batch of 8, and at another batch position: the same four numbers, bit for bit
    for i in (0, 3, 7):
        alone = ops.image_metrics(p[i:i + 1], t[i:i + 1], clamp=(0.0, 1.0))
        assert torch.equal(alone[0], a[i]), i
    perm = torch.tensor([5, 0, 7, 2, 1, 6, 3, 4], device=dev)
    moved = ops.image_metrics(p[perm].contiguous(), t[perm].contiguous(), clamp=(0.0, 1.0))
    assert torch.equal(moved, a[perm])
    # multi-channel, ragged size
    p3, t3 = O.make_pair((4, 3, 33, 31), 0.1, seed=12)
    p3, t3 = p3.to(dev), t3.to(dev)
    a3 = ops.image_metrics(p3, t3)
    assert torch.equal(ops.image_metrics(p3[2:3], t3[2:3])[0], a3[2]) and torch.equal(ops.image_metrics(p3, t3), a3)


def test_non_contiguous_and_out_argument(dev):
    from pti_ldm_vae_amd import ops
    p, t = O.make_pair((2, 3, 64, 48), 0.1, seed=13)
    p, t = p.to(dev), t.to(dev)
    want = ops.image_metrics(p, t, clamp=(0.0, 1.0))
    p_nc = p.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)            # same values, channels-last strides
    t_nc = torch.cat([t, t], dim=3)[..., :48]                                # a view with a row stride of 96
    assert not p_nc.is_contiguous() and not t_nc.is_contiguous()
    assert torch.equal(ops.image_metrics(p_nc, t_nc, clamp=(0.0, 1.0)), want)
    out = torch.full((2, 4), float("nan"), device=dev)
    assert ops.image_metrics(p, t, clamp=(0.0, 1.0), out=out) is out and torch.equal(out, want)
    pack = torch.zeros(3 + 8, device=dev)
    ops.image_metrics(p, t, clamp=(0.0, 1.0), out=pack[3:].view(2, 4))       # an offset view, as evaluate() uses
    assert torch.equal(pack[3:].view(2, 4), want) and float(pack[:3].abs().max()) == 0.0
    for bad in (lambda: ops.image_metrics(p, t[:, :2]), lambda: ops.image_metrics(p[0], t[0]),
                lambda: ops.image_metrics(p, t, out=torch.zeros(3, 4, device=dev)),
                lambda: ops.image_metrics(p.cpu(), t.cpu()), lambda: ops.image_metrics(p.long(), t.long())):
        with pytest.raises((ValueError, TypeError)):
            bad()


def test_graph_capture_and_replay_equals_eager(dev):
    """One stream, no parallel branches, a fresh capture: the two launches replay to the eager result."""
    from pti_ldm_vae_amd import ops
    p, t = O.make_pair((3, 1, 100, 76), 0.1, seed=14)
    p, t = p.to(dev), t.to(dev)
    eager = ops.image_metrics(p, t, clamp=(0.0, 1.0)).clone()
    out = torch.zeros(3, 4, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.image_metrics(p, t, clamp=(0.0, 1.0), out=out)                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.image_metrics(p, t, clamp=(0.0, 1.0), out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # new values in the captured input buffers: the replay follows them
    p2, t2 = O.make_pair((3, 1, 100, 76), 0.5, seed=15)
    p.copy_(p2)
    t.copy_(t2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.image_metrics(p, t, clamp=(0.0, 1.0)))


def test_compute_psnr_and_ssim_are_the_kernel_columns(dev):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.utils import compute_psnr, compute_ssim
    p, t = O.make_pair((4, 1, 64, 64), 0.1, seed=16)
    p, t = p.to(dev), t.to(dev)
    m = ops.image_metrics(p, t)
    ps, ss = compute_psnr(p, t), compute_ssim(p, t)
    assert ps.shape == (4,) and ss.shape == (4,) and ps.device == p.device and ss.device == p.device
    assert torch.equal(ps, m[:, 2]) and torch.equal(ss, m[:, 3])
    m2 = ops.image_metrics(p, t, data_range=2.0, k1=0.02, k2=0.05)
    assert torch.equal(compute_psnr(p, t, data_range=2.0), m2[:, 2])
    assert torch.equal(compute_ssim(p, t, 2.0, 0.02, 0.05), m2[:, 3])
    ref = O.metrics(p, t, data_range=2.0, k1=0.02, k2=0.05)
    assert float((m2[:, 3].cpu().double() - ref["ssim"]).abs().max()) <= 1e-5
    assert float((m2[:, 2].cpu().double() - ref["psnr"]).abs().max()) <= 1e-4


# ---- evaluate_vae / inference_vae end to end ---------------------------------------------------------------------------
def _write_tifs(folder, n):
    from pti_ldm_vae_amd.data import write_tiff
    rng = np.random.default_rng(21)
    folder.mkdir(parents=True)
    for i in range(n):
        h, w = 96 + 8 * (i % 5), 120 - 4 * (i % 7)
        a = rng.standard_normal((h, w)).astype(np.float32) * 300 + 900
        yy, xx = np.mgrid[0:h, 0:w]
        a[((xx - w / 2) / (0.4 * w)) ** 2 + ((yy - h / 2) / (0.32 * h)) ** 2 > 1.0] = 0.0
        write_tiff(str(folder / f"img_{i:03d}.tif"), a, rows_per_strip=16 if i % 2 else None)


def _setup(tmp_path, perceptual_weight=0.0):
    from oracle.autoencoderkl import CONFIG_A, build_oracle
    _write_tifs(tmp_path / "imgs", 12)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64], perceptual_weight=perceptual_weight)
    cf = tmp_path / "cfg_eval.json"
    cf.write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)
    return str(cf), str(ck), str(tmp_path / "imgs")


def _std_tolerance(key, gate, values):
    """Tolerance of a ``*_mean`` / ``*_std`` entry given per-value bounds: the mean of values each within ``e`` of their
    reference is within ``e``; the population standard deviation is 1-Lipschitz in the RMS of the perturbation, so it
    is within ``e`` as well.  For the relative metrics ``e = bound * max |value|``."""
    kind = {"recon_loss": "mae", "kl_loss": "mae", "loss_total": "mae"}.get(key, key)
    return gate.bound[kind] * (max(abs(v) for v in values) if O.RELATIVE[kind] else 1.0)


def test_evaluate_and_inference_end_to_end(dev, tmp_path, gate_and_ref):
    from oracle import losses as OL
    from pti_ldm_vae_amd import evaluate_vae, inference_vae
    from pti_ldm_vae_amd.data import create_vae_inference_dataloader, read_tiff
    from pti_ldm_vae_amd.utils.cli_common import load_config_and_model
    gate, _ = gate_and_ref
    cf, ck, imgs = _setup(tmp_path)
    out = tmp_path / "eval_out"
    evaluate_vae.main(["-c", cf, "--checkpoint", ck, "--input-dir", imgs, "--output-dir", str(out), "--batch-size", "5"])
    doc = json.load(open(out / "metrics.json"))
    assert set(doc) == {"args", "metrics", "files"}
    want_keys = {f"{k}_{s}" for k in ("recon_loss", "kl_loss", "psnr", "ssim", "loss_total", "mse", "mae") for s in ("mean", "std")}
    assert set(doc["metrics"]) == want_keys                                    # no perceptual keys without the weight files
    assert doc["files"] == sorted(str(tmp_path / "imgs" / f"img_{i:03d}.tif") for i in range(12))
    assert doc["args"]["batch_size"] == 5 and doc["args"]["checkpoint"] == ck

    # the same evaluation called directly with the same seed, watching the tensors of each batch
    config, model = load_config_and_model(cf, ck, dev)
    loader, paths = create_vae_inference_dataloader(imgs, (64, 64), 5, device=dev)
    assert paths == doc["files"]
    seen = []
    torch.manual_seed(42)
    summary = evaluate_vae.evaluate(model, loader, dev, "l1", on_batch=lambda *ts: seen.append([x.detach().cpu().clone() for x in ts]))
    assert summary == doc["metrics"]                                           # bitwise reproducible, seed included
    assert [s[0].shape[0] for s in seen] == [5, 5, 2]                          # the short last batch is kept
    vals = {k: [] for k in ("recon_loss", "kl_loss", "loss_total") + O.METRICS}
    for images, recon, mu, third in seen:
        assert recon.shape == images.shape == (images.shape[0], 1, 64, 64)
        rl = float((recon.double() - images.double()).abs().mean())
        kl = float(OL.kl_loss(mu.double(), third.double()))
        vals["recon_loss"].append(rl)
        vals["kl_loss"].append(kl)
        vals["loss_total"].append(rl + kl)
        m = O.metrics(recon, images, clamp=(0.0, 1.0))
        for k in O.METRICS:
            vals[k].extend(m[k].tolist())
    assert len(vals["psnr"]) == 12
    bad = []
    for k, v in vals.items():
        tol = _std_tolerance(k, gate, v)
        for stat, want in (("mean", float(np.mean(v))), ("std", float(np.std(v)))):
            got = doc["metrics"][f"{k}_{stat}"]
            print(f"{k}_{stat}: {got:.9g} vs fp64 {want:.9g} (|d| {abs(got - want):.2e}, tolerance {tol:.2e})")
            if not abs(got - want) <= tol:
                bad.append((k, stat, got, want, tol))
    assert not bad, bad

    # inference on the same folder
    inf = tmp_path / "inf_out"
    inference_vae.main(["-c", cf, "--checkpoint", ck, "--input-dir", imgs, "--output-dir", str(inf), "--batch-size", "5"])
    loader, _ = create_vae_inference_dataloader(imgs, (64, 64), 5, device=dev)
    idx = 0
    from PIL import Image
    with torch.no_grad():
        for batch in loader:
            rec = model.reconstruct_deterministic(batch).float().cpu().numpy()
            inp = batch.cpu().numpy()
            for i in range(inp.shape[0]):
                a = read_tiff(str(inf / "results_tif" / f"image{idx:04d}.tif"))
                assert a.dtype == np.float32 and a.shape == (64, 128)
                assert np.array_equal(a[:, :64], inp[i, 0]) and np.array_equal(a[:, 64:], rec[i, 0])
                png = Image.open(inf / "results_png" / f"image{idx:04d}.png")
                assert png.size == (128, 64) and png.mode == "L"
                idx += 1
    assert idx == 12 and len(list((inf / "results_tif").iterdir())) == 12 and len(list((inf / "results_png").iterdir())) == 12
    # --num-samples caps the list
    inf2 = tmp_path / "inf2"
    inference_vae.main(["-c", cf, "--checkpoint", ck, "--input-dir", imgs, "--output-dir", str(inf2), "--num-samples", "3"])
    assert sorted(p.name for p in (inf2 / "results_tif").iterdir()) == [f"image{i:04d}.tif" for i in range(3)]


def test_evaluate_perceptual_branch(dev, tmp_path):
    """With weight files (random-init values: the real ones cannot be fetched) the term is reported and enters
    ``loss_total`` with the config's weight; without them a non-zero weight is refused, or dropped on request."""
    from pti_ldm_vae_amd import evaluate_vae
    from pti_ldm_vae_amd.models.perceptual import SqueezeLPIPS
    cf, ck, imgs = _setup(tmp_path, perceptual_weight=0.5)
    torch.manual_seed(11)
    sd = SqueezeLPIPS().state_dict()
    torch.save({k: v for k, v in sd.items() if k.startswith("features.")}, tmp_path / "squeezenet1_1.pth")
    torch.save({k: v.abs() for k, v in sd.items() if k.startswith("lin")}, tmp_path / "lpips_squeeze.pth")
    common = ["-c", cf, "--checkpoint", ck, "--input-dir", imgs, "--batch-size", "5", "--num-samples", "7"]
    out = tmp_path / "with"
    evaluate_vae.main(common + ["--output-dir", str(out), "--perceptual-weights", str(tmp_path / "squeezenet1_1.pth"),
                                str(tmp_path / "lpips_squeeze.pth")])
    m = json.load(open(out / "metrics.json"))["metrics"]
    assert "perceptual_loss_mean" in m and "perceptual_loss_std" in m and m["perceptual_loss_mean"] > 0
    # the mean is linear: mean(total) = mean(recon) + mean(kl) + 0.5 * mean(perceptual), all from the same per-batch values
    want = m["recon_loss_mean"] + m["kl_loss_mean"] + 0.5 * m["perceptual_loss_mean"]
    assert m["loss_total_mean"] == pytest.approx(want, rel=1e-12)
    with pytest.raises(SystemExit) as e:
        evaluate_vae.main(common + ["--output-dir", str(tmp_path / "refused")])
    assert "perceptual_weight" in str(e.value) and not (tmp_path / "refused" / "metrics.json").exists()
    out2 = tmp_path / "without"
    evaluate_vae.main(common + ["--output-dir", str(out2), "--ignore-unavailable-terms"])
    m2 = json.load(open(out2 / "metrics.json"))["metrics"]
    assert not any(k.startswith("perceptual_loss") for k in m2)
    assert m2["loss_total_mean"] == pytest.approx(m2["recon_loss_mean"] + m2["kl_loss_mean"], rel=1e-12)
    assert len(json.load(open(out2 / "metrics.json"))["files"]) == 7

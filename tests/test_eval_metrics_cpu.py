"""CPU tests of the evaluation side: the tests' torch restatement of the metrics is pinned to the reference's recorded
outputs, the gate built on it rejects the plausible mistakes, and the host-side pieces of ``evaluate_vae`` /
``inference_vae`` (argument parsing, directory names, path listing, ``metrics.json``, display normalisation, the
validation paths of the C entry points that return before any launch) behave as the reference's.

``tests/golden/eval_metrics_golden.npz`` was written by ``tools/make_eval_golden.py``, which ran the reference's own
``compute_psnr`` / ``compute_ssim`` (imported by path).  ``normalize_batch_for_display`` stays UNPINNED: the reference's
``visualization.py`` imports MONAI at module level and cannot be imported where the fixtures are made, so it is tested
against hand-computed small cases instead."""
import argparse
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import eval_metrics_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics_golden.npz")


@pytest.fixture(scope="module")
def gate():
    """D_ref over the kernel's whole case list (fp32 restatement vs fp64 restatement) -> Gate."""
    g, _ = O.reference_deviation()
    print("D_ref", g.d_ref)
    return g


def test_fp32_restatement_equals_the_reference_outputs():
    """Pins the oracle to the reference: SSIM within 1e-6 absolute, PSNR within 1e-4 dB, on the raw and the clamped images."""
    z = np.load(GOLDEN)
    n_cases = len([k for k in z.files if k.startswith("pred")])
    assert n_cases >= 4
    for i in range(n_cases):
        p, t = torch.from_numpy(z[f"pred{i}"]), torch.from_numpy(z[f"target{i}"])
        assert p.shape[1] == 1 and ((p > 1).any() or (p < 0).any())
        for clamp, suffix in ((None, ""), ((0.0, 1.0), "_clamped")):
            m = O.metrics(p, t, dtype=torch.float32, clamp=clamp)
            d_ssim = np.abs(m["ssim"].numpy() - z[f"ssim{suffix}{i}"]).max()
            d_psnr = np.abs(m["psnr"].numpy() - z[f"psnr{suffix}{i}"]).max()
            print(f"case {i}{suffix}: |ssim - ref| {d_ssim:.2e}, |psnr - ref| {d_psnr:.2e} dB")
            assert d_ssim <= 1e-6 and d_psnr <= 1e-4
    # the identical pair: PSNR 120 dB, SSIM 1
    last = n_cases - 1
    assert np.abs(z[f"psnr{last}"] - 120.0).max() <= 1e-4 and np.abs(z[f"ssim{last}"] - 1.0).max() <= 1e-6


def test_window_taps_equal_the_reference_taps_bit_for_bit():
    from pti_ldm_vae_amd import ops
    taps = np.load(GOLDEN)["taps"]
    assert taps.dtype == np.float32 and taps.shape == (11,)
    assert np.array_equal(ops.ssim_taps().numpy(), taps)
    assert np.array_equal(O.window(torch.float32).numpy(), taps)
    assert abs(float(taps.sum()) - 1.0) <= 1e-6 and np.array_equal(taps, taps[::-1])


def test_gate_rejects_every_mutation_on_the_oracle(gate):
    """The five mistakes (shorter window, other sigma, reflect padding / border renormalisation, other k2, missing
    clamp) applied to the fp64 restatement: the gate as coded rejects each one on every case with H, W >= 64 and
    noise >= 0.01; and the clean fp32 restatement passes it by construction, the clean fp64 one trivially."""
    assert gate.d_ref["ssim"] <= 1e-6 and gate.d_ref["psnr"] <= 1e-4, gate.d_ref     # the yardstick itself is sane
    assert all(v > 0 for v in gate.d_ref.values())
    survivors = O.mutation_survivors(gate)
    assert survivors == [], survivors


def test_c_entry_points_validate_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    ws = h.pti_image_metrics_ws_floats
    assert ws(32, 1, 256, 256) == 32 * 64 * 3 and ws(1, 1, 1, 1) == 3 and ws(2, 3, 64, 48) == 2 * 3 * 4 * 3
    assert ws(1, 1, 33, 31) == 2 * 3                                              # partial tiles count
    assert ws(1, 1, 0, 8) == 0 and ws(1, 1, 8, 0) == 0 and ws(0, 1, 8, 8) == 0 and ws(1, 0, 8, 8) == 0 and ws(1, 1, -4, 8) == 0
    sizes = [ws(n, c, hh, ww) for n, c, hh, ww in ((1, 1, 8, 8), (1, 1, 64, 64), (2, 1, 64, 64), (2, 3, 64, 64), (2, 3, 65, 64),
                                                   (2, 3, 65, 300))]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)               # monotone in every dimension
    p = C.c_void_p(256)                                                           # never dereferenced: refused first
    taps = (C.c_float * 11)(*([1.0 / 11] * 11))
    args = (1, 1, 8, 8, 1, 0.0, 1.0, 1.0, 0.01, 0.03)
    for bad in range(5):
        ptrs = [p, p, taps, p, p]
        ptrs[bad] = None
        rc = h.pti_image_metrics(ptrs[0], ptrs[1], *args, ptrs[2], ptrs[3], ptrs[4], None)
        assert rc == -1 and b"null" in h.pti_last_error_string()
    for shape in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -1)):
        rc = h.pti_image_metrics(p, p, *shape, 1, 0.0, 1.0, 1.0, 0.01, 0.03, taps, p, p, None)
        assert rc == -2 and b"shape" in h.pti_last_error_string()
    rc = h.pti_image_metrics(p, p, 1, 1, 8, 8, 1, 1.0, 0.0, 1.0, 0.01, 0.03, taps, p, p, None)    # empty clamp range
    assert rc == -2 and b"clamp" in h.pti_last_error_string()
    with pytest.raises(_lib.PtiError):
        _lib.check(rc, "image_metrics")


def test_cpu_tensors_are_refused():
    from pti_ldm_vae_amd import _lib, ops
    from pti_ldm_vae_amd.utils import compute_psnr, compute_ssim
    x = torch.rand(2, 1, 16, 16)
    for fn in (compute_psnr, compute_ssim):
        with pytest.raises(_lib.PtiError, match="no CPU/PyTorch fallback"):
            fn(x, x)
    with pytest.raises(ValueError):
        ops.image_metrics(x, x)


def test_shared_arguments_and_defaults():
    from pti_ldm_vae_amd import evaluate_vae, inference_vae
    from pti_ldm_vae_amd.utils.cli_common import add_shared_io_args
    p = argparse.ArgumentParser()
    add_shared_io_args(p, output_help="out")
    a = p.parse_args(["-c", "cfg.json", "--checkpoint", "ck.pth", "--input-dir", "imgs"])
    assert vars(a) == dict(config_file="cfg.json", checkpoint="ck.pth", input_dir="imgs", output_dir=None, num_samples=None,
                           batch_size=8, num_workers=4, seed=42)
    a = p.parse_args(["--config-file", "c", "--checkpoint", "k", "--input-dir", "i", "--output-dir", "o", "--num-samples", "3",
                      "--batch-size", "2", "--num-workers", "1", "--seed", "7"])
    assert (a.output_dir, a.num_samples, a.batch_size, a.num_workers, a.seed) == ("o", 3, 2, 1, 7)
    for missing in (["--checkpoint", "k", "--input-dir", "i"], ["-c", "c", "--input-dir", "i"], ["-c", "c", "--checkpoint", "k"]):
        with pytest.raises(SystemExit):
            p.parse_args(missing)
    e = evaluate_vae.parse_args(["-c", "c", "--checkpoint", "k", "--input-dir", "i", "--perceptual-weights", "A", "B"])
    assert e.perceptual_weights == ["A", "B"] and e.ignore_unavailable_terms is False and e.batch_size == 8
    i = inference_vae.parse_args(["-c", "c", "--checkpoint", "k", "--input-dir", "i"])
    assert i.seed == 42 and not hasattr(i, "perceptual_weights")


def test_serialize_args_and_output_directories(tmp_path, monkeypatch):
    from pti_ldm_vae_amd.utils import serialize_args
    from pti_ldm_vae_amd.utils.cli_common import resolve_eval_output_dir, resolve_inference_output_dirs
    from pti_ldm_vae_amd.utils.vae_loader import default_eval_output_dir
    ns = argparse.Namespace(path=Path("a/b.json"), pair=("x", Path("y")), items=[1, 2], n=3, f=0.5, none=None, s="t", flag=True)
    got = serialize_args(ns)
    assert got == dict(path="a/b.json", pair=["x", "y"], items=["1", "2"], n=3, f=0.5, none=None, s="t", flag=True)
    json.dumps(got)
    assert default_eval_output_dir("config/vae_dente_no_adv.json") == Path("evals") / "vae_dente_no_adv"
    assert default_eval_output_dir("/x/y/cfg.v2.json", root_dir="r") == Path("r") / "cfg.v2"
    monkeypatch.chdir(tmp_path)
    root, tif, png = resolve_inference_output_dirs("weights/checkpoint_epoch73.pth", None)
    assert root == Path("inference_vae_checkpoint_epoch73") and tif == root / "results_tif" and png == root / "results_png"
    assert tif.is_dir() and png.is_dir()
    root, tif, png = resolve_inference_output_dirs("ck.pth", str(tmp_path / "o" / "p"))
    assert root == tmp_path / "o" / "p" and tif.is_dir() and png.is_dir()
    assert resolve_eval_output_dir("c/my_cfg.json", None) == Path("evals/my_cfg") and Path("evals/my_cfg").is_dir()
    assert resolve_eval_output_dir("c/my_cfg.json", str(tmp_path / "e")) == tmp_path / "e" and (tmp_path / "e").is_dir()


def test_inference_path_listing(tmp_path):
    from pti_ldm_vae_amd.data import create_vae_inference_dataloader, list_inference_paths
    flat = tmp_path / "flat"
    flat.mkdir()
    for name in ("b.tif", "a.tif", "c.tif", "notes.txt", "d.png"):
        (flat / name).write_bytes(b"")
    assert [os.path.basename(p) for p in list_inference_paths(str(flat))] == ["a.tif", "b.tif", "c.tif"]
    assert [os.path.basename(p) for p in list_inference_paths(str(flat), 2)] == ["a.tif", "b.tif"]
    assert len(list_inference_paths(str(flat), 10)) == 3
    both = tmp_path / "both"
    for sub, names in (("dente", ("z.tif", "y.tif")), ("edente", ("m.tif",))):
        (both / sub).mkdir(parents=True)
        for name in names:
            (both / sub / name).write_bytes(b"")
    got = list_inference_paths(str(both))
    assert [os.path.relpath(p, both) for p in got] == ["edente/m.tif", "dente/y.tif", "dente/z.tif"]     # edente first
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        list_inference_paths(str(empty))
    with pytest.raises(FileNotFoundError):                                   # raised before a device is needed
        create_vae_inference_dataloader(str(empty), (64, 64), 4)


def test_metrics_json_schema(tmp_path):
    from pti_ldm_vae_amd.evaluate_vae import parse_args, save_metrics
    args = parse_args(["-c", "cfg.json", "--checkpoint", "ck.pth", "--input-dir", "imgs", "--perceptual-weights", "A", "B"])
    summary = {"recon_loss_mean": 0.25, "recon_loss_std": 0.0, "psnr_mean": 30.5, "psnr_std": 1.5}
    save_metrics(tmp_path, summary, ["imgs/a.tif", "imgs/b.tif"], args)
    doc = json.load(open(tmp_path / "metrics.json"))
    assert set(doc) == {"args", "metrics", "files"}
    assert doc["metrics"] == summary and doc["files"] == ["imgs/a.tif", "imgs/b.tif"]
    assert doc["args"]["config_file"] == "cfg.json" and doc["args"]["batch_size"] == 8 and doc["args"]["seed"] == 42
    assert doc["args"]["perceptual_weights"] == ["A", "B"]


def test_normalize_batch_for_display_hand_computed():
    """Unpinned against the reference (see the module docstring): hand-computed cases of the documented rule."""
    from pti_ldm_vae_amd.utils.visualization import normalize_batch_for_display
    # non-zero pixels 1..5 (2-D order irrelevant), low=0 / high=100: min 1, max 5 -> (v - 1) / 4; zeros stay zero
    x = torch.tensor([[[[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]]])
    y = normalize_batch_for_display(x, low=0, high=100)
    assert y.shape == x.shape and y.dtype == torch.float32
    assert torch.allclose(y, torch.tensor([[[[0.0, 0.0, 0.25], [0.5, 0.75, 1.0]]]]), atol=1e-6)
    # percentiles with linear interpolation: values 1..5 -> p25 = 2, p75 = 4 -> clip((v - 2) / 2, 0, 1)
    y = normalize_batch_for_display(x, low=25, high=75)
    assert torch.allclose(y, torch.tensor([[[[0.0, 0.0, 0.0], [0.5, 1.0, 1.0]]]]), atol=1e-6)
    # results below 1e-3 become 0: 2.0005 maps to 0.0005 / 2 -> 0; negative values are foreground too (non-zero)
    x2 = torch.tensor([[[[-1.0, 1.0, 2.0005, 3.0]]]])
    y2 = normalize_batch_for_display(x2, low=0, high=100)
    assert torch.allclose(y2, torch.tensor([[[[0.0, 0.5, 0.750125, 1.0]]]]), atol=1e-6)
    x3 = torch.tensor([[[[1.0, 1.0004, 3.0]]]])
    assert normalize_batch_for_display(x3, low=0, high=100)[0, 0, 0, 1].item() == 0.0
    # all-zero plane stays zero; constant non-zero plane: (v - v) / 1e-8 = 0; planes are normalised independently
    x4 = torch.zeros(2, 2, 3, 3)
    x4[0, 1] = 7.0
    x4[1, 0, 0, 0], x4[1, 0, 1, 1] = 2.0, 4.0
    y4 = normalize_batch_for_display(x4, low=0, high=100)
    assert float(y4[0].abs().max()) == 0.0 and float(y4[1, 1].abs().max()) == 0.0
    assert y4[1, 0, 0, 0].item() == 0.0 and y4[1, 0, 1, 1].item() == pytest.approx(1.0, abs=1e-6)
    # default percentiles 2 / 98 on 101 non-zero values 1..101: p2 = 3, p98 = 99
    x5 = torch.arange(1, 102, dtype=torch.float32).view(1, 1, 1, 101)
    y5 = normalize_batch_for_display(x5)
    assert y5[0, 0, 0, 0].item() == 0.0 and y5[0, 0, 0, 100].item() == 1.0
    assert y5[0, 0, 0, 50].item() == pytest.approx((51 - 3) / 96, abs=1e-6)

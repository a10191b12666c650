"""CPU tests of the regression head's evaluation side: the tests' torch restatement is pinned to recorded outputs of the
reference's own modules, the gate built on it rejects nine plausible mistakes, and the host-side pieces of
``evaluate_regression`` / ``inference_regression`` (argument defaults, run directory, loader factories, head packing, the
validation paths of the C entry points that return before any launch) behave as the reference's.

``tests/golden/regression_eval_golden.npz`` was written by ``python tests/regression_head_oracle.py <reference checkout>``:
it ran the reference's ``LatentRegressor``, ``TargetNormalizer``, ``build_loss_fn``, ``validate_one_epoch`` and
``compute_regression_metrics``, loaded by path.  ``models/autoencoder.py`` and ``utils/vae_loader.py`` import MONAI, which
was not installed where the fixture was made; they were replaced by placeholders (the fixture's ``stubbed`` entry names
them) -- nothing recorded runs through either."""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import regression_head_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regression_eval_golden.npz")


@pytest.fixture(scope="module")
def gate():
    g, _ = O.reference_deviation(O.golden_cases() + O.mutation_cases())
    print("D_ref", g.d_ref)
    return g


def test_fp32_restatement_equals_the_reference_outputs():
    """Pins the oracle to the reference: head output and de-normalised predictions within 1e-6 of the largest value,
    val_loss / MAE / MSE within 1e-6 relative (the reference adds the batch losses as Python floats)."""
    z = np.load(GOLDEN)
    cases = O.golden_cases()
    assert len(cases) >= 4 and max(c.x.shape[1] for c in cases) == 513
    assert {c.act for c in cases} == set(O.ACTS) and {c.loss for c in cases} == {"mse", "smooth_l1"}
    for i, c in enumerate(cases):
        assert str(z[f"name{i}"]) == c.name
        out = O.head_forward(c.x, c.weights, c.biases, c.act, dtype=torch.float32)
        res = O.evaluate(c, dtype=torch.float32)
        d_out = np.abs(out.numpy() - z[f"out{i}"]).max() / np.abs(z[f"out{i}"]).max()
        d_pred = np.abs(res["pred"].numpy() - z[f"pred{i}"]).max() / np.abs(z[f"pred{i}"]).max()
        d_fold = (np.abs(res["fold"].double().numpy() - z[f"fold{i}"]) / np.abs(z[f"fold{i}"])).max()
        print(f"{c.name}: out {d_out:.2e} pred {d_pred:.2e} fold {d_fold:.2e}")
        assert d_out <= 1e-6 and d_pred <= 1e-6 and d_fold <= 1e-6


def test_case_inputs_can_show_every_mistake():
    """Negative pre-activations, errors on both sides of 1 and a short last batch in the mutation cases."""
    for c in O.mutation_cases():
        pre = c.x.double() @ c.weights[0].double().t() + c.biases[0].double()
        assert (pre < -0.5).any() and (pre > 0.5).any()
        out = O.head_forward(c.x, c.weights, c.biases, c.act)
        err = (out - (c.targets.double() - c.mean.double()) / c.std.double()).abs()
        assert (err < 0.9).any() and (err > 1.1).any()
        assert c.x.shape[0] % c.batch != 0 and c.x.shape[0] > c.batch
        assert not torch.equal(c.mean, c.std) and (c.biases[-1].abs() > 1e-3).all()


def test_gate_rejects_every_mutation_on_the_oracle(gate):
    assert all(0 < v <= 1e-5 for v in gate.d_ref.values()), gate.d_ref          # the yardstick itself is sane
    assert len(O.MUTATIONS) == 9
    survivors = O.mutation_survivors(gate)
    assert survivors == [], survivors
    for c in O.golden_cases() + O.mutation_cases():                              # the clean fp32 restatement passes
        assert gate.violations(O.deviation(O.evaluate(c, dtype=torch.float32), O.evaluate(c))) == []


def _dims(*v):
    return (C.c_int32 * len(v))(*v)


def test_c_entry_points_validate_before_any_launch():
    from pti_ldm_vae_amd import _lib, ops
    h = _lib.lib()
    ws = h.pti_mlp_head_ws_floats
    # one plane [n][h1] on the direct route, one per 512-column slab on the split route
    assert ws(8, 4096, _dims(4096, 256, 32, 6), 3) == 8 * 8 * 256 and ops.mlp_head_route(8, 4096, 256) == "split"
    assert ws(200, 4096, _dims(4096, 256, 32, 6), 3) == 200 * 256 and ops.mlp_head_route(200, 4096, 256) == "direct"
    assert ws(3, 512, _dims(512, 6), 1) == 3 * 6 and ops.mlp_head_route(3, 512, 6) == "direct"
    assert ws(1, 40960, _dims(40960, 32, 6), 2) == 80 * 32 and ops.mlp_head_route(1, 40960, 32) == "split"
    for n, d, h1 in ((1, 513, 1024), (17, 513, 1024), (16, 1027, 1024), (33, 1027, 32), (257, 1027, 64), (256, 1027, 64)):
        planes = -(-d // 512) if ops.mlp_head_route(n, d, h1) == "split" else 1
        assert ws(n, d, _dims(d, h1, 2), 2) == planes * n * h1, (n, d, h1)
    nine = _dims(16, 8, 8, 8, 8, 8, 8, 8, 8, 2)
    assert ws(4, 16, nine, 9) == 0 and ws(4, 16, _dims(16, 1025, 2), 2) == 0 and ws(4, 16, _dims(16, 8, 65), 2) == 0
    assert ws(4, 16, _dims(16, 1024, 64), 2) > 0 and ws(4, 16, _dims(16, 8, 8, 8, 8, 8, 8, 8, 2), 8) > 0
    assert ws(0, 16, _dims(16, 2), 1) == 0 and ws(4, 16, _dims(15, 2), 1) == 0 and ws(4, 16, _dims(16, 0, 2), 2) == 0
    assert ws(4, 16, None, 1) == 0 and ws(4, 16, _dims(16, 2), 0) == 0
    p = C.c_void_p(256)                                                           # never dereferenced: refused first

    def fwd(dims, layers, *, x=p, params=p, mean=None, std=None, targets=None, pred=p, rowloss=None, wsp=p, n=4, d=16,
            ldx=16, act=0, loss=0):
        return h.pti_mlp_head_fwd(x, ldx, n, d, params, dims, layers, act, mean, std, targets, loss, pred, rowloss, wsp, None)

    ok = _dims(16, 8, 2)
    for kw in (dict(x=None), dict(params=None), dict(pred=None), dict(wsp=None), dict(mean=p), dict(std=p),
               dict(targets=p)):                                                  # targets without rowloss
        assert fwd(ok, 2, **kw) == -1 and b"null" in h.pti_last_error_string(), kw
    assert fwd(None, 2) == -1 and b"null" in h.pti_last_error_string()
    for kw in (dict(n=0), dict(d=0), dict(ldx=15)):
        assert fwd(ok, 2, **kw) == -1, kw
    assert fwd(_dims(16, 0, 2), 2) == -1 and fwd(_dims(15, 8, 2), 2) == -1 and fwd(ok, 0) == -1
    for dims, layers, word in ((nine, 9, b"LAYERS"), (_dims(16, 1025, 2), 2, b"WIDTH"), (_dims(16, 8, 65), 2, b"OUT")):
        assert fwd(dims, layers) == -2 and word in h.pti_last_error_string()
    assert fwd(ok, 2, act=4) == -2 and b"activation" in h.pti_last_error_string()
    assert fwd(ok, 2, loss=2) == -2 and b"loss" in h.pti_last_error_string()
    with pytest.raises(_lib.PtiError):
        _lib.check(-2, "mlp_head_fwd")
    met = h.pti_regression_metrics
    for bad in range(4):
        ptrs = [p, p, p, p]
        ptrs[bad] = None
        assert met(ptrs[0], ptrs[1], ptrs[2], 4, 2, 8, ptrs[3], None) == -1 and b"null" in h.pti_last_error_string()
    assert met(p, p, p, 0, 2, 8, p, None) == -1 and met(p, p, p, 4, 0, 8, p, None) == -1 and met(p, p, p, 4, 2, 0, p, None) == -1
    assert met(p, p, p, 4, 65, 8, p, None) == -2 and b"OUT" in h.pti_last_error_string()


def test_mlp_head_pack_order_and_dims():
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.models import LatentRegressor
    torch.manual_seed(0)
    head = LatentRegressor(12, [5, 3], 2, dropout=0.3, activation="elu")
    params, dims, act = ops.mlp_head_pack(head)
    lin = [m for m in head.mlp if isinstance(m, torch.nn.Linear)]
    want = torch.cat([t.detach().reshape(-1) for m in lin for t in (m.weight, m.bias)])
    assert dims == [12, 5, 3, 2] and act == 3 and params.dtype == torch.float32 and torch.equal(params, want)
    assert params.numel() == 12 * 5 + 5 + 5 * 3 + 3 + 3 * 2 + 2
    assert torch.equal(params[:60].view(5, 12), lin[0].weight.detach()) and torch.equal(params[60:65], lin[0].bias.detach())
    for name, code in (("relu", 0), ("gelu", 1), ("leaky_relu", 2), ("elu", 3)):
        assert ops.mlp_head_pack(LatentRegressor(4, [3], 1, activation=name))[2] == code
    assert ops.mlp_head_pack(LatentRegressor(4, [], 3, activation="gelu"))[1:] == ([4, 3], 0)
    assert ops.mlp_head_supported([4096, 256, 32, 6]) and ops.mlp_head_supported([40960, 6]) and ops.mlp_head_supported([1, 1024, 64])
    assert not ops.mlp_head_supported([16, 1025, 2]) and not ops.mlp_head_supported([16, 8, 65])
    assert not ops.mlp_head_supported([16] + [8] * 8 + [2]) and not ops.mlp_head_supported([16]) and not ops.mlp_head_supported([16, 0, 2])
    with pytest.raises(ValueError):                                               # CPU tensors are refused, no fallback
        ops.mlp_head_fwd(torch.zeros(2, 4), torch.zeros(4 * 3 + 3), [4, 3], 0)


class _RecordingLoader:
    """Stands in for DeviceImageLoader (its constructor needs a HIP device): keeps what the factory passed."""

    def __init__(self, paths, batch_size, patch_size, device, **kw):
        self.paths, self.batch, self.patch, self.device, self.kw = list(paths), batch_size, tuple(patch_size), device, kw


def test_loader_factories_paths_and_targets(tmp_path, monkeypatch):
    from pti_ldm_vae_amd import data
    from pti_ldm_vae_amd.data import loader as loader_mod
    monkeypatch.setattr(loader_mod, "DeviceImageLoader", _RecordingLoader)
    d = tmp_path / "imgs" / "edente"
    d.mkdir(parents=True)
    table = {}
    for i, name in enumerate(("c.tif", "a.tif", "b.tif", "d.tif")):
        (d / name).write_bytes(b"")
        table[name] = {"height": 10.0 + i, "width": 2.0 * i, "unused": -1.0}
    (d / "notes.txt").write_bytes(b"")
    af = tmp_path / "attrs.json"
    af.write_text(json.dumps(table))
    ld, paths = data.create_regression_eval_dataloader(str(tmp_path / "imgs"), str(af), ["width", "height"], (64, 48), 3,
                                                       num_workers=2, num_samples=3, device="cpu")
    assert [os.path.basename(p) for p in paths] == ["a.tif", "b.tif", "c.tif"] and ld.paths == paths
    assert (ld.batch, ld.patch, ld.device) == (3, (64, 48), "cpu")
    assert ld.kw["shuffle"] is False and ld.kw["num_workers"] == 2 and ld.kw["target_names"] == ["width", "height"]
    got = [[a[k] for k in ("width", "height")] for a in ld.kw["attributes"]]
    assert got == [[2.0, 11.0], [4.0, 12.0], [0.0, 10.0]]                         # path order, target order
    ld, paths = data.create_regression_eval_dataloader(str(tmp_path / "imgs"), str(af), ["height"], (64, 64), 8,
                                                       normalize_attributes={"enabled": True, "divisor": 2.0}, device="cpu")
    assert len(paths) == 4 and len(ld.kw["attributes"]) == 4
    with pytest.raises(ValueError):
        data.create_regression_eval_dataloader(str(tmp_path / "imgs"), str(af), [], (64, 64), 8, device="cpu")
    ld, paths = data.create_regression_inference_dataloader(str(tmp_path / "imgs"), (32, 32), 2, num_samples=2, device="cpu")
    assert [os.path.basename(p) for p in paths] == ["a.tif", "b.tif"] and ld.paths == paths and ld.kw["shuffle"] is False
    assert "attributes" not in ld.kw
    import inspect
    sig = inspect.signature(data.create_regression_eval_dataloader)
    assert list(sig.parameters)[:9] == ["input_dir", "attributes_path", "targets", "patch_size", "batch_size", "num_workers",
                                        "num_samples", "data_source", "normalize_attributes"]
    assert (sig.parameters["num_workers"].default, sig.parameters["num_samples"].default,
            sig.parameters["data_source"].default, sig.parameters["normalize_attributes"].default) == (4, None, "edente", None)
    sig = inspect.signature(data.create_regression_inference_dataloader)
    assert list(sig.parameters)[:5] == ["input_dir", "patch_size", "batch_size", "num_samples", "num_workers"]


def test_cli_defaults_equal_the_reference():
    from pti_ldm_vae_amd import evaluate_regression, inference_regression
    e = evaluate_regression.parse_args(["-c", "cfg.json", "--checkpoint", "head.pth"])
    assert vars(e) == dict(config_file="cfg.json", checkpoint="head.pth", input_dir=None, attributes_path=None, output_dir=None,
                           batch_size=None, num_workers=None, num_samples=None, seed=42, random_init_vae=False, head="hip")
    i = inference_regression.parse_args(["--config-file", "c", "--checkpoint", "k", "--input-dir", "imgs"])
    assert vars(i) == dict(config_file="c", checkpoint="k", input_dir="imgs", output_dir=None, batch_size=None,
                           num_workers=None, num_samples=None, seed=42, random_init_vae=False, head="hip")
    i = inference_regression.parse_args(["-c", "c", "--checkpoint", "k", "--input-dir", "i", "--head", "torch", "--batch-size",
                                         "3", "--num-samples", "5", "--num-workers", "1", "--seed", "7", "--output-dir", "o"])
    assert (i.head, i.batch_size, i.num_samples, i.num_workers, i.seed, i.output_dir) == ("torch", 3, 5, 1, 7, "o")
    for mod, argv in ((inference_regression, ["-c", "c", "--checkpoint", "k"]), (evaluate_regression, ["-c", "c"]),
                      (evaluate_regression, ["-c", "c", "--checkpoint", "k", "--head", "cuda"])):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)


def test_run_dir_and_output_files(tmp_path, monkeypatch):
    from pti_ldm_vae_amd import evaluate_regression, inference_regression
    from pti_ldm_vae_amd.utils.cli_common import load_json_config, resolve_run_dir
    monkeypatch.chdir(tmp_path)
    cf = tmp_path / "my_reg.v2.json"
    cf.write_text(json.dumps({"targets": ["a"]}))
    cfg = load_json_config(str(cf))
    assert cfg == {"targets": ["a"]}
    run = resolve_run_dir(cfg, str(cf))
    assert run == Path("runs") / "my_reg.v2" and run.is_dir() and cfg["run_dir"] == str(run)
    cfg2 = {"run_dir": str(tmp_path / "x" / "y")}
    assert resolve_run_dir(cfg2, str(cf)) == tmp_path / "x" / "y" and (tmp_path / "x" / "y").is_dir()
    assert evaluate_regression.load_optional_normalizer(run, ["a"]) is None
    (run / "trained_weights").mkdir()
    (run / "trained_weights" / "target_norm_stats.json").write_text(json.dumps({"target_names": ["a"], "mean": [2.0], "std": [0.0]}))
    norm = evaluate_regression.load_optional_normalizer(run, ["a"])
    assert norm.mean.tolist() == [2.0] and norm.std.tolist() == [1.0]             # zero std replaced on the host
    args = evaluate_regression.parse_args(["-c", str(cf), "--checkpoint", "k"])
    evaluate_regression.save_metrics(run / "eval", {"val_loss": 0.5, "mae": 1.0, "mse": 2.0, "mae_a": 1.0, "mse_a": 2.0}, args,
                                     ["d/a.tif"])
    doc = json.load(open(run / "eval" / "metrics.json"))
    assert set(doc) == {"metrics", "args", "files"} and doc["files"] == ["d/a.tif"] and doc["metrics"]["val_loss"] == 0.5
    assert doc["args"]["seed"] == 42 and doc["args"]["head"] == "hip"
    inference_regression.save_predictions(run / "inference", ["a", "b"], ["d/x.tif", "d/y.tif"], torch.tensor([[1.0, 2.0], [3.0, 4.0]]))
    doc = json.load(open(run / "inference" / "predictions.json"))
    assert doc == {"predictions": {"x.tif": {"a": 1.0, "b": 2.0}, "y.tif": {"a": 3.0, "b": 4.0}}}

"""GPU tests of the regression head's evaluation side: ``pti_mlp_head_fwd`` against the fp64 restatement through the gate
of ``tests/regression_head_oracle.py`` (bound = 8 x the fp32 CPU restatement's own deviation from fp64, relative to the
case's largest fp64 output), its bitwise properties (repeatable, row-local, route-independent), ``pti_regression_metrics``
against the fp64 restatement, and ``evaluate_regression`` / ``inference_regression`` end to end on a TIFF directory.

Shapes are the smallest at which the kernel can go wrong: d below / at / above one 512-column slab and off the 16-byte
grid, the config-5 latent (4 096) and the AR model's (40 960), row counts around the 16-row tile and the 4-row tail tile,
first layers of one and of sixteen 64-unit blocks, a head without hidden layers, 1 / 6 / 64 targets."""
import json
import os

import numpy as np
import pytest
import torch

import regression_head_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, n, d, hidden, T, act, norm, targets, loss, row stride - d
FORWARD = [
    ("d1 n1 [] T1", 1, 1, [], 1, "relu", False, False, "mse", 0),
    ("d3 n2 [7,5] T6 gelu huber strided", 2, 3, [7, 5], 6, "gelu", True, True, "smooth_l1", 5),
    ("d511 n16 [32] T6 leaky", 16, 511, [32], 6, "leaky_relu", True, True, "mse", 0),
    ("d512 n17 [256,32] T6 elu", 17, 512, [256, 32], 6, "elu", True, True, "mse", 0),
    ("d513 n33 [1024] T64 relu huber", 33, 513, [1024], 64, "relu", True, True, "smooth_l1", 0),
    ("d1027 n33 [256,32] T6 gelu no-norm strided", 33, 1027, [256, 32], 6, "gelu", False, True, "mse", 5),
    ("d1027 n1 [1024] T1 leaky huber no-norm", 1, 1027, [1024], 1, "leaky_relu", False, True, "smooth_l1", 0),
    ("d4096 n16 [256,32] T6 relu", 16, 4096, [256, 32], 6, "relu", True, True, "mse", 0),
    ("d4096 n2 [] T64 no-targets strided", 2, 4096, [], 64, "relu", True, False, "mse", 8),
    ("d4096 n33 [1024] T6 elu strided", 33, 4096, [1024], 6, "elu", True, True, "mse", 8),
    ("d40960 n2 [32] T1 elu huber", 2, 40960, [32], 1, "elu", True, True, "smooth_l1", 0),
    ("d40960 n17 [32] T6 gelu no-targets", 17, 40960, [32], 6, "gelu", True, False, "mse", 0),
]


def _case(spec, seed):
    name, n, d, hidden, t, act, norm, targets, loss, _ = spec
    return O.make_case(name, n, (1, 1, d), hidden, t, act=act, norm=norm, targets=targets, loss=loss, batch=8, seed=seed)


@pytest.fixture(scope="module")
def oracle():
    """(cases, gate, fp64 outputs): computed once on the CPU and shared."""
    torch.set_num_threads(16)
    cases = [_case(spec, 20 + i) for i, spec in enumerate(FORWARD)]
    gate, ref = O.reference_deviation(cases)
    print("D_ref", gate.d_ref)
    return cases, gate, ref


def _run(case, dev, pad=0, rows=None):
    """The kernel on ``case`` (rows ``rows`` of it) -> {"pred", "rowloss"} device tensors."""
    from pti_ldm_vae_amd import ops
    x = case.x if rows is None else case.x[rows]
    tg = case.targets if (rows is None or case.targets is None) else case.targets[rows]
    n, d = x.shape
    buf = torch.zeros(n, d + pad, device=dev)
    buf[:, :d] = x.to(dev)
    params = torch.cat([t.reshape(-1) for w, b in zip(case.weights, case.biases) for t in (w, b)]).to(dev)
    kw = {}
    if case.mean is not None:
        kw.update(mean=case.mean.to(dev), std=case.std.to(dev))
    if tg is not None:
        kw.update(targets=tg.to(dev).contiguous(), loss=case.loss)
    pred, rowloss = ops.mlp_head_fwd(buf[:, :d], params, case.dims, O.ACTS.index(case.act) if len(case.dims) > 2 else 0, **kw)
    return {"pred": pred, "rowloss": rowloss}


def test_forward_against_the_fp64_restatement(dev, oracle):
    from pti_ldm_vae_amd import ops
    cases, gate, ref = oracle
    routes, bad = set(), []
    for spec, case in zip(FORWARD, cases):
        got = _run(case, dev, pad=spec[9])
        r64 = {k: v for k, v in ref[case.name].items() if k != "fold"}
        dev_k = O.deviation({k: v for k, v in got.items() if v is not None}, r64)
        route = ops.mlp_head_route(spec[1], spec[2], case.dims[1])
        routes.add(route)
        print(f"{case.name} [{route}]: " + " ".join(f"{k} {v:.2e}" for k, v in dev_k.items()))
        assert (got["rowloss"] is None) == (case.targets is None)
        bad += [f"{case.name}: {v}" for v in gate.violations(dev_k)]
    print("bound", gate.bound)
    assert routes == {"split", "direct"}
    assert bad == [], bad


def test_second_call_and_row_locality_are_bitwise(dev, oracle):
    cases, _, _ = oracle
    for idx in (4, 5, 9):                                   # n = 33: d 513 (scalar), 1027 (scalar, strided), 4096 (16-byte loads)
        case, pad = cases[idx], FORWARD[idx][9]
        a, b = _run(case, dev, pad=pad), _run(case, dev, pad=pad)
        assert torch.equal(a["pred"], b["pred"]) and torch.equal(a["rowloss"], b["rowloss"])
        alone = _run(case, dev, pad=pad, rows=slice(20, 21))
        assert torch.equal(alone["pred"][0], a["pred"][20]) and torch.equal(alone["rowloss"][0], a["rowloss"][20]), case.name


@pytest.mark.parametrize("idx", [4, 9])
def test_both_routes_give_the_same_bits(dev, oracle, idx):
    """33 rows into a 1024-unit first layer take the direct route, the same row alone the split route."""
    from pti_ldm_vae_amd import ops
    cases, _, _ = oracle
    case, (_, n, d, hidden, *_), pad = cases[idx], FORWARD[idx], FORWARD[idx][9]
    assert ops.mlp_head_route(n, d, hidden[0]) == "direct" and ops.mlp_head_route(1, d, hidden[0]) == "split"
    full, alone = _run(case, dev, pad=pad), _run(case, dev, pad=pad, rows=slice(20, 21))
    assert torch.equal(alone["pred"][0], full["pred"][20]) and torch.equal(alone["rowloss"][0], full["rowloss"][20])


@pytest.mark.parametrize("n", [1, 8, 9, 1000])
def test_regression_metrics_against_fp64(dev, n):
    from pti_ldm_vae_amd import ops
    for t in (1, 6, 64):
        pred = O.uniform((n, t), 3 * n + t, -50.0, 50.0)
        tg = O.uniform((n, t), 5 * n + t, -50.0, 50.0)
        rl = O.uniform((n,), 7 * n + t, 0.0, 9.0)
        got = ops.regression_metrics(pred.to(dev), tg.to(dev), rl.to(dev), 8)
        want = O.fold_metrics(pred, tg, rl, 8, dtype=torch.float64)
        assert got.dtype == torch.float64 and got.shape == (2 * t + 3,)
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-12, atol=0)


# ---- end to end ---------------------------------------------------------------------------------------------------------
TARGETS = ["height_0", "width_0"]


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """16 tiny TIFFs, a [32, 64]-channel VAE at 64x64 and two epochs of train_regression (as tests/test_gpu_regression.py)."""
    from pti_ldm_vae_amd import train_regression
    from pti_ldm_vae_amd.data import write_tiff
    tmp = tmp_path_factory.mktemp("reg_eval")
    rng = np.random.default_rng(9)
    d = tmp / "data" / "dente"
    d.mkdir(parents=True)
    table = {}
    for i in range(16):
        img = np.zeros((80, 72), np.float32)
        hh, ww = 20 + 3 * i, 10 + 2 * i
        img[10:10 + hh // 2, 8:8 + ww] = 1.0 + rng.random((hh // 2, ww), dtype=np.float32)
        write_tiff(str(d / f"img_{i:03d}.tif"), img)
        table[f"img_{i:03d}.tif"] = {"height_0": float(hh), "width_0": float(ww), "other": 0.0}
    af = tmp / "attrs.json"
    af.write_text(json.dumps(table))
    vae_cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_no_adv.json")))
    vae_cfg["autoencoder_def"].update(channels=[32, 64], attention_levels=[False, False], num_res_blocks=1)
    vf = tmp / "vae.json"
    vf.write_text(json.dumps(vae_cfg))
    cfg = json.load(open(os.path.join(ROOT, "config", "reg_edente_from_dente.json")))
    cfg.update(run_dir=str(tmp / "run"), targets=TARGETS)
    cfg["data"].update(data_base_dir=str(tmp / "data"), attributes_path=str(af), patch_size=[64, 64], num_workers=2,
                       data_source="dente")
    cfg["vae"].update(config_file=str(vf), checkpoint=str(tmp / "nope.pth"))
    cfg["regressor_def"].update(hidden_dims=[32], dropout=0.0)
    cfg["regression_train"].update(batch_size=4, lr=3e-3, max_epochs=2, target_norm="standard")
    cfg.pop("evaluation", None)
    cf = tmp / "reg.json"
    cf.write_text(json.dumps(cfg))
    train_regression.main(["-c", str(cf), "--random-init-vae"])
    head = tmp / "run" / "trained_weights" / "head_best.pth"
    assert head.exists() and (tmp / "run" / "trained_weights" / "target_norm_stats.json").exists()
    return dict(tmp=tmp, cfg=str(cf), head=str(head), data=str(tmp / "data"), attrs=str(af), config=cfg)


def _fold_vector(m):
    return torch.tensor([m["val_loss"]] + [m[f"mae_{t}"] for t in TARGETS] + [m[f"mse_{t}"] for t in TARGETS] + [m["mae"], m["mse"]],
                        dtype=torch.float64)


def test_evaluate_regression_end_to_end(dev, run, oracle):
    from pti_ldm_vae_amd import evaluate_regression as E
    from pti_ldm_vae_amd.data import create_regression_eval_dataloader
    from pti_ldm_vae_amd.utils import regression_utils as R
    _, gate, _ = oracle
    base = ["-c", run["cfg"], "--checkpoint", run["head"], "--random-init-vae", "--batch-size", "5"]
    E.main(base)                                                                  # default output dir, default head
    doc = json.load(open(run["tmp"] / "run" / "eval" / "metrics.json"))
    assert set(doc) == {"metrics", "args", "files"} and len(doc["files"]) == 16
    assert set(doc["metrics"]) == {"val_loss", "mae", "mse"} | {f"{k}_{t}" for k in ("mae", "mse") for t in TARGETS}
    assert doc["args"]["head"] == "hip" and doc["args"]["resolved_input_dir"] == run["data"]
    assert doc["args"]["resolved_attributes_path"] == run["attrs"] and doc["args"]["seed"] == 42
    assert all(np.isfinite(v) for v in doc["metrics"].values())
    E.main(base + ["--head", "torch", "--output-dir", str(run["tmp"] / "eval_torch")])
    doc_t = json.load(open(run["tmp"] / "eval_torch" / "metrics.json"))
    hip, tor = _fold_vector(doc["metrics"]), _fold_vector(doc_t["metrics"])
    dev_fold = float((hip - tor).abs().max() / tor.abs().max())
    print(f"evaluate_regression: hip vs torch fold deviation {dev_fold:.2e} (bound {gate.bound['fold']:.2e})")
    assert dev_fold <= gate.bound["fold"]
    # --head torch IS validate_one_epoch on the same loader
    torch.manual_seed(42)
    config = json.load(open(run["cfg"]))
    model = E.build_model(config, TARGETS, dev, True)
    R.load_regression_checkpoint(E.Path(run["head"]), model, TARGETS)
    loader, _ = create_regression_eval_dataloader(run["data"], run["attrs"], TARGETS, (64, 64), 5, num_workers=2,
                                                  data_source="dente", device=dev)
    norm = E.load_optional_normalizer(run["tmp"] / "run", TARGETS)
    assert norm is not None
    val, metrics = R.validate_one_epoch(model, loader, R.build_loss_fn("mse"), dev, TARGETS, norm)
    want = _fold_vector({"val_loss": val, **metrics})
    assert float((tor - want).abs().max() / want.abs().max()) <= 1e-6


def test_inference_regression_end_to_end(dev, run):
    from pti_ldm_vae_amd import inference_regression as I
    base = ["-c", run["cfg"], "--checkpoint", run["head"], "--random-init-vae", "--input-dir", run["data"]]

    def predictions(extra, out=None):
        I.main(base + extra + (["--output-dir", str(run["tmp"] / out)] if out else []))
        path = (run["tmp"] / out if out else run["tmp"] / "run" / "inference") / "predictions.json"
        return json.load(open(path))["predictions"]

    full = predictions(["--batch-size", "8"])                                      # default output dir
    assert list(full) == [f"img_{i:03d}.tif" for i in range(16)]
    assert all(list(v) == TARGETS and all(np.isfinite(x) for x in v.values()) for v in full.values())
    assert len({v["height_0"] for v in full.values()}) > 1                         # the head sees the images
    five = predictions(["--batch-size", "8", "--num-samples", "5"], "inf5")
    assert five == {k: full[k] for k in list(full)[:5]}
    assert predictions(["--batch-size", "3"], "inf_b3") == full


def test_a_head_outside_the_limits_takes_the_torch_path_and_says_so(dev, run, capsys):
    from pti_ldm_vae_amd import evaluate_regression as E
    from pti_ldm_vae_amd.data import create_regression_eval_dataloader
    from pti_ldm_vae_amd.utils import regression_utils as R
    torch.manual_seed(42)
    config = json.load(open(run["cfg"]))
    config["regressor_def"]["hidden_dims"] = [2048]
    model = E.build_model(config, TARGETS, dev, True)
    loader, _ = create_regression_eval_dataloader(run["data"], run["attrs"], TARGETS, (64, 64), 8, num_workers=2,
                                                  num_samples=8, data_source="dente", device=dev)
    capsys.readouterr()
    val, metrics = R.evaluate_on_device(model, loader, "mse", TARGETS, None, 8)
    said = capsys.readouterr().out
    assert said.count("using the torch head") == 1 and "2048" in said
    want = R.validate_one_epoch(model, loader, R.build_loss_fn("mse"), dev, TARGETS, None)
    assert (val, metrics) == want
    pred = R.predict_on_device(model, loader, None)
    assert capsys.readouterr().out.count("using the torch head") == 1 and pred.shape == (8, 2) and pred.is_cuda

"""GPU tests of the guarded optimiser step (``csrc/optim_guard.hip``) against the fp64 oracle of
``tests/optim_guard_oracle.py``: the norm pass, detection of non-finite gradients, a clip / skip / EMA sequence, the
inactive guard against ``ops.adam_step``, bitwise reproducibility, the guard on a real model through ``VAETrainer``, and
``train_vae.main`` end to end.

Bounds (u = 2^-53):
  * ``sumsq`` against the exactly rounded sum (``math.fsum`` of the squares, which are exact in fp64): (n + 2) u relative,
    the worst case of any summation order of n non-negative terms.
  * ``norm`` against ``grad_scale * sqrt`` of the record's own ``sumsq``: 4 ulp (2^-50 relative).  The device code of the
    gfx950 build holds the refined fp64 square root (v_rsq_f64 plus the correction steps), not the bare instruction.
  * ``coef`` against the oracle: 2^-22 relative (its division is the fast-math reciprocal sequence).
  * parameters and moments: ``_report(..., 1e-6, 1e-6)``; one step's update: 2.4e-7 absolute, half an fp32 ulp of a parameter
    below 4 -- the bounds of ``test_adam_matches_torch`` for the same arithmetic.
The oracle gets the betas as the kernels see them: rounded to fp32 first (``pti_adam_step`` does the same)."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from optim_guard_oracle import GuardOracle
from test_gpu_ops import _report
from test_gpu_train import SMALL

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BETAS32 = (float(np.float32(0.9)), float(np.float32(0.999)))
LR = 2.5e-5


def _rec(ctl):
    from pti_ldm_vae_amd import ops
    return dict(zip(ops.GRAD_GUARD_COLUMNS, ctl.tolist()))


def _place(data, dev, misaligned):
    """``data`` on the device, contiguous; ``misaligned``: as ``buf[1:]``, whose pointer is 4-byte aligned only."""
    if not misaligned:
        g = data.to(dev)
        assert g.data_ptr() % 16 == 0
        return g
    buf = torch.empty(data.numel() + 1, device=dev)
    g = buf[1:]
    g.copy_(data)
    assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    return g


def _exact_sumsq(data):
    g = data.double().numpy()
    return math.fsum((g * g).tolist())


def _state(n, dev, seed, with_ema=True):
    """p (|p| < 4: half an fp32 ulp is below 2.4e-7), zero moments, EMA = p."""
    gen = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=gen) * 0.5).clamp_(-3.9, 3.9).to(dev)
    return p, torch.zeros_like(p), torch.zeros_like(p), (p.clone() if with_ema else None)


def _check_state(tag, got, orc):
    p, m, v, ema = got
    _report(f"{tag} p", p, torch.from_numpy(orc.p), 1e-6, 1e-6)
    _report(f"{tag} m", m, torch.from_numpy(orc.m), 1e-6, 1e-6)
    _report(f"{tag} v", v, torch.from_numpy(orc.v), 1e-6, 1e-6)
    if ema is not None:
        _report(f"{tag} ema", ema, torch.from_numpy(orc.ema), 1e-6, 1e-6)


def _check_update(tag, p_before, p_after, update):
    err = np.abs((p_after.double() - p_before.double()).cpu().numpy() - (-update)).max()
    print(f"{tag}: max |update - oracle's| = {err:.3e}")
    assert err <= 2.4e-7, (tag, err)


# ---- 1. norm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4097, 2 ** 20 + 3])
def test_norm(dev, n):
    from pti_ldm_vae_amd import ops
    gen = torch.Generator().manual_seed(100 + n % 97)
    base = torch.randn(n, generator=gen)
    ctl = ops.grad_guard_ctl(dev)
    worst = 0.0
    for scale in (1e-3, 1.0, 1e18):
        data = (base * scale).float()
        exact = _exact_sumsq(data)
        for misaligned in (False, True):
            g = _place(data, dev, misaligned)
            for grad_scale in (1.0, 0.5):
                ops.grad_guard(g, ctl=ctl, grad_scale=grad_scale, betas=BETAS32)
                r = _rec(ctl)
                rel = abs(r["sumsq"] - exact) / exact
                worst = max(worst, rel / ((n + 2) * U))
                assert rel <= (n + 2) * U, (scale, misaligned, grad_scale, r["sumsq"], exact, rel)
                want = grad_scale * math.sqrt(r["sumsq"])
                assert abs(r["norm"] - want) <= 2.0 ** -50 * want, (scale, misaligned, grad_scale, r["norm"], want)
                assert abs(r["norm"] - grad_scale * math.sqrt(exact)) <= ((n + 2) * U + 2.0 ** -50) * want
                assert r["coef"] == 1.0 and r["skip"] == 0.0 and r["grad_mul"] == grad_scale
    print(f"n={n}: worst sumsq error = {worst:.3f} of the bound (n + 2) u; 12 guarded norms -> applied_steps {r['applied_steps']}")
    assert r["applied_steps"] == 12.0 and r["skipped_steps"] == 0.0


def test_norm_of_zeros_and_of_huge_finite_gradients(dev):
    from pti_ldm_vae_amd import ops
    ctl = ops.grad_guard_ctl(dev)
    ops.grad_guard(torch.zeros(4097, device=dev), ctl=ctl, max_norm=1.0, skip_nonfinite=True, betas=BETAS32)
    r = _rec(ctl)
    assert r["sumsq"] == 0.0 and r["norm"] == 0.0 and r["coef"] == 1.0 and r["skip"] == 0.0 and r["applied_steps"] == 1.0
    # 1e30 is finite and its square is far outside fp32: the fp64 accumulation keeps the norm finite
    data = torch.zeros(4097)
    data[[0, 1000, 4096]] = torch.tensor([1e30, -1e30, 1e30])
    ops.grad_guard(data.to(dev), ctl=ctl, max_norm=1.0, skip_nonfinite=True, betas=BETAS32)
    r = _rec(ctl)
    want = math.sqrt(_exact_sumsq(data))
    assert math.isfinite(r["norm"]) and abs(r["norm"] - want) <= 2.0 ** -50 * want
    assert r["skip"] == 0.0 and r["skipped_steps"] == 0.0 and r["applied_steps"] == 2.0
    assert r["coef"] == pytest.approx(1.0 / (want + 1e-6), rel=2.0 ** -22)


# ---- 2. detection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 2 ** 20 + 3])
def test_nonfinite_gradient_is_detected_and_skipped(dev, n):
    from pti_ldm_vae_amd import ops
    gen = torch.Generator().manual_seed(7)
    clean = torch.randn(2, n, generator=gen) * 0.01
    p, m, v, ema = _state(n, dev, 11)
    ctl = ops.grad_guard_ctl(dev)
    orc = GuardOracle(p.cpu().numpy(), lr=LR, betas=BETAS32, skip_nonfinite=True, ema_decay=0.999)

    def step(g):
        ops.grad_guard(g, ctl=ctl, skip_nonfinite=True, betas=BETAS32, ema_decay=0.999)
        ops.adam_step_guarded(p, g, m, v, ctl=ctl, lr=LR, betas=BETAS32, ema=ema)

    step(clean[0].to(dev))          # one applied step first: the moments are not zero when the poison arrives
    orc.step(clean[0].numpy())
    skipped = 0
    for value in (float("nan"), float("inf"), float("-inf")):
        for where in (0, n // 2, n - 1):
            bad = clean[1].clone()
            bad[where] = value
            g = bad.to(dev)
            # without skip_nonfinite the record says bad and nothing else changes in how the step would be applied
            probe = ctl.clone()
            ops.grad_guard(g, ctl=probe, max_norm=1.0, betas=BETAS32)
            r = _rec(probe)
            assert not math.isfinite(r["norm"]) and r["skip"] == 0.0 and r["coef"] == 1.0, (value, where, r)
            before = [t.clone() for t in (p, m, v, ema)]
            step(g)
            skipped += 1
            r = _rec(ctl)
            assert r["skip"] == 1.0 and not math.isfinite(r["norm"]), (value, where, r)
            assert r["applied_steps"] == 1.0 and r["skipped_steps"] == float(skipped), (value, where, r)
            for name, a, b in zip("p m v ema".split(), (p, m, v, ema), before):
                assert torch.equal(a, b), (value, where, name)
    # the next clean step uses t = applied + 1 = 2: an oracle that never saw the poisoned steps
    p_before = p.clone()
    step(clean[1].to(dev))
    d = orc.step(clean[1].numpy())
    r = _rec(ctl)
    assert r["applied_steps"] == 2.0 == float(orc.applied) and r["skipped_steps"] == 9.0 and r["skip"] == 0.0
    assert r["bias1"] == pytest.approx(d["bias1"], rel=1e-12) and r["bias2_sqrt"] == pytest.approx(d["bias2_sqrt"], rel=1e-12)
    _check_update(f"n={n} clean step after 9 skipped", p_before, p, d["update"])
    _check_state(f"n={n}", (p, m, v, ema), orc)


# ---- 3. sequence ----------------------------------------------------------------------------------------------------
def test_clip_skip_ema_sequence(dev):
    from pti_ldm_vae_amd import ops
    n, decay, max_norm = 10007, 0.999, 1.0
    gen = torch.Generator().manual_seed(21)
    grads = [torch.randn(n, generator=gen) * s for s in (1e-3, 1.0, 1.0, 2.0, 1e-3, 1e-3)]   # norms ~0.1, 100, -, 200, 0.1, 0.1
    grads[2][n // 3] = float("nan")
    p, m, v, ema = _state(n, dev, 22)
    ctl = ops.grad_guard_ctl(dev)
    orc = GuardOracle(p.cpu().numpy(), lr=LR, betas=BETAS32, max_norm=max_norm, skip_nonfinite=True, ema_decay=decay)
    for i, gh in enumerate(grads):
        g = gh.to(dev)
        p_before = p.clone()
        ops.grad_guard(g, ctl=ctl, max_norm=max_norm, skip_nonfinite=True, betas=BETAS32, ema_decay=decay)
        ops.adam_step_guarded(p, g, m, v, ctl=ctl, lr=LR, betas=BETAS32, ema=ema)
        d = orc.step(gh.numpy())
        r = _rec(ctl)
        print(f"step {i}: norm {r['norm']:.6g} coef {r['coef']:.6g} skip {r['skip']} applied {r['applied_steps']} "
              f"skipped {r['skipped_steps']} ema decay {r['ema_decay']:.6g}")
        assert (r["skip"] == 1.0) == d["skip"] == (i == 2)
        assert (r["applied_steps"], r["skipped_steps"]) == (float(d["applied_steps"]), float(d["skipped_steps"]))
        assert abs(r["coef"] - d["coef"]) <= 2.0 ** -22 * d["coef"], (i, r["coef"], d["coef"])
        assert (d["coef"] < 1.0) == (i in (1, 3))
        if not d["skip"]:
            assert r["ema_decay"] == pytest.approx(d["ema_decay"], rel=1e-14)     # a few ulp: the fast-math fp64 division
        _check_update(f"step {i}", p_before, p, d["update"])
    assert (orc.applied, orc.skipped) == (5, 1)
    _check_state("sequence", (p, m, v, ema), orc)
    assert not torch.equal(ema, p)


# ---- 4. inactive guard ----------------------------------------------------------------------------------------------
def test_inactive_guard_is_adam_step(dev):
    from pti_ldm_vae_amd import ops
    n = 10007
    gen = torch.Generator().manual_seed(31)
    p, m, v, _ = _state(n, dev, 32, with_ema=False)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ctl = ops.grad_guard_ctl(dev)
    for step in range(1, 4):
        g = (torch.randn(n, generator=gen) * 0.01).to(dev)
        ops.adam_step(p2, g, m2, v2, lr=LR, step=step, grad_scale=0.5)
        ops.grad_guard(g, ctl=ctl, grad_scale=0.5, max_norm=1e30, betas=BETAS32)
        ops.adam_step_guarded(p, g, m, v, ctl=ctl, lr=LR, betas=BETAS32)
        assert _rec(ctl)["coef"] == 1.0
    diff = (p.double() - p2.double()).abs().max().item()
    print(f"guard with max_norm 1e30 vs adam_step after 3 steps: max |dp| = {diff:.3e}; bitwise equal: "
          f"{torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)}")
    assert diff <= 2.4e-7


# ---- 5. reproducibility ---------------------------------------------------------------------------------------------
def test_guarded_step_is_bitwise_reproducible(dev):
    from pti_ldm_vae_amd import ops
    n = 2 ** 20 + 3
    gen = torch.Generator().manual_seed(41)
    grads = [(torch.randn(n, generator=gen) * s).to(dev) for s in (0.01, 3.0)]
    runs = []
    for _ in range(2):
        p, m, v, ema = _state(n, dev, 42)
        ctl = ops.grad_guard_ctl(dev)
        parts = []
        for g in grads:
            ws = ops.grad_guard(g, ctl=ctl, max_norm=1.0, skip_nonfinite=True, betas=BETAS32, ema_decay=0.999)
            parts.append(ws.clone())
            ws.fill_(float("nan"))          # the next launch may not depend on what the scratch held
            ops.adam_step_guarded(p, g, m, v, ctl=ctl, lr=LR, betas=BETAS32, ema=ema)
        runs.append((ctl.clone(), parts, p, m, v, ema))
    a, b = runs
    assert a[1][0].numel() * 4 == 16 * 257       # 2^20 + 3 elements: 257 workgroups, one {sumsq, count} pair each
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)


def test_ops_refuse_bad_arguments(dev):
    from pti_ldm_vae_amd import _lib, ops
    g = torch.zeros(8, device=dev)
    ctl = ops.grad_guard_ctl(dev)
    with pytest.raises(ValueError):
        ops.grad_guard(g, ctl=torch.zeros(8, dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        ops.grad_guard(g, ctl=torch.zeros(10, device=dev))
    with pytest.raises(TypeError):
        ops.grad_guard(g.double(), ctl=ctl)
    with pytest.raises(_lib.PtiError):
        ops.grad_guard(g, ctl=ctl, max_norm=float("nan"))
    with pytest.raises(_lib.PtiError):
        ops.grad_guard(g, ctl=ctl, ema_decay=1.0)
    with pytest.raises(ValueError):
        ops.adam_step_guarded(g, g, g, torch.zeros(9, device=dev), ctl=ctl, lr=1e-3)
    assert not ctl.any()


# ---- 6. on a real model ---------------------------------------------------------------------------------------------
def _model(dev, seed=0):
    from pti_ldm_vae_amd.models import VAEModel
    torch.manual_seed(seed)
    return VAEModel.from_config(SMALL).to(dev)


def _check_norm_over_parameters(tag, net, ctl):
    """The record's norm is taken over the whole arena; the parameters' own gradients must give the same: whatever the
    arena holds besides them (strided slots, alignment gaps) is zero in the gradient arena at step() time."""
    flat = np.concatenate([p.grad.double().cpu().numpy().ravel() for _, p in net.named_parameters()])
    exact = math.fsum((flat * flat).tolist())
    n = net.grad_arena.numel()
    r = _rec(ctl)
    rel = abs(r["sumsq"] - exact) / exact
    print(f"{tag}: arena {n} elements, {flat.size} of them parameters; norm {r['norm']:.6g}; sumsq error {rel / U:.1f} u")
    assert rel <= (n + 2) * U, (tag, r["sumsq"], exact)
    assert abs(r["norm"] - math.sqrt(r["sumsq"])) <= 2.0 ** -50 * r["norm"]
    return r


def test_guard_on_the_vae_trainer(dev):
    from pti_ldm_vae_amd.trainer import VAETrainer
    torch.manual_seed(1)
    x = torch.randn(2, 1, 64, 64, device=dev)
    eps = torch.randn(2, 4, 32, 32, device=dev)
    m = _model(dev)
    net = m.autoencoder
    lr, clip = 1e-3, 1e-3
    tr = VAETrainer(m, lr=lr, clip_norm=clip, skip_nonfinite=True, ema_decay=0.999)
    opt = tr.opt
    p0 = net.param_arena.clone()
    assert torch.equal(opt.ema, p0)
    out = tr.step(x, eps)
    torch.cuda.synchronize()
    assert math.isfinite(out["loss"].item())
    r = _check_norm_over_parameters("VAE", net, opt.ctl)
    assert r["coef"] < 1.0 and r["skip"] == 0.0 and r["applied_steps"] == 1.0          # the clip is certainly active
    orc = GuardOracle(p0.cpu().numpy(), lr=lr, betas=BETAS32, max_norm=clip, skip_nonfinite=True, ema_decay=0.999)
    d = orc.step(net.grad_arena.cpu().numpy())
    assert abs(r["coef"] - d["coef"]) <= 2.0 ** -22 * d["coef"]
    _check_update("VAE step", p0, net.param_arena, d["update"])
    _check_state("VAE step", (net.param_arena, opt.exp_avg, opt.exp_avg_sq, opt.ema), orc)
    stats = opt.guard_stats()
    assert stats == {"grad_norm": r["norm"], "clip_coef": r["coef"], "skipped": False, "applied_steps": 1, "skipped_steps": 0}
    assert opt.step_count == 1 and float(opt.state_dict()["state"][0]["step"]) == 1.0
    # a poisoned gradient arena: the step is skipped, nothing moves
    before = [t.clone() for t in (net.param_arena, opt.exp_avg, opt.exp_avg_sq, opt.ema)]
    net.grad_arena[net.grad_arena.numel() // 2] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    for a, b in zip((net.param_arena, opt.exp_avg, opt.exp_avg_sq, opt.ema), before):
        assert torch.equal(a, b)
    stats = opt.guard_stats()
    assert stats["skipped"] and stats["applied_steps"] == 1 and stats["skipped_steps"] == 1 and opt.step_count == 1
    out = tr.step(x, eps)
    assert math.isfinite(out["loss"].item())
    assert opt.guard_stats()["applied_steps"] == 2 and not torch.equal(net.param_arena, before[0])


def test_guard_on_the_discriminator(dev):
    from pti_ldm_vae_amd.models import PatchDiscriminator
    from pti_ldm_vae_amd.trainer import VAETrainer
    torch.manual_seed(2)
    x = torch.randn(2, 1, 64, 64, device=dev)
    eps = torch.randn(2, 4, 32, 32, device=dev)
    m = _model(dev)
    torch.manual_seed(3)
    disc = PatchDiscriminator(spatial_dims=2, num_layers_d=3, channels=32, in_channels=1, out_channels=1, norm="INSTANCE").to(dev)
    tr = VAETrainer(m, lr=1e-4, discriminator=disc, adv_weight=0.5, clip_norm=1e-3, skip_nonfinite=True, ema_decay=0.999)
    assert tr.opt_d.guarded and not hasattr(tr.opt_d, "ema") and tr.opt_d.ctl.data_ptr() != tr.opt.ctl.data_ptr()
    d0 = disc.param_arena.clone()
    out = tr.step(x, eps, adversarial=True)
    torch.cuda.synchronize()
    assert math.isfinite(out["loss"].item()) and math.isfinite(out["adv_disc"].item())
    _check_norm_over_parameters("VAE (adversarial step)", m.autoencoder, tr.opt.ctl)
    r = _check_norm_over_parameters("discriminator", disc, tr.opt_d.ctl)
    assert r["coef"] < 1.0 and r["applied_steps"] == 1.0
    orc = GuardOracle(d0.cpu().numpy(), lr=1e-4, betas=BETAS32, max_norm=1e-3, skip_nonfinite=True)
    d = orc.step(disc.grad_arena.cpu().numpy())
    _check_update("discriminator step", d0, disc.param_arena, d["update"])
    _check_state("discriminator step", (disc.param_arena, tr.opt_d.exp_avg, tr.opt_d.exp_avg_sq, None), orc)


def test_guarded_step_graph_mode_is_bitwise_the_eager_step(dev, monkeypatch):
    from pti_ldm_vae_amd.trainer import VAETrainer
    torch.manual_seed(5)
    x = torch.randn(4, 2, 1, 64, 64, device=dev)
    eps = torch.randn(4, 2, 4, 32, 32, device=dev)
    state = {k: v.clone() for k, v in _model(dev).state_dict().items()}
    runs = []
    for graph in ("0", "1"):
        monkeypatch.setenv("PTI_STEP_GRAPH", graph)
        m = _model(dev, seed=9)
        m.load_state_dict(state)
        tr = VAETrainer(m, lr=1e-3, clip_norm=1e-3, skip_nonfinite=True, ema_decay=0.999)
        assert tr.step_graph is (graph == "1")
        arenas = []
        for i in range(4):        # the first two steps of a trainer are eager in either mode; the graph replays from the third
            tr.step(x[i], eps[i])
            if i in (1, 3):
                torch.cuda.synchronize()
                arenas.append((m.autoencoder.param_arena.clone(), tr.opt.ema.clone(), tr.opt.ctl.clone()))
        runs.append((arenas, len(tr._graphs)))
    assert runs[0][1] == 0 and runs[1][1] == 1
    for (p0, e0, c0), (p1, e1, c1) in zip(runs[0][0], runs[1][0]):
        assert torch.equal(p0, p1) and torch.equal(e0, e1) and torch.equal(c0.view(torch.int64), c1.view(torch.int64))
    assert runs[0][0][1][2][0].item() == 4.0


# ---- 7. train_vae.main end to end -----------------------------------------------------------------------------------
NEW_METRICS = ("train/grad_norm", "train/grad_clip_coef", "train/skipped_steps")


def _config(tmp_path, name, **train_keys):
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "config", "vae_dente_no_adv.json")))
    cfg["run_dir"] = str(tmp_path / name)
    cfg["autoencoder_def"].update(channels=[32, 64], attention_levels=[False, False], num_res_blocks=1)
    cfg["autoencoder_train"].update(batch_size=2, patch_size=[64, 64], max_epochs=2, perceptual_weight=0.0, **train_keys)
    cf = tmp_path / f"{name}.json"
    cf.write_text(json.dumps(cfg))
    return cfg, cf


def test_train_script_with_the_guard(dev, tmp_path, capsys):
    from pti_ldm_vae_amd import train_vae
    from pti_ldm_vae_amd.models import VAEModel
    from pti_ldm_vae_amd.optim import FlatAdam
    from pti_ldm_vae_amd.utils import read_config
    from pti_ldm_vae_amd.utils.vae_loader import load_vae_config, load_vae_model
    _, cf = _config(tmp_path, "guarded", grad_clip_norm=1.0, skip_nonfinite_steps=True, ema_decay=0.999)
    train_vae.main(["-c", str(cf), "--synthetic", "8", "--log-every", "1"])
    lines = [json.loads(l) for l in open(tmp_path / "guarded" / "metrics.jsonl")]
    train = [l for l in lines if "train/loss_total" in l]
    assert train and all(set(NEW_METRICS) <= set(l) for l in train)
    assert all(math.isfinite(l["train/grad_norm"]) and l["train/grad_norm"] > 0 for l in train)
    assert all(0 < l["train/grad_clip_coef"] <= 1 and l["train/skipped_steps"] == 0 for l in train)
    wdir = tmp_path / "guarded" / "trained_weights"
    files = sorted(os.listdir(wdir))
    best = [f for f in files if f.startswith("checkpoint_epoch")]
    assert len(best) == 1
    epoch = best[0][16:-4]
    assert "autoencoder_ema_last.pt" in files and f"autoencoder_ema_epoch{epoch}.pth" in files
    assert len([f for f in files if f.startswith("autoencoder_ema_epoch")]) == 1
    last = torch.load(wdir / "autoencoder_last.pt", weights_only=True)
    for name in ("autoencoder_ema_last.pt", f"autoencoder_ema_epoch{epoch}.pth"):
        ema = torch.load(wdir / name, weights_only=True)
        assert list(ema) == list(last) and all(ema[k].shape == last[k].shape and ema[k].dtype == last[k].dtype for k in last)
        assert any(not torch.equal(ema[k], last[k]) for k in last)
    vae = load_vae_model(load_vae_config(str(cf)), str(wdir / "autoencoder_ema_last.pt"), dev)
    with torch.no_grad():
        assert vae.encode_deterministic(torch.zeros(1, 1, 64, 64, device=dev)).shape == (1, 4, 32, 32)
    ck = torch.load(wdir / best[0], weights_only=True)
    assert "ema_state_dict" in ck and list(ck["ema_state_dict"]) == list(last)
    # resume: the EMA comes back bit for bit; a checkpoint without the key starts it from the loaded weights and says so
    args = types.SimpleNamespace(resume_ckpt=True, checkpoint_dir=str(wdir / best[0]))
    model = VAEModel.from_config(read_config(str(cf))["autoencoder_def"]).to(dev)
    opt = FlatAdam(model.autoencoder, 1e-4, clip_norm=1.0, skip_nonfinite=True, ema_decay=0.999)
    train_vae.load_checkpoint(args, model, opt, dev)
    for n, _ in model.autoencoder.named_parameters():
        assert torch.equal(model.autoencoder.slot_view(opt.ema, n).cpu(), ck["ema_state_dict"][n]), n
    assert opt.step_count == int(float(ck["optimizer_g_state_dict"]["state"][0]["step"])) > 0
    old = {k: v for k, v in ck.items() if k != "ema_state_dict"}
    torch.save(old, tmp_path / "old.pth")
    capsys.readouterr()
    train_vae.load_checkpoint(types.SimpleNamespace(resume_ckpt=True, checkpoint_dir=str(tmp_path / "old.pth")), model, opt, dev)
    assert "EMA starts from the loaded weights" in capsys.readouterr().out
    for n, _ in model.autoencoder.named_parameters():
        assert torch.equal(model.autoencoder.slot_view(opt.ema, n).cpu(), ck["autoencoder_state_dict"][n]), n
    # without the keys: none of the new files, none of the new metric names
    _, cf2 = _config(tmp_path, "plain")
    train_vae.main(["-c", str(cf2), "--synthetic", "8", "--log-every", "1"])
    plain_files = os.listdir(tmp_path / "plain" / "trained_weights")
    assert not [f for f in plain_files if "ema" in f]
    plain_best = [f for f in plain_files if f.startswith("checkpoint_epoch")]
    assert "ema_state_dict" not in torch.load(tmp_path / "plain" / "trained_weights" / plain_best[0], weights_only=True)
    for l in (json.loads(l) for l in open(tmp_path / "plain" / "metrics.jsonl")):
        assert not set(NEW_METRICS) & set(l)

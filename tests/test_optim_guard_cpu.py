"""CPU tests of the guarded optimiser step's host side: the fp64 oracle against ``clip_grad_norm_`` +
``torch.optim.Adam``, the partials query, ``FlatAdam``'s new constructor arguments and (de)serialisation, and the config
keys.  No GPU compute: the kernels are tested in ``tests/test_gpu_optim_guard.py``."""
import glob
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from optim_guard_oracle import GuardOracle, ema_decay_in_effect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_model():
    from oracle.autoencoderkl import CONFIG_A
    from pti_ldm_vae_amd.models import VAEModel
    return VAEModel.from_config(dict(CONFIG_A, channels=[32, 32], attention_levels=[False, False], norm_num_groups=16))


def test_oracle_matches_clip_grad_norm_and_torch_adam():
    """Six steps -- small, large (clipped), NaN (skipped: torch's side does not call step()), large, small, small -- on
    fp64 CPU tensors: norm, coefficient, parameters, both moments and the step counter within 1e-12 relative (both
    sides are fp64); the EMA against torch's ``lerp`` with the warm-up decay."""
    rng = np.random.default_rng(3)
    n, lr, max_norm, decay, grad_scale = 1001, 1e-3, 1.0, 0.999, 0.5
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * s for s in (1e-3, 10.0, 1.0, 10.0, 1e-3, 1e-3)]
    grads[2][n // 2] = float("nan")
    orc = GuardOracle(p0, lr=lr, max_norm=max_norm, skip_nonfinite=True, ema_decay=decay)
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr)
    ema = p.detach().clone()
    applied = 0
    for i, g in enumerate(grads):
        d = orc.step(g, grad_scale)
        p.grad = torch.tensor(g, dtype=torch.float64) * grad_scale
        if not bool(torch.isfinite(p.grad).all()):
            assert d["skip"] and d["bad"] and d["coef"] == 1.0 and not d["update"].any(), i
            continue
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        assert not d["skip"]
        assert d["norm"] == pytest.approx(float(total), rel=1e-12)
        assert (d["coef"] < 1.0) == (float(total) > max_norm), i
        assert d["coef"] == pytest.approx(min(1.0, max_norm / (float(total) + 1e-6)), rel=1e-12)
        opt.step()
        applied += 1
        ema.lerp_(p.detach(), 1.0 - ema_decay_in_effect(decay, applied))
        st = opt.state[p]
        assert float(st["step"]) == orc.applied == applied
        for name, got, ref in (("p", orc.p, p.detach()), ("m", orc.m, st["exp_avg"]), ("v", orc.v, st["exp_avg_sq"]),
                               ("ema", orc.ema, ema)):
            ref = ref.numpy()
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err <= 1e-12, (i, name, err)
    assert (orc.applied, orc.skipped) == (5, 1)
    assert [ema_decay_in_effect(decay, t) for t in (1, 2)] == [2.0 / 11.0, 3.0 / 12.0] and ema_decay_in_effect(decay, 10 ** 6) == decay
    # without skip_nonfinite the poisoned step goes through, as it does today
    d = GuardOracle(p0, lr=lr, max_norm=max_norm).step(grads[2])
    assert d["bad"] and not d["skip"] and d["coef"] == 1.0 and d["applied_steps"] == 1


def test_partials_query_is_host_arithmetic():
    from pti_ldm_vae_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "pti_vae.h")).read()
    cap = int(re.search(r"#define PTI_GRAD_GUARD_PARTIALS_CAP (\d+)", text).group(1))
    cols = int(re.search(r"#define PTI_GRAD_GUARD_COLUMNS (\d+)", text).group(1))
    assert ops.GRAD_GUARD_PARTIALS_CAP == _lib.GRAD_GUARD_PARTIALS_CAP == cap
    assert ops.GRAD_GUARD_COLUMNS is _lib.GRAD_GUARD_COLUMNS and len(_lib.GRAD_GUARD_COLUMNS) == cols
    assert _lib.GRAD_GUARD_COLUMNS[:6] == ("applied_steps", "skipped_steps", "sumsq", "norm", "coef", "skip")
    q = _lib.lib().pti_grad_guard_partials
    assert q(1) == 1 and q(0) == 0 and q(-5) == 0
    sizes = sorted({1, 3, 255, 256, 257, 4096, 4097, 10007, 2 ** 20 + 3, 2 ** 22, 2 ** 22 + 1, 83_000_000, 2 ** 31 + 5, 2 ** 40}
                   | {int(1.37 ** k) for k in range(1, 70)})
    got = [q(n) for n in sizes]
    assert all(1 <= g <= cap for g in got)
    assert all(a <= b for a, b in zip(got, got[1:]))
    assert q(4097) == 2 and q(2 ** 40) == cap


def test_flat_adam_refuses_bad_guard_arguments():
    from pti_ldm_vae_amd.optim import FlatAdam
    net = _small_model().autoencoder
    for bad in (0, -1.0, float("inf"), float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="clip_norm"):
            FlatAdam(net, 1e-4, clip_norm=bad)
    for bad in (0, 1, 1.5, -0.1, float("nan"), "0.999", True):
        with pytest.raises(ValueError, match="ema_decay"):
            FlatAdam(net, 1e-4, ema_decay=bad)
    opt = FlatAdam(net, 1e-4, clip_norm=1.0, ema_decay=0.999, skip_nonfinite=True)
    assert opt.guarded and opt.clip_norm == 1.0 and opt.ema_decay == 0.999 and opt.skip_nonfinite


def test_flat_adam_with_the_guard_off_is_todays_object():
    """All three options off: no ``ema``, no control record, ``step_count`` a plain host integer, and the torch-format
    state exactly what tests/test_host_cpu.py::test_flat_adam_state_dict_is_torch_adam_compatible pins."""
    from pti_ldm_vae_amd.optim import FlatAdam
    m = _small_model()
    opt = FlatAdam(m.autoencoder, lr=1e-4)
    assert not opt.guarded and not hasattr(opt, "ema") and not hasattr(opt, "ctl")
    assert opt.step_count == 0 and opt.state_dict()["state"] == {}
    with pytest.raises(RuntimeError):
        opt.guard_stats()
    with pytest.raises(RuntimeError):
        opt.ema_state_dict()
    opt.step_count = 3
    opt.exp_avg.fill_(0.5)
    opt.exp_avg_sq.fill_(0.25)
    sd = opt.state_dict()
    names = [n for n, _ in m.autoencoder.named_parameters()]
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(len(names)))
    assert sd["param_groups"] == [{"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False,
                                   "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                                   "fused": None, "decoupled_weight_decay": False, "params": list(range(len(names)))}]
    for i, (n, p) in enumerate(m.autoencoder.named_parameters()):
        st = sd["state"][i]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 3.0
        assert st["exp_avg"].shape == p.shape and torch.all(st["exp_avg"] == 0.5) and torch.all(st["exp_avg_sq"] == 0.25)
    ref = torch.optim.Adam(m.parameters(), lr=1.0)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 1e-4 and float(ref.state[next(iter(m.parameters()))]["step"]) == 3


def test_guarded_state_dict_and_ema_round_trip_on_cpu():
    """The guarded object keeps its step counter in the control record: the torch-format state still loads into
    ``torch.optim.Adam`` and back, and the EMA travels as a plain state dict with the model's keys and shapes."""
    from pti_ldm_vae_amd.models import VAEModel
    from pti_ldm_vae_amd.optim import FlatAdam
    torch.manual_seed(5)
    m = _small_model()
    net = m.autoencoder
    opt = FlatAdam(net, lr=1e-4, clip_norm=2.0, skip_nonfinite=True, ema_decay=0.99)
    assert torch.equal(opt.ema, net.param_arena) and opt.ema.data_ptr() != net.param_arena.data_ptr()
    assert opt.ctl.dtype == torch.float64 and opt.ctl.numel() == 10 and not opt.ctl.any()
    opt.step_count = 7
    assert opt.step_count == 7 and float(opt.ctl[0]) == 7.0
    opt.ctl[1] = 2.0
    opt.ctl[3], opt.ctl[4] = 3.5, 0.25
    assert opt.guard_stats() == {"grad_norm": 3.5, "clip_coef": 0.25, "skipped": False, "applied_steps": 7, "skipped_steps": 2}
    opt.exp_avg.normal_()
    opt.exp_avg_sq.uniform_()
    sd = opt.state_dict()
    ref = torch.optim.Adam(m.parameters(), lr=1.0)
    ref.load_state_dict(sd)
    assert float(ref.state[next(iter(m.parameters()))]["step"]) == 7
    opt2 = FlatAdam(net, lr=5.0, ema_decay=0.5)
    opt2.load_state_dict(ref.state_dict())
    assert opt2.step_count == 7 and opt2.lr == 1e-4
    for n, _ in net.named_parameters():
        assert torch.equal(net.slot_view(opt2.exp_avg, n), net.slot_view(opt.exp_avg, n))
        assert torch.equal(net.slot_view(opt2.exp_avg_sq, n), net.slot_view(opt.exp_avg_sq, n))
    # EMA: model-format keys and shapes, other values; loads into a VAEModel like any weights; round-trips bitwise
    opt.ema.add_(torch.randn_like(opt.ema))
    esd, msd = opt.ema_state_dict(), m.state_dict()
    assert list(esd) == list(msd) and all(esd[k].shape == msd[k].shape for k in msd)
    assert any(not torch.equal(esd[k], msd[k]) for k in msd)
    for n, _ in net.named_parameters():
        assert torch.equal(esd[n], net.slot_view(opt.ema, n))
    m2 = _small_model()
    m2.load_state_dict(esd)
    assert all(torch.equal(v, esd[k]) for k, v in m2.state_dict().items())
    opt2.load_ema_state_dict(esd)
    for n, _ in net.named_parameters():
        assert torch.equal(net.slot_view(opt2.ema, n), net.slot_view(opt.ema, n))
    with pytest.raises(ValueError, match="missing"):
        opt2.load_ema_state_dict({})


def test_discriminator_optimiser_takes_clip_and_skip():
    from pti_ldm_vae_amd.models import PatchDiscriminator
    from pti_ldm_vae_amd.optim import FlatAdam
    net = PatchDiscriminator()
    opt = FlatAdam(net, 1e-3, clip_norm=1.0, skip_nonfinite=True)
    assert opt.guarded and not hasattr(opt, "ema")
    opt.step_count = 4
    ref = torch.optim.Adam(net.parameters(), lr=1e-3)
    ref.load_state_dict(opt.state_dict())
    assert float(ref.state[next(iter(net.parameters()))]["step"]) == 4


def test_resolve_guard_settings():
    from pti_ldm_vae_amd.utils import read_config, resolve_guard_settings
    shipped = sorted(glob.glob(os.path.join(ROOT, "config", "*.json")))
    assert len(shipped) >= 5
    for path in shipped:
        cfg = read_config(path)
        if "autoencoder_train" in cfg:
            assert resolve_guard_settings(cfg["autoencoder_train"]) == (None, False, None), path
    assert resolve_guard_settings({}) == (None, False, None)
    tr = json.loads('{"lr": 1e-4, "grad_clip_norm": 1, "skip_nonfinite_steps": true, "ema_decay": 0.999}')
    assert resolve_guard_settings(tr) == (1.0, True, 0.999)
    assert resolve_guard_settings({"grad_clip_norm": None, "skip_nonfinite_steps": "false", "ema_decay": None}) == (None, False, None)
    assert resolve_guard_settings({"skip_nonfinite_steps": "true"}) == (None, True, None)
    for key, bad in (("grad_clip_norm", 0), ("grad_clip_norm", -2.0), ("grad_clip_norm", float("inf")), ("grad_clip_norm", "1.0"),
                     ("grad_clip_norm", True), ("ema_decay", 0.0), ("ema_decay", 1.0), ("ema_decay", 1.5), ("ema_decay", "0.9"),
                     ("ema_decay", float("nan")), ("skip_nonfinite_steps", 1), ("skip_nonfinite_steps", [True])):
        with pytest.raises(ValueError, match=key):
            resolve_guard_settings({key: bad})
    assert math.isclose(resolve_guard_settings({"ema_decay": 0.9999})[2], 0.9999)

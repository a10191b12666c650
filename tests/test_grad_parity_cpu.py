"""CPU checks of the per-tensor gradient comparator (tests/grad_parity.py) on the oracle's own gradients.

Config A and config AR at 32x32, batch 2: the fp32 oracle's autograd gradients must pass against the fp64 oracle's,
with and without synthetic 16-bit-sized noise (g * (1 + 2^-8 randn) per element, bf16's rounding step); every mutation
of the comparator's self-check must be flagged on both; and the structural zeros must be exactly the attention key
biases.  The gate is ``grad_parity.GATE``, the one the GPU tests use (tests/test_gpu_grad_per_tensor.py), so this
also shows that the tolerances chosen from MI355X measurements still catch every mutation.
"""
import functools

import pytest
import torch

from grad_parity import CLASSES, GATE, Comparator, failures, report, tensor_class, worst
from oracle.autoencoderkl import CONFIG_A, CONFIG_AR, build_oracle, synthetic_images
from oracle.losses import train_step_losses

CFGS = {"A": CONFIG_A, "AR": CONFIG_AR}
N_PARAMS = {"A": 218, "AR": 182}


@functools.lru_cache(maxsize=None)
def _grads(tag, dtype):
    cfg = CFGS[tag]
    torch.manual_seed(0)
    oracle = build_oracle(cfg, 42).to(dtype)
    x = synthetic_images(2, cfg["in_channels"], 32, seed=42).to(dtype)
    lat = 32 // 2 ** (len(cfg["channels"]) - 1)
    eps = torch.randn(2, cfg["latent_channels"], lat, lat, generator=torch.Generator().manual_seed(43)).to(dtype)
    loss, _, _, _ = train_step_losses(oracle, x, eps)
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in oracle.named_parameters()}


def _noisy(g, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return {n: t * (1 + 2.0 ** -8 * torch.randn(t.shape, generator=gen, dtype=t.dtype)) for n, t in g.items()}


@pytest.mark.parametrize("tag", list(CFGS))
def test_structural_zeros_are_exactly_the_key_biases(tag):
    g64 = _grads(tag, torch.float64)
    cmp = Comparator(g64)
    assert len(g64) == N_PARAMS[tag]
    keys = {n for n in g64 if n.endswith(".attn.to_k.bias")}
    assert len(keys) == 2                                 # encoder and decoder mid-block attention
    assert cmp.zeros == keys, sorted(cmp.zeros ^ keys)
    # every class is populated, so every bound of the gate is exercised
    assert {tensor_class(n, t.numel()) for n, t in g64.items()} == set(CLASSES)


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("tag", list(CFGS))
def test_fp32_oracle_passes_against_fp64(tag, noise):
    g64, g32 = _grads(tag, torch.float64), _grads(tag, torch.float32)
    if noise:
        g32 = _noisy(g32)
    cmp = Comparator(g64)
    rows = cmp.rows(g32)
    print("\n" + report(rows, f"{tag}@32 fp32{' + 2^-8 noise' if noise else ''} vs fp64"))
    assert len(rows) == N_PARAMS[tag]
    bad = failures(rows, GATE)
    assert not bad, "\n".join(bad)
    w = worst(rows)
    if not noise:      # fp32 autograd agrees with fp64 to ~1e-5 on every tensor
        assert all(a <= 1e-4 and r <= 1e-4 for a, r in (w[c] for c in CLASSES)), w
        assert w["zeros"] <= 1e-3, w


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("tag", list(CFGS))
def test_every_mutation_is_flagged(tag, noise):
    g64, g32 = _grads(tag, torch.float64), _grads(tag, torch.float32)
    if noise:
        g32 = _noisy(g32)
    cmp = Comparator(g64)
    count, missed = cmp.self_check(g32, GATE)
    n = N_PARAMS[tag]
    # five value mutations per tensor except the two structural zeros, plus a swap wherever a same-shaped partner exists
    swaps = sum(cmp.swap_partner(k) is not None for k in g64)
    assert count == 5 * (n - 2) + swaps, (count, swaps)
    # the tensors without a swap partner are exactly those with a shape of their own (13 in both configs)
    unique = {k for k in g64 if sum(t.shape == g64[k].shape for t in g64.values()) == 1}
    assert {k for k in g64 if cmp.swap_partner(k) is None} == unique and swaps == n - len(unique) == n - 13
    assert not missed, missed[:10]


def test_gate_catches_a_mis_scaled_structural_zero_partner():
    """A key bias gradient routed to the query bias slot (and vice versa) is flagged on both tensors."""
    g64, g32 = _grads("A", torch.float64), _grads("A", torch.float32)
    cmp = Comparator(g64)
    k = next(n for n in g64 if n.endswith(".attn.to_k.bias"))
    q = k.replace("to_k", "to_q")
    assert cmp.row(q, g32[k]).failure(GATE) is not None
    assert cmp.row(k, g32[q]).failure(GATE) is not None
    assert cmp.row(k, g32[k]).failure(GATE) is None

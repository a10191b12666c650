"""Per-tensor gradient parity of the native training step (``VAETrainer.step``) and of the drop-in autograd path
against the float64 oracle, and ``VAETrainer.eval_losses`` against the oracle's sampled forward.

The whole-arena gates elsewhere (cosine >= 0.999, norm ratio within 1e-2) cannot see a GroupNorm affine, a conv bias
or most attention and latent-head tensors: each holds < 0.2 % of the squared norm.  Here every one of the 218 tensors
of config A and the 182 of config AR is gated on its own by tests/grad_parity.py (scale alpha, residual rho, the
attention key biases as structural zeros), and the comparator's mutation self-check runs on the real HIP gradients of
every case, so each gate is shown to catch a zeroed, negated, 5 %-scaled, stale-accumulated or swapped tensor there.

Reference: the oracle with the same fp32 weights upcast to float64, the same images and the same injected eps (its
fp32 gradients agree with fp64 to <= 2e-5 on every tensor).  The native step runs with lr = 0, so the captured step
of graph mode (the third call) is compared at the same weights as the eager first step; both are gated.

Knob variants are environment variables that the engine or the trainer reads when it is built (or per call:
PTI_WGRAD_V6): each variant builds a fresh model and trainer.  Knobs cached per process are not toggled here.

Measured on MI355X, worst |alpha - 1| / rho per class (tables per case with -s; the gate: grad_parity.GATE):
    A1 64^2, every variant but bf16 activations   conv_w 4.4e-3 / 3.6e-2   small_w 6.3e-3 / 3.2e-2
                                                  bias 1.2e-2 / 3.6e-2 (exemptions aside)   gn 1.7e-2 / 4.2e-2
                                                  attn 8.9e-3 / 3.6e-2    zeros 4.8e-3
    A3 64^2 (MFMA and direct conv_in)             all classes <= 1.2e-2 / 3.5e-2            zeros 1.1e-2
    A1 256^2                                      all classes <= 1.1e-2 / 2.4e-2            zeros 1.6e-3
    AR 256^2 b1                                   all classes <= 2.1e-3 / 1.8e-2            zeros 9.8e-4
    AR 64^2 b4 + AR term                          all classes <= 8.7e-3 / 3.9e-2            zeros 1.7e-3
    A1 64^2 step 3 (graph and eager)              all classes <= 8.1e-3 / 2.2e-2            zeros 4.3e-3
    drop-in autograd A 64^2 / AR 64^2             as A1 default / <= 1.2e-2 / 2.9e-2
    The eager first step and the replayed graph step measured the same in every case.
    eval_losses: recon, kl and ar within 1.4e-4 relative of fp64 (batch 2 / 4, 3 and 1).
"""
import functools
import os
import warnings

import pytest
import torch

from grad_parity import GATE, Comparator, Gate, failures, report, worst
from oracle.autoencoderkl import CONFIG_A, CONFIG_AR, build_oracle, synthetic_images
from oracle.losses import ar_vae_loss, kl_loss, train_step_losses

pytestmark = pytest.mark.gpu

KNOBS = ("PTI_STEP_GRAPH", "PTI_WGRAD_STREAM", "PTI_WGRAD_BATCH", "PTI_WGRAD_FLUSH_UP", "PTI_WGRAD_V6",
         "PTI_SAVE_ACT_MIN_HW", "PTI_GNBWD_CHAIN", "PTI_FWD_ACT_DTYPE", "PTI_IMG_MFMA")
N_PARAMS = {"A": 218, "AR": 182}
CONFIGS = {"A": CONFIG_A, "A3": dict(CONFIG_A, in_channels=3, out_channels=3), "AR": CONFIG_AR}
_GN_SILU_ALWAYS = str(1 << 30)     # no map is large enough to save SiLU(GN(x)): every ResBlock conv's weight gradient
                                   # takes the GroupNorm+SiLU prologue (the default, 0, saves it at every size)
AR_CONFIG_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config",
                              "ar_vae_dente_kl1e3.json")


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _inputs(cfg, batch, size, seed=42):
    """CPU fp32 images and eps (the recipe of tests/test_gpu_model.py)."""
    x = synthetic_images(batch, cfg["in_channels"], size, seed=seed)
    lat = size // 2 ** (len(cfg["channels"]) - 1)
    eps = torch.randn(batch, cfg["latent_channels"], lat, lat, generator=torch.Generator().manual_seed(seed + 1))
    return x, eps


@functools.lru_cache(maxsize=None)
def _ar_settings():
    """(ARSettings, mapping, delta_global) of the shipped AR-VAE config (gamma 0.5, six attributes, pairwise 'all')."""
    from pti_ldm_vae_amd.trainer import ARSettings
    from pti_ldm_vae_amd.utils import read_config, resolve_ar_settings
    cfg = read_config(AR_CONFIG_FILE)
    ra = cfg["regularized_attributes"]
    enabled, gamma, pairwise, _ = resolve_ar_settings(cfg["autoencoder_train"], ra)
    assert enabled and pairwise == "all"
    st = ARSettings.from_config(ra, gamma, CONFIG_AR["latent_channels"])
    mapping = {k: v for k, v in ra["attribute_latent_mapping"].items() if not k.startswith("_")}
    return st, mapping, ra.get("delta_global", {})


def _attributes(names, batch, seed=43):
    g = torch.Generator().manual_seed(seed + 100)
    return {k: torch.rand(batch, generator=g) for k in names}


def _oracle_f64(cfg, state=None):
    o = build_oracle(cfg, 42)
    if state is not None:
        o.load_state_dict(state)
    return o.double()


def _oracle_grads(cfg, x, eps, state=None, attrs=None):
    """{name: fp64 gradient} of L1 + 1e-3 KL (+ gamma * AR with ``attrs``) at ``state`` (default: the seeded init)."""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    o = _oracle_f64(cfg, state)
    loss, _, _, (_, mu, _) = train_step_losses(o, x.double(), eps.double())
    if attrs is not None:
        st, mapping, dg = _ar_settings()
        ar, _, _, _ = ar_vae_loss(mu, {k: v.double() for k, v in attrs.items()}, mapping, "all", None, dg)
        loss = loss + st.gamma * ar
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in o.named_parameters()}


@pytest.fixture(scope="module")
def reference():
    """-> get(tag, size, batch, ar=False): (images, eps, attributes or None, Comparator) for the seeded weights, cached
    for the module (one fp64 oracle step per configuration and size)."""
    cache = {}

    def get(tag, size, batch, ar=False):
        key = (tag, size, batch, ar)
        if key not in cache:
            cfg = CONFIGS[tag]
            x, eps = _inputs(cfg, batch, size)
            attrs = _attributes(_ar_settings()[0].names, batch) if ar else None
            cache[key] = (x, eps, attrs, Comparator(_oracle_grads(cfg, x, eps, attrs=attrs)))
        return cache[key]
    return get


def _model(cfg, dev):
    from pti_ldm_vae_amd.models import VAEModel
    model = VAEModel.from_config(cfg)
    model.load_state_dict(build_oracle(cfg, 42).state_dict())
    return model.to(dev)


def _hip_grads(ae):
    return {n: ae.grad_view(n).detach().cpu().clone() for n, _ in ae.named_parameters()}


def _gate(cmp, g_h, tag, label, gate=GATE):
    """Every tensor against ``gate``, the structural zeros, and the mutation self-check on these HIP gradients.
    -> worst(rows)."""
    rows = cmp.rows(g_h)
    print("\n" + report(rows, label))
    assert len(rows) == N_PARAMS["AR" if tag == "AR" else "A"]
    assert cmp.zeros == {n for n in cmp.ref if n.endswith(".attn.to_k.bias")} and len(cmp.zeros) == 2, cmp.zeros
    bad = failures(rows, gate)
    assert not bad, f"[{label}] {len(bad)} tensors outside the gate:\n" + "\n".join(bad)
    count, missed = cmp.self_check(g_h, gate)
    assert count > 5 * len(rows) and not missed, (count, missed[:10])
    return worst(rows)


def _native_steps(cfg, dev, x, eps, steps, lr=0.0, ar=None, attrs=None):
    """``steps`` calls of VAETrainer.step on the same batch -> ([{name: gradient} after each call], trainer)."""
    from pti_ldm_vae_amd.trainer import VAETrainer
    model = _model(cfg, dev)
    tr = VAETrainer(model, lr=lr, ar=ar)
    xd, epsd = x.to(dev), eps.to(dev)
    ad = None if attrs is None else {k: v.to(dev) for k, v in attrs.items()}
    grads = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(steps):
            tr.step(xd, epsd, attributes=ad)
            grads.append(_hip_grads(model.autoencoder))
    torch.cuda.synchronize()
    assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
    return grads, tr


# name -> environment of one A1 variant (defaults first)
A1_VARIANTS = {
    "default": {},
    "step_graph_0": {"PTI_STEP_GRAPH": "0"},
    "wgrad_stream_0": {"PTI_WGRAD_STREAM": "0"},
    "wgrad_batch_1": {"PTI_WGRAD_BATCH": "1"},
    "flush_up_0": {"PTI_WGRAD_FLUSH_UP": "0"},
    "flush_up_2": {"PTI_WGRAD_FLUSH_UP": "2"},
    "v6_0": {"PTI_WGRAD_V6": "0"},
    "v6_1": {"PTI_WGRAD_V6": "1"},
    "v6_2": {"PTI_WGRAD_V6": "2"},
    "gn_silu_prologue": {"PTI_SAVE_ACT_MIN_HW": _GN_SILU_ALWAYS},
    "gnbwd_chain": {"PTI_GNBWD_CHAIN": "1"},
    "act_bf16": {"PTI_FWD_ACT_DTYPE": "bf16"},
}
# PTI_FWD_ACT_DTYPE=bf16 stores the forward activations with 8x fp16's rounding step, and every gradient carries it:
# measured |alpha - 1| / rho per class conv_w 2.2e-2 / 9.9e-2, small_w 1.3e-2 / 9.5e-2, bias 1.1e-1 / 9.7e-2 (the
# one-element decoder.blocks.16.conv.bias, the L1 sign count of GATE's exemption), gn 6.4e-2 / 1.35e-1, attn 4.1e-2 /
# 9.6e-2.  That is the default gate's worst case times the rounding ratio, so this variant gets its own A as well as R
# (R stays far below the 0.47 a swap produces; the scale mutations grow to 2.5 A)
BF16_GATE = Gate(bounds={"conv_w": (4e-2, 0.15), "small_w": (4e-2, 0.15), "bias": (0.15, 0.15), "gn": (0.1, 0.2),
                         "attn": (0.08, 0.15)},
                 tau=GATE.tau, exempt=GATE.exempt)
VARIANT_GATE = {"act_bf16": BF16_GATE}


# (tag, size, batch, variant environment); the A1 variants are added below
CASES = {f"A1-64-{k}": ("A", 64, 2, v) for k, v in A1_VARIANTS.items()}
CASES.update({
    "A3-64-default": ("A3", 64, 2, {}),
    "A3-64-img_mfma_0": ("A3", 64, 2, {"PTI_IMG_MFMA": "0"}),
    "A1-256-default": ("A", 256, 2, {}),        # the map-size rules: V6 mode 3 up to 128^2 maps, flush-up at larger maps
    "AR-256-default": ("AR", 256, 1, {}),       # 256-channel convs at 64^2, attention at L = 4096
})


@pytest.mark.parametrize("case", list(CASES))
def test_native_step_per_tensor_vs_fp64(dev, monkeypatch, reference, case):
    """One native step per tensor against fp64: the eager first call and (graph mode) the captured third call, lr = 0."""
    tag, size, batch, env = CASES[case]
    variant = case.split("-", 2)[2]
    _set_env(monkeypatch, env)
    x, eps, _, cmp = reference(tag, size, batch)
    graph = env.get("PTI_STEP_GRAPH") != "0"
    grads, tr = _native_steps(CONFIGS[tag], dev, x, eps, 3 if graph else 1)
    assert len(tr._graphs) == (1 if graph else 0)
    gate = VARIANT_GATE.get(variant, GATE)
    _gate(cmp, grads[0], tag, f"{case} eager", gate)
    if graph:
        _gate(cmp, grads[2], tag, f"{case} graph", gate)


def test_native_step_with_ar_term_per_tensor_vs_fp64(dev, monkeypatch, reference):
    """Config AR + the AR-VAE term (the shipped config: gamma 0.5, six attributes, pairwise 'all') at 64x64, batch 4:
    the oracle adds gamma * AR(mu) in fp64.  The step with an AR term is always eager."""
    _set_env(monkeypatch, {})
    x, eps, attrs, cmp = reference("AR", 64, 4, ar=True)
    grads, tr = _native_steps(CONFIG_AR, dev, x, eps, 1, ar=_ar_settings()[0], attrs=attrs)
    _gate(cmp, grads[0], "AR", "AR-64-b4 + AR term")


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_third_step_per_tensor_vs_fp64(dev, monkeypatch, mode):
    """Config A at 64x64, batch 2, lr = 2e-4, three steps on three batches: the third step's gradients against the fp64
    oracle at the weights the trainer holds before that step.  Catches what the first step cannot show: stale packed
    weights, accumulators that are not cleared, side-stream state left over from the previous step.  In graph mode the
    third call is the one that captures and replays the step."""
    _set_env(monkeypatch, {"PTI_STEP_GRAPH": "1" if mode == "graph" else "0"})
    from pti_ldm_vae_amd.trainer import VAETrainer
    model = _model(CONFIG_A, dev)
    ae = model.autoencoder
    tr = VAETrainer(model, lr=2e-4)
    batches = [_inputs(CONFIG_A, 2, 64, seed=42 + 7 * i) for i in range(3)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for x, eps in batches[:2]:
            tr.step(x.to(dev), eps.to(dev))
        torch.cuda.synchronize()
        state = {n: p.detach().cpu().clone() for n, p in ae.named_parameters()}
        x, eps = batches[2]
        tr.step(x.to(dev), eps.to(dev))
        torch.cuda.synchronize()
    assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
    assert len(tr._graphs) == (1 if mode == "graph" else 0)
    init = build_oracle(CONFIG_A, 42).state_dict()
    assert max((state[n] - init[n]).abs().max().item() for n in state) > 1e-4     # the weights did move
    cmp = Comparator(_oracle_grads(CONFIG_A, x, eps, state=state))
    _gate(cmp, _hip_grads(ae), "A", f"A1-64 step 3 ({mode})")


@pytest.mark.parametrize("tag,batch", [("A", 2), ("AR", 1)])
def test_dropin_autograd_per_tensor_vs_fp64(dev, monkeypatch, reference, tag, batch):
    """The drop-in path (``autoencoder.encode`` / ``decode`` + ``loss.backward()``) at 64x64, every tensor gated: the
    tensors under 1024 elements that test_training_step_parity leaves out included."""
    from pti_ldm_vae_amd.models import compute_kl_loss
    _set_env(monkeypatch, {})
    x, eps, _, cmp = reference(tag, 64, batch)
    model = _model(CONFIGS[tag], dev)
    ae = model.autoencoder
    xd = x.to(dev)
    mu, sig = ae.encode(xd)
    rec = ae.decode(mu + eps.to(dev) * sig)
    (torch.nn.functional.l1_loss(rec, xd) + 1e-3 * compute_kl_loss(mu, sig)).backward()
    torch.cuda.synchronize()
    g = {n: p.grad.detach().cpu().clone() for n, p in ae.named_parameters()}
    _gate(cmp, g, tag, f"{tag}-64-b{batch} drop-in autograd")


def _eval_vs_oracle(tr, cfg, x, attrs, label):
    """``tr.eval_losses`` on ``x`` against the fp64 oracle's sampled forward at the trainer's current weights, with the
    eps the call drew from ``tr.gen`` (replayed from a clone of its state)."""
    dev = tr.net.param_arena.device
    state = tr.gen.get_state().clone()
    ad = None if attrs is None else {k: v.to(dev) for k, v in attrs.items()}
    res, _ = tr.eval_losses(x.to(dev), attributes=ad)
    torch.cuda.synchronize()
    g = torch.Generator(device=dev)
    g.set_state(state)
    lat = x.shape[2] // 2 ** (len(cfg["channels"]) - 1)
    eps = torch.randn((x.shape[0], cfg["latent_channels"], lat, lat), generator=g, device=dev).cpu()
    params = {n: p.detach().cpu().clone() for n, p in tr.net.named_parameters()}
    with torch.no_grad():
        o = _oracle_f64(cfg, params)
        rec, mu, sig = o(x.double(), eps.double())
        want = {"recon": torch.nn.functional.l1_loss(rec, x.double()).item(), "kl": kl_loss(mu, sig).item()}
        if attrs is not None:
            _, mapping, dg = _ar_settings()
            want["ar"] = ar_vae_loss(mu, {k: v.double() for k, v in attrs.items()}, mapping, "all", None, dg)[0].item()
    got = {k: res[k].item() for k in want}
    # (batch 1 has no attribute pairs: the AR term is exactly 0 on both sides)
    rel = {k: abs(got[k] - want[k]) / (abs(want[k]) or 1.0) for k in want}
    print(f"[eval {label}] " + "  ".join(f"{k} {got[k]:.6f} vs {want[k]:.6f} (rel {rel[k]:.1e})" for k in want))
    return rel


@pytest.mark.parametrize("tag", ["A", "AR"])
def test_eval_losses_vs_fp64(dev, monkeypatch, tag):
    """``VAETrainer.eval_losses`` (the validation forward that picks the best checkpoint) against the fp64 oracle's
    sampled forward: after one native step with lr > 0 (so the inference graphs and repacked weights are the updated
    ones) on the step's batch, then on a ragged batch of 3 and one of 1 (new inference-graph shapes).  recon, kl and
    (AR config, with attributes) the AR term within 1e-3 relative."""
    from pti_ldm_vae_amd.trainer import VAETrainer
    _set_env(monkeypatch, {})
    cfg = CONFIGS[tag]
    ar = _ar_settings()[0] if tag == "AR" else None
    batch = 4 if tag == "AR" else 2
    model = _model(cfg, dev)
    tr = VAETrainer(model, lr=2e-4, ar=ar)
    x, eps = _inputs(cfg, batch, 64)
    attrs = _attributes(ar.names, batch) if ar else None
    tr.step(x.to(dev), eps.to(dev), attributes=None if attrs is None else {k: v.to(dev) for k, v in attrs.items()})
    torch.cuda.synchronize()
    init = build_oracle(cfg, 42).state_dict()
    assert any(not torch.equal(p.detach().cpu(), init[n]) for n, p in model.autoencoder.named_parameters())
    for b in (batch, 3, 1):
        xb, _ = _inputs(cfg, b, 64, seed=60 + b)
        ab = None if ar is None else _attributes(ar.names, b, seed=60 + b)
        rel = _eval_vs_oracle(tr, cfg, xb, ab, f"{tag} b{b}")
        for k, v in rel.items():
            assert v <= 1e-3, (tag, b, k, v)

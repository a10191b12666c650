"""Torch restatement of the regression head's evaluation path (test helper, like ``tests/eval_metrics_oracle.py``): the
checker of ``pti_mlp_head_fwd`` / ``pti_regression_metrics``.

``head_forward`` / ``row_loss`` / ``fold_metrics`` follow the reference's ``LatentRegressor`` in eval mode
(``src/pti_ldm_vae/models/regression_head.py:30-78``), ``TargetNormalizer`` and ``validate_one_epoch``
(``src/pti_ldm_vae/utils/regression_utils.py:239-265,350-388``) and ``compute_regression_metrics``
(``src/pti_ldm_vae/utils/metrics.py:6-37``) with a ``dtype`` argument.  In fp32 the restatement is pinned to recorded
outputs of those reference modules by ``tests/test_regression_eval_cpu.py`` (``tests/golden/regression_eval_golden.npz``,
written by ``python tests/regression_head_oracle.py <reference checkout>``, see ``__main__`` below).

Case inputs come from an integer hash (``uniform``), not from a random generator: they are the same bits on every
machine and torch version, so the fixture holds only outputs.

The gate (``Gate``): for each output (``pred``, ``rowloss``, ``fold``) ``D_ref`` is the largest deviation of the fp32 CPU
restatement from the fp64 one over the case list, relative to ``max |fp64 output|`` of the case; a result passes when its
deviation from fp64 is at most ``8 * D_ref``.  The yardstick is the fp32 arithmetic of the reference's modules, never the
kernel.  ``MUTATIONS`` are nine plausible implementation mistakes applied to the fp64 restatement; the gate has to reject
every one of them on every case it applies to (``mutation_survivors``).
"""
from __future__ import annotations

import dataclasses
import math

import torch
import torch.nn.functional as F

OUTPUTS = ("pred", "rowloss", "fold")
GATE_FACTOR = 8.0
ACTS = ("relu", "gelu", "leaky_relu", "elu")


# ---- deterministic inputs ---------------------------------------------------------------------------------------------
def uniform(shape, seed: int, lo: float = -1.0, hi: float = 1.0) -> torch.Tensor:
    """fp32 tensor of ``shape`` with values in [lo, hi): a 32-bit integer hash of (element index, seed), exact integer
    arithmetic in int64, so the bits do not depend on the machine or the torch version."""
    n = int(math.prod(shape))
    m = 0xFFFFFFFF
    x = (torch.arange(n, dtype=torch.int64) + (int(seed) * 0x9E3779B1 & m) + 1) & m
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & m
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & m
    x = x ^ (x >> 16)
    u = (x >> 8).to(torch.float64) / float(1 << 24)          # 24 bits: exact in fp32
    return (lo + (hi - lo) * u).to(torch.float32).reshape(shape)


@dataclasses.dataclass
class Case:
    """One evaluation problem.  ``mu`` is the latent as the encoder returns it, NCHW; ``x = flatten(mu, 1)``."""
    name: str
    mu: torch.Tensor                    # [n, c, h, w] fp32
    weights: list                       # nn.Linear layout [out, in]
    biases: list
    act: str
    mean: torch.Tensor | None           # [T] (std already free of zeros)
    std: torch.Tensor | None
    targets: torch.Tensor | None        # [n, T] raw scale
    loss: str                           # "mse" | "smooth_l1"
    batch: int

    @property
    def x(self) -> torch.Tensor:
        return torch.flatten(self.mu, 1)

    @property
    def dims(self) -> list:
        return [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]


def make_case(name, n, chw, hidden, t, act="relu", norm=True, targets=True, loss="mse", batch=8, seed=0) -> Case:
    c, h, w = chw
    d = c * h * w
    dims = [d, *hidden, t]
    mu = uniform((n, c, h, w), 11 * seed + 1, -1.7, 1.7)                  # about unit variance, as z_mu
    weights, biases = [], []
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        s = 3.0 / math.sqrt(a)                                            # pre-activations of variance ~3: both signs, |.| > 1 common
        weights.append(uniform((b, a), 11 * seed + 2 + 2 * l, -s, s))
        biases.append(uniform((b,), 11 * seed + 3 + 2 * l, -0.5, 0.5))
    mean = std = tg = None
    if norm:
        mean = 20.0 + 3.0 * torch.arange(t, dtype=torch.float32)
        std = 5.0 - 4.0 * torch.arange(t, dtype=torch.float32) / max(t, 1)
    if targets:
        z = uniform((n, t), 11 * seed + 9, -2.5, 2.5)                      # normalised-scale targets: errors on both sides of 1
        tg = z * std + mean if norm else z
    return Case(name, mu, weights, biases, act, mean, std, tg, loss, batch)


# ---- the restatement --------------------------------------------------------------------------------------------------
def activation(v: torch.Tensor, act: str) -> torch.Tensor:
    if act == "relu":
        return F.relu(v)
    if act == "gelu":
        return F.gelu(v)                      # nn.GELU(): the exact erf form
    if act == "leaky_relu":
        return F.leaky_relu(v, 0.01)
    if act == "elu":
        return F.elu(v, 1.0)
    raise ValueError(act)


def head_forward(x, weights, biases, act, *, dtype=torch.float64, drop_last_bias=False, keep_cols=None):
    """``LatentRegressor.forward`` in eval mode: Linear, activation, ..., Linear -> [n, T] (normalised scale).
    ``drop_last_bias`` / ``keep_cols`` (first-layer columns beyond it are ignored) exist for the mutation check only."""
    v = x.to(dtype)
    last = len(weights) - 1
    for l, (w, b) in enumerate(zip(weights, biases)):
        w, b = w.to(dtype), b.to(dtype)
        if l == 0 and keep_cols is not None:
            v, w = v[:, :keep_cols], w[:, :keep_cols]
        v = v @ w.t() if (l == last and drop_last_bias) else F.linear(v, w, b)
        if l != last:
            v = activation(v, act)
    return v


def loss_terms(out, want, loss: str, *, huber_on_square=False):
    df = out - want
    if loss == "mse":
        return df * df
    a = df * df if huber_on_square else df.abs()
    return torch.where(a < 1.0, 0.5 * df * df, a - 0.5)


def row_loss(out, targets, mean, std, loss, *, dtype=torch.float64, denormalised=False, huber_on_square=False):
    """[n]: sum over the targets of the loss terms on the NORMALISED scale (``validate_one_epoch``: ``loss_fn(out,
    normalizer.normalize(targets))`` is their mean over the batch's elements)."""
    out, tg = out.to(dtype), targets.to(dtype)
    if mean is None:
        return loss_terms(out, tg, loss, huber_on_square=huber_on_square).sum(dim=1)
    mean, std = mean.to(dtype), std.to(dtype)
    if denormalised:
        return loss_terms(out * std + mean, tg, loss, huber_on_square=huber_on_square).sum(dim=1)
    return loss_terms(out, (tg - mean) / std, loss, huber_on_square=huber_on_square).sum(dim=1)


def fold_metrics(pred, targets, rowloss, batch, *, dtype=torch.float64, global_mean=False):
    """[2T + 3]: val_loss (mean over the chunks of ``batch`` rows of the chunk's mean loss), MAE per target, MSE per target,
    mean MAE, mean MSE (``compute_regression_metrics``)."""
    pred, targets, rowloss = pred.to(dtype), targets.to(dtype), rowloss.to(dtype)
    n, t = pred.shape
    if global_mean:
        val = rowloss.sum() / (n * t)
    else:
        means = [rowloss[i:i + batch].sum() / (min(batch, n - i) * t) for i in range(0, n, batch)]
        val = torch.stack(means).sum() / len(means)
    err = pred - targets
    mae, mse = err.abs().mean(dim=0), (err * err).mean(dim=0)
    return torch.cat([val.reshape(1), mae, mse, mae.mean().reshape(1), mse.mean().reshape(1)])


def evaluate(case: Case, *, dtype=torch.float64, mutation: str | None = None) -> dict:
    """-> {"pred" [n, T], and with targets "rowloss" [n], "fold" [2T + 3]} in ``dtype``; ``mutation``: a key of MUTATIONS."""
    m = mutation
    x = torch.flatten(case.mu.permute(0, 2, 3, 1), 1) if m == "nhwc flatten" else case.x
    d = x.shape[1]
    keep = {"columns past the last whole slab dropped": (d // 512) * 512,
            "columns past the last multiple of 4 dropped": (d // 4) * 4}.get(m)
    out = head_forward(x, case.weights, case.biases, "relu" if m == "relu for the activation" else case.act, dtype=dtype,
                       drop_last_bias=m == "last bias omitted", keep_cols=keep)
    mean, std = case.mean, case.std
    if m == "mean and std swapped" and mean is not None:
        mean, std = std, mean
    res = {"pred": out if mean is None else out * std.to(dtype) + mean.to(dtype)}
    if case.targets is not None:
        res["rowloss"] = row_loss(out, case.targets, mean, std, case.loss, dtype=dtype,
                                  denormalised=m == "loss on the de-normalised scale",
                                  huber_on_square=m == "huber threshold on the squared error")
        res["fold"] = fold_metrics(res["pred"], case.targets, res["rowloss"], case.batch, dtype=dtype,
                                   global_mean=m == "val_loss as the global mean")
    return res


# mistake -> whether it can show on a case at all (the gate must reject it on EVERY such case of the mutation list)
MUTATIONS = {
    "nhwc flatten": lambda c: c.mu.shape[1] > 1 and c.mu.shape[2] * c.mu.shape[3] > 1,
    "columns past the last whole slab dropped": lambda c: c.x.shape[1] > 512 and c.x.shape[1] % 512 != 0,
    "columns past the last multiple of 4 dropped": lambda c: c.x.shape[1] > 4 and c.x.shape[1] % 4 != 0,
    "last bias omitted": lambda c: True,
    "relu for the activation": lambda c: c.act != "relu" and len(c.weights) > 1,
    "mean and std swapped": lambda c: c.mean is not None,
    "loss on the de-normalised scale": lambda c: c.mean is not None and c.targets is not None,
    "val_loss as the global mean": lambda c: c.targets is not None and c.x.shape[0] % c.batch != 0 and c.x.shape[0] > c.batch,
    # the smooth-L1 formula fed the squared error: same below |e| = 1, e^2 - 0.5 instead of |e| - 0.5 above
    "huber threshold on the squared error": lambda c: c.targets is not None and c.loss == "smooth_l1",
}


def deviation(got: dict, ref64: dict) -> dict:
    """Per output: max |got - fp64| / max |fp64| over the case's elements."""
    out = {}
    for k in OUTPUTS:
        if k in ref64:
            r = ref64[k].double()
            out[k] = float((got[k].detach().cpu().double() - r).abs().max() / r.abs().max().clamp_min(1e-300))
    return out


@dataclasses.dataclass
class Gate:
    d_ref: dict

    @property
    def bound(self) -> dict:
        return {k: GATE_FACTOR * v for k, v in self.d_ref.items()}

    def violations(self, dev: dict) -> list:
        return [f"{k}: {dev[k]:.3e} > {self.bound[k]:.3e}" for k in dev if not dev[k] <= self.bound[k]]


def reference_deviation(case_list):
    """-> (Gate, {case name: fp64 outputs}): D_ref[k] = max over the cases of the fp32 restatement's deviation from fp64."""
    d_ref = {k: 0.0 for k in OUTPUTS}
    ref = {}
    for c in case_list:
        r64 = evaluate(c, dtype=torch.float64)
        for k, v in deviation(evaluate(c, dtype=torch.float32), r64).items():
            d_ref[k] = max(d_ref[k], v)
        ref[c.name] = r64
    return Gate(d_ref), ref


# ---- the CPU case lists -------------------------------------------------------------------------------------------------
def golden_cases():
    """The small cases whose reference outputs are recorded (the largest has d = 513 = 3 x 9 x 19)."""
    return [
        make_case("d513 [7,5] T3 gelu huber", 11, (3, 9, 19), [7, 5], 3, act="gelu", loss="smooth_l1", batch=4, seed=1),
        make_case("d48 [16] T6 relu mse", 10, (3, 4, 4), [16], 6, act="relu", loss="mse", batch=8, seed=2),
        make_case("d20 [] T2 mse no-norm", 5, (5, 2, 2), [], 2, norm=False, loss="mse", batch=2, seed=3),
        make_case("d36 [8] T4 elu huber", 9, (4, 3, 3), [8], 4, act="elu", loss="smooth_l1", batch=4, seed=4),
        make_case("d36 [8,8] T1 leaky mse", 7, (4, 3, 3), [8, 8], 1, act="leaky_relu", loss="mse", batch=3, seed=5),
    ]


def mutation_cases():
    """Cases on which every mutation applies to at least one: non-relu activations, d = 513 and 1027 (= 13 x 79 x 1),
    a normaliser, both losses, a short last batch."""
    return [
        make_case("m513 gelu huber", 11, (3, 9, 19), [7, 5], 3, act="gelu", loss="smooth_l1", batch=4, seed=1),
        make_case("m1027 elu mse", 9, (13, 79, 1), [32], 6, act="elu", loss="mse", batch=8, seed=6),
        make_case("m1027 leaky huber", 17, (13, 79, 1), [16, 8], 2, act="leaky_relu", loss="smooth_l1", batch=8, seed=7),
    ]


def mutation_survivors(gate: Gate, case_list=None, base_of=None):
    """Mutations the gate does NOT reject on some case they apply to, plus mutations that apply to no case.
    ``base_of(case) -> outputs``: what the mutated fp64 values are gated against (default: the clean fp64 restatement)."""
    survivors, applied = [], set()
    for c in (case_list if case_list is not None else mutation_cases()):
        base = base_of(c) if base_of is not None else evaluate(c)
        for name, applies in MUTATIONS.items():
            if not applies(c):
                continue
            applied.add(name)
            if not gate.violations(deviation(base, evaluate(c, mutation=name))):
                survivors.append(f"{name} @ {c.name}")
    return survivors + [f"{name}: applies to no case" for name in MUTATIONS if name not in applied]


# ---- recording recipe: python tests/regression_head_oracle.py <reference checkout> [out.npz] -------------------------------
def _load_reference(ref_root: str):
    """The reference's own modules, loaded by path.  ``pti_ldm_vae.models.autoencoder`` imports MONAI and
    ``pti_ldm_vae.utils.vae_loader`` imports it in turn; where those packages are missing the two are replaced by
    placeholders (neither is used by the code recorded here).  -> (modules, list of the placeholders used)."""
    import importlib.util
    import os
    import sys
    import types
    src = os.path.join(ref_root, "src", "pti_ldm_vae")
    stubbed = []

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(src, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    for pkg in ("pti_ldm_vae", "pti_ldm_vae.models", "pti_ldm_vae.utils"):
        sys.modules[pkg] = types.ModuleType(pkg)
        sys.modules[pkg].__path__ = []
    try:
        load("pti_ldm_vae.models.autoencoder", "models/autoencoder.py")
    except ImportError:
        stub = types.ModuleType("pti_ldm_vae.models.autoencoder")
        stub.VAEModel = torch.nn.Module
        sys.modules["pti_ldm_vae.models.autoencoder"] = stub
        stubbed.append("pti_ldm_vae.models.autoencoder")
    head = load("pti_ldm_vae.models.regression_head", "models/regression_head.py")
    sys.modules["pti_ldm_vae.models"].LatentRegressor = head.LatentRegressor
    sys.modules["pti_ldm_vae.models"].VAELatentRegressor = head.VAELatentRegressor
    load("pti_ldm_vae.utils.metrics", "utils/metrics.py")
    try:
        load("pti_ldm_vae.utils.vae_loader", "utils/vae_loader.py")
    except ImportError:
        stub = types.ModuleType("pti_ldm_vae.utils.vae_loader")
        stub.load_vae_config = stub.load_vae_model = None
        sys.modules["pti_ldm_vae.utils.vae_loader"] = stub
        stubbed.append("pti_ldm_vae.utils.vae_loader")
    utils = load("pti_ldm_vae.utils.regression_utils", "utils/regression_utils.py")
    return head, utils, stubbed


def record(ref_root: str, out_path: str) -> None:
    """Run the reference's ``LatentRegressor``, ``TargetNormalizer``, ``build_loss_fn``, ``validate_one_epoch`` and
    ``compute_regression_metrics`` (fp32, CPU) on ``golden_cases()`` and store their outputs."""
    import numpy as np
    head, utils, stubbed = _load_reference(ref_root)
    blob = {"stubbed": np.array(stubbed), "recorded_from": np.array(
        ["models/regression_head.py:LatentRegressor", "utils/regression_utils.py:TargetNormalizer,build_loss_fn,"
         "validate_one_epoch", "utils/metrics.py:compute_regression_metrics"])}
    for i, c in enumerate(golden_cases()):
        dims = c.dims
        model = head.LatentRegressor(dims[0], dims[1:-1], dims[-1], dropout=0.25, activation=c.act).eval()
        linears = [m for m in model.mlp if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for m, w, b in zip(linears, c.weights, c.biases):
                m.weight.copy_(w)
                m.bias.copy_(b)
            out = model(c.x)
        norm = utils.TargetNormalizer(c.mean, c.std) if c.mean is not None else None
        names = [f"t{k}" for k in range(dims[-1])]
        loader = [(c.x[j:j + c.batch], c.targets[j:j + c.batch]) for j in range(0, c.x.shape[0], c.batch)]
        val, metrics = utils.validate_one_epoch(model, loader, utils.build_loss_fn(c.loss), torch.device("cpu"), names, norm)
        blob[f"out{i}"] = out.numpy()
        blob[f"pred{i}"] = (norm.denormalize(out) if norm is not None else out).numpy()
        blob[f"fold{i}"] = np.array([val] + [metrics[f"mae_{k}"] for k in names] + [metrics[f"mse_{k}"] for k in names]
                                    + [metrics["mae"], metrics["mse"]], dtype=np.float64)
        blob[f"name{i}"] = np.array(c.name)
    np.savez_compressed(out_path, **blob)
    print(f"wrote {out_path}: {len(golden_cases())} cases; placeholders for {stubbed or 'nothing'}")


if __name__ == "__main__":
    import os
    import sys
    if len(sys.argv) < 2:
        raise SystemExit("usage: python tests/regression_head_oracle.py <reference checkout> [out.npz]")
    default = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regression_eval_golden.npz")
    record(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else default)

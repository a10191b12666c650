"""Torch restatement of the four evaluation metrics (test helper, like ``tests/grad_parity.py``): the checker of
``pti_image_metrics``.

``metrics(pred, target, dtype=...)`` follows the reference's ``compute_psnr`` / ``compute_ssim``
(``src/pti_ldm_vae/utils/eval_metrics.py:6-64``) and the two plain means of ``vae_scripts/evaluate_vae.py:97-98`` with a
``dtype`` argument.  The reference function itself cannot run in float64 (its window tensor is always fp32 and
``conv2d`` raises on the mixed types) nor for ``C > 1`` (its ``[1, 1, 11, 11]`` window does not fit ``groups = C``); here
the window is repeated per channel (depthwise), which is how this project defines ``C > 1``.  In fp32 the restatement is
pinned to the reference's recorded outputs by ``tests/test_eval_metrics_cpu.py`` (``tests/golden/eval_metrics_golden.npz``).

The gate (``Gate``): for each metric, ``D_ref`` is the largest deviation of the fp32 restatement from the fp64 one over
the whole case list -- absolute for SSIM and PSNR (dB), relative for MSE and MAE -- and a result passes when its
deviation from fp64 is at most ``8 * D_ref``.  The yardstick is the reference's own fp32 arithmetic, never the code
under test.  ``MUTATIONS`` are five plausible implementation mistakes applied to the fp64 restatement; the gate has to
reject every one of them (``mutation_survivors``).
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn.functional as F

METRICS = ("mse", "mae", "psnr", "ssim")
RELATIVE = {"mse": True, "mae": True, "psnr": False, "ssim": False}
GATE_FACTOR = 8.0

# (n, c, h, w) of the kernel cases
SHAPES = [(32, 1, 256, 256), (8, 1, 256, 256), (3, 1, 64, 64), (2, 1, 100, 76), (2, 1, 9, 13), (1, 1, 1, 1), (2, 3, 64, 48),
          (1, 8, 33, 31)]
NOISES = [0.0, 0.01, 0.1, 0.5]
CLAMPS = [(0.0, 1.0), None]


def window(dtype, size=11, sigma=1.5):
    """1-D taps: exp(-(i - size//2)^2 / (2 sigma^2)), normalised to sum 1, in ``dtype``."""
    coords = torch.arange(size) - size // 2
    g = torch.exp((-(coords ** 2) / (2 * sigma * sigma)).to(dtype))
    return g / g.sum()


def ssim(pred, target, *, dtype=torch.float64, data_range=1.0, k1=0.01, k2=0.03, size=11, sigma=1.5, pad_mode="zeros",
         renormalise=False):
    """SSIM per sample, [B].  ``size`` / ``sigma`` / ``pad_mode`` / ``renormalise`` exist for the mutation check only."""
    x, y = pred.to(dtype), target.to(dtype)
    c = x.shape[1]
    g = window(dtype, size, sigma)
    k2d = (g[:, None] @ g[None, :])[None, None].repeat(c, 1, 1, 1)
    pad = size // 2

    def filt(t):
        if pad_mode == "reflect":
            # reflect needs pad < size of the map; fall back to zeros on smaller maps (mutations run on maps >= 64 only)
            if min(t.shape[-2:]) > pad:
                return F.conv2d(F.pad(t, (pad, pad, pad, pad), mode="reflect"), k2d, groups=c)
        out = F.conv2d(t, k2d, padding=pad, groups=c)
        if renormalise:
            out = out / F.conv2d(torch.ones_like(t), k2d, padding=pad, groups=c)
        return out

    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mu_x, mu_y = filt(x), filt(y)
    mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
    s_xx, s_yy, s_xy = filt(x * x) - mu_xx, filt(y * y) - mu_yy, filt(x * y) - mu_xy
    m = ((2 * mu_xy + c1) * (2 * s_xy + c2)) / ((mu_xx + mu_yy + c1) * (s_xx + s_yy + c2))
    return m.mean(dim=(1, 2, 3))


def psnr(pred, target, *, dtype=torch.float64, data_range=1.0):
    x, y = pred.to(dtype), target.to(dtype)
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3)).clamp(min=1e-12)
    return 10 * torch.log10(torch.tensor(data_range, dtype=dtype) ** 2 / mse)


def metrics(pred, target, *, dtype=torch.float64, clamp=None, data_range=1.0, k1=0.01, k2=0.03, **ssim_variant):
    """-> {"mse", "mae", "psnr", "ssim"}: [B] tensors of ``dtype`` (CPU)."""
    x, y = pred.detach().cpu().to(dtype), target.detach().cpu().to(dtype)
    if clamp is not None:
        x, y = x.clamp(clamp[0], clamp[1]), y.clamp(clamp[0], clamp[1])
    return {"mse": ((x - y) ** 2).mean(dim=(1, 2, 3)), "mae": (x - y).abs().mean(dim=(1, 2, 3)),
            "psnr": psnr(x, y, dtype=dtype, data_range=data_range),
            "ssim": ssim(x, y, dtype=dtype, data_range=data_range, k1=k1, k2=k2, **ssim_variant)}


def make_pair(shape, noise, seed):
    """(pred, target) fp32 with the data's character: a textured elliptical foreground on an exactly-zero background
    (what LocalNormalizeByMask leaves), target values mostly inside [0, 1] with some above 1 and below 0 inside the mask;
    pred = target + noise inside the mask + a faint 0.002 noise everywhere (so the background is not bit-equal either,
    except at noise 0 where pred == target exactly)."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    planes = []
    for i in range(n * c):
        r = 0.5 + 0.4 * torch.rand((), generator=g)
        mask = ((xx / r) ** 2 + (yy / (0.7 * r)) ** 2 < 1).float()
        if h * w < 16:
            mask = torch.ones(h, w)
        tex = 0.55 + 0.4 * torch.sin(8 * xx * (i % 5 + 1)) * torch.cos(6 * yy) + 0.15 * torch.randn(h, w, generator=g)
        planes.append(mask * tex)          # range about [-0.3, 1.4]: values outside [0, 1] are present
    t = torch.stack(planes).view(n, c, h, w)
    if noise == 0.0:
        return t.clone(), t
    p = t + noise * torch.randn(t.shape, generator=g) * (t != 0) + 0.002 * torch.randn(t.shape, generator=g)
    return p, t


def cases(shapes=None):
    """Every (shape, noise, clamp) case: yields (case id, pred, target, clamp)."""
    for si, shape in enumerate(shapes or SHAPES):
        for ni, noise in enumerate(NOISES):
            p, t = make_pair(shape, noise, seed=1000 * si + ni)
            for clamp in CLAMPS:
                yield f"{'x'.join(map(str, shape))}/noise{noise}/{'clamp01' if clamp else 'noclamp'}", p, t, clamp


def deviation(got: dict, ref64: dict) -> dict:
    """Largest deviation over the samples per metric: relative for mse / mae (0 where both are exactly 0), absolute else."""
    out = {}
    for k in METRICS:
        g, r = got[k].detach().cpu().double(), ref64[k].double()
        d = (g - r).abs()
        if RELATIVE[k]:
            d = torch.where(r.abs() > 0, d / r.abs().clamp_min(1e-300), d)
        out[k] = float(d.max())
    return out


@dataclasses.dataclass
class Gate:
    """``bound[k] = GATE_FACTOR * D_ref[k]``; ``D_ref`` from ``reference_deviation`` over the case list."""
    d_ref: dict

    @property
    def bound(self) -> dict:
        return {k: GATE_FACTOR * v for k, v in self.d_ref.items()}

    def violations(self, dev: dict) -> list[str]:
        return [f"{k}: {dev[k]:.3e} > {self.bound[k]:.3e}" for k in METRICS if not dev[k] <= self.bound[k]]


def reference_deviation(case_list=None):
    """-> (Gate, {case id: fp64 metrics}): D_ref[k] = max over all cases of |fp32 restatement - fp64 restatement|."""
    d_ref = {k: 0.0 for k in METRICS}
    ref = {}
    for cid, p, t, clamp in (case_list if case_list is not None else cases()):
        r64 = metrics(p, t, dtype=torch.float64, clamp=clamp)
        d = deviation(metrics(p, t, dtype=torch.float32, clamp=clamp), r64)
        for k in METRICS:
            d_ref[k] = max(d_ref[k], d[k])
        ref[cid] = r64
    return Gate(d_ref), ref


# the five mistakes of the mutation check: name -> keyword arguments of ``metrics`` that produce it
MUTATIONS = {
    "window of 9 taps": dict(size=9),
    "sigma 1.4": dict(sigma=1.4),
    "reflect padding": dict(pad_mode="reflect"),
    "border renormalisation": dict(renormalise=True),
    "k2 = 0.02": dict(k2=0.02),
}


def mutation_cases():
    """The cases the mutation check runs on: H, W >= 64, noise >= 0.01, clamp on (the evaluation's setting)."""
    for si, shape in enumerate(SHAPES):
        if shape[2] < 64 or shape[3] < 64:
            continue
        for ni, noise in enumerate(NOISES):
            if noise >= 0.01:
                p, t = make_pair(shape, noise, seed=1000 * si + ni)
                yield f"{'x'.join(map(str, shape))}/noise{noise}", p, t, (0.0, 1.0)


def mutation_survivors(gate: Gate, base_of=None):
    """Apply every mutation to the fp64 restatement on every mutation case and return those the gate does NOT reject
    on some case.  ``base_of(case id, pred, target, clamp) -> metrics dict``: the result the mutated fp64 values are gated
    against (default: the clean fp64 restatement; the GPU test passes the kernel's outputs).  The missing clamp is the
    sixth mistake of the list in the issue; it moves MSE / MAE / PSNR as well and is checked the same way."""
    survivors = []
    for cid, p, t, clamp in mutation_cases():
        base = base_of(cid, p, t, clamp) if base_of is not None else metrics(p, t, clamp=clamp)
        muts = {name: metrics(p, t, clamp=clamp, **kw) for name, kw in MUTATIONS.items()}
        muts["missing clamp"] = metrics(p, t, clamp=None)
        for name, m in muts.items():
            if not gate.violations(deviation(base, m)):      # the case's deviation: the largest over its samples
                survivors.append(f"{name} @ {cid}")
    return survivors

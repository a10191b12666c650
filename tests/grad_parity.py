"""Per-tensor gradient comparator: HIP gradients against a float64 reference, one row per parameter tensor.

A whole-arena cosine cannot see a small tensor: every GroupNorm affine and every conv bias holds well under 0.2 % of
the gradient's squared norm, so any of them could be zeroed, negated or doubled with the arena cosine still >= 0.999.
This module gates every tensor on its own, with no element-count cutoff:

  * scale ``alpha = <g_h, g_o> / |g_o|^2``: the projection coefficient of the HIP gradient on the reference.  The
    rounding noise of the 16-bit forward and backward is nearly orthogonal to g_o, so alpha stays near 1 even where the
    relative error does not; zeroing, negating, scaling, stale accumulation and swaps move it directly;
  * residual ``rho = |g_h - alpha g_o| / |g_o|``: the error that is not a change of scale;
  * structural zeros: tensors whose reference norm is <= 1e-12 of the arena's.  The only ones in this model are the
    attention key biases (softmax is invariant to a per-query shift, so ``to_k.bias`` has an exact gradient of 0);
    ``structural_zeros`` returns them and the tests assert that set, so a new vanishing gradient is noticed.  They are
    gated absolutely: ``|g_h| <= tau |g_o(to_q.bias of the same block)|``.

``self_check`` applies the mutations a wrong kernel or a wrong schedule would produce (zero, negate, x0.95, x1.05, +g_o
for a stale accumulation, a swap with a same-shaped tensor whose reference cosine is < 0.9) to one tensor at a time and
returns those the gate did not flag: it proves the gate has teeth at the tolerances actually chosen.  With |alpha - 1|
<= A <= 2e-2 a 5 % scale error always lands outside the band (a tensor with a wider, named exemption takes a 2.5 A
step instead), and a swap always gives rho > 0.47 (cosine < 0.9 bounds the partner's component orthogonal to g_o), so
the check can only fail if R is set above that.
"""
from __future__ import annotations

import dataclasses
import re

import torch

CLASSES = ("conv_w", "small_w", "bias", "gn", "attn")
ZERO_REL = 1e-12          # |g_o| <= ZERO_REL * |arena|: structural zero
SWAP_MAX_COS = 0.9
_GN = re.compile(r"(\.norm\d*|blocks\.\d+)\.(weight|bias)$")


def tensor_class(name: str, numel: int) -> str:
    """conv weights with >= 1024 elements, smaller conv weights (image side, latent head, post_quant), conv biases,
    GroupNorm affine (ResBlock norms, attention norms, the closing norm of encoder and decoder), attention projections
    (the q / k / v / out Linear layers, weights and biases)."""
    if ".attn." in name:
        return "attn"
    if _GN.search(name):
        return "gn"
    if name.endswith(".bias"):
        return "bias"
    return "conv_w" if numel >= 1024 else "small_w"


def zero_partner(name: str) -> str:
    """The tensor whose reference norm sets the absolute scale of a structural zero."""
    return name.replace(".to_k.bias", ".to_q.bias")


@dataclasses.dataclass
class Gate:
    """|alpha - 1| <= bounds[cls][0] and rho <= bounds[cls][1] for every tensor; structural zeros |g_h| <= tau * scale.
    ``exempt``: {name: (A, R, reason)} for a tensor that needs wider bounds than its class (the reason is part of the
    gate; an exemption never tightens a class bound)."""
    bounds: dict
    tau: float
    exempt: dict = dataclasses.field(default_factory=dict)

    def limits(self, name, cls):
        a, r = self.bounds[cls]
        e = self.exempt.get(name)
        return (max(a, e[0]), max(r, e[1])) if e is not None else (a, r)

    def scale_step(self, name, cls):
        """The scale mutation the self-check applies: 5 %, or 2.5 A where A is wider (with |alpha - 1| <= A a scale
        error s > 2 A / (1 - A) always leaves the band)."""
        return max(0.05, 2.5 * self.limits(name, cls)[0])


@dataclasses.dataclass
class Row:
    name: str
    cls: str
    numel: int
    alpha: float          # nan for a structural zero
    rho: float            # |g_h| / |g_o(partner)| for a structural zero
    zero: bool

    def failure(self, gate: Gate):
        """None when the row passes ``gate``, else a one-line reason."""
        if not (self.rho == self.rho) or (not self.zero and not (self.alpha == self.alpha)):
            return f"{self.name}: non-finite (alpha {self.alpha}, rho {self.rho})"
        if self.zero:
            return None if self.rho <= gate.tau else \
                f"{self.name}: structural zero, |g_h| = {self.rho:.3e} x |g_o(to_q.bias)| > tau {gate.tau:.1e}"
        a, r = gate.limits(self.name, self.cls)
        if abs(self.alpha - 1.0) > a or self.rho > r:
            return f"{self.name} [{self.cls}, {self.numel}]: alpha {self.alpha:.5f} (|alpha-1| <= {a:.1e}), " \
                   f"rho {self.rho:.3e} (<= {r:.1e})"
        return None


def _f64(t):
    return t.detach().to("cpu", torch.float64).flatten()


def structural_zeros(g_ref: dict) -> set:
    """Names whose reference gradient norm is <= ZERO_REL of the whole arena's."""
    arena = torch.sqrt(sum(_f64(g).square().sum() for g in g_ref.values()))
    return {n for n, g in g_ref.items() if _f64(g).norm() <= ZERO_REL * arena}


class Comparator:
    """Holds the float64 reference and its structural zeros; ``row`` / ``rows`` evaluate HIP gradients against it."""

    def __init__(self, g_ref: dict):
        self.ref = {n: _f64(g) for n, g in g_ref.items()}
        self.shape = {n: tuple(g.shape) for n, g in g_ref.items()}
        self.zeros = structural_zeros(self.ref)
        self.sq = {n: (g @ g).item() for n, g in self.ref.items()}

    def row(self, name, g_h) -> Row:
        h, o = _f64(g_h), self.ref[name]
        if h.numel() != o.numel():
            raise ValueError(f"{name}: {h.numel()} elements vs {o.numel()} in the reference")
        cls = tensor_class(name, o.numel())
        if name in self.zeros:
            return Row(name, cls, o.numel(), float("nan"), (h.norm() / self.ref[zero_partner(name)].norm()).item(), True)
        alpha = (h @ o).item() / self.sq[name]
        rho = ((h - alpha * o).norm().item()) / self.sq[name] ** 0.5
        return Row(name, cls, o.numel(), alpha, rho, False)

    def rows(self, g_hip: dict) -> list:
        missing = set(self.ref) ^ set(g_hip)
        if missing:
            raise ValueError(f"tensor names differ from the reference: {sorted(missing)[:8]}")
        return [self.row(n, g_hip[n]) for n in self.ref]

    def swap_partner(self, name):
        """The next tensor in arena order (wrapping) with the same shape and a reference cosine < SWAP_MAX_COS with
        ``name`` (neighbours are the likeliest mis-routing), or None."""
        names = list(self.ref)
        i = names.index(name)
        o = self.ref[name]
        for m in names[i + 1:] + names[:i]:
            if self.shape[m] != self.shape[name]:
                continue
            p = self.ref[m]
            den = (o.norm() * p.norm()).item()
            if den == 0.0 or (o @ p).item() / den < SWAP_MAX_COS:
                return m
        return None

    def mutations(self, g_hip: dict, gate: Gate):
        """-> (label, name, mutated g_h of ``name``) for every tensor.  A structural zero only takes the swap: zeroing,
        negating, scaling or adding g_o (= 0) to an exact zero leaves a correct gradient.  The scale step is 5 %
        wherever A <= 2e-2 (``Gate.scale_step``)."""
        for n, h in g_hip.items():
            h = _f64(h)
            if n not in self.zeros:
                s = gate.scale_step(n, tensor_class(n, h.numel()))
                yield "zero", n, torch.zeros_like(h)
                yield "negate", n, -h
                yield f"x{1 - s:.3g}", n, (1 - s) * h
                yield f"x{1 + s:.3g}", n, (1 + s) * h
                yield "+g_o (stale accumulation)", n, h + self.ref[n]
            m = self.swap_partner(n)
            if m is not None:
                yield f"swap with {m}", n, _f64(g_hip[m])

    def self_check(self, g_hip: dict, gate: Gate):
        """-> (number of mutations applied, [(label, name) the gate did NOT flag])."""
        count, missed = 0, []
        for label, n, h in self.mutations(g_hip, gate):
            count += 1
            if self.row(n, h).failure(gate) is None:
                missed.append((label, n))
        return count, missed


# The gate of every native-path test (tests/test_gpu_grad_per_tensor.py), set from MI355X measurements: config A at
# 64^2 (1 and 3 image channels, every knob variant but PTI_FWD_ACT_DTYPE=bf16) and 256^2, config AR at 64^2 with the
# AR term and at 256^2, the third step, the drop-in autograd path.  Worst measured |alpha - 1| / rho per class:
#   conv_w 5.6e-3 / 3.6e-2, small_w 8.1e-3 / 3.2e-2, bias 1.2e-2 / 3.6e-2 (two exemptions below), gn 1.7e-2 / 4.2e-2,
#   attn 1.2e-2 / 3.6e-2; structural zeros |g_h| / |g_o(to_q.bias)| <= 1.1e-2.
GATE = Gate(
    bounds={"conv_w": (2e-2, 5e-2), "small_w": (2e-2, 5e-2), "bias": (2e-2, 6e-2), "gn": (2e-2, 6e-2),
            "attn": (2e-2, 6e-2)},
    tau=2.5e-2,
    exempt={
        # the sum over every pixel of the bf16 gradient entering the first ResBlock, which mostly cancels (the
        # GroupNorm backward removes each group's mean): measured |alpha - 1| 2.1e-2 at one image channel, 64^2 (2.4e-2
        # with PTI_GNBWD_CHAIN=1), the same on the drop-in path; 6.4e-3 at 256^2 and <= 1.1e-2 at three channels on both
        # conv_in paths, so not a property of the direct kernel that computes it
        "encoder.blocks.0.conv.bias": (4e-2, 6e-2, "pixel sum of a mostly cancelling bf16 gradient (64^2, 1 channel)"),
        # one element: the L1 loss's sign count (#(recon > x) - #(recon < x)) / N.  The exact-zero background makes
        # many residuals tiny, and 16-bit forward rounding flips their signs: measured |alpha - 1| 3.7e-2 with
        # PTI_SAVE_ACT_MIN_HW above every map (the GroupNorm+SiLU prologue path); a CPU emulation of fp16 activations
        # with bf16 gradients gives 5.6e-2 on the same tensor
        "decoder.blocks.16.conv.bias": (6e-2, 0.0, "L1 sign count over pixels flipped by 16-bit forward rounding"),
    })


def failures(rows, gate: Gate) -> list:
    return [f for f in (r.failure(gate) for r in rows) if f is not None]


def report(rows, tag="") -> str:
    """Compact table: per class the tensor count, the worst |alpha - 1| and the worst rho with their tensors; the
    structural zeros' |g_h| / |g_o(to_q.bias)|."""
    lines = [f"[{tag}] {len(rows)} tensors"]
    for cls in CLASSES:
        rs = [r for r in rows if r.cls == cls and not r.zero]
        if not rs:
            continue
        wa = max(rs, key=lambda r: abs(r.alpha - 1.0))
        wr = max(rs, key=lambda r: r.rho)
        lines.append(f"  {cls:8s} n={len(rs):3d}  worst |alpha-1| {abs(wa.alpha - 1.0):.2e} ({wa.name})  "
                     f"worst rho {wr.rho:.2e} ({wr.name})")
    zs = [r for r in rows if r.zero]
    if zs:
        w = max(zs, key=lambda r: r.rho)
        lines.append(f"  zeros    n={len(zs):3d}  worst |g_h|/|g_o(to_q.bias)| {w.rho:.2e} ({w.name})")
    return "\n".join(lines)


def worst(rows) -> dict:
    """{class: (worst |alpha - 1|, worst rho)} and {"zeros": worst ratio}: what the tests record and print."""
    out = {}
    for cls in CLASSES:
        rs = [r for r in rows if r.cls == cls and not r.zero]
        if rs:
            out[cls] = (max(abs(r.alpha - 1.0) for r in rs), max(r.rho for r in rs))
    zs = [r.rho for r in rows if r.zero]
    if zs:
        out["zeros"] = max(zs)
    return out

"""fp64 numpy restatement of the guarded optimiser step (``csrc/optim_guard.hip``): the global gradient
norm, the clip / skip decision, Adam, the EMA of the weights and the two step counters.  No torch, no GPU: the checker of
``tests/test_optim_guard_cpu.py`` (which pins it to ``clip_grad_norm_`` + ``torch.optim.Adam``) and of
``tests/test_gpu_optim_guard.py``."""
import math

import numpy as np


def ema_decay_in_effect(ema_decay, t):
    """min(ema_decay, (1 + t) / (10 + t)): the warm-up of the LDM code bases; ``t`` = applied steps, this one included."""
    return min(float(ema_decay), (1.0 + t) / (10.0 + t))


class GuardOracle:
    """State ``p, m, v[, ema]`` (fp64 copies) and counters ``applied, skipped``; ``step(g)`` -> what the control record
    holds after that step, plus the update that was applied (zeros on a skipped step)."""

    def __init__(self, p, *, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=None, skip_nonfinite=False, ema_decay=None,
                 m=None, v=None, ema=None, applied=0, skipped=0):
        self.p = np.asarray(p, dtype=np.float64).copy()
        self.m = np.zeros_like(self.p) if m is None else np.asarray(m, dtype=np.float64).copy()
        self.v = np.zeros_like(self.p) if v is None else np.asarray(v, dtype=np.float64).copy()
        self.ema = None
        if ema_decay is not None:
            self.ema = self.p.copy() if ema is None else np.asarray(ema, dtype=np.float64).copy()
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_norm, self.skip_nonfinite, self.ema_decay = max_norm, bool(skip_nonfinite), ema_decay
        self.applied, self.skipped = int(applied), int(skipped)

    def decide(self, g, grad_scale=1.0):
        g = np.asarray(g, dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            sumsq = float(np.sum(g * g))
            norm = float(grad_scale) * math.sqrt(sumsq) if sumsq == sumsq else float("nan")
        bad = bool((~np.isfinite(g)).any()) or not math.isfinite(norm)
        skip = bad and self.skip_nonfinite
        coef = 1.0
        if self.max_norm is not None and not bad:       # torch.nn.utils.clip_grad_norm_
            coef = min(1.0, float(self.max_norm) / (norm + 1e-6))
        return {"sumsq": sumsq, "norm": norm, "bad": bad, "skip": skip, "coef": coef}

    def step(self, g, grad_scale=1.0):
        d = self.decide(g, grad_scale)
        d["update"] = np.zeros_like(self.p)
        if d["skip"]:
            self.skipped += 1
        else:
            self.applied += 1
            t = self.applied
            b1, b2 = self.betas
            d["bias1"], d["bias2_sqrt"] = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
            with np.errstate(over="ignore", invalid="ignore"):
                gr = np.asarray(g, dtype=np.float64) * (float(grad_scale) * d["coef"])
                self.m = b1 * self.m + (1.0 - b1) * gr
                self.v = b2 * self.v + (1.0 - b2) * gr * gr
                d["update"] = (self.lr / d["bias1"]) * (self.m / (np.sqrt(self.v) / d["bias2_sqrt"] + self.eps))
                self.p = self.p - d["update"]
            if self.ema is not None:
                d["ema_decay"] = ema_decay_in_effect(self.ema_decay, t)
                self.ema = self.ema + (1.0 - d["ema_decay"]) * (self.p - self.ema)
        d["applied_steps"], d["skipped_steps"] = self.applied, self.skipped
        return d

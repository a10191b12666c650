"""``FlatAdam`` — ``torch.optim.Adam`` (defaults; reference ``vae_scripts/train_vae.py:301,304``) as ONE HIP
kernel over a model's flat fp32 parameter arena (``AutoencoderKL``: instead of ~220 per-tensor updates;
``PatchDiscriminator``: the same kernel over its arena).

``state_dict()`` / ``load_state_dict()`` use ``torch.optim.Adam``'s format over ``VAEModel.parameters()``
order, so ``checkpoint_epoch*.pth`` files (train_vae.py:752-765) are interchangeable with the
reference's ``optimizer_g_state_dict``.

The guarded step (``clip_norm`` / ``skip_nonfinite`` / ``ema_decay``, all off by default): global-norm
gradient clipping, skipping the update when a gradient is not finite, and an exponential moving average of the weights,
decided and applied on the device (``ops.grad_guard`` + ``ops.adam_step_guarded``) without a host synchronisation.  With
all three off nothing is allocated and ``step()`` is the single ``ops.adam_step`` launch.
"""
from __future__ import annotations

import math

import torch

from . import ops


class FlatAdam:
    def __init__(self, net, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, *, clip_norm: float | None = None,
                 skip_nonfinite: bool = False, ema_decay: float | None = None):
        if clip_norm is not None and not (isinstance(clip_norm, (int, float)) and not isinstance(clip_norm, bool)
                                          and math.isfinite(clip_norm) and clip_norm > 0):
            raise ValueError(f"FlatAdam: clip_norm must be a finite positive number or None, got {clip_norm!r}")
        if ema_decay is not None and not (isinstance(ema_decay, (int, float)) and not isinstance(ema_decay, bool)
                                          and 0.0 < ema_decay < 1.0):
            raise ValueError(f"FlatAdam: ema_decay must lie in (0, 1) or be None, got {ema_decay!r}")
        self.net = net
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.guarded = self.clip_norm is not None or self.skip_nonfinite or self.ema_decay is not None
        self._step_count = 0
        arena = net.param_arena
        self.exp_avg = torch.zeros_like(arena)
        self.exp_avg_sq = torch.zeros_like(arena)
        if self.guarded:
            # the device-side control record (ops.GRAD_GUARD_COLUMNS): the step counters live there, not on the host
            self.ctl = torch.zeros(len(ops.GRAD_GUARD_COLUMNS), dtype=torch.float64, device=arena.device)
        if self.ema_decay is not None:
            self.ema = arena.detach().clone()

    def zero_grad(self, set_to_none: bool = True):
        # gradients live in the arena; the trainer clears it with one memset per step
        self.net.grad_arena.zero_()

    # ---- step counter: Adam's t.  On the guarded path the device decides whether a step counts -------------------
    @property
    def step_count(self) -> int:
        if self.guarded:
            return int(self.ctl[0].item())      # one small D2H copy, on demand
        return self._step_count

    @step_count.setter
    def step_count(self, value: int):
        if self.guarded:
            self.ctl[0] = float(int(value))
        else:
            self._step_count = int(value)

    def step(self, grad_scale: float = 1.0):
        net = self.net
        if self.guarded:        # three launches, no host synchronisation
            ops.grad_guard(net.grad_arena, ctl=self.ctl, grad_scale=grad_scale, max_norm=self.clip_norm,
                           skip_nonfinite=self.skip_nonfinite, betas=self.betas, ema_decay=self.ema_decay)
            ops.adam_step_guarded(net.param_arena, net.grad_arena, self.exp_avg, self.exp_avg_sq, ctl=self.ctl, lr=self.lr,
                                  betas=self.betas, eps=self.eps, ema=self.ema if self.ema_decay is not None else None)
        else:
            self._step_count += 1
            ops.adam_step(net.param_arena, net.grad_arena, self.exp_avg, self.exp_avg_sq, lr=self.lr, beta1=self.betas[0],
                          beta2=self.betas[1], eps=self.eps, step=self._step_count, grad_scale=grad_scale)
        net.mark_weights_dirty()

    def guard_stats(self) -> dict:
        """What the guard saw at the last step, from one 64-byte copy (a host synchronisation: call it where the caller
        synchronises anyway).  ``grad_norm`` is taken after ``grad_scale`` and before clipping."""
        if not self.guarded:
            raise RuntimeError("guard_stats: this FlatAdam has no guard (clip_norm / skip_nonfinite / ema_decay are all off)")
        c = dict(zip(ops.GRAD_GUARD_COLUMNS, self.ctl[:ops.GRAD_GUARD_HOST_COLUMNS].tolist()))
        return {"grad_norm": c["norm"], "clip_coef": c["coef"], "skipped": bool(c["skip"]),
                "applied_steps": int(c["applied_steps"]), "skipped_steps": int(c["skipped_steps"])}

    # ---- torch.optim.Adam-compatible (de)serialisation ---------------------------------------------
    def _ordered(self):
        return [(n, p) for n, p in self.net.named_parameters()]

    def state_dict(self):
        state = {}
        step_count = self.step_count
        if step_count > 0:
            for i, (n, p) in enumerate(self._ordered()):
                state[i] = {"step": torch.tensor(float(step_count)),
                            "exp_avg": self.net.slot_view(self.exp_avg, n).clone(memory_format=torch.contiguous_format),
                            "exp_avg_sq": self.net.slot_view(self.exp_avg_sq, n).clone(memory_format=torch.contiguous_format)}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(self._ordered())))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(g["lr"]), tuple(g["betas"]), float(g["eps"])
        names = [n for n, _ in self._ordered()]
        if len(g["params"]) != len(names):
            raise ValueError("optimizer state does not match the model's parameter list")
        step_count = 0
        for i, n in enumerate(names):
            st = sd["state"].get(i)
            if st is None:
                continue
            self.net.slot_view(self.exp_avg, n).copy_(st["exp_avg"])
            self.net.slot_view(self.exp_avg_sq, n).copy_(st["exp_avg_sq"])
            step_count = int(float(st["step"]))
        self.step_count = step_count

    # ---- EMA of the weights, in state_dict() layout ---------------------------------------------------------------
    def _need_ema(self, who):
        if self.ema_decay is None:
            raise RuntimeError(f"{who}: this FlatAdam keeps no EMA (ema_decay is None)")

    def ema_state_dict(self):
        """The averaged weights as ``net.state_dict()`` would hold them: every parameter from the EMA arena, anything
        else the module keeps (buffers) as it is.  A plain state dict: the loaders take it like any weights."""
        self._need_ema("ema_state_dict")
        sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        for n, _ in self._ordered():
            if n not in sd or sd[n].shape != self.net.slot_view(self.ema, n).shape:
                raise RuntimeError(f"ema_state_dict: parameter {n} is not a state_dict entry of its own shape")
            sd[n] = self.net.slot_view(self.ema, n).detach().clone(memory_format=torch.contiguous_format)
        return sd

    def load_ema_state_dict(self, sd):
        self._need_ema("load_ema_state_dict")
        names = [n for n, _ in self._ordered()]
        missing = [n for n in names if n not in sd]
        if missing:
            raise ValueError(f"load_ema_state_dict: missing {missing[:3]}{' ...' if len(missing) > 3 else ''}")
        for n in names:
            self.net.slot_view(self.ema, n).copy_(sd[n])

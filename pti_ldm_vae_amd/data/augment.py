"""Train-time augmentation policy and per-sample parameter draws.

The pipeline is the one the reference defines in ``src/pti_ldm_vae/data/augmentation.py``
(``get_albumentations_transform``: horizontal flip p 0.5, vertical flip p 0.5, 90-degree rotation p 0.5, shift / scale /
rotate +-0.1 / +-0.1 / +-15 degrees with a zero border p 0.5, elastic transform alpha 50 sigma 5 with a zero border p 0.3)
and never wires into its loaders.  Here the host only DRAWS: per sample one 2x3 inverse map, one 64-bit key and one
elastic amplitude; the device does the work (``ops.elastic_field``, ``ops.augment_warp``) on the loader's copy stream.

Deviations from albumentations, on purpose:
  * ONE resampling.  albumentations resamples after the shift / scale / rotate and again for the elastic transform (flips
    and quarter turns are exact there too).  Here every drawn transform is composed into a single inverse map and the
    image is interpolated once: sharper, and the only form that fits in one gather.
  * The quarter turn draws k from {1, 2, 3} (albumentations: {0, 1, 2, 3}); on a non-square patch from {2} only.
  * ``alpha_affine`` of the elastic transform is not mirrored: the shift / scale / rotate stage already covers it.
  * The random stream is this module's own (albumentations' cannot be matched without it).

Random numbers.  Sample ``(seed, epoch, index)`` -- ``index`` is the position in the loader's path list -- owns the stream
``u_j = splitmix64(state + (j + 1) * 0x9E3779B97F4A7C15)``, ``state = mix(mix(mix(seed) ^ epoch) ^ index)`` with ``mix``
the splitmix64 finaliser, all modulo 2^64; a uniform in [0, 1) is the top 53 bits.  Every slot is always consumed, so one
parameter never depends on whether another transform was drawn, and nothing depends on batch size, batch position, rank
or world size.  Slots, in order:

    0 hflip (u < hflip_p)      1 vflip (u < vflip_p)     2 rot90 (u < rot90_p)     3 k = 1 + floor(3 u)  (non-square: 2)
    4 shift/scale/rotate (u < ssr_p)     5 dx = shift_limit (2u - 1) W     6 dy = shift_limit (2u - 1) H
    7 scale = 1 + scale_limit (2u - 1)   8 angle = rotate_limit (2u - 1) degrees
    9 elastic (u < elastic_p -> alpha = elastic_alpha, else 0)            10 key = the 64 raw bits
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, fields

import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z: int) -> int:
    """splitmix64 finaliser (Steele, Lea, Flood 2014; public domain reference implementation by S. Vigna)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_state(seed: int, epoch: int, index: int) -> int:
    return _mix64(_mix64(_mix64(int(seed)) ^ (int(epoch) & _M64)) ^ (int(index) & _M64))


def slot_bits(state: int, slot: int) -> int:
    """64 raw bits of slot ``slot`` of a sample's stream."""
    return _mix64(state + (slot + 1) * _GOLDEN)


def slot_uniform(state: int, slot: int) -> float:
    return (slot_bits(state, slot) >> 11) * (1.0 / (1 << 53))


@dataclass(frozen=True)
class AugmentPolicy:
    """Probabilities and limits of the geometric pipeline; the defaults are the reference's values."""

    hflip_p: float = 0.5
    vflip_p: float = 0.5
    rot90_p: float = 0.5
    ssr_p: float = 0.5
    shift_limit: float = 0.1      # fraction of W (x) and H (y)
    scale_limit: float = 0.1      # scale in 1 +- scale_limit
    rotate_limit: float = 15.0    # degrees
    elastic_p: float = 0.3
    elastic_alpha: float = 50.0   # amplitude of the smoothed [-1, 1) noise, pixels
    elastic_sigma: float = 5.0    # Gaussian sigma, pixels

    def __post_init__(self):
        for f in fields(self):
            v = getattr(self, f.name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"augment: {f.name} must be a non-negative number, got {v!r}")
            if f.name.endswith("_p") and v > 1:
                raise ValueError(f"augment: {f.name} is a probability, got {v!r}")
        if self.elastic_sigma <= 0:
            raise ValueError("augment: elastic_sigma must be positive")

    def to_dict(self) -> dict:
        return asdict(self)

    @classmethod
    def from_config(cls, value, ar_vae_enabled: bool = False) -> "AugmentPolicy | None":
        """The config's ``augment`` value -> policy: ``False`` / ``None`` -> ``None``; ``True`` -> the defaults; a dict
        overrides single fields (an unknown key raises ``ValueError``); an ``AugmentPolicy`` passes through unchanged.

        With ``ar_vae_enabled`` the attributes that ride along are physical heights and widths of the imaged object: a
        scale change or an elastic warp makes the image disagree with them, flips, quarter turns, shifts and small
        rotations do not.  ``scale_limit`` and ``elastic_p`` therefore become 0 unless the dict names them, and the policy
        says so once on stdout."""
        if value is None or value is False:
            return None
        if isinstance(value, cls):
            return value
        if value is True:
            given = {}
        elif isinstance(value, dict):
            given = dict(value)
        else:
            raise ValueError(f"augment: expected true, false or an object of policy fields, got {value!r}")
        known = [f.name for f in fields(cls)]
        unknown = sorted(set(given) - set(known))
        if unknown:
            raise ValueError(f"augment: unknown key(s) {unknown}; known: {known}")
        if ar_vae_enabled:
            zeroed = [k for k in ("scale_limit", "elastic_p") if k not in given]
            for k in zeroed:
                given[k] = 0.0
            if zeroed:
                print(f"[augment] AR-VAE attributes are physical sizes: {' and '.join(zeroed)} set to 0 "
                      "(name them in the config's augment object to keep them)")
        return cls(**given)


def draw_raw(policy: AugmentPolicy, seed: int, epoch: int, index: int, H: int, W: int) -> dict:
    """The drawn transform of ONE sample as plain numbers: ``hflip``, ``vflip`` (bool), ``k`` (quarter turns, 0 = none),
    ``ssr`` (bool), ``dx``, ``dy`` (pixels), ``scale``, ``angle`` (degrees), ``alpha``, ``key``.  Slot order: module doc."""
    st = sample_state(seed, epoch, index)
    u = [slot_uniform(st, j) for j in range(10)]
    k = 0
    if u[2] < policy.rot90_p:
        k = 1 + min(2, int(3.0 * u[3])) if H == W else 2
    ssr = u[4] < policy.ssr_p
    return {"hflip": u[0] < policy.hflip_p, "vflip": u[1] < policy.vflip_p, "k": k, "ssr": ssr,
            "dx": policy.shift_limit * (2.0 * u[5] - 1.0) * W if ssr else 0.0,
            "dy": policy.shift_limit * (2.0 * u[6] - 1.0) * H if ssr else 0.0,
            "scale": 1.0 + policy.scale_limit * (2.0 * u[7] - 1.0) if ssr else 1.0,
            "angle": policy.rotate_limit * (2.0 * u[8] - 1.0) if ssr else 0.0,
            "alpha": float(policy.elastic_alpha) if u[9] < policy.elastic_p else 0.0,
            "key": slot_bits(st, 10)}


_EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _compose(m, n):
    """2x3 affine maps as row-major 6-tuples: p -> m(n(p)), in Python floats (fp64)."""
    return (m[0] * n[0] + m[1] * n[3], m[0] * n[1] + m[1] * n[4], m[0] * n[2] + m[1] * n[5] + m[2],
            m[3] * n[0] + m[4] * n[3], m[3] * n[1] + m[4] * n[4], m[3] * n[2] + m[4] * n[5] + m[5])


def inverse_map(raw: dict, H: int, W: int) -> np.ndarray:
    """fp64 3x3 map from an output pixel to its source position for ``raw`` (``draw_raw``): the inverse of hflip, then
    vflip, then ``np.rot90`` by k, then shift / scale / rotate about the centre ``((W-1)/2, (H-1)/2)``.  A transform that
    was not drawn contributes the exact identity, so flips and quarter turns alone give entries 0 / +-1 and integer
    offsets.  (Plain Python floats: the loader draws a whole batch between two optimiser steps.)"""
    w1, h1 = float(W - 1), float(H - 1)
    m = (-1.0, 0.0, w1, 0.0, 1.0, 0.0) if raw["hflip"] else _EYE
    if raw["vflip"]:
        m = _compose(m, (1.0, 0.0, 0.0, 0.0, -1.0, h1))
    k = raw["k"]
    if k in (1, 3) and H != W:
        raise ValueError("augment: a quarter turn by 1 or 3 needs a square patch")
    if k:   # output (x, y) of np.rot90(a, k) reads a at: k=1 (W-1-y, x); k=2 (W-1-x, H-1-y); k=3 (y, H-1-x)
        m = _compose(m, {1: (0.0, -1.0, w1, 1.0, 0.0, 0.0), 2: (-1.0, 0.0, w1, 0.0, -1.0, h1), 3: (0.0, 1.0, 0.0, -1.0, 0.0, h1)}[k])
    if raw["ssr"]:
        cx, cy = w1 / 2.0, h1 / 2.0
        th = math.radians(raw["angle"])
        c, s, inv = math.cos(th), math.sin(th), 1.0 / raw["scale"]
        # forward p' = ctr + scale * Rot(th) (p - ctr) + t  ->  p = ctr + Rot(-th) (p' - ctr - t) / scale
        a00, a01, a10, a11 = c * inv, s * inv, -s * inv, c * inv
        tx, ty = cx + raw["dx"], cy + raw["dy"]
        m = _compose(m, (a00, a01, cx - (a00 * tx + a01 * ty), a10, a11, cy - (a10 * tx + a11 * ty)))
    return np.array([m[:3], m[3:], (0.0, 0.0, 1.0)])


def draw_params(policy: AugmentPolicy, seed: int, epoch: int, index: int, H: int, W: int):
    """``(mat[6] float32, key uint64, alpha float32)`` of ONE sample, a function of ``(policy, seed, epoch, index, H, W)``
    only.  ``mat`` is the row-major 2x3 inverse map of ``ops.augment_warp`` (composed in fp64, cast once); ``key`` and
    ``alpha`` feed ``ops.elastic_field`` (``alpha`` 0: no elastic transform).  This is ONE resampling of the image where
    albumentations would do up to three passes over the image (module doc): sharper, and the only form that fits in one gather."""
    raw = draw_raw(policy, seed, epoch, index, H, W)
    mat = inverse_map(raw, H, W)[:2].reshape(6).astype(np.float32)
    return mat, np.uint64(raw["key"]), np.float32(raw["alpha"])

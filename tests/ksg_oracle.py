"""Plain numpy restatement of the k-nearest-neighbour (KSG, estimator 1) mutual information behind ``evaluate_disentanglement
--mi-estimator ksg`` (``pti_ksg_counts`` + ``utils/disentanglement.ksg_mutual_information``).  numpy only: the GPU tests
import it where scipy and sklearn may be missing.

For one pair of fp32 columns ``x``, ``y`` and a neighbour count ``k``, with boolean / fp32 ``[n, n]`` tables:

1. ``dx_ij = |x_i - x_j|``, ``dy_ij = |y_i - y_j|`` (one fp32 subtraction each), ``d_ij = max(dx_ij, dy_ij)`` for ``j != i``;
2. ``eps_i`` = the k-th smallest ``d_ij`` over ``j != i``, with multiplicity;
3. ``r_i`` = the largest fp32 below ``eps_i``, 0 when ``eps_i == 0``;
4. ``nx_i = #{j != i: dx_ij <= r_i}``, ``ny_i = #{j != i: dy_ij <= r_i}``;
5. ``MI = max(0, psi(n) + psi(k) - mean_i psi(nx_i + 1) - mean_i psi(ny_i + 1))`` in nats.

That is scikit-learn's ``_compute_mi_cc`` (tests/test_ksg_cpu.py compares the two).  ``pair_tables`` takes switches that
MUTATE the definition; the CPU tests show that each is caught by an exact table.

``tools/make_ksg_golden.py`` records ``tests/golden/ksg_golden.npz`` from ``case_tables``.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ksg_golden.npz")
TABLES = ("eps", "nx", "ny")
EULER_GAMMA = 0.5772156649015328606

# name, n, L, na, neighbour counts, seed, kind, (ldz - n, lda - n) of the GPU run
CASES = [
    ("n2", 2, 1, 1, (1,), 41, "plain", (0, 0)),             # the minimum: the other row is the neighbour
    ("n4", 4, 1, 1, (3,), 42, "plain", (0, 0)),             # n = k + 1
    ("n17", 17, 2, 1, (16,), 43, "plain", (0, 0)),          # the largest k at n = k + 1
    ("n65", 65, 2, 2, (3,), 44, "plain", (0, 0)),           # one row past a wavefront
    ("n257", 257, 10, 6, (3,), 45, "plain", (0, 0)),        # one row past a workgroup / LDS tile; the AR config's L and na
    ("n1030", 1030, 16, 16, (5,), 46, "coarse", (0, 0)),    # all 256 pairs; several tiles with a ragged last one
    ("n2500", 2500, 2, 2, (1, 16), 47, "plain", (12, 60)),  # many tiles; padded strides; the smallest and the largest k
    ("ties", 300, 3, 3, (3,), 48, "ties", (0, 0)),          # 5- and 21-valued attributes, 40 duplicate rows: eps = 0
    ("kth_tie", 64, 1, 1, (3,), 49, "lattice", (0, 0)),     # the 3rd and 4th neighbour at the same distance
    ("const", 97, 2, 2, (3,), 50, "const", (0, 0)),         # a constant channel and a constant attribute: MI = 0.0
    ("tiny", 33, 1, 1, (3,), 51, "tiny", (0, 0)),           # subnormal values and differences; -0.0 next to 0.0
]
GRID = 2.0 ** -20   # "plain" values are multiples of it below 8 in magnitude: their fp32 and fp64 differences coincide


def make_case(name, n, l, na, ks, seed, kind="plain"):
    """Seeded inputs ``z`` [n, L], ``attrs`` [na, n] (fp32) on dyadic grids, so that every difference is exact in fp32 and
    the same in fp64.  Attribute q follows channel (3 q + 1) % L loosely, so that the estimates are not all noise."""
    rng = np.random.default_rng(seed)
    step = 1.0 / 8.0 if kind == "coarse" else GRID
    z = np.clip(np.round(rng.normal(0.0, 1.0, (n, l)) / step) * step, -7.0, 7.0)
    channels = [(3 * q + 1) % l for q in range(na)]
    attrs = np.stack([0.8 * z[:, channels[q]] + 0.6 * rng.normal(0.0, 1.0, n) for q in range(na)])
    attrs = np.clip(np.round(attrs / step) * step, -7.0, 7.0)
    if kind == "coarse":                                            # integer attributes 0 .. 39, as pixel counts are
        attrs = np.clip(np.round(20.0 + 6.0 * attrs), 0.0, 39.0)
    if kind == "ties":
        attrs[0] = rng.integers(0, 5, n)
        attrs[1] = rng.integers(0, 21, n)
        rows = rng.choice(n, 40, replace=False)
        z[rows, 1] = z[rows[0], 1]                                  # 40 rows with one value: duplicates of (x, y) with attrs[0]
    if kind == "lattice":                                           # an 8 x 8 integer lattice: up to 8 neighbours at distance 1
        idx = rng.permutation(n)
        z[:, 0], attrs[0] = idx % 8, idx // 8
    if kind == "const":
        z[:, 1] = 0.3
        attrs[1] = 7.0
    z, attrs = z.astype(np.float32), attrs.astype(np.float32)
    if kind == "tiny":                                              # multiples of the smallest subnormal, about 1e-40
        unit = np.float32(2.0 ** -149)
        z = (rng.integers(-2 ** 17, 2 ** 17, (n, l)).astype(np.float32) * unit).astype(np.float32)
        attrs = (rng.integers(-2 ** 17, 2 ** 17, (na, n)).astype(np.float32) * unit).astype(np.float32)
        z[:4, 0] = (0.0, -0.0, 0.0, -0.0)                           # four exact duplicates that differ in the sign of zero
        attrs[0, :4] = (-0.0, 0.0, 0.0, -0.0)
    return SimpleNamespace(name=name, n=n, l=l, na=na, ks=tuple(ks), z=z, attrs=attrs)


def all_cases():
    return [make_case(*spec[:7]) for spec in CASES]


def digamma_int(m_max):
    """``psi(m) = -gamma + H_(m - 1)`` for m = 1 .. m_max as fp64 ``[m_max + 1]`` (entry 0 unused: -inf); the harmonic
    numbers by compensated (Kahan) summation, so every entry is within an ulp or two of the true value."""
    out = np.full(m_max + 1, -np.inf)
    total, comp = 0.0, 0.0
    for m in range(1, m_max + 1):
        out[m] = total - EULER_GAMMA
        term = 1.0 / m - comp
        new = total + term
        comp = (new - total) - term
        total = new
    return out


def pair_tables(x, y, k, *, include_self=False, le_eps=False, no_zero_rule=False, euclidean=False):
    """-> ``(eps, nx, ny)``: fp32 [n], int32 [n], int32 [n] of one pair of columns.  The keyword switches are the mutations:
    self counted as its own neighbour; ``<= eps`` in place of ``<= r``; strict ``< eps`` also at ``eps == 0`` (duplicates
    dropped); the Euclidean distance in place of the Chebyshev one.  All False is the definition."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    n = x.size
    dx = np.abs(x[:, None] - x[None, :])                            # fp32 [n, n]
    dy = np.abs(y[:, None] - y[None, :])
    d = np.sqrt(dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2).astype(np.float32) if euclidean else np.maximum(dx, dy)
    other = np.ones((n, n), bool) if include_self else ~np.eye(n, dtype=bool)
    eps = np.partition(np.where(other, d, np.float32(np.inf)), k - 1, axis=1)[:, k - 1].astype(np.float32)   # k-th smallest
    if no_zero_rule:
        in_x, in_y = dx < eps[:, None], dy < eps[:, None]
    else:
        r = eps if le_eps else np.where(eps > 0, np.nextafter(eps, np.float32(0.0)), np.float32(0.0)).astype(np.float32)
        in_x, in_y = dx <= r[:, None], dy <= r[:, None]
    return eps, (in_x & other).sum(1).astype(np.int32), (in_y & other).sum(1).astype(np.int32)


def mutual_information(nx, ny, n, k):
    """Rule 5 for one pair, in scikit-learn's order of operations."""
    psi = digamma_int(n)
    return max(0.0, psi[n] + psi[k] - float(np.mean(psi[np.asarray(nx) + 1])) - float(np.mean(psi[np.asarray(ny) + 1])))


def case_tables(z, attrs, k, **mutations):
    """-> dict: ``eps`` fp32 [na, L, n], ``nx`` / ``ny`` int32 [na, L, n] and ``mi`` fp64 [na, L] of every (attribute, channel)."""
    z, attrs = np.asarray(z, np.float32), np.asarray(attrs, np.float32)
    n, l = z.shape
    na = attrs.shape[0]
    eps, nx, ny = np.zeros((na, l, n), np.float32), np.zeros((na, l, n), np.int32), np.zeros((na, l, n), np.int32)
    mi = np.zeros((na, l))
    for q in range(na):
        for c in range(l):
            eps[q, c], nx[q, c], ny[q, c] = pair_tables(z[:, c], attrs[q], k, **mutations)
            mi[q, c] = mutual_information(nx[q, c], ny[q, c], n, k)
    return dict(eps=eps, nx=nx, ny=ny, mi=mi)


def load_golden():
    with np.load(GOLDEN) as f:
        return {key: f[key] for key in f.files}

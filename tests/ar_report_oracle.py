"""Plain numpy restatement of the attribute-ordering report (``pti_rank_agreement`` + ``utils/ar_metrics.py``).

Everything is spelled out over ``np.triu_indices``: a sign table per attribute and per channel, the five pair classes as
boolean sums (integers, no tolerance), the loss summand in fp64.  ``report`` takes switches that MUTATE the definition
(tests/test_ar_report_cpu.py shows that every one of them is caught), ``ar_loss_fp32`` is the straightforward fp32
restatement whose deviation from fp64 sets the gate of the loss.

Run as ``python tests/ar_report_oracle.py`` to (re)write ``tests/golden/ar_report_golden.npz``: per case the exact counts,
the fp64 ``ar_loss`` and ``gate`` = 2 x the largest relative deviation of the fp32 restatement from it -- measured on the
CPU, never from the kernel.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ar_report_golden.npz")
CLASSES = ("concordant", "discordant", "z_tied", "a_tied", "both_tied")

# name, n, L, na, seed, kind, (ldz - n, lda - n) of the GPU run
CASES = [
    ("n2", 2, 1, 1, 11, "plain", (0, 0)),                 # a single pair
    ("n3", 3, 2, 1, 12, "plain", (0, 0)),                 # smallest multi-pair
    ("n65", 65, 3, 2, 13, "plain", (0, 0)),               # crosses a wavefront
    ("n257", 257, 10, 6, 14, "plain", (0, 0)),            # one past a 256 tile; the AR config's L and na
    ("n1030", 1030, 16, 16, 15, "plain", (0, 0)),         # both limits; several ragged tiles
    ("n2500", 2500, 10, 6, 16, "plain", (12, 60)),        # many tiles; padded strides
    ("n97_equal_attrs", 97, 4, 3, 17, "equal", (0, 0)),   # pairs = 0, ar_loss = 0, tau undefined
    ("n97_const_channel", 97, 5, 3, 18, "const", (0, 0)), # one constant channel; channels[1] = -1
]


def make_case(name, n, l, na, seed, kind="plain"):
    """Seeded inputs: attributes are integers 0..39, z is rounded to 0.1, a tenth of the rows are copies of other rows."""
    rng = np.random.default_rng(seed)
    z = np.round(rng.normal(0.0, 1.0, (n, l)), 1).astype(np.float32)
    attrs = rng.integers(0, 40, (na, n)).astype(np.float32)
    if n == 2:
        attrs[:, 1] = attrs[:, 0] + 3.0        # the one pair must qualify
        z[1] = z[0] - 0.5
    for k in range(n // 10):                   # duplicated rows: both-tied pairs
        src, dst = rng.integers(0, n, 2)
        z[dst], attrs[:, dst] = z[src], attrs[:, src]
    channels = np.array([(3 * q + 1) % l for q in range(na)], np.int32)
    deltas = rng.uniform(0.5, 2.0, na).astype(np.float32)
    if kind == "equal":
        attrs[:] = 7.0
    if kind == "const":
        z[:, 2] = 0.3
        channels[:3] = (2, -1, 4)
    return SimpleNamespace(name=name, n=n, l=l, na=na, z=z, attrs=attrs, channels=channels, deltas=deltas)


def all_cases():
    return [make_case(*spec[:6]) for spec in CASES]


def _pairs(n, ordered):
    if ordered:
        i, j = np.nonzero(~np.eye(n, dtype=bool))
        return i, j
    return np.triu_indices(n, 1)


def report(z, attrs, channels, deltas, *, ordered=False, z_ties_concordant=False, flip_sign=False, mean_over_all=False,
           tau_a=False):
    """-> dict: counts int64 [na, L, 5], loss_sum / ar_loss fp64 [na], pairs int64 [na, L], concordance / kendall_tau_b
    fp64 [na, L] (NaN where undefined).  The keyword switches are the mutations; all False is the definition."""
    z = np.asarray(z, np.float32)
    attrs = np.asarray(attrs, np.float32)
    n, l = z.shape
    na = attrs.shape[0]
    i, j = _pairs(n, ordered)
    sa = np.sign(attrs[:, j].astype(np.float64) - attrs[:, i].astype(np.float64)).astype(np.int8)   # [na, P]
    if flip_sign:
        sa = -sa
    sz = np.sign(z[j].astype(np.float64) - z[i].astype(np.float64)).astype(np.int8).T                # [L, P]
    counts = np.zeros((na, l, 5), np.int64)
    for q in range(na):
        a_ne = sa[q] != 0
        for c in range(l):
            z_ne = sz[c] != 0
            both = a_ne & z_ne
            conc = int((both & (sa[q] == sz[c])).sum())
            disc = int(both.sum()) - conc
            z_t = int((a_ne & ~z_ne).sum())
            if z_ties_concordant:
                conc, z_t = conc + z_t, 0
            counts[q, c] = (conc, disc, z_t, int((~a_ne & z_ne).sum()), int((~a_ne & ~z_ne).sum()))
    loss_sum = np.zeros(na, np.float64)
    for q in range(na):
        ch = int(channels[q])
        if ch < 0:
            continue
        keep = sa[q] != 0
        d = z[j, ch].astype(np.float64)[keep] - z[i, ch].astype(np.float64)[keep]
        e = np.tanh(np.float64(np.float32(deltas[q])) * d) - sa[q][keep].astype(np.float64)
        loss_sum[q] = float(np.sum(e * e))
    conc, disc, z_t, a_t = (counts[..., k].astype(np.float64) for k in range(4))
    pairs = counts[..., 0] + counts[..., 1] + counts[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        concordance = conc / pairs
        den = np.sqrt((conc + disc + z_t) * (conc + disc + a_t))
        if tau_a:
            den = counts.sum(-1).astype(np.float64)
        tau = np.where(den > 0, (conc - disc) / den, np.nan)
        denom = counts.sum(-1)[:, 0] if mean_over_all else pairs[:, 0]
        ar_loss = np.where(denom > 0, loss_sum / np.maximum(denom, 1), 0.0)
    return dict(counts=counts, loss_sum=loss_sum, ar_loss=ar_loss, pairs=pairs, concordance=concordance, kendall_tau_b=tau)


def ar_loss_fp32(z, attrs, channels, deltas):
    """The same mean with every value and every sum in fp32 (numpy's pairwise ``sum``): a straightforward restatement."""
    z = np.asarray(z, np.float32)
    attrs = np.asarray(attrs, np.float32)
    i, j = np.triu_indices(z.shape[0], 1)
    out = np.zeros(attrs.shape[0], np.float32)
    for q in range(attrs.shape[0]):
        ch = int(channels[q])
        s = np.sign(attrs[q, j] - attrs[q, i]).astype(np.float32)
        keep = s != 0
        if ch < 0 or not keep.any():
            continue
        e = np.tanh(np.float32(deltas[q]) * (z[j, ch][keep] - z[i, ch][keep])) - s[keep]
        out[q] = np.sum(e * e, dtype=np.float32) / np.float32(keep.sum())
    return out


def gate_of(ar64, ar32):
    """2 x the largest deviation of the fp32 restatement, relative to the case's largest fp64 value (0 for an all-zero case)."""
    top = float(np.max(np.abs(ar64)))
    return 0.0 if top == 0.0 else 2.0 * float(np.max(np.abs(ar32.astype(np.float64) - ar64))) / top


def loss_deviation(got, ar64):
    top = float(np.max(np.abs(ar64)))
    dev = float(np.max(np.abs(np.asarray(got, np.float64) - ar64)))
    return dev if top == 0.0 else dev / top


def load_golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def main():
    out = {}
    for case in all_cases():
        r = report(case.z, case.attrs, case.channels, case.deltas)
        gate = gate_of(r["ar_loss"], ar_loss_fp32(case.z, case.attrs, case.channels, case.deltas))
        out[f"{case.name}/counts"] = r["counts"]
        out[f"{case.name}/ar_loss"] = r["ar_loss"]
        out[f"{case.name}/gate"] = np.float64(gate)
        print(f"{case.name}: pairs {case.n * (case.n - 1) // 2} ar_loss max {r['ar_loss'].max():.6f} gate {gate:.3e}")
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()

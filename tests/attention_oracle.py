"""Float64 references and exact structured inputs for the flash-style attention kernels (csrc/attention.hip):
tests/test_gpu_attention.py compares the kernels with what is built here, tests/test_attention_cpu.py shows on the CPU
that every expected value below follows from ``reference`` alone.

Method (as tests/exact_util.py for the convs).  With random inputs one key of 4096 carries 1/4096 of a query's mass and a
dropped 64-key tile stays under any tolerance a bf16 kernel can be held to.  The builders here choose inputs for which the
right answer is EXACT, so a wrong index, a dropped or repeated key, a leaked pad row or a missed rescale is a bit
difference:

  ``onehot_case``   q_i = 128 * code of key pi(i): the winning score leads by >= 184 log2 units, every other probability
                    underflows to 0 in fp32, P is a permutation-like 0/1 matrix: o = v[pi], dq = dk = 0, dv = scatter(do).
  ``pair_case``     two keys (first and last streamed tile) carry the same code: P = 1/2, 1/2 across two tiles.
  ``uniform_case``  q = 0: every score is 0, P = 1/L; only the masks keep the zero-filled pad rows out; integer sums.

All tensors are float64 on the CPU and bf16-representable where the kernel takes bf16.  ``qkv`` is [B, L, 3C] (q | k | v),
``dout`` [B, L, C].  The kernel contract that the closed forms rely on: scores are q.k * fp32(C^-1/2) in fp32, P and dS are
rounded to bf16 (nearest even) before their MFMA products, fp32 accumulation, one bf16 rounding of o / dq / dk / dv, lse2 =
running max + log2(row sum) in log2 units, delta = sum_d do * o from the bf16 o.
"""
import math
from types import SimpleNamespace

import torch

F64 = torch.float64
LOG2E = 1.4426950408889634

# ---- the case lists shared by the CPU and the GPU file -----------------------------------------------------------------
C_LIST = (64, 128, 256)
ONEHOT_L = (1, 31, 33, 64, 65, 127, 128, 129, 191, 257, 1000)
ONEHOT_BIG = ((1, 4096, 256), (2, 4096, 128))            # random permutation and all -> L-1 only (the reference is a gather)
POW2_L = (64, 128, 256, 1024, 4096)                      # pair / uniform: exact throughout
RAGGED_L = (7, 117, 129, 1000)                           # pair / uniform: dq and dv of the uniform case are bounded
GRID_STRIDE = {256: 129, 128: 257, 64: 513}              # C -> smallest B whose B * 256 rows exceed 4096 blocks of 256 / (C / 8)
ROW_L = (1, 33, 65, 129, 191, 257)
ROW_KINDS = ("randn", "spike_key", "spike_query", "large_logit")
EXTENT_CASES = ((1, 64), (129, 128), (40, 256), (257, 256))
PI_FAMILIES = ("identity", "reversal", "random", "all_first", "all_last", "halved")
MARGIN_LOG2 = 150.0            # exp2(-150) is below the smallest fp32 denormal (2^-149): a losing probability is exactly 0

# ---- the row-wise bounds of test_attention_rowwise_vs_fp64 -------------------------------------------------------------
# CONTRACT_DEV[kind][t]: the largest row-wise deviation (``rowwise_err``) of ``contract`` from ``reference`` over the
# ROW_L x C_LIST inputs of that kind at B = 2, i.e. how far the documented bf16 roundings alone move tensor t (measured
# values rounded up by 2 %).  tests/test_attention_cpu.py::test_contract_deviation_matches_constants measures them again
# and fails when they drift.  The kernel is held to 3 x that: fp32 accumulation order and the hardware exp2 / log2 are far
# below one bf16 rounding.  They are kept per kind of input, so that the well-conditioned kinds are not measured against
# the worst one (the largest over the four kinds would be the one bound per tensor; no kind's is wider than that).
# dq under ``spike_key`` and dq / dk under ``large_logit`` are of order 10: where one key takes nearly all of a query's
# mass, dS = P (dP - delta) cancels to ~0 in float64, while delta from the bf16 o leaves 2^-9 |do.o| behind, times |k|;
# that row's dq is then 10^-3 of the tensor's median and the floor of ``rowwise_err`` does not reach it.  The row-wise
# metric says little there; the exact one-hot cases cover that regime.
CONTRACT_DEV = {
    "randn":       {"o": 5.29e-3, "dq": 6.40e-3, "dk": 6.07e-3, "dv": 5.79e-3},
    "spike_key":   {"o": 5.18e-3, "dq": 34.3,    "dk": 1.54e-2, "dv": 5.62e-3},
    "spike_query": {"o": 5.29e-3, "dq": 1.25e-2, "dk": 1.19e-2, "dv": 5.75e-3},
    "large_logit": {"o": 4.64e-3, "dq": 32.6,    "dk": 6.95,    "dv": 6.21e-3},
}
ROW_BOUND = {kind: {k: 3.0 * v for k, v in d.items()} for kind, d in CONTRACT_DEV.items()}
LSE_RTOL = LSE_ATOL = 1e-5
DELTA_RTOL = 1e-5              # of sum_d |do * o|
ONEHOT_LSE_RTOL = 2.0 ** -22   # one fp32 rounding of log2(e) C^-1/2 and the exact product with 128 C
# The uniform case at an L that is no power of two (p = 1 / L rounds).  dq_i = sum_j bf16(dS_ij) k_j rounded to bf16: two
# bf16 roundings, taken as 2^-9 relative each (the half ulp of a full mantissa), 2^-8 together, and a factor 2 for fp32
# accumulation: 2^-7 of the row's largest |dq|.  dv_j = bf16(bf16(p) * sum_i do_i) with an exact integer sum: the two
# roundings are at most 2^-8 relative each (the half ulp of a mantissa of 1.0) on every ELEMENT, (1 + 2^-8)^2 - 1 plus the
# 2^-21 of the hardware exp2 / log2 behind p: 2^-7 (1 + 2^-7) of |dv_j| itself, which is tighter than a row bound.
UNIFORM_DQ_ROW_RTOL = 2.0 ** -7
UNIFORM_DV_RTOL = 2.0 ** -7 * (1.0 + 2.0 ** -7)


def round_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64.  (A cast through torch.bfloat16 rounds twice.)"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def is_bf16(x):
    return bool((round_bf16(x) == x).all())


def split(qkv):
    c = qkv.shape[-1] // 3
    return qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]


def delta_of(o_bf16, dout):
    """sum_d do * o in float64 from the bf16 o that the backward was handed -> [B, L]."""
    return (o_bf16.to(F64) * dout.to(F64)).sum(-1)


# ---- references --------------------------------------------------------------------------------------------------------
def reference(qkv, dout):
    """The materialised float64 softmax(q k^T C^-1/2) v and its gradients in closed form -> o, lse2 (log2 units), dq, dk,
    dv, delta (from the float64 o) and ``delta_of(o_bf16)`` for the o that a kernel produced."""
    qkv, dout = qkv.to(F64), dout.to(F64)
    q, k, v = split(qkv)
    scale = q.shape[-1] ** -0.5
    s = torch.einsum("blc,bmc->blm", q, k) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    delta = (o * dout).sum(-1)
    ds = p * (dout @ v.transpose(1, 2) - delta[..., None]) * scale
    return SimpleNamespace(o=o, lse2=lse * LOG2E, dq=ds @ k, dk=ds.transpose(1, 2) @ q, dv=p.transpose(1, 2) @ dout,
                           delta=delta, delta_of=lambda o_bf16: delta_of(o_bf16, dout))


def contract(qkv, dout):
    """``reference`` with the roundings the kernel documents and float64 everywhere else: P rounded to bf16 before P.V
    with the row sum taken from the unrounded P; in the backward P and dS rounded to bf16 before their products and delta
    taken from the bf16 o; o and the gradients rounded once.  Only for measuring how far those roundings move a result
    (CONTRACT_DEV); never what a kernel is compared with."""
    qkv, dout = qkv.to(F64), dout.to(F64)
    q, k, v = split(qkv)
    scale = q.shape[-1] ** -0.5
    s2 = torch.einsum("blc,bmc->blm", q, k) * (scale * LOG2E)
    m = s2.max(-1, keepdim=True).values
    p = torch.exp2(s2 - m)
    lsum = p.sum(-1, keepdim=True)
    o = round_bf16(round_bf16(p) @ v / lsum)
    lse2 = m + torch.log2(lsum)
    pb = torch.exp2(s2 - lse2)
    delta = (o * dout).sum(-1)
    ds = round_bf16(pb * (dout @ v.transpose(1, 2) - delta[..., None]) * scale)
    return SimpleNamespace(o=o, lse2=lse2[..., 0], dq=round_bf16(ds @ k), dk=round_bf16(ds.transpose(1, 2) @ q),
                           dv=round_bf16(round_bf16(pb).transpose(1, 2) @ dout), delta=delta)


def rowwise_err(got, ref):
    """Per token row: max_d |got - ref| over max_d |ref| of that row, the denominator floored at 2^-8 of the tensor's
    median row maximum (near-zero rows) -> [B, L] float64.  A NaN in ``got`` gives inf."""
    got, ref = got.to(F64), ref.to(F64)
    rmax = ref.abs().amax(-1)
    floor = 2.0 ** -8 * rmax.median()
    err = (got - ref).abs().amax(-1) / torch.maximum(rmax, floor).clamp_min(1e-300)
    return torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)


# ---- fp32 emulation of the streamed algorithm (CPU test only) ----------------------------------------------------------
def scale_f32(c):
    return torch.tensor(c ** -0.5, dtype=torch.float32)


def c_log2_f32(c):
    return torch.tensor(LOG2E * c ** -0.5, dtype=torch.float32)


def stream_fwd_fp32(qkv, tile=64):
    """The forward as the kernel streams it, in fp32: key tiles of ``tile`` rows zero-filled past L and masked with -1e30,
    running maximum, ``alpha = exp2(m - m_new)`` rescale, P rounded to bf16 before P.V, row sum from the unrounded P
    -> o (bf16 values), lse2 (fp32), both as float64."""
    f32 = torch.float32
    q, k, v = (t.to(f32) for t in split(qkv))
    b, l, c = q.shape
    cl2 = c_log2_f32(c)
    m = torch.full((b, l), -1e30, dtype=f32)
    lsum = torch.zeros(b, l, dtype=f32)
    oacc = torch.zeros(b, l, c, dtype=f32)
    for k0 in range(0, l, tile):
        kt, vt = torch.zeros(b, tile, c, dtype=f32), torch.zeros(b, tile, c, dtype=f32)
        n = min(tile, l - k0)
        kt[:, :n], vt[:, :n] = k[:, k0:k0 + n], v[:, k0:k0 + n]
        s = torch.einsum("blc,bmc->blm", q, kt) * cl2
        s[:, :, n:] = -1e30
        mn = torch.maximum(m, s.amax(-1))
        alpha = torch.exp2(m - mn)
        p = torch.exp2(s - mn[..., None])
        lsum = lsum * alpha + p.sum(-1)
        oacc = oacc * alpha[..., None] + p.to(torch.bfloat16).to(f32) @ vt
        m = mn
    o = (oacc * (1.0 / lsum)[..., None]).to(torch.bfloat16)
    return o.to(F64), (m + torch.log2(lsum)).to(F64)


def bwd_fp32(qkv, dout, o_bf16, lse2):
    """The backward in fp32 with the kernel's roundings (not streamed: every sum it forms is exact on the structured
    inputs) -> dq, dk, dv (bf16 values), delta, as float64."""
    f32 = torch.float32
    q, k, v = (t.to(f32) for t in split(qkv))
    do, c = dout.to(f32), q.shape[-1]
    delta = (o_bf16.to(f32) * do).sum(-1)
    p = torch.exp2(torch.einsum("blc,bmc->blm", q, k) * c_log2_f32(c) - lse2.to(f32)[..., None])
    ds = (p * (do @ v.transpose(1, 2) - delta[..., None]) * scale_f32(c)).to(torch.bfloat16).to(f32)
    pb = p.to(torch.bfloat16).to(f32)
    r = lambda t: t.to(torch.bfloat16).to(F64)
    return r(ds @ k), r(ds.transpose(1, 2) @ q), r(pb.transpose(1, 2) @ do), delta.to(F64)


# ---- builders ----------------------------------------------------------------------------------------------------------
def _ints(gen, shape):
    return torch.randint(-4, 5, tuple(shape), generator=gen).to(F64)


def codes(L, C):
    """k_j[d] = +1 if bit (d mod 16) of j is set, else -1 -> [L, C].  Distinct j < 65536 differ in >= C/16 coordinates."""
    assert L <= 65536 and C % 16 == 0
    j, d = torch.arange(L).view(L, 1), torch.arange(C).view(1, C) % 16
    return (((j >> d) & 1) * 2 - 1).to(F64)


def pi_family(name, B, L, seed=0):
    """-> int64 [B, L]: the key that each query selects."""
    i = torch.arange(L)
    if name == "identity":
        pi = i
    elif name == "reversal":
        pi = L - 1 - i
    elif name == "random":        # a different permutation for each image
        return torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(7919 * seed + b + 1)) for b in range(B)])
    elif name == "all_first":
        pi = torch.zeros_like(i)
    elif name == "all_last":      # the key next to the masked tail: the running maximum arrives in the last tile
        pi = torch.full_like(i, L - 1)
    elif name == "halved":
        pi = i // 2
    else:
        raise ValueError(name)
    return pi.expand(B, L).contiguous()


def pi_families(B, L, names=PI_FAMILIES):
    """(name, pi) of every family that L admits: one that coincides with an earlier one (L = 1, 2) is left out."""
    out = []
    for name in names:
        pi = pi_family(name, B, L)
        if not any(torch.equal(pi, p) for _, p in out):
            out.append((name, pi))
    return out


def winning_score_log2(C):
    return 128.0 * math.sqrt(C) * LOG2E


def _case(kind, qkv, dout, **kw):
    assert is_bf16(qkv) and is_bf16(dout), f"{kind}: inputs are not bf16-representable"
    return SimpleNamespace(kind=kind, qkv=qkv, dout=dout, **kw)


def onehot_case(B, L, C, pi, seed=0):
    """q_i = 128 * k_{pi[b][i]}; v, dout random integers in [-4, 4].  Exact: o_i = v_{pi(i)}, dq = dk = 0, dv_j = the sum of
    do_i over the queries that select j (rounded once to bf16), delta_i = do_i . v_{pi(i)}; lse2 = 128 C^1/2 log2(e)."""
    gen = torch.Generator().manual_seed(100 + seed)
    k = codes(L, C)
    v, dout = _ints(gen, (B, L, C)), _ints(gen, (B, L, C))
    qkv = torch.cat([128.0 * k[pi], k.expand(B, L, C), v], -1)
    idx = pi[..., None].expand(B, L, C)
    o = torch.gather(v, 1, idx)
    dv_sum = torch.zeros(B, L, C, dtype=F64).scatter_add_(1, idx, dout)
    zero = torch.zeros(B, L, C, dtype=F64)
    return _case("onehot", qkv, dout, o=o, lse2=torch.full((B, L), winning_score_log2(C), dtype=F64), dq=zero, dk=zero,
                 dv=round_bf16(dv_sum), dv_sum=dv_sum, delta=(o * dout).sum(-1), pi=pi)


def pair_case(B, L, C, a, b, seed=0):
    """Key b carries key a's code and every query selects it: P = 1/2 at a and at b.  Exact: o = (v_a + v_b) / 2, lse2 =
    the winning score + 1, delta, dq = 0 (dS_b = -dS_a bit for bit and k_b = k_a), dv_a = dv_b = (sum_i do_i) / 2, every
    other row of dk and dv 0, dk_b = -dk_a.  dk_a = sum_i bf16(dS_ia) q_i is given unrounded in float64 with ``dk_abs`` =
    sum_i |dS_ia q_i|, the scale of its rounding error."""
    assert 0 <= a < b < L
    gen = torch.Generator().manual_seed(200 + seed)
    k = codes(L, C)
    k[b] = k[a]
    v, dout = _ints(gen, (B, L, C)), _ints(gen, (B, L, C))
    qkv = torch.cat([(128.0 * k[a]).expand(B, L, C), k.expand(B, L, C), v], -1)
    o = ((v[:, a] + v[:, b]) / 2)[:, None].expand(B, L, C).contiguous()
    delta = (o * dout).sum(-1)
    dv = torch.zeros(B, L, C, dtype=F64)
    dv[:, a] = dv[:, b] = round_bf16(dout.sum(1) / 2)
    ds_a = 0.5 * (dout @ v[:, a, :, None])[..., 0].sub(delta) * C ** -0.5            # [B, L]: dS_ia; dS_ib = -dS_ia
    dk = torch.zeros(B, L, C, dtype=F64)
    dk[:, a] = ds_a.sum(1)[:, None] * 128.0 * k[a]
    dk[:, b] = -dk[:, a]
    return _case("pair", qkv, dout, o=o, lse2=torch.full((B, L), winning_score_log2(C) + 1.0, dtype=F64),
                 dq=torch.zeros(B, L, C, dtype=F64), dk=dk, dk_abs=ds_a.abs().sum(1) * 128.0, dv=dv, dv_sum=dout.sum(1),
                 delta=delta, a=a, b=b)


def uniform_v(L, C):
    j, d = torch.arange(L).view(L, 1), torch.arange(C).view(1, C)
    return (1 + (j + d) % 3).to(F64)


def uniform_o(L, C, inv_ulps=0):
    """bf16(fp32(sum_j v_j) * inv) per column with inv = fp32(1 / L) moved by ``inv_ulps`` ulps -> [C] float64."""
    colsum = uniform_v(L, C).sum(0)
    assert colsum.max().item() < 2 ** 24
    inv = torch.tensor(1.0 / L, dtype=torch.float32)
    for _ in range(abs(inv_ulps)):
        inv = torch.nextafter(inv, torch.tensor(math.inf if inv_ulps > 0 else -math.inf, dtype=torch.float32))
    return round_bf16((colsum.to(torch.float32) * inv).to(F64))


def is_pow2(n):
    return n & (n - 1) == 0


SHIFT_Q0, SHIFT_K0 = -512.0, 4.0     # shifted uniform case: every score is -2048 C^-1/2 log2(e) = -369 / -261 / -185 log2 units


def uniform_case(B, L, C, seed=0, shift=False):
    """q = 0; k, dout random integers in [-4, 4]; v[j][d] = 1 + ((j + d) mod 3).  Every score is 0, a zero-filled pad
    row's too.  Exact: lsum = L, lse2 = log2 L, o = bf16(fp32(sum_j v_j) * fp32(1 / L)), delta (from that o), dk = 0.  At a
    power-of-two L the backward's p = 1 / L is exact, and so are dv = bf16((sum_i do_i) / L) and dq (below); at other L
    ``dq`` / ``dv`` are None and the kernel is compared with ``reference``.

    ``shift`` (ragged L): coordinate 0 of every query is -512 and of every key 4, so every score is the same -2048 (a power
    of two: its fp32 product with log2(e) C^-1/2 is exact) and lse2 is below -128.  The softmax, o, delta and dv do not move.
    A zero-filled pad KEY still scores 0, so in the backward its p = exp2(0 - lse2) overflows to inf, and only the ragged-key
    mask of the dq kernel keeps inf * 0 = NaN out of dq.  dq and dk (column 0 of dk is no longer 0) come as the float64 sums
    ``dq_f64`` / ``dk_f64`` over dS = (do.v - delta) C^-1/2 / L with delta from the bf16 o, as the kernel is handed it, and
    ``dq_abs`` / ``dk_abs``, the sums of |terms|: the kernel's two bf16 roundings move each element by at most 2^-8 of
    both."""
    gen = torch.Generator().manual_seed(300 + seed)
    k, dout = _ints(gen, (B, L, C)), _ints(gen, (B, L, C))
    v = uniform_v(L, C)
    q = torch.zeros(B, L, C, dtype=F64)
    lse2 = math.log2(L)
    if shift:
        q[..., 0], k[..., 0] = SHIFT_Q0, SHIFT_K0
        lse2 += SHIFT_Q0 * SHIFT_K0 * c_log2_f32(C).to(F64).item()
    qkv = torch.cat([q, k, v.expand(B, L, C)], -1)
    o = uniform_o(L, C).expand(B, L, C).contiguous()
    delta = (o * dout).sum(-1)
    case = _case("uniform", qkv, dout, o=o, lse2=torch.full((B, L), lse2, dtype=F64), delta=delta,
                 dk=None if shift else torch.zeros(B, L, C, dtype=F64), dq=None, dv=None, dv_sum=dout.sum(1),
                 dq_proven=None, shift=shift)
    if shift:
        assert not is_pow2(L)
        ds = (dout @ v.t() - delta[..., None]) * (C ** -0.5 / L)
        case.dq_f64, case.dq_abs = ds @ k, ds.abs() @ k.abs()
        case.dk_f64, case.dk_abs = ds.transpose(1, 2) @ q, ds.abs().transpose(1, 2) @ q.abs()
        return case
    if is_pow2(L):
        case.dv = round_bf16(dout.sum(1) / L)[:, None].expand(B, L, C).contiguous()
        # dq_i = sum_j bf16(dS_ij) k_j.  v_j depends on j mod 3 only, so dS_ij = dS_i,(j mod 3): three values per query,
        # each ONE fp32 rounding (of the product with fp32(C^-1/2); 1 / L is a power of two) and one bf16 rounding.
        x = dout @ v[:3].t() - delta[..., None]                                       # [B, L, 3], exact
        ds = round_bf16(((x.to(torch.float32) * scale_f32(C)) * torch.tensor(1.0 / L, dtype=torch.float32)).to(F64))
        kr = torch.stack([k[:, r::3].sum(1) for r in range(3)], 1)                    # [B, 3, C]
        case.dq = round_bf16(torch.einsum("blr,brc->blc", ds, kr))
        # Rows for which the fp32 sum is PROVEN exact: every term is a multiple of the row's grid g (the lowest set bit of
        # its three dS values; k is integer), and every partial sum the kernel can form -- a prefix of the keys in 16-key
        # MFMA steps plus the 16 products in flight -- stays below 2^24 g.
        kpre = torch.stack([torch.cumsum(torch.where((torch.arange(L) % 3 == r).view(1, L, 1), k, torch.zeros(())), 1)
                            .abs().amax(1) for r in range(3)], 1)                     # [B, 3, C]: max_n |prefix|
        bound = torch.einsum("blr,brc->blc", ds.abs(), kpre + 24.0).amax(-1)          # 6 keys of a residue in flight, |k| <= 4
        m, e = torch.frexp(ds)
        mi = (m.abs() * 256.0).to(torch.int64)
        low = torch.where(mi == 0, torch.full_like(m, math.inf), torch.ldexp((mi & -mi).to(F64), e - 8))
        case.dq_proven = bound < 2.0 ** 24 * low.amin(-1)                              # [B, L] bool
    return case


def rowwise_case(kind, B, L, C, seed=0):
    """The inputs of test_attention_rowwise_vs_fp64: ``randn``; the existing test's two spikes one at a time (key row L-3
    times 6: the running maximum jumps late in the stream; query row 5 times 4); ``large_logit``."""
    if kind == "large_logit":
        return large_logit_case(B, L, C, seed)
    gen = torch.Generator().manual_seed(400 + seed)
    qkv = torch.randn(B, L, 3 * C, generator=gen, dtype=F64)
    dout = round_bf16(torch.randn(B, L, C, generator=gen, dtype=F64))
    if kind == "spike_key":
        qkv[:, max(L - 3, 0), C:2 * C] *= 6.0
    elif kind == "spike_query":
        qkv[:, min(5, L - 1), :C] *= 4.0
    elif kind != "randn":
        raise ValueError(kind)
    return _case(kind, round_bf16(qkv), dout)


def large_logit_case(B, L, C, seed=0):
    """randn with q and k scaled by 15^1/2 each: the scores q.k C^-1/2 then have standard deviation 15 natural units and
    their extremes over a few 10^4 pairs (4 sigma) reach +-60, the logit scale of a trained network.  Rounded to bf16
    after scaling."""
    gen = torch.Generator().manual_seed(500 + seed)
    qkv = torch.randn(B, L, 3 * C, generator=gen, dtype=F64)
    qkv[..., :2 * C] *= 15.0 ** 0.5
    return _case("large_logit", round_bf16(qkv), round_bf16(torch.randn(B, L, C, generator=gen, dtype=F64)))

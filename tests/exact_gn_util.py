"""Exact parity cases for the kernels that CONSUME GroupNorm statistics (tests/test_gpu_exact_groupnorm.py; every case and
condition is also built and checked on the CPU by tests/test_exact_gn_util_cpu.py).  Companion of tests/exact_util.py.

Method.  Every such kernel takes the Q47.16 ``{sum, sumsq}`` table per (sample, group) as an INPUT, so a test writes it by
hand: ``sum = cnt * m`` with an integer m and ``sumsq = cnt * (m^2 + v)`` with ``v + eps`` a power of four.  With ``cnt`` a
power of two the kernel's ``mean = sum / cnt`` is m and ``var + eps`` is 4^k exactly in fp32, so ``rstd = 2^-k`` -- given that
the hardware reciprocal square root is exact there, which the GPU file's probe measures per kernel family.  The table need
not be the statistics of the tensor it is used with: the kernels evaluate formulas of (x, table), and so does the reference.
With integer x, dy, dres, gamma in {0, +-1/2, +-1, +-2, 4} and small integer beta every fp32 intermediate of

    a  = (x - m) * rstd * gamma + beta                     (kernels: x * sc + sh, sc = rstd * gamma, sh = beta - m * sc)
    S1 = sum dy,  S2 = sum dy * xhat,  xhat = (x - m) * rstd
    c1 = sum_group(gamma * S1) / cnt,  c2 = sum_group(gamma * S2) / cnt
    dx = rstd * (gamma * dy - c1 - xhat * c2) + dres,  dgamma = sum_n S2,  dbeta = sum_n S1

(the formulas of csrc/groupnorm.hip's header comment) is a multiple of a power-of-two unit u with magnitude below 2^24 u.
``exact_sum`` asserts that for every sum: all terms multiples of u, sum |terms| < 2^24 u -- then every partial sum in ANY
order, with or without FMA contraction or re-association, is exact.  The only rounding left is the final 16-bit store of an
exactly known value: one round-to-nearest-even, which torch reproduces (``round16``).

Two regimes, asserted when a case is built:
  * power-of-two count (cpg * H * W = 2^k): varying integer means and rstd per (sample, group) (neighbouring groups and
    neighbouring samples differ), non-zero c1 and c2 for every (sample, group).
  * ragged (H * W not a power of two): 1 / cnt is inexact, so everything multiplied by it must be zero: the table is all
    zero (mean 0, rstd = rsq(eps)) and dy is built so that every group's gamma-weighted S1 and S2 cancel -- channel pairs
    (2j, 2j+1) of a group share gamma and x and carry opposite dy; with one channel per group, pixel pairs do.  Each
    channel's own sums, hence dgamma / dbeta, stay non-zero where a group has >= 2 channels.  Any leak (a masked tail lane,
    a neighbouring sample, a padding pixel) makes c1 / c2 non-zero and breaks every element of the group.

Conditions (assertions, on the reference alone): the sum condition above; every MFMA operand representable in its 16-bit
type; every conv result that is stored in 16 bits and consumed again (dy_out of the fused epilogue) an integer <= 256; at
most 25 % of any expected output zero; for backward cases at least half of the dx elements change when rounded to bf16 (in
the ragged regime only with ``dres``: there dx = rstd * gamma * dy is a bf16 value times a power of two, which never rounds;
the residual is large -- multiples of 8 up to 512 -- so that the sum does).

Plain torch on the CPU, float64 throughout, NCHW.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import exact_util as E
from exact_util import F64, LIMIT32, STAT_SCALE, check_sum32, ints, ternary

MAX_ZERO = 0.25
MIN_ROUNDED = 0.5
GAMMAS = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0)          # and one 0 in every 32 channels
# the chained launch rounds the applied gradient to bf16 and convolves it: its smallest magnitude sets the unit of every
# later sum, so the chained GroupNorm's |gamma| is >= 1 (with gamma = 0, dx = -rstd * (c1 + xhat * c2): ~2^-8)
CHAIN_GAMMAS = (1.0, -1.0, 2.0, -2.0)
B16, H16, F32 = torch.bfloat16, torch.float16, torch.float32


# ---- statistics --------------------------------------------------------------------------------------------------------
def stat_f(table):
    """What the kernels' ``stat_f`` makes of a Q47.16 value, in fp32: float(high half) * 65536 + float(low half) / 65536."""
    hi = (table >> 32).to(F32)                                   # arithmetic shift: the signed high half
    lo = (table & 0xFFFFFFFF).to(F32)
    return hi * 65536.0 + lo * (1.0 / 65536.0)


def make_gn_stats(n, groups, cnt, means, variances):
    """int64 [n, groups, 2] Q47.16 {cnt * m, cnt * (m^2 + v)}.  Asserts that both 32-bit halves of every entry convert to
    fp32 exactly and that ``stat_f`` gives the exact value."""
    means = torch.as_tensor(means, dtype=F64).expand(n, groups)
    variances = torch.as_tensor(variances, dtype=F64).expand(n, groups)
    val = torch.stack([cnt * means, cnt * (means * means + variances)], -1)
    q = val * STAT_SCALE
    assert bool((q == q.round()).all()), "make_gn_stats: a sum is no multiple of 2^-16"
    table = q.round().to(torch.int64)
    for half, nm in (((table >> 32), "high"), ((table & 0xFFFFFFFF), "low")):
        assert bool((half.to(F32).to(torch.int64) == half).all()), f"make_gn_stats: a {nm} half does not convert to fp32 exactly"
    assert bool((stat_f(table).to(F64) == val).all()), "make_gn_stats: stat_f does not reproduce the value"
    return table


# ---- conditions --------------------------------------------------------------------------------------------------------
def check_f32(name, t):
    assert bool((t.to(F32).to(F64) == t).all()), f"{name}: not representable in fp32"


def check_repr16(name, t, dtype):
    assert bool((t.to(F32).to(dtype).to(F64) == t).all()), f"{name}: not representable in {dtype}"


def exact_sum(name, terms, unit, dim=None):
    """Every term a multiple of ``unit`` (a power of two; a tensor broadcasts) and sum |terms| < 2^24 unit, where the sum
    runs over the list and, with ``dim``, over those dimensions of every term."""
    unit = torch.as_tensor(unit, dtype=F64)
    total = 0
    for t in terms:
        k = t / unit
        assert bool((k == k.round()).all()), f"{name}: a term is no multiple of the unit"
        a = k.abs()
        total = total + (a.sum(dim, keepdim=True) if dim is not None else a)
    m = float(torch.as_tensor(total).max())
    assert m < LIMIT32, f"{name}: sum |terms| = {m:g} units >= 2^24: an fp32 partial sum could round"
    return m


def check_zero(name, t):
    z = (t == 0).to(F64).mean().item()
    assert z <= MAX_ZERO, f"{name}: {z:.3f} of the reference is zero"
    return z


def round16(t, dtype=B16):
    """The one rounding of a 16-bit store: the value is fp32-exact (asserted), then round-to-nearest-even."""
    check_f32("value before the 16-bit store", t)
    return t.to(F32).to(dtype).to(F64)


def rounded_share(t, dtype=B16):
    return (round16(t, dtype) != t).to(F64).mean().item()


# ---- parameters --------------------------------------------------------------------------------------------------------
def affine(gen, c, cpg, paired=False, gammas=None):
    """gamma [c] from GAMMAS with one 0 in every 32 channels, beta [c] integer in [-2, 2].  ``paired``: channels 2j and
    2j+1 share gamma (the ragged regime's cancelling pairs)."""
    idx = torch.randint(0, len(gammas or GAMMAS), (c,), generator=gen)
    gamma = torch.tensor(gammas or GAMMAS, dtype=F64)[idx]
    if gammas is None:
        gamma[torch.arange(5, c, 32)] = 0.0
    if paired and cpg >= 2:
        gamma[1::2] = gamma[0::2]
    beta = ints(gen, (c,), -2, 2)
    return gamma, beta


def group_table(n, groups, rstds):
    """Integer means in [-3, 3] and rstd from ``rstds`` per (sample, group), neighbours differing in both directions."""
    i, g = torch.meshgrid(torch.arange(n), torch.arange(groups), indexing="ij")
    mean = ((3 * g + 5 * i) % 7 - 3).to(F64)
    rstd = torch.tensor(rstds, dtype=F64)[(g + 2 * i) % len(rstds)] if len(rstds) > 1 else torch.full((n, groups), float(rstds[0]), dtype=F64)
    if groups > 1:
        assert bool((mean[:, 1:] != mean[:, :-1]).all())
        assert len(rstds) == 1 or bool((rstd[:, 1:] != rstd[:, :-1]).all())
    if n > 1:
        assert bool((mean[1:] != mean[:-1]).all())
    return mean, rstd


def _per_channel(t, cpg):
    """[n, groups] -> [n, c, 1, 1]"""
    return t.repeat_interleave(cpg, 1)[:, :, None, None]


def setup(n, c, groups, h, w, rstds, seed, eps=0.25, gammas=None):
    """The statistics half of a case.  Power-of-two count: means / rstd from ``group_table``, variance = rstd^-2 - eps.
    Otherwise (ragged): an all-zero table and rstd = eps^-1/2 (eps a power of four)."""
    cpg = c // groups
    cnt = cpg * h * w
    s = SimpleNamespace(n=n, c=c, groups=groups, h=h, w_=w, cpg=cpg, cnt=cnt, pow2=(cnt & (cnt - 1)) == 0, eps=eps)
    s.gen = torch.Generator().manual_seed(4000 + seed)
    if s.pow2:
        s.mean, s.rstd = group_table(n, groups, rstds)
        var = 1.0 / (s.rstd * s.rstd) - eps
        assert bool((var >= 0).all()), "setup: eps too large for the largest rstd"
        s.stats = make_gn_stats(n, groups, cnt, s.mean, var)
        # what the kernels compute from the table, in fp32: mean and var + eps exactly
        inv = torch.tensor(1.0 / cnt, dtype=F32)
        mean32 = stat_f(s.stats[..., 0]) * inv
        ve32 = stat_f(s.stats[..., 1]) * inv - mean32 * mean32 + torch.tensor(eps, dtype=F32)
        assert bool((mean32.to(F64) == s.mean).all()) and bool((ve32.to(F64) == 1.0 / (s.rstd * s.rstd)).all())
    else:
        r = eps ** -0.5
        assert r in (0.25, 0.5, 1.0, 2.0), "setup: ragged cases need eps in {16, 4, 1, 1/4}"
        s.mean, s.rstd = torch.zeros(n, groups, dtype=F64), torch.full((n, groups), r, dtype=F64)
        s.stats = torch.zeros(n, groups, 2, dtype=torch.int64)
    s.gamma, s.beta = affine(s.gen, c, cpg, paired=not s.pow2, gammas=gammas)
    s.m4, s.r4 = _per_channel(s.mean, cpg), _per_channel(s.rstd, cpg)
    s.g4, s.b4 = s.gamma.view(1, -1, 1, 1), s.beta.view(1, -1, 1, 1)
    return s


# ---- forward affine ----------------------------------------------------------------------------------------------------
def gn_affine_ref(s, x):
    """a = (x - m) * rstd * gamma + beta in float64, with the kernels' form x * sc + sh checked exact in fp32."""
    a = (x - s.m4) * s.r4 * s.g4 + s.b4
    sc = s.r4 * s.g4
    unit = s.rstd.min().item() * 0.5
    exact_sum("forward affine", [x * sc, s.b4.expand_as(x), s.m4 * sc.expand_as(x)], unit)
    return a


def _tile_block_sum(t, tile=E.TILE, cblock=4):
    """Largest sum of a non-negative NCHW map over one (8 x 16 pixel tile, aligned channel quad): an upper bound of every
    fp32 partial sum of the fused statistics (a lane adds the quad's values of its pixels, 32 lanes are folded, and the
    result goes to the fixed-point table)."""
    th, tw = tile
    n, c, h, w = t.shape
    t = F.pad(t, (0, -w % tw, 0, -h % th))
    t = F.avg_pool2d(t, (th, tw)) * (th * tw)
    return t.reshape(n, c // cblock, cblock, -1).sum(2).max().item()


def make_prologue_case(row):
    """Forward conv on a = GN(x) (no SiLU): x (integers, NCHW), stats, gamma, beta, eps, w (ternary), bias, res ->
    a (bf16-representable: the MFMA operand and the ``act_out`` side output), conv, y = round16(conv + bias [+ res]) in
    bf16 and fp16, and the fused statistics of the ROUNDED y (what the epilogue sums) as Q47.16 int64."""
    n, cin, cout, h, w, ks, mode = (row[k] for k in ("n", "cin", "cout", "h", "w", "ks", "mode"))
    s = setup(n, cin, row["g"], h, w, row["rstds"], row["seed"], row["eps"])
    tag = f"prologue[{row['id']}]"
    gen = s.gen
    x = s.m4 + ints(gen, (n, cin, h, w), -2, 2)
    c = SimpleNamespace(s=s, x=x, row=row, info={})
    check_repr16(tag + " x", x, B16)
    c.a = gn_affine_ref(s, x)
    check_repr16(tag + " a", c.a, B16)
    check_repr16(tag + " a", c.a, H16)
    c.info["zero_a"] = check_zero(tag + " a", c.a)
    c.w = ternary(gen, (cout, cin, ks, ks), row["wdens"])
    c.info["density"] = E.check_density(tag, c.w)
    c.bias = ints(gen, (cout,), -3, 3)
    c.conv = E.conv_expr(c.a, c.w, None, ks, mode)
    c.res = ints(gen, c.conv.shape, -8, 8)
    unit = s.rstd.min().item() * 0.5
    c.info["sum32"] = exact_sum(tag + " accumulator", [E.conv_expr(c.a.abs(), c.w.abs(), None, ks, mode),
                                                       c.bias.abs().view(1, -1, 1, 1).expand_as(c.conv), c.res.abs()], unit)
    c.ref = {}
    for name, full in (("plain", c.conv), ("bias", c.conv + c.bias.view(1, -1, 1, 1)),
                       ("full", c.conv + c.bias.view(1, -1, 1, 1) + c.res)):
        for dt in (B16, H16):
            y = round16(full, dt)
            c.ref[name, dt] = y
            check_zero(f"{tag} y[{name}]", y)
            if row.get("stats") and name != "plain":
                # the epilogue sums the rounded values in fp32 per lane and wave half, then adds to the fixed-point table
                exact_sum(f"{tag} fused statistics [{name}]", [torch.tensor(_tile_block_sum(y.abs()))], unit)
                exact_sum(f"{tag} fused statistics [{name}]", [torch.tensor(_tile_block_sum(y * y))], unit * unit)
                yg = y.reshape(n, E.STATS_GROUPS, -1)
                q = torch.stack([yg.sum(-1), (yg * yg).sum(-1)], -1) * STAT_SCALE
                assert bool((q == q.round()).all())
                c.ref[name + "_stats", dt] = q.round().to(torch.int64)
    return c


def make_wgrad_prologue_case(row):
    """Weight gradient of conv(GN(x)): x, stats, gamma, beta, dy (integers) -> dw, db (float64 autograd on a)."""
    c = make_prologue_case(row)
    s, tag = c.s, f"wgrad prologue[{row['id']}]"
    n, cin, cout, ks, mode = row["n"], row["cin"], row["cout"], row["ks"], row["mode"]

    def grads(a, g):
        wt = torch.zeros(cout, cin, ks, ks, dtype=F64, requires_grad=True)
        b = torch.zeros(cout, dtype=F64, requires_grad=True)
        E.conv_expr(a, wt, b, ks, mode).backward(g)
        return wt.grad, b.grad
    c.dy = ints(s.gen, c.conv.shape, -2, 2)
    c.dw, c.db = grads(c.a, c.dy)
    aw, ab = grads(c.a.abs(), c.dy.abs())
    unit = s.rstd.min().item() * 0.5
    exact_sum(tag, [aw, ab.max().expand(1)], unit)
    assert bool((2 * aw / unit < LIMIT32).all()), f"{tag}: twice the sum (accumulate=True) leaves 2^24 units"
    check_zero(tag + " dW", c.dw)
    return c


# ---- backward ----------------------------------------------------------------------------------------------------------
def _signs(gen, shape, p_plus=0.5):
    return 2 * (torch.rand(tuple(shape), generator=gen, dtype=F64) < p_plus).to(F64) - 1


def _biased_x_dy(s, gen, bias=True):
    """x - m in [-1, 2] and dy in {-2, -1, 1, 2} with P(dy > 0) = 3/4: sums S1 and S2 with a non-zero expectation, so that
    no group's c1 or c2 vanishes by chance.  ``bias=False`` (the chained launch): symmetric, so that c1 and c2 stay small
    against gamma * dy and no dx cancels to a tiny value (the smallest |dx| sets the unit of every sum of the rounded dx)."""
    shape = (s.n, s.c, s.h, s.w_)
    if not bias:
        return s.m4 + ints(gen, shape, -1, 1), _signs(gen, shape) * ints(gen, shape, 1, 2)
    return s.m4 + ints(gen, shape, -1, 2), _signs(gen, shape, 0.75) * ints(gen, shape, 1, 2)


def _cancelling_dy(s, gen, lo=1, hi=3):
    """dy (and x) of the ragged regime.  >= 2 channels per group: channels 2j / 2j+1 share gamma and x and carry opposite
    dy.  One channel per group: pixel pairs (2i, 2i+1) of the flattened map share x and carry opposite dy; an odd last
    pixel gets dy = 0."""
    n, c, h, w = s.n, s.c, s.h, s.w_
    sign = 2 * torch.randint(0, 2, (n, c, h, w), generator=gen).to(F64) - 1
    dy = sign * ints(gen, (n, c, h, w), lo, hi)
    x = ints(gen, (n, c, h, w), -2, 2)
    if s.cpg >= 2:
        dy[:, 1::2] = -dy[:, 0::2]
        x[:, 1::2] = x[:, 0::2]
    else:
        dyf, xf = dy.reshape(n, c, -1), x.reshape(n, c, -1)
        hw = h * w
        dyf[..., 1:hw - hw % 2:2] = -dyf[..., 0:hw - hw % 2:2]
        xf[..., 1:hw - hw % 2:2] = xf[..., 0:hw - hw % 2:2]
        if hw % 2:
            dyf[..., -1] = 0
        dy, x = dyf.reshape(n, c, h, w), xf.reshape(n, c, h, w)
    return x, dy


def gn_bwd_ref(s, x, dy, dres=None, act_prime=None, tag="gn_bwd", chained=False):
    """float64 backward of GroupNorm with the table of ``s``.  ``dy`` is the gradient w.r.t. the normalised-and-affine
    output (``act_prime``: multiplied first, the SiLU plumbing's exact 1/2).  -> SimpleNamespace(dy_act, S1, S2 [n, c],
    sums [n, c, 2], c1, c2 [n, groups], dx, dx16, dgamma, dbeta), every sum checked with ``exact_sum``."""
    n, c, g, cpg = s.n, s.c, s.groups, s.cpg
    r = SimpleNamespace()
    r.dy_act = dy if act_prime is None else dy * act_prime
    xh = (x - s.m4) * s.r4
    ru = s.rstd.min().item()
    u_dy = 1.0 if act_prime is None else act_prime
    exact_sum(tag + " xhat", [x * s.r4, (s.m4 * s.r4).expand_as(x)], ru)
    exact_sum(tag + " S1", [r.dy_act], u_dy, dim=(0, 2, 3))                     # over pixels and, for dbeta, samples
    exact_sum(tag + " S2", [r.dy_act * xh], u_dy * ru, dim=(0, 2, 3))
    r.S1, r.S2 = r.dy_act.sum((2, 3)), (r.dy_act * xh).sum((2, 3))
    r.sums = torch.stack([r.S1, r.S2], -1)
    r.dbeta, r.dgamma = r.S1.sum(0), r.S2.sum(0)
    w1, w2 = s.gamma * r.S1, s.gamma * r.S2
    exact_sum(tag + " gamma * S1 over a group", [w1.reshape(n, g, cpg)], 0.5 * u_dy, dim=2)
    exact_sum(tag + " gamma * S2 over a group", [w2.reshape(n, g, cpg)], 0.5 * u_dy * ru, dim=2)
    t1, t2 = w1.reshape(n, g, cpg).sum(2), w2.reshape(n, g, cpg).sum(2)
    if s.pow2:
        r.c1, r.c2 = t1 / s.cnt, t2 / s.cnt
        live = (s.gamma.reshape(g, cpg) != 0).any(1)                # (a one-channel group whose gamma is 0 has none)
        assert bool((r.c1[:, live] != 0).all()) and bool((r.c2[:, live] != 0).all()), f"{tag}: a (sample, group) has c1 or c2 == 0"
    else:
        assert bool((t1 == 0).all()) and bool((t2 == 0).all()), f"{tag}: the ragged regime needs cancelling group sums"
        r.c1, r.c2 = t1, t2
        if cpg >= 2:
            assert bool((r.dgamma[s.gamma != 0] != 0).to(F64).mean() > 0.9) and bool((r.dbeta != 0).to(F64).mean() > 0.9)
    c1, c2 = _per_channel(r.c1, cpg), _per_channel(r.c2, cpg)
    # rstd * (gamma * dy - c1 - xhat * c2) + dres: the unit per (sample, group) is what xhat * c2 needs
    u_in = (0.5 * u_dy / s.cnt * (ru * s.rstd).clamp(max=1.0) if s.pow2 else torch.full_like(s.rstd, 0.5 * u_dy))
    u_in4 = _per_channel(u_in, cpg)
    inner = [s.g4 * r.dy_act, c1.expand_as(x), xh * c2]
    exact_sum(tag + " gamma * dy - c1 - xhat * c2", inner, u_in4)
    core = s.r4 * (inner[0] - inner[1] - inner[2])
    terms = [core] + ([dres] if dres is not None else [])
    exact_sum(tag + " dx", [s.r4 * (inner[0].abs() + inner[1].abs() + inner[2].abs())] + terms[1:], u_in4 * s.r4)
    # the chained loader's association: sc * g + b * h + d with b = -rstd^2 c2, d = -rstd c1 - b * mean
    if chained:
        exact_sum(tag + " dx, chained form", [s.r4 * s.g4 * r.dy_act, s.r4 * s.r4 * c2 * x, (s.r4 * c1).expand_as(x),
                                              (s.r4 * s.r4 * c2 * s.m4).expand_as(x)], u_in4 * s.r4)
    r.dx = sum(terms)
    r.dx16 = round16(r.dx)
    return r


def plumbing_ref(s, x, dy, tag):
    """The SiLU plumbing: gamma = beta = 0, so every pre-activation is exactly 0 and act' exactly 1/2 while xhat is not
    zero: dy_act = dy / 2, its sums and the affine gradients (dx is rstd * 0 = 0 plus the residual)."""
    assert bool((s.gamma == 0).all()) and bool((s.beta == 0).all())
    r = SimpleNamespace(dy_act=dy * 0.5)
    xh = (x - s.m4) * s.r4
    ru = s.rstd.min().item()
    exact_sum(tag + " S1", [r.dy_act], 0.5, dim=(0, 2, 3))
    exact_sum(tag + " S2", [r.dy_act * xh], 0.5 * ru, dim=(0, 2, 3))
    r.S1, r.S2 = r.dy_act.sum((2, 3)), (r.dy_act * xh).sum((2, 3))
    r.sums = torch.stack([r.S1, r.S2], -1)
    r.dbeta, r.dgamma = r.S1.sum(0), r.S2.sum(0)
    check_repr16(tag + " dy_act", r.dy_act, B16)
    check_zero(tag + " dy_act", r.dy_act)
    check_zero(tag + " dgamma", r.dgamma)
    return r


def make_silu_bwd_case(row):
    """gn_bwd(silu=True) with gamma = beta = 0 on the data of ``make_bwd_case``'s row."""
    n, ch, h, w = row["n"], row["c"], row["h"], row["w"]
    s = setup(n, ch, row["g"], h, w, row["rstds"], row["seed"] + 50, row["eps"])
    s.gamma, s.beta = torch.zeros(ch, dtype=F64), torch.zeros(ch, dtype=F64)
    s.g4, s.b4 = s.gamma.view(1, -1, 1, 1), s.beta.view(1, -1, 1, 1)
    c = SimpleNamespace(s=s, row=row)
    c.x = s.m4 + ints(s.gen, (n, ch, h, w), -1, 2)
    c.dy = _signs(s.gen, (n, ch, h, w), 0.75) * ints(s.gen, (n, ch, h, w), 1, 2)
    c.dres = ints(s.gen, (n, ch, h, w), -4, 4)
    c.ref = plumbing_ref(s, c.x, c.dy, f"gn_bwd silu[{row['id']}]")
    return c


def make_bwd_case(row):
    """x, dy, dres (integers), the table, gamma, beta -> references with and without ``dres`` (``ref``, ``ref_res``)."""
    n, ch, h, w = row["n"], row["c"], row["h"], row["w"]
    s = setup(n, ch, row["g"], h, w, row["rstds"], row["seed"], row["eps"])
    tag = f"gn_bwd[{row['id']}]"
    gen = s.gen
    c = SimpleNamespace(s=s, row=row, info={})
    if s.pow2:
        c.x, c.dy = _biased_x_dy(s, gen)
        c.dres = ints(gen, (n, ch, h, w), -4, 4)
    else:
        c.x, c.dy = _cancelling_dy(s, gen)
        # large, so that the sum rounds: 16 k with 16 <= |k| <= 128 (bf16 values of 256 .. 2048, spacing 2 .. 8)
        c.dres = 16 * _signs(gen, (n, ch, h, w)) * ints(gen, (n, ch, h, w), 16, 128)
    for t in (c.x, c.dy, c.dres):
        check_repr16(tag + " input", t, B16)
    c.ref = gn_bwd_ref(s, c.x, c.dy, None, tag=tag)
    c.ref_res = gn_bwd_ref(s, c.x, c.dy, c.dres, tag=tag + " +dres")
    for r, nm in ((c.ref, "dx"), (c.ref_res, "dx + dres")):
        c.info["zero " + nm] = check_zero(f"{tag} {nm}", r.dx16)
        c.info["rounded " + nm] = rounded_share(r.dx)
    assert c.info["rounded dx + dres"] >= MIN_ROUNDED, f"{tag}: only {c.info['rounded dx + dres']:.2f} of dx + dres rounds"
    if s.pow2:
        assert c.info["rounded dx"] >= MIN_ROUNDED, f"{tag}: only {c.info['rounded dx']:.2f} of dx rounds"
    if s.cpg >= 2 or s.pow2:          # (ragged with one channel per group: each channel's own sums are zero by construction)
        check_zero(tag + " dgamma", c.ref.dgamma)
        check_zero(tag + " dbeta", c.ref.dbeta)
    return c


def fp32_shuffled_eval(c, with_res, seed=0):
    """The backward in fp32 torch with the pixels in a shuffled order (another summation order than the reference's):
    -> (sums [n, c, 2], dx [n, c, h, w] fp32, dgamma, dbeta).  Must EQUAL the float64 reference."""
    s = c.s
    n, ch, h, w = c.x.shape
    perm = torch.randperm(h * w, generator=torch.Generator().manual_seed(seed))
    f = lambda t: t.to(F32)
    x, dy = f(c.x).reshape(n, ch, -1)[..., perm], f(c.dy).reshape(n, ch, -1)[..., perm]
    m, r, g = f(s.m4).reshape(n, ch, 1), f(s.r4).reshape(n, ch, 1), f(s.gamma).view(1, ch, 1)
    xh = (x - m) * r
    S1, S2 = torch.zeros(n, ch, dtype=F32), torch.zeros(n, ch, dtype=F32)
    for k in range(0, h * w, 37):                                  # odd-sized slabs, added one after the other
        S1 += dy[..., k:k + 37].sum(-1)
        S2 += (dy[..., k:k + 37] * xh[..., k:k + 37]).sum(-1)
    inv = torch.tensor(1.0 / s.cnt, dtype=F32)
    t1 = (g[..., 0] * S1).reshape(n, s.groups, s.cpg).flip(2).sum(2) * inv
    t2 = (g[..., 0] * S2).reshape(n, s.groups, s.cpg).flip(2).sum(2) * inv
    c1, c2 = t1.repeat_interleave(s.cpg, 1)[..., None], t2.repeat_interleave(s.cpg, 1)[..., None]
    dx = r * (g * dy - c1 - xh * c2)
    if with_res:
        dx = dx + f(c.dres).reshape(n, ch, -1)[..., perm]
    out = torch.empty_like(dx)
    out[..., perm] = dx
    return torch.stack([S1, S2], -1), out.reshape(n, ch, h, w), S2.flip(0).sum(0), S1.flip(0).sum(0)


# ---- fused epilogue and chained launch -----------------------------------------------------------------------------------
def _dgrad(dy, wf, ks):
    """Data gradient of the stride-1 conv with forward weight wf [cout, cin, ks, ks]: dy [n, cout, h, w] -> [n, cin, h, w]."""
    return F.conv_transpose2d(dy, wf, padding=ks // 2)


def make_fused_case(row, silu_plumbing=False):
    """conv_mfma_gnbwd: dy_in (integers, ``cout`` channels), forward weight wf [cout, cin, ks, ks] (ternary), gx (the
    GroupNorm input, ``cin`` channels) and its table -> g = conv^T(dy_in) (integer, |g| <= 256: stored in bf16 and read
    again by gn_bwd_apply), the backward reference on it.  ``silu_plumbing``: gamma = beta = 0, so every pre-activation is
    0 and act' is 1/2: dy_out = g / 2."""
    n, cin, cout, h, w, ks = (row[k] for k in ("n", "cin", "cout", "h", "w", "ks"))
    s = setup(n, cin, row["g"], h, w, row["rstds"], row["seed"], row["eps"])
    tag = f"gnbwd[{row['id']}{' silu' if silu_plumbing else ''}]"
    gen = s.gen
    c = SimpleNamespace(s=s, row=row)
    if silu_plumbing:
        s.gamma, s.beta = torch.zeros(cin, dtype=F64), torch.zeros(cin, dtype=F64)
        s.g4, s.b4 = s.gamma.view(1, -1, 1, 1), s.beta.view(1, -1, 1, 1)
    c.wf = ternary(gen, (cout, cin, ks, ks), row["wdens"])
    E.check_density(tag, c.wf)
    c.gx = s.m4 + ints(gen, (n, cin, h, w), -2, 2)
    c.dres = ints(gen, (n, cin, h, w), -4, 4)
    if s.pow2 or silu_plumbing:
        c.dy_in = ints(gen, (n, cout, h, w), -2, 2)
    else:
        # ragged: the group sums of gamma * S1 and gamma * S2 must cancel AFTER the conv: weight columns of the channel
        # pairs are opposite (conv^T is linear in them) and gx is shared by the pair
        c.dy_in = ints(gen, (n, cout, h, w), -2, 2)
        c.wf[:, 1::2] = -c.wf[:, 0::2]
        c.gx[:, 1::2] = c.gx[:, 0::2]
    c.g = _dgrad(c.dy_in, c.wf, ks)
    E.check_store16(tag + " conv^T(dy)", c.g)
    check_sum32(tag + " accumulator", _dgrad(c.dy_in.abs(), c.wf.abs(), ks).max().item())
    if silu_plumbing:
        c.ref = plumbing_ref(s, c.gx, c.g, tag)
        return c
    check_zero(tag + " dy_out", c.g)
    c.ref = gn_bwd_ref(s, c.gx, c.g, None, tag=tag)
    c.ref_res = gn_bwd_ref(s, c.gx, c.g, c.dres, tag=tag + " +dres")
    check_zero(tag + " dx", c.ref.dx16)
    return c


def make_chain_case(row):
    """conv_mfma_gnbwd_chain.  The layer above: g_in (integers), x_in, its table / gamma and its finalized sums (computed
    from g_in and x_in, as conv_mfma_gnbwd would have left them) -> dx_in = round16(applied gradient); then
    dy_out = round16(conv^T(dx_in, rounded)) and the backward sums of the epilogue GroupNorm (input gx) on the UNROUNDED
    conv result, which is what the epilogue adds up."""
    n, ch, h, w = row["n"], row["c"], row["h"], row["w"]
    up = setup(n, ch, row["g"], h, w, row["rstds"], row["seed"], row["eps"], gammas=CHAIN_GAMMAS)
    tag = f"chain[{row['id']}]"
    gen = up.gen
    c = SimpleNamespace(up=up, row=row)
    if up.pow2:
        c.x_in, c.g_in = _biased_x_dy(up, gen, bias=False)
    else:
        c.x_in, c.g_in = _cancelling_dy(up, gen)
    c.up_ref = gn_bwd_ref(up, c.x_in, c.g_in, None, tag=tag + " applied gradient", chained=True)
    c.dx_in = c.up_ref.dx16
    check_zero(tag + " dx_in", c.dx_in)
    # the conv in between and the epilogue GroupNorm: its own table (same eps: one launch argument), gamma, beta
    lo = setup(n, ch, row["g"], h, w, row["rstds"], row["seed"] + 500, row["eps"])
    c.lo = lo
    c.wf = ternary(gen, (ch, ch, 3, 3), row["wdens"])
    E.check_density(tag, c.wf)
    c.gx = lo.m4 + ints(gen, (n, ch, h, w), -2, 2)
    conv = _dgrad(c.dx_in, c.wf, 3)
    # the accumulator: every term is a bf16 value; the sum must be exact in fp32 whatever the order
    lsb = _min_lsb(c.dx_in)
    exact_sum(tag + " accumulator", [_dgrad(c.dx_in.abs(), c.wf.abs(), 3)], lsb)
    check_f32(tag + " conv", conv)
    c.conv = conv
    c.dy_out = round16(conv)
    check_zero(tag + " dy_out", c.dy_out)
    xh = (c.gx - lo.m4) * lo.r4
    exact_sum(tag + " S1", [conv], lsb, dim=(2, 3))
    exact_sum(tag + " S2", [conv * xh], lsb * lo.rstd.min().item(), dim=(2, 3))
    c.gsums = torch.stack([conv.sum((2, 3)), (conv * xh).sum((2, 3))], -1)
    check_f32(tag + " gsums", c.gsums)
    return c


def _min_lsb(t):
    """A power of two that divides every element of a tensor of bf16 values: a bf16 value v is a multiple of
    2^(floor(log2 |v|) - 7), and so is every value of larger magnitude."""
    _, e = torch.frexp(t[t != 0].abs().min())
    return 2.0 ** (int(e) - 1 - 7)


# ---- the case tables shared by the CPU and the GPU file --------------------------------------------------------------
ALL_RSTD = (2.0, 1.0, 0.5, 0.25)
# rstd values each kernel family returns EXACTLY for var + eps in {1/4, 1, 4, 16}, as the probe of
# tests/test_gpu_exact_groupnorm.py measured on an MI355X (the probe asserts this table); the cases of a family draw only
# from its entry
EXACT_RSTD = {
    "gn_bwd": ALL_RSTD, "gn_bwd_apply": ALL_RSTD, "conv_mfma_v2": ALL_RSTD, "conv_mfma_s2": ALL_RSTD, "conv_direct": ALL_RSTD,
    "wgrad_direct": ALL_RSTD, "conv_wgrad_mfma": ALL_RSTD, "conv_mfma_gnbwd": ALL_RSTD, "chain": ALL_RSTD,
}


def common_rstd(*families):
    return tuple(r for r in ALL_RSTD if all(r in EXACT_RSTD[f] for f in families))


# the issue's seven shapes: (n, c, groups, h, w)
BASE_SHAPES = [(2, 32, 16, 16, 16), (2, 64, 16, 8, 16), (2, 128, 16, 8, 8), (1, 256, 16, 8, 16), (2, 32, 32, 16, 16),
               (1, 128, 16, 13, 19), (3, 64, 16, 9, 7)]
# ... plus the grids of the backward: two workgroups per sample (three shapes), 128 partial rows per sample (the four-way
# unrolled loop of gn_sums_finalize), ragged with several workgroups / a partly filled last batch / a short last block,
# three samples with different statistics
BWD_SHAPES = BASE_SHAPES + [(2, 32, 16, 32, 32), (2, 128, 16, 16, 16), (2, 512, 32, 8, 8), (1, 512, 32, 64, 64),
                            (2, 128, 16, 13, 19), (2, 32, 32, 23, 29), (3, 32, 16, 16, 16)]


def _pow2(n, c, g, h, w):
    k = (c // g) * h * w
    return (k & (k - 1)) == 0


def _only(rstds, allowed):
    """The exact rstd values a case may use (1 is the floor: a family that does not return it has no exact cases)."""
    return tuple(r for r in rstds if r in allowed) or (1.0,)


def bwd_rows(rstds=None):
    rstds = rstds or common_rstd('gn_bwd', 'gn_bwd_apply')
    rows = []
    for k, (n, c, g, h, w) in enumerate(BWD_SHAPES):
        # 2^16 elements per group: c2 is a multiple of 2^-17 rstd, so xhat * c2 leaves the 24 bits with rstd < 1
        rs = _only(rstds, (2.0, 1.0)) if (c // g) * h * w >= 1 << 16 else tuple(rstds)
        rows.append(dict(n=n, c=c, g=g, h=h, w=w, seed=k, eps=0.0625 if _pow2(n, c, g, h, w) else (0.25, 1.0, 4.0)[k % 3],
                         rstds=rs, id=f"{n}x{c}g{g}@{h}x{w}"))
    return rows


def prologue_rows(rstds=None):
    """conv_mfma with the GN prologue: the seven shapes as 3x3 s1 (cout = cin), then 1x1, s2 and up on a subset."""
    rows = []
    rstds = rstds or common_rstd("conv_mfma_v2", "conv_mfma_s2")

    def add(n, cin, cout, g, h, w, ks, mode, **kw):
        d = dict(n=n, cin=cin, cout=cout, g=g, h=h, w=w, ks=ks, mode=mode, seed=len(rows),
                 eps=0.0625 if _pow2(n, cin, g, h, w) else (0.25, 1.0, 4.0)[len(rows) % 3], rstds=tuple(rstds),
                 wdens=0.25 if cin <= 64 else 0.125, f16=False, stats=False)
        d.update(kw)
        if d["stats"]:
            # the fused statistics add y^2 (unit: the square of y's) over a tile in fp32: rstd >= 1 keeps that unit at 1/4
            d["rstds"] = _only(rstds, (2.0, 1.0))
            d["wdens"] = min(d["wdens"], 0.125 if cin <= 128 else 0.09375)
        d["id"] = (f"{mode}-k{ks}-{n}x{cin}to{cout}g{g}@{h}x{w}" + ("-f16" if d["f16"] else "") + ("-stats" if d["stats"] else ""))
        rows.append(d)
    for n, c, g, h, w in BASE_SHAPES:
        add(n, c, c, g, h, w, 3, "s1")
    for n, c, g, h, w in BASE_SHAPES[:1] + BASE_SHAPES[2:6]:
        add(n, c, c, g, h, w, 3, "s1", stats=True)
    add(2, 64, 64, 16, 8, 16, 3, "s1", stats=True, f16=True)
    add(2, 64, 64, 16, 8, 16, 3, "s2", stats=True)
    add(2, 128, 128, 16, 8, 8, 3, "up", stats=True)
    add(2, 128, 128, 16, 8, 8, 3, "s1", f16=True)          # fp16 storage and operands
    add(1, 128, 128, 16, 13, 19, 3, "s1", f16=True)
    add(2, 64, 64, 16, 8, 16, 3, "s1", f16=True)
    add(2, 128, 384, 16, 8, 8, 1, "s1")                     # the fused q, k, v projection
    add(2, 32, 64, 16, 16, 16, 1, "s1")
    add(3, 64, 64, 16, 9, 7, 1, "s1", f16=True)
    add(2, 32, 32, 16, 16, 16, 3, "s2")                     # the stride-2 (v1) kernel
    add(1, 256, 256, 16, 8, 16, 3, "s2")
    add(1, 128, 128, 16, 13, 19, 3, "s2")
    add(3, 64, 64, 16, 9, 7, 3, "s2", f16=True)
    add(2, 64, 64, 16, 8, 16, 3, "up")
    add(2, 128, 128, 16, 8, 8, 3, "up", f16=True)
    add(3, 64, 64, 16, 9, 7, 3, "up")
    return rows


# conv_direct with prologue=1 (the prologue rows of tests/test_gpu_ops.py::DIRECT_CASES, and one ragged):
# (n, cin, cout, h, w, groups, output layout)
DIRECT_PROLOGUE = [(2, 32, 1, 16, 16, 16, "nchw_f32"), (2, 64, 3, 12, 10, 16, "nchw_f32"), (2, 128, 4, 8, 8, 16, "nhwc_f32"),
                   (1, 256, 10, 8, 8, 16, "nhwc_f32")]
# wgrad_direct with prologue=1: fewcout (n, cw, cn, h, w)
WGRAD_DIRECT_PROLOGUE = [(2, 32, 1, 16, 16), (2, 128, 4, 8, 8), (1, 64, 3, 13, 19)]
# conv_wgrad_mfma with prologue=1: (n, cin, cout, groups, h, w, ks, mode)
WGRAD_PROLOGUE = [(2, 32, 32, 16, 16, 16, 3, "s1"), (2, 128, 128, 16, 8, 8, 3, "s1"), (1, 256, 256, 16, 8, 16, 3, "s1"),
                  (1, 128, 128, 16, 13, 19, 3, "s1"), (3, 64, 64, 16, 9, 7, 3, "s1"), (2, 32, 32, 32, 16, 16, 3, "s1"),
                  (2, 128, 384, 16, 8, 8, 1, "s1"), (2, 64, 64, 16, 8, 16, 3, "s2"), (2, 64, 64, 16, 8, 16, 3, "up")]


def direct_row(n, cin, cout, h, w, g, rstds=None, k=0):
    rstds = rstds or common_rstd('conv_direct', 'wgrad_direct')
    return dict(n=n, cin=cin, cout=cout, g=g, h=h, w=w, ks=3, mode="s1", seed=100 + k, rstds=tuple(rstds), f16=False,
                eps=0.0625 if _pow2(n, cin, g, h, w) else 0.25, wdens=1.0 if cout <= 16 else 0.25,
                id=f"direct-{n}x{cin}to{cout}g{g}@{h}x{w}")


def wgrad_rows(rstds=None):
    rstds = rstds or common_rstd('conv_wgrad_mfma')
    return [dict(n=n, cin=cin, cout=cout, g=g, h=h, w=w, ks=ks, mode=mode, seed=200 + k, rstds=tuple(rstds), f16=False,
                 eps=0.0625 if _pow2(n, cin, g, h, w) else 1.0, wdens=0.25 if cin <= 64 else 0.125,
                 id=f"wgrad-{mode}-k{ks}-{n}x{cin}to{cout}g{g}@{h}x{w}")
            for k, (n, cin, cout, g, h, w, ks, mode) in enumerate(WGRAD_PROLOGUE)]


def fused_rows(rstds=None):
    """conv_mfma_gnbwd: forward cin -> cout (the GroupNorm is on the cin side; dy_in has cout channels)."""
    rstds = rstds or common_rstd("conv_mfma_gnbwd", "gn_bwd_apply")
    shapes = [(2, 32, 32, 16, 16, 3), (2, 128, 128, 16, 16, 3), (1, 128, 128, 13, 19, 3), (2, 128, 384, 8, 8, 1),
              (1, 256, 256, 8, 16, 3)]
    # conv^T(dy) reaches ~80 and gamma 4: with rstd 1/4 the unit of xhat * c2 (2^-16 on 2048 elements) leaves the 24 bits
    rstds = _only(rstds, (2.0, 1.0, 0.5))
    return [dict(n=n, cin=cin, cout=cout, g=16, h=h, w=w, ks=ks, seed=300 + k, rstds=tuple(rstds),
                 eps=0.0625 if _pow2(n, cin, 16, h, w) else 0.25, wdens=0.25 if cout <= 64 else 0.125 if cout <= 128 else 0.09375,
                 id=f"k{ks}-{n}x{cin}to{cout}@{h}x{w}")
            for k, (n, cin, cout, h, w, ks) in enumerate(shapes)]


def chain_rows(rstds=None):
    rstds = rstds or common_rstd('chain', 'conv_mfma_gnbwd')
    shapes = [(2, 128, 16, 16), (2, 128, 13, 21), (1, 256, 8, 16)]
    # dx_in is rounded to bf16 and summed again (conv, S1, S2): with rstd >= 1 and |gamma| >= 1 its smallest magnitude
    # is ~1/2, every later term a multiple of 2^-9 (see CHAIN_GAMMAS)
    rstds = _only(rstds, (2.0, 1.0))
    return [dict(n=n, c=c, g=16, h=h, w=w, seed=400 + k, rstds=tuple(rstds), eps=0.0625 if _pow2(n, c, 16, h, w) else 0.25,
                 wdens=0.125, id=f"{n}x{c}@{h}x{w}")
            for k, (n, c, h, w) in enumerate(shapes)]


def make_tie_in_case(n=2, c=64, groups=16, h=8, w=16, seed=0):
    """x in {m - 1, m + 1}, balanced per (sample, group): the statistics that ops.gn_stats produces are then sum = cnt * m,
    sumsq = cnt * (m^2 + 1), and with eps = 3 the consumers see var + eps = 4, rstd = 1/2."""
    s = setup(n, c, groups, h, w, (0.5,), 900 + seed, eps=3.0)
    gen = s.gen
    half = s.cnt // 2
    pm = torch.cat([torch.ones(half), -torch.ones(half)]).to(F64)
    xg = torch.stack([pm[torch.randperm(s.cnt, generator=gen)] for _ in range(n * groups)]).reshape(n, c, h, w)
    x = s.m4 + xg
    yg = x.reshape(n, groups, -1)
    table = (torch.stack([yg.sum(-1), (yg * yg).sum(-1)], -1) * STAT_SCALE).round().to(torch.int64)
    assert torch.equal(table, s.stats), "tie-in: the hand-written table is not the statistics of x"
    check_sum32("tie-in statistics", (yg * yg).sum(-1).max().item())
    dy = _signs(gen, x.shape, 0.75) * ints(gen, x.shape, 1, 2)
    return SimpleNamespace(s=s, x=x, a=gn_affine_ref(s, x), dy=dy, ref=gn_bwd_ref(s, x, dy, None, tag="tie-in"))

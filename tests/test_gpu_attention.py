"""GPU parity of the flash-style mid-block attention (forward + backward, C-ABI) against the
materialised softmax(q k^T C^-0.5) v of MONAI's SABlock restated with torch fp32 on CPU.

Tolerance: o / dq / dk / dv are bf16 and P is rounded to bf16 before the P.V product, so
max-abs <= 2% of the reference scale and rel-L2 <= 1e-2.  One case spikes a key row so that the
running max jumps mid-stream (forces the online-softmax rescale branch).

Below that first test: inputs for which the right answer is EXACT (tests/attention_oracle.py: one-hot, pair and uniform
softmax; a dropped key, a leaked pad row or a missed rescale is a bit difference there, where it is 1/4096 of a tolerance
above), the delta kernel's grid-stride loop, a per-row error against float64 at unit and at trained-network logit scale,
the memory extent of every kernel, batch independence and the argument checks.
"""
from types import SimpleNamespace

import pytest
import torch

import attention_oracle as A
import bounds_util as B
from test_gpu_ops import _r, _report

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.mark.parametrize("b,l,c,spike", [(2, 64, 128, False), (2, 256, 128, True), (1, 128, 256, False),
                                         (1, 192, 64, True), (1, 1024, 128, False),
                                         # token counts that are not a multiple of the 64 / 32-token tiles (e.g. a 72x104
                                         # image has a 9x13 latent): masked tail keys / queries
                                         (2, 117, 128, True), (3, 96, 128, False), (1, 40, 256, False), (2, 7, 64, False),
                                         # the AR config's real mid-block shape (256x256 image, 3 levels): L = 64*64, C = 256,
                                         # and the same token count at C = 128 (the 4096^2 fp32 reference matrix is 64 MB)
                                         (1, 4096, 256, True), (2, 4096, 128, False)])
def test_attention_fwd_bwd(dev, b, l, c, spike):
    from pti_ldm_vae_amd import ops
    torch.manual_seed(10)
    qkv = _r(torch.randn(b, l, 3 * c))
    if spike:  # a key far along the stream that dominates some queries
        qkv[:, l - 3, c:2 * c] *= 6.0
        qkv[:, 5, 0:c] *= 4.0
        qkv = _r(qkv)   # keep the inputs bf16-representable so both sides see identical numbers
    qkv.requires_grad_(True)
    q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    att = torch.softmax(torch.einsum("blc,bmc->blm", q, k) * c ** -0.5, dim=-1)
    o_ref = torch.einsum("blm,bmc->blc", att, v)
    dout = _r(torch.randn(b, l, c))
    o_ref.backward(dout)
    qd = qkv.detach().to(dev, torch.bfloat16)
    o = torch.full((b, l, c), float("nan"), dtype=torch.bfloat16, device=dev)
    lse2 = torch.empty(b, l, device=dev)
    ops.attention_fwd(qd, o, lse2)
    torch.cuda.synchronize()
    _report(f"attn fwd[{l},{c}]", o, o_ref.detach(), max_frac=2e-2, l2=1e-2)
    lse_ref = torch.logsumexp(torch.einsum("blc,bmc->blm", q, k).detach() * c ** -0.5, dim=-1) * 1.4426950408889634
    _report("attn lse2", lse2, lse_ref, max_frac=1e-3, l2=1e-4)
    dqkv = torch.full((b, l, 3 * c), float("nan"), dtype=torch.bfloat16, device=dev)
    delta = torch.empty(b, l, device=dev)
    # the backward consumes the bf16 forward output, as the engine does
    ops.attention_bwd(qd, o, dout.to(dev, torch.bfloat16), lse2, delta, dqkv)
    torch.cuda.synchronize()
    g = qkv.grad
    _report("attn dq", dqkv[..., :c], g[..., :c], max_frac=2e-2, l2=1.5e-2)
    _report("attn dk", dqkv[..., c:2 * c], g[..., c:2 * c], max_frac=2e-2, l2=1.5e-2)
    _report("attn dv", dqkv[..., 2 * c:], g[..., 2 * c:], max_frac=2e-2, l2=1.5e-2)


# ---- exact structured parity, ragged grid, memory extent (tests/attention_oracle.py; its conditions are proven on the CPU
# by tests/test_attention_cpu.py) ----------------------------------------------------------------------------------------
def _run(dev, qkv, dout, alloc=None, wrap=None):
    """Forward then backward as the engine chains them (the backward consumes the kernel's own bf16 o and lse2); every
    output pre-filled with NaN.  ``alloc(name, shape, dtype)`` / ``wrap(tensor)``: the memory-extent test's buffers."""
    from pti_ldm_vae_amd import ops
    alloc = alloc or (lambda name, shape, dtype: torch.full(shape, NAN, dtype=dtype, device=dev))
    wrap = wrap or (lambda t: t)
    b, l, c3 = qkv.shape
    c = c3 // 3
    qd, dd = wrap(qkv.to(dev, BF16)), wrap(dout.to(dev, BF16))
    o, lse2 = alloc("o", (b, l, c), BF16), alloc("lse2", (b, l), F32)
    ops.attention_fwd(qd, o, lse2)
    dqkv, delta = alloc("dqkv", (b, l, c3), BF16), alloc("delta", (b, l), F32)
    ops.attention_bwd(qd, wrap(o), dd, lse2, delta, dqkv)
    torch.cuda.synchronize()
    g = dqkv.cpu().to(F64)
    return SimpleNamespace(o=o.cpu().to(F64), lse2=lse2.cpu().to(F64), delta=delta.cpu().to(F64), dq=g[..., :c],
                           dk=g[..., c:2 * c], dv=g[..., 2 * c:], raw=dict(o=o, lse2=lse2, delta=delta, dqkv=dqkv))


def _diff(tag, name, got, exp, fails):
    """Bit equality after the exact cast to float64 (-0 equals 0; NaN equals nothing); a mismatch is located."""
    bad = ~(got == exp)
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        first = tuple(idx[0].tolist())
        rows = sorted({(i[0], i[1]) for i in idx.tolist()})
        fails.append(f"{tag} {name}: {idx.shape[0]} of {exp.numel()} differ; first (image, token[, d]) {first}: got "
                     f"{got[first].item():g} expected {exp[first].item():g}; (image, token) rows hit: {rows[:12]}"
                     f"{' ...' if len(rows) > 12 else ''} ({len(rows)} rows; 64-token tiles {sorted({r[1] // 64 for r in rows})[:12]})")


def _close(tag, name, got, exp, lim, fails):
    err = (got - exp).abs()
    bad = ~(err <= lim)
    if bool(bad.any()):
        first = tuple(torch.nonzero(bad)[0].tolist())
        fails.append(f"{tag} {name}: {int(bad.sum())} of {exp.numel()} outside the bound; first {first}: got "
                     f"{got[first].item():.9g} expected {exp[first].item():.9g}")


def _check_exact(tag, case, got, fails, lse_exact=False):
    """Everything a structured case gives in closed form.  ``fails`` collects the messages."""
    for name in ("o", "delta", "dq", "dk", "dv"):
        exp = getattr(case, name)
        if exp is None or (case.kind == "pair" and name == "dk"):
            continue
        if case.kind == "uniform" and name == "dq":
            # bit-exact on the rows whose fp32 partial sums are proven exact (all of them at C = 64 and 256), within the
            # derived bound on all rows (below)
            rows = case.dq_proven
            _diff(tag, "dq (rows proven exact)", torch.where(rows[..., None], got.dq, exp), exp, fails)
            continue
        _diff(tag, name, getattr(got, name), exp, fails)
    if lse_exact:
        _diff(tag, "lse2", got.lse2, case.lse2.to(F32).to(F64), fails)
    else:
        _close(tag, "lse2", got.lse2, case.lse2, A.ONEHOT_LSE_RTOL * case.lse2.abs(), fails)


@pytest.mark.parametrize("c", A.C_LIST)
@pytest.mark.parametrize("l", A.ONEHOT_L)
def test_attention_exact_onehot(dev, l, c):
    """q_i = 128 x the code of key pi(i): P is exactly 0 / 1, so o = v[pi], dq = dk = 0, dv = scatter-add of do, delta =
    do . v[pi] are bit-exact; every pi family that L admits (all -> L-1: the maximum arrives in the last, masked tile)."""
    fails = []
    for name, pi in A.pi_families(2, l):
        case = A.onehot_case(2, l, c, pi)
        _check_exact(f"onehot[{name}, L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("b,l,c", A.ONEHOT_BIG)
def test_attention_exact_onehot_real_shape(dev, b, l, c):
    """The AR config's L = 4096: one key of 4096 is the whole answer.  The reference is a gather."""
    fails = []
    for name, pi in A.pi_families(b, l, ("random", "all_last")):
        case = A.onehot_case(b, l, c, pi)
        _check_exact(f"onehot[{name}, L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    assert not fails, "\n".join(fails)


def _check_pair(tag, case, got, fails):
    _check_exact(tag, case, got, fails, lse_exact=True)     # the winning score + 1 stays in its binade: exact in fp32
    a, b = case.a, case.b
    rest = torch.ones(case.dk.shape[1], dtype=torch.bool)
    rest[[a, b]] = False
    _diff(tag, "dk (rows other than a, b)", got.dk[:, rest], case.dk[:, rest], fails)
    _diff(tag, "dk_b = -dk_a", got.dk[:, b], -got.dk[:, a], fails)
    # dk_a = bf16(sum_i bf16(dS_ia) q_i): a half ulp (<= 2^-8 relative) of every term and of the result
    _close(tag, "dk_a", got.dk[:, a], case.dk[:, a], 2.0 ** -8 * (case.dk_abs[:, None] + case.dk[:, a].abs()), fails)


def _check_uniform(tag, case, got, fails):
    l = case.o.shape[1]
    _check_exact(tag, case, got, fails, lse_exact=A.is_pow2(l))   # log2 of a power of two is exact; else one fp32 rounding
    if case.shift:
        # two bf16 roundings (dS, the output): a half ulp, <= 2^-8 relative, of every term and of the result; the 1 + 2^-6
        # covers p = exp2(-369 - lse2) (lse2 rounds at 2^-16) and fp32 accumulation.  dk beyond column 0 has no terms: 0.
        for name in ("dq", "dk"):
            f64, ab = getattr(case, name + "_f64"), getattr(case, name + "_abs")
            _close(tag, name, getattr(got, name), f64, 2.0 ** -8 * (ab * (1.0 + 2.0 ** -6) + f64.abs()), fails)
        dv = (case.dv_sum / l)[:, None].expand_as(got.dv)
        _close(tag, "dv", got.dv, dv, A.UNIFORM_DV_RTOL * dv.abs(), fails)
        return
    ref = None
    if case.dq is None:               # L no power of two: p = 1 / L rounds; bounds derived at A.UNIFORM_DQ_ROW_RTOL
        ref = A.reference(case.qkv, case.dout)
        _close(tag, "dv", got.dv, ref.dv, A.UNIFORM_DV_RTOL * ref.dv.abs() + 1e-12, fails)
    dq = case.dq if ref is None else ref.dq
    err = A.rowwise_err(got.dq, dq)
    print(f"{tag}: dq row-wise max error {err.max().item():.4e} (bound {A.UNIFORM_DQ_ROW_RTOL:.4e})")
    if not bool((err <= A.UNIFORM_DQ_ROW_RTOL).all()):
        fails.append(f"{tag} dq: row-wise error {err.max().item():.4e} > 2^-7 of the row's max at (image, token) "
                     f"{tuple(torch.nonzero(err == err.max())[0].tolist())}")


@pytest.mark.parametrize("c", A.C_LIST)
@pytest.mark.parametrize("l", A.POW2_L + A.RAGGED_L)
def test_attention_exact_pair_and_uniform(dev, l, c):
    """pair: P = 1/2, 1/2 on a key of the first and one of the last streamed tile; uniform: q = 0, P = 1 / L, integer sums
    that one missing, extra or repeated key changes.  Exact throughout at a power-of-two L; at the ragged L exact for o,
    lse2 (up to the fp32 rounding of log2 L), dk and delta, dq and dv of the uniform case within their derived bounds."""
    fails = []
    case = A.pair_case(2, l, c, 1, l - 2)
    _check_pair(f"pair[L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    case = A.uniform_case(2, l, c)
    _check_uniform(f"uniform[L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    if not A.is_pow2(l):      # every score -2048 C^-1/2: a pad key's p overflows in the backward unless it is masked
        case = A.uniform_case(2, l, c, shift=True)
        _check_uniform(f"uniform shifted[L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("c", A.C_LIST)
def test_attention_delta_grid_stride(dev, c):
    """attn_delta_kernel's grid is capped at 4096 blocks of 256 / (C / 8) rows: B x 256 rows just beyond that, with a
    remainder that is no multiple of the rows per block, make its grid-stride loop iterate a second time."""
    b, l = A.GRID_STRIDE[c], 256
    rpb = 256 // (c // 8)
    assert b * l > 4096 * rpb and (b - 1) * l <= 4096 * rpb
    fails = []
    case = A.uniform_case(b, l, c)
    _check_uniform(f"uniform[B={b}, L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    case = A.onehot_case(b, l, c, A.pi_family("random", b, l))
    _check_exact(f"onehot[random, B={b}, L={l}, C={c}]", case, _run(dev, case.qkv, case.dout), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("c", A.C_LIST)
@pytest.mark.parametrize("l", A.ROW_L)
@pytest.mark.parametrize("kind", A.ROW_KINDS)
def test_attention_rowwise_vs_fp64(dev, kind, l, c):
    """Error per token ROW against the float64 reference (max_d |got - ref| over that row's max_d |ref|, floored at 2^-8
    of the tensor's median row maximum), every row counted: an ordinary row is not measured against a spiked one.  The
    bound of each tensor is 3 x what the documented bf16 roundings alone do to it (A.ROW_BOUND, measured on the CPU)."""
    case = A.rowwise_case(kind, 2, l, c)
    ref, got = A.reference(case.qkv, case.dout), _run(dev, case.qkv, case.dout)
    fails = []
    for name in ("o", "dq", "dk", "dv"):
        if l == 1 and name in ("dq", "dk"):
            # One key: P = 1 whatever the score, so dq = dk = 0 identically and an error relative to the row has no
            # denominator.  The kernel's dS = P (dP - delta) subtracts two fp32 sums of the same C products do_d v_d, formed
            # in different orders (MFMA / the delta kernel): each within (C - 1) 2^-24 of sum_d |do_d v_d|.  That residue,
            # times C^-1/2 and |k| (dq) or |q| (dk), with two bf16 roundings on top (1 + 2^-6 covers them), is the bound.
            q, k, v = A.split(case.qkv)
            lim = (2.0 * c * 2.0 ** -24 * (case.dout.abs() * v.abs()).sum(-1, keepdim=True) * c ** -0.5
                   * (k if name == "dq" else q).abs() * (1.0 + 2.0 ** -6))
            assert not bool(getattr(ref, name).abs().max() > 1e-12)
            print(f"{kind}[L=1, C={c}] {name}: max |got| {getattr(got, name).abs().max().item():.4e} (limit {lim.max().item():.4e})")
            _close(kind, name, getattr(got, name), torch.zeros_like(lim), lim, fails)
            continue
        err, bound = A.rowwise_err(getattr(got, name), getattr(ref, name)), A.ROW_BOUND[kind][name]
        print(f"{kind}[L={l}, C={c}] {name}: row-wise max error {err.max().item():.4e} (bound {bound:.4e})")
        if not bool((err <= bound).all()):
            fails.append(f"{name}: row-wise error {err.max().item():.4e} > {bound:.4e} at (image, token) "
                         f"{tuple(torch.nonzero(err == err.max())[0].tolist())}; {int((err > bound).sum())} rows over")
    _close(kind, "lse2", got.lse2, ref.lse2, A.LSE_RTOL * ref.lse2.abs() + A.LSE_ATOL, fails)
    dref = ref.delta_of(got.o)
    _close(kind, "delta", got.delta, dref, A.DELTA_RTOL * (got.o * case.dout).abs().sum(-1), fails)
    assert not fails, f"{kind}[L={l}, C={c}]\n" + "\n".join(fails)


@pytest.mark.parametrize("l,c", A.EXTENT_CASES)
def test_attention_memory_extent(dev, l, c):
    """Every attention kernel clamps or masks rows >= L by hand: with the inputs inside NaN-poisoned buffers and the
    outputs between canary words the result is bit-equal to the run on plain tensors and no canary is touched.  (The pads
    belong to the helper's own allocations: nothing here can fault.)"""
    case = A.rowwise_case("randn", 2, l, c, seed=1)
    plain = _run(dev, case.qkv, case.dout)
    handles = {}

    def alloc(name, shape, dtype):
        handles[name] = B.with_canary(dev, shape, dtype, NAN)
        return handles[name].view

    guard = _run(dev, case.qkv, case.dout, alloc=alloc, wrap=lambda t: B.guarded(dev, t, B.POISON_NAN))
    for name, h in handles.items():
        assert B.intact(h), f"[L={l}, C={c}] {name}: a canary round the output was overwritten"
        assert bool(torch.isfinite(h.view).all()), f"[L={l}, C={c}] {name}: not finite (a read past row B*L brings NaN in)"
        assert torch.equal(h.view, plain.raw[name]), f"[L={l}, C={c}] {name}: differs from the run on plain tensors"
    assert bool(torch.isfinite(plain.raw["dqkv"]).all()) and guard.o.shape == plain.o.shape


@pytest.mark.parametrize("b,l,c", [(3, 117, 128), (2, 257, 256)])
def test_attention_batch_independent_and_reproducible(dev, b, l, c):
    """Image i of a batched call is bit-equal to a call on that image alone, and two identical calls are bit-equal."""
    case = A.rowwise_case("randn", b, l, c, seed=2)
    full, again = _run(dev, case.qkv, case.dout), _run(dev, case.qkv, case.dout)
    for name in ("o", "lse2", "dqkv", "delta"):
        assert torch.equal(full.raw[name], again.raw[name]), f"{name}: two identical calls differ"
        assert bool(torch.isfinite(full.raw[name]).all()), name
    for i in range(b):
        one = _run(dev, case.qkv[i:i + 1], case.dout[i:i + 1])
        for name in ("o", "lse2", "dqkv", "delta"):
            assert torch.equal(one.raw[name][0], full.raw[name][i]), f"{name}: image {i} of the batch differs from the call on it alone"


def test_attention_rejects(dev):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd._lib import PtiError
    qkv = torch.zeros(1, 96, 3 * 96, dtype=torch.bfloat16, device=dev)   # head dim 96 is not supported
    with pytest.raises(PtiError):
        ops.attention_fwd(qkv, torch.zeros(1, 96, 96, dtype=torch.bfloat16, device=dev), torch.zeros(1, 96, device=dev))
    # every other bad argument is refused before any launch too: the output buffers still hold their fill
    FILL = 7.0

    def bufs(b, l, c):
        return SimpleNamespace(qkv=torch.zeros(b, l, 3 * c, dtype=BF16, device=dev),
                               o=torch.full((b, l, c), FILL, dtype=BF16, device=dev),
                               dout=torch.zeros(b, l, c, dtype=BF16, device=dev),
                               lse2=torch.full((b, l), FILL, device=dev), delta=torch.full((b, l), FILL, device=dev),
                               dqkv=torch.full((b, l, 3 * c), FILL, dtype=BF16, device=dev))

    def untouched(t):
        torch.cuda.synchronize()
        for x in (t.o, t.lse2, t.delta, t.dqkv):
            assert bool((x == FILL).all()), "a rejected call wrote to an output"

    fwd = lambda t, **kw: ops.attention_fwd(kw.get("qkv", t.qkv), kw.get("o", t.o), kw.get("lse2", t.lse2))
    bwd = lambda t, **kw: ops.attention_bwd(kw.get("qkv", t.qkv), kw.get("o", t.o), t.dout, kw.get("lse2", t.lse2),
                                            kw.get("delta", t.delta), t.dqkv)
    err = (PtiError, ValueError, TypeError)     # a wrong dtype is a TypeError in every launcher of ops (ops._chk)
    t = bufs(1, 96, 96)                          # head dim 96, backward
    with pytest.raises(PtiError):
        bwd(t)
    untouched(t)
    t = bufs(1, 0, 64)                           # L = 0
    for call in (fwd, bwd):
        with pytest.raises((PtiError, ValueError)):
            call(t)
    t = bufs(2, 40, 64)
    wide = torch.zeros(2, 40, 6 * 64, dtype=BF16, device=dev)
    for call in (fwd, bwd):
        with pytest.raises(err):
            call(t, qkv=t.qkv.float())           # fp32 qkv
        with pytest.raises(ValueError):
            call(t, qkv=wide[..., ::2])          # non-contiguous qkv of the right shape
        untouched(t)
    with pytest.raises(ValueError):
        fwd(t, lse2=torch.full((2, 39), FILL, device=dev))
    with pytest.raises(ValueError):
        bwd(t, lse2=torch.full((2, 39), FILL, device=dev))
    with pytest.raises(ValueError):
        bwd(t, delta=torch.full((2, 41), FILL, device=dev))
    untouched(t)

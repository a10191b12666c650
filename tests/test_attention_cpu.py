"""CPU proof of tests/attention_oracle.py: every structured generator meets the conditions that make its expected values
exact, every closed form equals the float64 ``reference`` on the same input, and an fp32 emulation of the tile-streamed
algorithm reproduces them bit for bit.  Also measures how far the documented bf16 roundings (``contract``) move a result:
the constants behind the row-wise bounds of tests/test_gpu_attention.py::test_attention_rowwise_vs_fp64."""
import math

import pytest
import torch

import attention_oracle as A

F64 = torch.float64
SMALL_L = (1, 7, 31, 33, 64, 65, 117, 128, 129)
ALL_L = sorted(set(A.ONEHOT_L) | set(A.POW2_L) | set(A.RAGGED_L) | {256})


def _pair_ab(L):
    return 1, L - 2


def _fp32_exact(t):
    return bool((t.to(torch.float32).to(F64) == t).all())


def test_round_bf16_is_the_cast_on_fp32_values():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)).to(F64) * 37.0
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 1.00390625, 1.01171875, 255.5, 256.5, 16384.0], dtype=F64)])
    assert torch.equal(A.round_bf16(x), x.to(torch.float32).to(torch.bfloat16).to(F64))
    assert A.round_bf16(torch.tensor([1.00390625], dtype=F64)).item() == 1.0          # tie -> even
    assert A.round_bf16(torch.tensor([1.01171875], dtype=F64)).item() == 1.015625     # tie -> even (up)


def test_codes_differ_in_c_over_16_coordinates():
    for c in A.C_LIST:
        k = A.codes(4096, c)
        g = k @ k.t()
        g.fill_diagonal_(-math.inf)
        assert g.max().item() <= c - 2 * (c // 16)
        assert A.is_bf16(k) and A.is_bf16(128.0 * k)


@pytest.mark.parametrize("c", A.C_LIST)
def test_onehot_and_pair_margin_is_150_log2_units(c):
    """In float64: the winning score leads every other by >= MARGIN_LOG2, at every L of the GPU lists (the queries are
    scaled codes, so the margin does not depend on pi)."""
    cl2 = A.LOG2E * c ** -0.5
    for L in ALL_L:
        k = A.codes(L, c)
        s = (128.0 * k) @ k.t() * cl2
        win = s.diagonal().clone()
        assert torch.equal(win, torch.full_like(win, 128.0 * c * cl2))
        assert abs(win[0].item() - A.winning_score_log2(c)) <= 1e-9
        s.fill_diagonal_(-math.inf)
        assert (win - s.amax(-1)).min().item() >= A.MARGIN_LOG2 if L > 1 else True
        if L >= 3:                    # the pair: keys a and b tie, every third key trails
            a, b = _pair_ab(L)
            case = A.pair_case(1, L, c, a, b)
            q, kk, _ = A.split(case.qkv)
            sp = (q[0, :1] @ kk[0].t() * cl2)[0]
            assert sp[a].item() == sp[b].item() == 128.0 * c * cl2
            rest = torch.cat([sp[:a], sp[a + 1:b], sp[b + 1:]])
            assert rest.numel() == 0 or sp[a].item() - rest.max().item() >= A.MARGIN_LOG2
    # the fp32 constants the kernel multiplies with keep the winning score exact: 128 C is a power of two
    assert (128.0 * c * A.c_log2_f32(c)).item() == 128.0 * c * A.c_log2_f32(c).to(F64).item()
    # ... and the pair's lse2 = that + 1 stays in its binade, so it is exact too and p = exp2(-1) in the backward
    w = 128.0 * c * A.c_log2_f32(c).to(F64)
    assert (w.to(torch.float32) + 1.0).to(F64).item() == w.item() + 1.0


@pytest.mark.parametrize("c", A.C_LIST)
def test_integer_sums_stay_below_2_24_and_outputs_are_representable(c):
    for B, L in [(2, L) for L in ALL_L]:     # the conditions are per image: the grid-stride batches add nothing to them
        cases = [A.onehot_case(B, L, c, pi) for _, pi in A.pi_families(B, L, ("random", "all_last", "halved"))]
        cases.append(A.uniform_case(B, L, c))
        if L >= 3:
            cases.append(A.pair_case(B, L, c, *_pair_ab(L)))
        for case in cases:
            q, k, v = A.split(case.qkv)
            tag = f"{case.kind}[{B},{L},{c}]"
            # scores, P.V, dP = do.v, delta, dv: sum of |terms| of every fp32 sum
            assert c * q.abs().max().item() * k.abs().max().item() < 2 ** 24, tag
            assert v.abs().sum(1).max().item() < 2 ** 24 and case.dout.abs().sum(1).max().item() < 2 ** 24, tag
            assert c * case.dout.abs().max().item() * v.abs().max().item() < 2 ** 24, tag
            assert (case.o.abs() * case.dout.abs()).sum(-1).max().item() < 2 ** 24 * 2.0 ** -7, tag   # o: multiples of 2^-7
            assert A.is_bf16(case.o) and _fp32_exact(case.delta), tag
            for name in ("dq", "dk", "dv"):
                t = getattr(case, name)
                if t is not None and not (case.kind == "pair" and name == "dk"):
                    assert A.is_bf16(t), f"{tag} {name}"
            if case.kind == "onehot":     # rounded exactly once, from an exact fp32 sum
                assert torch.equal(case.dv, A.round_bf16(case.dv_sum)) and _fp32_exact(case.dv_sum), tag
            if case.kind == "uniform" and not A.is_pow2(L):
                # 1 / L is a hardware reciprocal (1 ulp) in the kernel: the expected o must not hinge on its last bits.
                # (At a power of two it is exact, and the product is then a plain bf16 rounding, ties included.)
                assert torch.equal(A.uniform_o(L, c, -2), A.uniform_o(L, c, 2)), \
                    f"{tag}: o depends on the last bits of the reciprocal of L"
                assert torch.equal(A.uniform_o(L, c, 0), A.uniform_o(L, c, 2)), tag
            if case.kind == "uniform":
                assert _fp32_exact(case.dv_sum / L) if A.is_pow2(L) else True, tag


@pytest.mark.parametrize("c", A.C_LIST)
def test_uniform_dq_sum_is_proven_exact(c):
    """At power-of-two L the closed-form dq of the uniform case is bit-exact for every row whose fp32 partial sums are
    proven representable: all of them where C^-1/2 is a power of two, nearly all at C = 128."""
    for L in A.POW2_L + (256,):
        case = A.uniform_case(2, L, c)
        share = case.dq_proven.to(F64).mean().item()
        print(f"uniform dq proven exact [{L},{c}]: {share:.4f} of the rows")
        assert share == 1.0 if c != 128 else share >= 0.9, (L, c, share)


@pytest.mark.parametrize("c", A.C_LIST)
def test_closed_forms_equal_the_reference(c):
    tol = 1e-9
    for L in SMALL_L:
        for name, pi in A.pi_families(2, L):
            case, tag = A.onehot_case(2, L, c, pi), f"onehot[{name},{L},{c}]"
            ref = A.reference(case.qkv, case.dout)
            for t, exp in (("o", case.o), ("dq", case.dq), ("dk", case.dk), ("dv", case.dv_sum), ("delta", case.delta)):
                assert (getattr(ref, t) - exp).abs().max().item() <= tol * max(1.0, exp.abs().max().item()), f"{tag} {t}"
            assert (ref.lse2 - case.lse2).abs().max().item() <= tol * case.lse2[0, 0].item(), tag
            assert torch.equal(ref.delta_of(case.o), case.delta), tag
        if L >= 3:
            a, b = _pair_ab(L)
            case, tag = A.pair_case(2, L, c, a, b), f"pair[{L},{c}]"
            ref = A.reference(case.qkv, case.dout)
            half = torch.zeros_like(ref.dv)
            half[:, a] = half[:, b] = case.dv_sum / 2
            for t, exp in (("o", case.o), ("dq", case.dq), ("dk", case.dk), ("dv", half), ("delta", case.delta)):
                assert (getattr(ref, t) - exp).abs().max().item() <= tol * max(1.0, exp.abs().max().item()), f"{tag} {t}"
            assert (ref.lse2 - case.lse2).abs().max().item() <= tol * case.lse2[0, 0].item(), tag
        case, tag = A.uniform_case(2, L, c), f"uniform[{L},{c}]"
        ref = A.reference(case.qkv, case.dout)
        assert (ref.o - case.o).abs().max().item() <= 2.0 ** -7 + 1e-12, tag      # one bf16 rounding of a mean in [1, 4)
        assert ref.dk.abs().max().item() <= tol and (ref.lse2 - case.lse2).abs().max().item() <= tol, tag
        assert (ref.dv - (case.dv_sum / L)[:, None]).abs().max().item() <= tol * 4.0 * L, tag
        if case.dq is not None:
            # dq is the float64 sum_j dS_ij k_j with delta taken from the bf16 o, as the kernel is handed it, up to the two
            # bf16 roundings the closed form applies: 2^-8 of each term and 2^-8 of the result
            q, k, v = A.split(case.qkv)
            ds = (case.dout @ v.transpose(1, 2) - ref.delta_of(case.o)[..., None]) * c ** -0.5 / L
            dq = ds @ k
            assert bool(((case.dq - dq).abs() <= 2.0 ** -8 * (ds.abs() @ k.abs() + dq.abs())).all()), tag


def _emulate(case):
    o, lse2 = A.stream_fwd_fp32(case.qkv)
    dq, dk, dv, delta = A.bwd_fp32(case.qkv, case.dout, o, lse2)
    return dict(o=o, lse2=lse2, dq=dq, dk=dk, dv=dv, delta=delta)


def _check_emulated(tag, case, got):
    for t in ("o", "delta", "dq", "dk", "dv"):
        exp = getattr(case, t)
        if exp is None or (case.kind == "pair" and t == "dk"):
            continue
        if case.kind == "uniform" and t == "dq":
            rows = case.dq_proven
            assert torch.equal(got[t][rows], exp[rows]), f"{tag} {t}"
            continue
        assert torch.equal(got[t], exp), f"{tag} {t}: the fp32 streamed emulation differs from the closed form"
    assert ((got["lse2"] - case.lse2).abs() <= A.ONEHOT_LSE_RTOL * case.lse2.abs()).all(), f"{tag} lse2"
    if case.kind == "pair":
        a, b = case.a, case.b
        rest = torch.ones(case.dk.shape[1], dtype=torch.bool)
        rest[[a, b]] = False
        assert not got["dk"][:, rest].any() and torch.equal(got["dk"][:, b], -got["dk"][:, a]), f"{tag} dk"
        lim = 2.0 ** -8 * (case.dk_abs[:, None] + case.dk[:, a].abs())
        assert ((got["dk"][:, a] - case.dk[:, a]).abs() <= lim).all(), f"{tag} dk_a"
        assert torch.equal(got["lse2"], case.lse2.to(torch.float32).to(F64)), f"{tag} lse2 exact"
    if case.kind == "uniform" and case.dq is None:
        ref = A.reference(case.qkv, case.dout)
        assert bool((A.rowwise_err(got["dq"], ref.dq) <= A.UNIFORM_DQ_ROW_RTOL).all()), f"{tag} dq"
        assert bool(((got["dv"] - ref.dv).abs() <= A.UNIFORM_DV_RTOL * ref.dv.abs() + 1e-12).all()), f"{tag} dv"


@pytest.mark.parametrize("c", A.C_LIST)
def test_fp32_streamed_emulation_reproduces_the_expectations(c):
    """64-key tiles, running maximum, alpha rescale, bf16 P, fp32 everywhere: bit for bit the closed forms."""
    for L in [l for l in ALL_L if l <= 1024]:
        for name, pi in A.pi_families(2, L):
            case = A.onehot_case(2, L, c, pi)
            _check_emulated(f"onehot[{name},{L},{c}]", case, _emulate(case))
        if L not in A.POW2_L + A.RAGGED_L + (256,):
            continue
        if L >= 3:
            case = A.pair_case(2, L, c, *_pair_ab(L))
            _check_emulated(f"pair[{L},{c}]", case, _emulate(case))
        case = A.uniform_case(2, L, c)
        _check_emulated(f"uniform[{L},{c}]", case, _emulate(case))
        if not A.is_pow2(L):
            case = A.uniform_case(2, L, c, shift=True)
            got = _emulate(case)
            tag = f"uniform shifted[{L},{c}]"
            assert torch.equal(got["o"], case.o) and torch.equal(got["delta"], case.delta), tag
            assert ((got["lse2"] - case.lse2).abs() <= A.ONEHOT_LSE_RTOL * case.lse2.abs()).all(), tag
            assert case.lse2.max().item() < -128.0 - math.log2(L), f"{tag}: a pad key's p = exp2(-lse2) must overflow"
            for t in ("dq", "dk"):
                f64, ab = getattr(case, t + "_f64"), getattr(case, t + "_abs")
                assert ((got[t] - f64).abs() <= 2.0 ** -8 * (ab * (1.0 + 2.0 ** -6) + f64.abs())).all(), f"{tag} {t}"
            ref = A.reference(case.qkv, case.dout)       # the closed forms against the reference (delta from the bf16 o)
            dv = (case.dv_sum / L)[:, None].expand_as(ref.dv)
            assert (ref.dv - dv).abs().max().item() <= 1e-9 and (ref.o - case.o).abs().max().item() <= 2.0 ** -7 + 1e-12, tag
            assert ((got["dv"] - dv).abs() <= A.UNIFORM_DV_RTOL * dv.abs()).all(), tag
            shift = (ref.delta_of(case.o) - ref.delta)[..., None] * c ** -0.5 / L     # dS moves by this with the fp64 delta
            k, q = A.split(case.qkv)[1], A.split(case.qkv)[0]
            assert (ref.dq - (case.dq_f64 + (shift.expand(-1, -1, L) @ k))).abs().max().item() <= 1e-9, tag
            assert (ref.dk - (case.dk_f64 + (shift.expand(-1, -1, L).transpose(1, 2) @ q))).abs().max().item() <= 1e-9, tag


def test_fp32_streamed_emulation_at_4096():
    L, c = 4096, 64
    for case in (A.onehot_case(1, L, c, A.pi_family("all_last", 1, L)), A.onehot_case(1, L, c, A.pi_family("random", 1, L)),
                 A.pair_case(1, L, c, *_pair_ab(L)), A.uniform_case(1, L, c)):
        _check_emulated(f"{case.kind}[{L},{c}]", case, _emulate(case))


def test_uniform_ragged_bounds_hold_for_the_contract():
    """The bounds that the GPU test uses for dq and dv of the uniform case at ragged L: the documented roundings alone
    (``contract`` against ``reference``) stay inside them."""
    for c in A.C_LIST:
        for L in A.RAGGED_L:
            case = A.uniform_case(2, L, c)
            ref, con = A.reference(case.qkv, case.dout), A.contract(case.qkv, case.dout)
            assert A.rowwise_err(con.dq, ref.dq).max().item() <= A.UNIFORM_DQ_ROW_RTOL, (L, c)
            assert bool(((con.dv - ref.dv).abs() <= A.UNIFORM_DV_RTOL * ref.dv.abs() + 1e-12).all()), (L, c)
            assert torch.equal(con.o, case.o) and torch.equal(con.delta, case.delta), (L, c)


def measured_contract_deviation(kind):
    dev = {k: 0.0 for k in A.CONTRACT_DEV[kind]}
    for c in A.C_LIST:
        for L in A.ROW_L:
            case = A.rowwise_case(kind, 2, L, c)
            ref, con = A.reference(case.qkv, case.dout), A.contract(case.qkv, case.dout)
            for k in dev:
                dev[k] = max(dev[k], A.rowwise_err(getattr(con, k), getattr(ref, k)).max().item())
            assert (con.lse2 - ref.lse2).abs().max().item() <= 1e-9 * max(1.0, ref.lse2.abs().max().item())
    return dev


@pytest.mark.parametrize("kind", A.ROW_KINDS)
def test_contract_deviation_matches_constants(kind):
    dev = measured_contract_deviation(kind)
    print(f"contract vs reference [{kind}], largest row-wise deviation:", {k: f"{v:.6e}" for k, v in dev.items()})
    for k, v in dev.items():
        const = A.CONTRACT_DEV[kind][k]
        assert 0.8 * const <= v <= const, (kind, k, v, const)
        assert A.ROW_BOUND[kind][k] == 3.0 * const
    for k in ("o", "dv"):         # never ill-conditioned: at most a few bf16 half-ulps, or the contract itself is off
        assert dev[k] <= 2.0 ** -7, (kind, k, dev[k])


def test_large_logit_case_spans_60_natural_units():
    for c in A.C_LIST:
        case = A.large_logit_case(2, 257, c)
        q, k, _ = A.split(case.qkv)
        s = torch.einsum("blc,bmc->blm", q, k) * c ** -0.5
        assert 45.0 <= s.max().item() <= 90.0 and -90.0 <= s.min().item() <= -45.0, (c, s.min().item(), s.max().item())


def test_uniform_dq_detects_a_scale_one_ulp_low(monkeypatch):
    """The softmax scale must be fp32(C^-1/2) to the bit: with 0.124999993 for 1/8 (a reciprocal-square-root estimate plus
    one Newton step, what `1.0f / sqrtf(64)` gave on the host under -ffast-math) the products x * scale that sit on a bf16
    tie fall below it, and the exact dq of the uniform case differs."""
    case = A.uniform_case(2, 64, 64)
    o, lse2 = A.stream_fwd_fp32(case.qkv)
    assert torch.equal(A.bwd_fp32(case.qkv, case.dout, o, lse2)[0], case.dq)
    low = torch.nextafter(torch.tensor(0.125, dtype=torch.float32), torch.tensor(0.0, dtype=torch.float32))
    monkeypatch.setattr(A, "scale_f32", lambda c: low)
    assert not torch.equal(A.bwd_fp32(case.qkv, case.dout, o, lse2)[0], case.dq)

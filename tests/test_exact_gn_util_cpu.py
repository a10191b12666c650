"""CPU checks of tests/exact_gn_util.py: (1) every case tests/test_gpu_exact_groupnorm.py runs is built here, which runs
every condition that makes an exact comparison valid -- on the reference alone; (2) every backward case evaluated once in
fp32 torch with a shuffled pixel order, slab-wise sums and reversed channel / sample order EQUALS the float64 reference:
the summation order cannot matter; (3) the hand-written statistics table and the comparator notice what they must.
"""
import pytest
import torch

import exact_gn_util as X
import exact_util as E
from test_gpu_ops import _report

BWD = X.bwd_rows()
PRO = X.prologue_rows()


@pytest.mark.parametrize("row", BWD, ids=[r["id"] for r in BWD])
def test_backward_cases_meet_the_conditions_in_any_summation_order(row):
    c = X.make_bwd_case(row)
    print(f"[exact gn] bwd {row['id']}: pow2={c.s.pow2} rstd={sorted(set(c.s.rstd.flatten().tolist()))} {c.info}")
    assert c.s.pow2 == (((c.s.cnt) & (c.s.cnt - 1)) == 0)
    for with_res, ref in ((False, c.ref), (True, c.ref_res)):
        sums, dx, dgamma, dbeta = X.fp32_shuffled_eval(c, with_res, seed=row["seed"])
        E.assert_exact("fp32 shuffled sums", sums, ref.sums, layout="flat")
        E.assert_exact("fp32 shuffled dx", dx, ref.dx)
        E.assert_exact("fp32 shuffled dx, stored", dx.to(torch.bfloat16), ref.dx16)
        E.assert_exact("fp32 shuffled dgamma", dgamma, ref.dgamma, layout="flat")
        E.assert_exact("fp32 shuffled dbeta", dbeta, ref.dbeta, layout="flat")


@pytest.mark.parametrize("row", PRO, ids=[r["id"] for r in PRO])
def test_prologue_cases_meet_the_conditions(row):
    c = X.make_prologue_case(row)
    print(f"[exact gn] prologue {row['id']}: {c.info}")
    # beta != 0 is what makes a normalised padding pixel visible: a pad pixel read as x = 0 would stage sh = beta - m * sc
    sh = c.s.b4 - c.s.m4 * c.s.r4 * c.s.g4
    assert (sh != 0).to(torch.float64).mean().item() >= 0.5


def test_direct_and_weight_gradient_prologue_cases_meet_the_conditions():
    for k, (n, cin, cout, h, w, g, _) in enumerate(X.DIRECT_PROLOGUE):
        c = X.make_prologue_case(X.direct_row(n, cin, cout, h, w, g, k=k))
        X.check_f32("conv_direct reference", c.conv + c.bias.view(1, -1, 1, 1))
    for k, (n, cw, cn, h, w) in enumerate(X.WGRAD_DIRECT_PROLOGUE):
        X.make_wgrad_prologue_case(X.direct_row(n, cw, cn, h, w, 16, k=10 + k))
    for row in X.wgrad_rows():
        X.make_wgrad_prologue_case(row)


def test_fused_chained_and_tie_in_cases_meet_the_conditions():
    for row in X.fused_rows():
        c = X.make_fused_case(row)
        print(f"[exact gn] fused {row['id']}: max |conv^T dy| = {c.g.abs().max().item():g}")
        X.make_fused_case(row, silu_plumbing=True)
    for row in X.chain_rows():
        c = X.make_chain_case(row)
        print(f"[exact gn] chain {row['id']}: {X.rounded_share(c.up_ref.dx):.2f} of dx_in and "
              f"{X.rounded_share(c.conv):.2f} of dy_out round")
    X.make_tie_in_case()
    for row in BWD[:1] + BWD[5:6]:
        X.make_silu_bwd_case(row)


# ---- (3) the helpers notice what they must ---------------------------------------------------------------------------
def test_statistics_table_is_read_back_exactly_and_inexact_tables_are_refused():
    t = X.make_gn_stats(2, 4, 512, torch.tensor([[-3., -1, 0, 2], [1, 2, 3, -2]]), 3.75)
    assert torch.equal(X.stat_f(t).double(), t.double() / X.STAT_SCALE)
    assert t[0, 0, 0].item() == -3 * 512 * 65536 and t[0, 0, 1].item() == int(512 * 12.75 * 65536)
    with pytest.raises(AssertionError):
        X.make_gn_stats(1, 1, 512, 1.0, 2.0 ** -30)                  # cnt * v is no multiple of 2^-16
    with pytest.raises(AssertionError):
        X.make_gn_stats(1, 1, 3 * 2 ** 20 + 1, 2 ** 11 + 1.0, 0.0)   # a high half beyond 24 bits


def test_exact_sum_refuses_a_sum_that_could_round():
    X.exact_sum("ok", [torch.tensor([2.0 ** 22, 0.5])], 0.5, dim=0)
    with pytest.raises(AssertionError):
        X.exact_sum("too long", [torch.tensor([2.0 ** 22, 0.5])], 0.125, dim=0)
    with pytest.raises(AssertionError):
        X.exact_sum("off grid", [torch.tensor([0.75])], 0.5)


def test_localised_mistakes_pass_the_tolerance_gates_and_fail_the_exact_comparison():
    """Localised mistakes, made here on the reference's own arithmetic: a store that truncates instead of rounding to
    nearest even passes the gates of tests/test_gpu_fused_gnbwd.py (1.5 % of the largest value, rel-L2 6e-3; here 3.7e-3), one
    tail element left out of the sums those of tests/test_gpu_ops2.py::test_gn_bwd (1 %, 3e-3), both against an unrounded
    reference; a third is one 8-channel piece read with its neighbour group's mean.  The exact comparison fails on each and says where."""
    c = X.make_bwd_case(BWD[8])                                         # 2 x 128 @ 16 x 16
    s, ref = c.s, c.ref
    trunc = (ref.dx.to(torch.float32).view(torch.int32) & -65536).view(torch.float32)
    _report("truncating store", trunc, ref.dx, max_frac=1.5e-2, l2=6e-3)    # (against the unrounded value, as those tests do)
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        E.assert_exact("truncating store", trunc, ref.dx16)
    # one element (channel 3, the last pixel) missing from S1 / S2 of sample 1: c1 and c2 of its group move, and with them
    # every element of the group
    dy_cut = c.dy.clone()
    dy_cut[1, 3, -1, -1] = 0
    cut = X.gn_bwd_ref(s, c.x, dy_cut)
    leak = s.r4 * (s.g4 * c.dy - X._per_channel(cut.c1, s.cpg) - (c.x - s.m4) * s.r4 * X._per_channel(cut.c2, s.cpg))
    _report("one tail pixel left out", X.round16(leak), ref.dx, max_frac=1e-2, l2=3e-3)
    with pytest.raises(AssertionError, match=r"\(n=1, "):
        E.assert_exact("one tail pixel left out", X.round16(leak), ref.dx16)
    assert E.mismatches(X.round16(leak)[:1], ref.dx16[:1])[0] == 0     # sample 0 is untouched
    # one 8-channel piece mapped to the wrong group
    m4 = s.m4.clone()
    m4[:, 8:16] = s.m4[:, 16:24]
    wrong = s.r4 * (s.g4 * c.dy - X._per_channel(ref.c1, s.cpg) - (c.x - m4) * s.r4 * X._per_channel(ref.c2, s.cpg))
    with pytest.raises(AssertionError, match="32-channel block 0"):
        E.assert_exact("wrong group", wrong.to(torch.float32).to(torch.bfloat16), ref.dx16)
    count, bad = E.mismatches(wrong.to(torch.float32).to(torch.bfloat16), ref.dx16)
    assert count > 0 and all(8 <= e["channel"] < 16 for e in bad)

"""CPU checks of tests/exact_util.py: (1) every case tests/test_gpu_exact_parity.py runs meets the conditions that make an
exact comparison valid -- on the reference alone; (2) the sensitivity gap: with the data of
tests/test_gpu_ops.py::test_conv_mfma, a 256 -> 256 3x3 output that lacks ONE x*w term of its 2304 passes ``_report`` at
its stated gates, and the same edit on the integer case is caught by ``assert_exact``; (3) ``assert_exact`` decodes tile
positions and channel blocks as placed by hand.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_util as E
from test_gpu_ops import _gn_ref, _r, _report


# ---- (1) the conditions hold for every case of the GPU file ----------------------------------------------------------
@pytest.mark.parametrize("row", E.FWD_CASES, ids=[r["id"] for r in E.FWD_CASES])
def test_forward_cases_meet_the_conditions(row):
    c = E.make_fwd_case(row)
    print(f"[exact cases] fwd {row['id']}: {c.info}")
    assert c.info["max16"] <= E.LIMIT16 and c.info["zero"] <= E.MAX_ZERO and c.info["density"] >= E.MIN_DENSITY
    assert c.info.get("sum32", 0.0) < E.LIMIT32
    assert (c.ref_full is not None) == row["residual"] and hasattr(c, "pool") == row["pooled"]


@pytest.mark.parametrize("name", list(E.WGRAD_CASES))
def test_weight_gradient_cases_meet_the_conditions(name):
    c = E.make_wgrad_case(name)
    print(f"[exact cases] wgrad {name}: {c.info}")
    assert 2 * c.info["sum32"] < E.LIMIT32          # the accumulate=True launch doubles every sum
    assert c.dw.shape == (c.cout, c.cin, c.ks, c.ks) and c.db.shape == (c.cout,)
    assert all(k in E.WGRAD_CASES for k in E.WGRAD_F16_X)


def test_batched_and_direct_weight_gradient_cases_meet_the_conditions():
    for i in range(len(E.BATCHED_JOBS)):
        assert 2 * E.make_batched_case(i).info["sum32"] < E.LIMIT32
    for row in E.WGRAD_DIRECT_CASES:
        c = E.make_wgrad_direct_case(*row)
        print(f"[exact cases] wgrad_direct {row}: {c.info}")
        assert c.info["sum32"] < E.LIMIT32


def test_direct_stats_and_pool_cases_meet_the_conditions():
    rows = E.direct_rows()
    assert len(rows) == 18
    for rid, n, cin, cout, h, w, il, ol in rows:
        c = E.make_direct_case(n, cin, cout, h, w, ol.endswith("bf16"))
        print(f"[exact cases] direct {rid}: {c.info}")
        assert c.info["sum32"] < E.LIMIT32 and (not ol.endswith("bf16") or c.info["max16"] <= E.LIMIT16)
    for k, shape in enumerate(E.STATS_CASES):
        c = E.make_stats_case(*shape, seed=k)
        assert c.ref.shape == (shape[0], E.STATS_GROUPS, 2) and c.ref.dtype == torch.int64
    assert E.make_pool_case().ref.abs().max().item() <= E.LIMIT16


def test_conditions_refuse_what_would_round():
    with pytest.raises(AssertionError, match="16-bit store"):
        E.check_store16("t", torch.tensor([1.0, -257.0], dtype=E.F64))
    with pytest.raises(AssertionError, match="not integer"):
        E.check_store16("t", torch.tensor([0.5], dtype=E.F64))
    with pytest.raises(AssertionError, match="2\\^24"):
        E.check_sum32("t", 2.0 ** 24)
    wt = torch.ones(64, 64, 3, 3, dtype=E.F64)
    assert E.check_density("t", wt) == 1.0
    wt[32:, :32, 1, 2] = 0
    wt[32:34, :31, 1, 2] = 1                      # 62 of 1024 < 1/16
    with pytest.raises(AssertionError, match="non-zero"):
        E.check_density("t", wt)
    with pytest.raises(AssertionError, match="is zero"):
        E.check_zero_fraction("t", torch.tensor([0.0] * 2 + [1.0] * 17, dtype=E.F64))
    E.check_zero_fraction("t", torch.tensor([0.0] * 2 + [1.0] * 18, dtype=E.F64))


# ---- (2) the sensitivity gap --------------------------------------------------------------------------------------------
def _existing_case(pro):
    """The (1, 256, 256, 8, 16, 3, 's1', 2, True, True) row of tests/test_gpu_ops.py::CONV_CASES as test_conv_mfma builds it
    (``pro`` = 0: the same draws without the GroupNorm + SiLU prologue, the distribution the gate's arithmetic speaks of)."""
    torch.manual_seed(1)
    n, cin, cout, h, w, ks = 1, 256, 256, 8, 16, 3
    x = _r(torch.randn(n, cin, h, w) * 1.3 + 0.2)
    wt = _r(torch.randn(cout, cin, ks, ks) / (cin * ks * ks) ** 0.5)
    bias = torch.randn(cout) * 0.1
    gamma = 1 + 0.2 * torch.randn(cin)
    beta = 0.1 * torch.randn(cin)
    a = _r(_gn_ref(x, 16, gamma, beta, 1e-6, pro == 2)) if pro else x
    ref = F.conv2d(a, wt, bias, padding=1)
    ref = ref + _r(torch.randn_like(ref))
    return a, wt, ref


@pytest.mark.parametrize("pro", [2, 0])
def test_tolerance_gate_accepts_a_missing_term_at_256_channels(pro):
    """One output element of the last output channel loses ONE x*w term, and ``_report`` at the gates of test_conv_mfma
    accepts the result.  Two elements: an interior pixel (all 2304 terms) and the tile's corner pixel (on this 8 x 16 map
    also the map's corner: 4 taps, 1024 terms).  The term removed is the centre tap of the last channel of the first
    128-channel cin chunk with the test's own data (pro 2), and the element's term of median magnitude in both variants.
    The share of each element's terms whose loss the gate accepts is printed and must be at least nine in ten: the gate is
    not blind to EVERY term (the few largest exceed it), it is blind to nearly all of them."""
    a, wt, ref = _existing_case(pro)
    co = 255
    gate = 1e-2 * ref.abs().max().item()
    for y, x in ((3, 7), (7, 15)):
        patch = F.pad(a, (1, 1, 1, 1))[0, :, y:y + 3, x:x + 3]
        terms = (patch * wt[co]).flatten()
        terms = terms[terms != 0]
        picks = [terms[terms.abs().argsort()[terms.numel() // 2]].item()]
        if pro == 2:
            picks.append((a[0, 127, y, x] * wt[co, 127, 1, 1]).item())
        for term in picks:
            assert term != 0.0
            broken = ref.clone()
            broken[0, co, y, x] -= term
            _report(f"one term of {terms.numel()} missing at ({y},{x}) (pro{pro}, term {term:+.4f})", _r(broken), ref)   # passes
        lost = (_r(ref[0, co, y, x] - terms) - ref[0, co, y, x]).abs()
        share = (lost <= gate).double().mean().item()
        print(f"[sensitivity pro{pro} ({y},{x})] max|ref| {ref.abs().max().item():.3f} -> gate {gate:.4f}; |term| median "
              f"{terms.abs().median().item():.4f} max {terms.abs().max().item():.4f} over {terms.numel()} terms; the gate "
              f"accepts the loss of {share:.1%} of them one at a time, and of "
              f"{int(gate / terms.abs().median().item())} median terms at once")
        assert share >= 0.9


def _integer_256():
    row = next(r for r in E.FWD_CASES if r["cin"] == 256 and r["mode"] == "s1")
    return E.make_fwd_case(row)


def test_exact_comparator_catches_the_same_missing_term():
    c = _integer_256()
    n, co, y, x = 0, 255, 7, 15
    ci = max(k for k in range(128) if c.x[n, k, y, x] * c.w[co, k, 1, 1] != 0)      # the last live channel of the first chunk
    term = (c.x[n, ci, y, x] * c.w[co, ci, 1, 1]).item()
    good = c.ref_full.to(torch.bfloat16)
    E.assert_exact("integer case, bf16 store", good, c.ref_full)                       # the bf16 store is exact
    E.assert_exact("integer case, fp16 store", c.ref_full.to(torch.float16), c.ref_full)
    broken = c.ref_full.clone()
    broken[n, co, y, x] -= term
    with pytest.raises(AssertionError) as info:
        E.assert_exact("one term of 2304 missing", broken.to(torch.bfloat16), c.ref_full)
    msg = str(info.value)
    print(msg)
    assert "1 of " in msg and "(n=0, y=7, x=15, channel=255)" in msg and "tile (0, 0) corner" in msg
    assert "32-channel block 7" in msg
    # ... while the tolerance gate takes the integer case's loss as well: |term| <= 2 against a gate of ~1.5
    _report("the same edit under the tolerance gate", broken.float(), c.ref_full.float())


# ---- (3) the comparator's decoding --------------------------------------------------------------------------------------
def test_assert_exact_locates_hand_placed_mismatches():
    ref = torch.arange(2 * 64 * 13 * 19, dtype=E.F64).reshape(2, 64, 13, 19) % 200
    got = ref.clone()
    placed = {
        (0, 0, 0, 0): ("corner", (0, 0), 0),
        (0, 31, 7, 15): ("corner", (0, 0), 0),
        (0, 32, 3, 5): ("interior", (0, 0), 1),
        (1, 33, 8, 7): ("edge", (1, 0), 1),
        (1, 63, 4, 16): ("edge", (0, 1), 1),
        (1, 5, 12, 3): ("interior, last row", (1, 0), 0),
        (0, 40, 12, 18): ("interior, last row, last column", (1, 1), 1),
        (1, 2, 8, 18): ("edge, last column", (1, 1), 0),
    }
    for idx in placed:
        got[idx] += 1
    count, bad = E.mismatches(got, ref)
    assert count == len(placed)
    for e in bad:
        where, tile, blk = placed[e["index"]]
        assert (e["where"], e["tile"], e["cblock"]) == (where, tile, blk), e
        assert e["got"] == e["ref"] + 1
    # the same through an NHWC tensor in a 16-bit format, as the kernels store it
    count2, bad2 = E.mismatches(got.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16), ref, layout="nhwc")
    assert [e["index"] for e in bad2] == [e["index"] for e in bad]
    with pytest.raises(AssertionError) as info:
        E.assert_exact("hand placed", got, ref, show=3)
    msg = str(info.value)
    assert "8 of" in msg and msg.count("got ") == 3 and "touched" in msg
    # a pooled output's tile is 4 x 8
    assert E.tile_position(3, 7, 6, 10, tile=(4, 8)) == "corner"
    assert E.tile_position(4, 9, 6, 10, tile=(4, 8)) == "edge, last column"


def test_assert_exact_on_weight_gradients_statistics_and_nan():
    ref = torch.ones(64, 96, 3, 3, dtype=E.F64)
    got = ref.float()
    got[40, 70, 2, 1] = 3
    with pytest.raises(AssertionError, match=r"\(cout=40, cin=70, tap=7\).*cout block 1, cin block 2"):
        E.assert_exact("dw", got, ref, layout="dw")
    st = torch.tensor([[[5, 25], [-3, 9]]], dtype=torch.int64)
    E.assert_exact("stats", st, st.to(E.F64), layout="flat")
    with pytest.raises(AssertionError, match=r"index \(0, 1, 0\): got -2 ref -3"):
        E.assert_exact("stats", st + torch.tensor([[[0, 0], [1, 0]]]), st.to(E.F64), layout="flat")
    nan = torch.ones(1, 32, 8, 16)
    nan[0, 3, 2, 2] = float("nan")
    with pytest.raises(AssertionError, match="1 of 4096"):
        E.assert_exact("nan", nan, torch.ones(1, 32, 8, 16, dtype=E.F64))
    with pytest.raises(AssertionError, match="shape"):
        E.assert_exact("shape", torch.ones(2, 2), torch.ones(2, 3, dtype=E.F64))

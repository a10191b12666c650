"""CPU tests of the uniform-window SSIM path: the oracles of ``tests/ssim_uniform_oracle.py`` against each other, against answers
worked by hand and against ``tests/golden/ssim_uniform_golden.npz``; the mistakes the golden cases must notice; the ``"SSIM"``
row of ``utils.compare_metrics``; and what ``ops.ssim_uniform`` / ``pti_ssim_uniform`` refuse before any launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ssim_uniform_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ssim_uniform_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return O.unpack_cases(z)


# ---- golden file and oracles --------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_generator_writes(gold):
    cases, expected = gold
    assert cases == O.case_list()
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert {(c["h"], c["w"]) for c in cases} == set(O.SHAPES)
    for c, want in zip(cases, expected):
        x, y = O.case_pair(c)
        got = O.ssim_valid(x, y)
        assert got[1] == want[1] and abs(got[0] - want[0]) <= 1e-15, c["name"]
        lit = O.ssim_scipy(x, y)
        assert lit[1] == want[1] and abs(lit[0] - want[0]) <= 1e-12, c["name"]
    by_name = {c["name"]: e for c, e in zip(cases, expected)}
    for shape in ("45x71", "64x64"):
        assert abs(by_name[f"{shape}_identical"][0] - 1.0) <= 1e-12
        assert by_name[f"{shape}_flat_gt"].tolist() == [0.0, 0.0]
        assert by_name[f"{shape}_offset-0.6"][1] < 0.51 and 100.0 < by_name[f"{shape}_offset+100"][1] < 101.0
        assert by_name[f"{shape}_noise0.2"][0] < by_name[shape][0] < by_name[f"{shape}_noise0.01"][0] < 1.0


def test_answers_worked_by_hand():
    rs = np.random.RandomState(5)
    x = rs.rand(23, 31).astype(np.float32)
    for fn in (O.ssim_valid, O.ssim_scipy, O.ssim_fp32):
        assert abs(fn(x, x)[0] - 1.0) <= (1e-12 if fn is not O.ssim_fp32 else 1e-6)          # identical images
        flat = np.full((9, 12), 0.375, dtype=np.float32)
        assert fn(flat, flat) == (0.0, 0.0)                                                   # no range: 0 / 0, reported as {0, 0}
        assert abs(fn(flat, flat, data_range=1.0)[0] - 1.0) <= 1e-12                          # a flat pair with a range given
        assert fn(flat, np.zeros_like(flat), data_range=0.0) == (0.0, 0.0)
    # 7 x 7: ONE window, the whole image -- plain means and the sample covariance matrix
    x, y = rs.rand(7, 7).astype(np.float32), rs.rand(7, 7).astype(np.float32)
    a, b = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
    cov = np.cov(np.stack([a, b]), ddof=1)
    R = float(x.max()) - float(x.min())
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    want = ((2 * a.mean() * b.mean() + c1) * (2 * cov[0, 1] + c2)) / ((a.mean() ** 2 + b.mean() ** 2 + c1) * (cov[0, 0] + cov[1, 1] + c2))
    for fn, tol in ((O.ssim_valid, 1e-13), (O.ssim_scipy, 1e-13), (O.ssim_fp32, 1e-5)):
        got = fn(x, y)
        assert got[1] == R and abs(got[0] - want) <= tol, fn.__name__
    # an explicit range is used as it is
    assert O.ssim_valid(x, y, data_range=2.5)[1] == 2.5 and O.ssim_valid(x, y, data_range=2.5)[0] != O.ssim_valid(x, y)[0]


def test_the_fp32_restatement_is_close_and_the_gates_follow_it(gold):
    cases, _ = gold
    d, g = O.d_ref(cases), O.gates(cases)
    by_name = {c["name"]: c for c in cases}
    assert O.FLOOR == 2.0 ** -24
    for c in cases:
        print(f"{c['name']:22s} D_ref {d[c['name']]:.3e} gate {g[c['name']]:.3e}")
        twin = d[f"{c['h']}x{c['w']}"] if c["offset"] != 0.0 else 0.0
        assert by_name[f"{c['h']}x{c['w']}"]["offset"] == 0.0 and g[c["name"]] == 8.0 * max(d[c["name"]], twin, 2.0 ** -24)
        # moments about a pixel of the window: fp32 stays within a few roundings of fp64 whatever the object's offset is
        assert d[c["name"]] <= 1e-6
    assert max(d[c["name"]] for c in cases if c["offset"] == 100.0) <= 1e-7


MUTATIONS = {
    "population covariance": lambda x, y, m: O.ssim_valid(x, y, cn=1.0),
    "window 5": lambda x, y, m: O.ssim_scipy(x, y, win=5),
    "window 9": lambda x, y, m: O.ssim_scipy(x, y, win=9),
    "no crop": lambda x, y, m: O.ssim_scipy(x, y, crop=False),
    "R = 1": lambda x, y, m: O.ssim_valid(x, y, data_range=1.0),
    "K2 = 0.02": lambda x, y, m: O.ssim_valid(x, y, k2=0.02),
    "raw prediction": lambda x, y, m: O.ssim_valid(x, np.where(m, y, np.float32(0.05)).astype(np.float32)),
}
MUTATION_CASES = [c for c in O.case_list() if c["variant"] == "noisy" and c["noise"] >= 0.05 and min(c["h"], c["w"]) >= 45]


@pytest.mark.parametrize("case", MUTATION_CASES, ids=lambda c: c["name"])
def test_golden_cases_tell_each_mistake_from_the_rule(case):
    """Each mutation must move the result by more than the case's gate, on every case with noise >= 0.05 and h, w >= 45.

    The gate is ``8 * max(D_ref(case), D_ref at offset 0, 2^-24)``: 4.8e-7 on every one of these cases (the fp32 restatement is
    6e-10 .. 7e-9 from fp64 on them, the +100 offset included, since the moments are taken about a pixel of the window).  The
    smallest movements: the population covariance's, 2.3e-6 at +100 (where C2 = 9.1 swamps the variance terms) and 6.2e-6 ..
    3.8e-5 elsewhere, then windows 5 and 9 at +100, 6.3e-6 .. 7.5e-6."""
    x, y = O.case_pair(case)
    m = O.ellipse_mask(case["h"], case["w"])
    base, gate = O.ssim_valid(x, y)[0], O.gates(O.case_list())[case["name"]]
    moved = {name: abs(fn(x, y, m)[0] - base) for name, fn in MUTATIONS.items()}
    print(case["name"], f"gate {gate:.3e}", {k: f"{v:.3e}" for k, v in moved.items()})
    assert {k: v for k, v in moved.items() if not v > gate} == {}


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------
def _rows(n):
    """Count and sum rows of n pairs that are measured: a 4 x 3 box on both sides."""
    from pti_ldm_vae_amd.utils import compare_metrics as M
    row = dict.fromkeys(M.COLUMNS, 0)
    row.update(n_gt=12, n_pred=12, components_gt=1, components_pred=1, kept_gt=12, kept_pred=12, filled_pred=12, intersection=12,
               union=12, gt_x=1, gt_y=1, gt_w=4, gt_h=3, pred_x=1, pred_y=1, pred_w=4, pred_h=3, gt_width_upper=4, gt_width_middle=4,
               gt_width_lower=4, pred_width_upper=4, pred_width_middle=4, pred_width_lower=4)
    counts = np.array([[row[k] for k in M.COLUMNS]] * n, dtype=np.int32)
    sums = np.array([[0.5 + i, 1.0, 0.75] for i in range(n)], dtype=np.float64)
    return counts, sums


def test_pair_metrics_aggregate_and_csv_rows_carry_the_ssim_row():
    from pti_ldm_vae_amd.utils import compare_metrics as M
    counts, sums = _rows(4)
    plain = M.pair_metrics(counts, sums, 9, 8)
    assert all(tuple(m) == M.METRIC_KEYS for m in plain)                                      # without the argument: as before
    ssim = np.array([[0.9, 0.75], [0.5, 1.5], [0.0, 0.0], [0.7, 0.8]])
    got = M.pair_metrics(counts, sums, 9, 8, ssim=ssim)
    want_keys = ("MSE", "SSIM") + M.METRIC_KEYS[1:]
    assert all(tuple(m) == want_keys for m in got)
    assert [m["SSIM"] for m in got] == [0.9, 0.5, None, 0.7]                                   # range 0: None, the pair stays
    for m, p in zip(got, plain):
        assert {k: v for k, v in m.items() if k != "SSIM"} == p
    assert json.dumps([{k: v for k, v in m.items() if k != "SSIM"} for m in got]) == json.dumps(plain)
    small = M.pair_metrics(counts, sums, 6, 40, ssim=np.zeros((4, 2)))                         # an edge below 7: None whatever the row says
    assert [m["SSIM"] for m in small] == [None] * 4 and small[0]["MSE"] == 0.5 / 240
    assert [m["SSIM"] for m in M.pair_metrics(counts, sums, 40, 6, ssim=ssim)] == [None] * 4
    with pytest.raises(ValueError, match="ssim rows"):
        M.pair_metrics(counts, sums, 9, 8, ssim=ssim[:3])
    counts[1, M.COLUMNS.index("kept_pred")] = 0                                                # a skipped pair is still skipped
    assert M.pair_metrics(counts, sums, 9, 8, ssim=ssim)[1] == M.NO_PRED
    counts, sums = _rows(4)
    # aggregate: the row sits after MSE, None is left out, the worst value is the SMALLEST
    agg, agg_plain = M.aggregate(got), M.aggregate(plain)
    assert list(agg) == list(want_keys) and "SSIM" in M.HIGHER_IS_BETTER_OPTIONAL and "SSIM" not in M.HIGHER_IS_BETTER
    a = agg["SSIM"]
    assert (a["n"], a["none"], a["worst"]) == (3, 1, 0.5) and abs(a["mean"] - 0.7) < 1e-15
    assert {k: v for k, v in agg.items() if k != "SSIM"} == agg_plain
    thresholds = M.threshold_counts(got)
    assert thresholds == M.threshold_counts(plain)
    rows, rows_plain = M.metrics_csv_rows(agg, thresholds, 4), M.metrics_csv_rows(agg_plain, thresholds, 4)
    assert [r["Metric"] for r in rows][:3] == ["MSE", "SSIM", "PSNR"] and rows[1]["Average"] == 0.7 and rows[1]["Worst Value"] == 0.5
    assert [r for r in rows if r["Metric"] != "SSIM"] == rows_plain
    assert M.aggregate(small)["SSIM"]["n"] == 0 and M.aggregate(small)["SSIM"]["mean"] is None


def test_the_flag_is_off_by_default_and_leaves_the_arguments_alone(tmp_path):
    from pti_ldm_vae_amd import compare_images as cli
    args = cli.parse_args(["--results-dir", str(tmp_path)])
    assert args.ssim is False
    assert cli.parse_args(["--results-dir", str(tmp_path), "--ssim", "--straighten"]).ssim is True


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
def test_ops_ssim_uniform_refuses_before_a_launch():
    from pti_ldm_vae_amd import ops
    assert ops.SSIM_UNIFORM_MIN_EDGE == O.WIN == 7 and ops.SSIM_UNIFORM_COLUMNS == ("ssim", "data_range")
    a = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="CUDA"):
        ops.ssim_uniform(a, a)                                          # right dtype, host tensors
    for gt, pred in ((a.double(), a), (a, a.half()), (a.numpy(), a), (a, None), (a.int(), a)):
        with pytest.raises(TypeError, match="float32"):
            ops.ssim_uniform(gt, pred)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="data_range"):
            ops.ssim_uniform(a, a, data_range=bad)
    with pytest.raises(TypeError, match="float32"):
        ops.mask_compare(a.double(), a, cleaned=True)


def test_pti_ssim_uniform_validates_before_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(64)      # never dereferenced: every call below returns before a launch
    ws = h.pti_ssim_uniform_ws_bytes

    def call(x=p, y=p, n=2, hh=8, w=9, rng=-1.0, out=p, wsp=p, ws_bytes=None):
        return h.pti_ssim_uniform(x, y, n, hh, w, rng, out, wsp, ws(n, hh, w) if ws_bytes is None else ws_bytes, None)

    for kw in ({"x": None}, {"y": None}, {"out": None}, {"wsp": None}):
        assert call(**kw) == -1, kw
        assert b"null pointer" in h.pti_last_error_string()
    for kw in ({"n": 0}, {"n": -1}):
        assert call(**dict(kw, ws_bytes=1 << 20)) == -1 and b"bad batch" in h.pti_last_error_string(), kw
    for kw in ({"hh": 6}, {"w": 6}, {"hh": 1025}, {"w": 1025}, {"hh": 0}, {"n": 65536}):
        assert call(**dict(kw, ws_bytes=1 << 40)) == -2 and b"unsupported" in h.pti_last_error_string(), kw
    assert call(rng=float("nan")) == -1 and b"NaN" in h.pti_last_error_string()
    for kw in ({"x": C.c_void_p(66)}, {"y": C.c_void_p(65)}, {"out": C.c_void_p(68)}):
        assert call(**kw) == -1 and b"misaligned" in h.pti_last_error_string(), kw
    assert call(wsp=C.c_void_p(68)) == -1 and b"8-byte aligned" in h.pti_last_error_string()
    assert call(ws_bytes=ws(2, 8, 9) - 1) == -1 and b"workspace of" in h.pti_last_error_string()
    assert call(hh=1024, w=1024, ws_bytes=8) == -1 and b"workspace of" in h.pti_last_error_string()   # the caps pass the shape test
    # the size query: pure host arithmetic -- one double per 32 x 32 tile of the valid region, 64 {min, max} pairs per image
    assert ws(1, 7, 7) == 8 + 512 and ws(1, 38, 38) == 8 + 512 and ws(1, 39, 39) == 4 * 8 + 512 and ws(3, 45, 71) == 3 * (2 * 3 * 8 + 512)
    assert ws(1, 1024, 1024) == 1024 * 8 + 512
    assert ws(0, 8, 8) == ws(1, 6, 8) == ws(1, 8, 6) == ws(1, 1025, 8) == ws(1, 8, 1025) == 0
    # the cleaned output of the comparison launch
    q = h.pti_mask_compare_ws_bytes(2, 8, 8)
    assert h.pti_mask_compare_cleaned(p, p, 2, 8, 8, 0.2, p, p, None, p, q, None) == -1 and b"null pointer" in h.pti_last_error_string()
    assert h.pti_mask_compare_cleaned(p, p, 2, 8, 8, 0.2, p, p, C.c_void_p(130), p, q, None) == -1 and b"misaligned" in h.pti_last_error_string()
    assert h.pti_mask_compare_cleaned(p, p, 2, 8, 8, 0.2, p, p, p, p, q, None) == -1 and b"alias" in h.pti_last_error_string()
    assert h.pti_mask_compare_cleaned(p, p, 2, 8, 1025, 0.2, p, p, C.c_void_p(128), p, q, None) == -2

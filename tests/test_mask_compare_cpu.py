"""CPU tests of the image-comparison path: the oracle of ``tests/mask_compare_oracle.py`` against hand-worked answers, its
two implementations (scipy, pure numpy) against each other on every golden input, the golden cases' power to tell each of
five plausible mistakes from the rule, ``utils.compare_metrics`` against a direct numpy restatement of the reference's
formulas, and every refusal of ``ops.mask_compare`` / ``pti_mask_compare`` / the command that returns before a launch."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import mask_compare_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mask_compare_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return O.unpack_cases(z)


def _row(g, r, **kw):
    return dict(zip(O.COLUMNS, O.table_masks(g, r, **kw)))


# ---- oracle against hand-worked answers ----------------------------------------------------------------------------------
def test_checkerboard_is_one_component_of_13_and_fills_to_17():
    box = np.zeros((5, 5), dtype=bool)
    box[1:4, 1:4] = True
    for impl in ("scipy", "numpy"):
        row = _row(box, O.CHECKER, impl=impl)
        assert (row["n_pred"], row["components_pred"], row["kept_pred"], row["filled_pred"]) == (13, 1, 13, 17)
        # P = the checkerboard plus its four enclosed gaps (1,2) (2,1) (2,3) (3,2); the eight gaps on the border stay open
        assert (row["intersection"], row["union"]) == (9, 17)
        assert [row[k] for k in ("pred_x", "pred_y", "pred_w", "pred_h")] == [0, 0, 5, 5]
        # rows 1, 2, 3 of P: .###.  #####  .###.
        assert [row[k] for k in ("pred_width_upper", "pred_width_middle", "pred_width_lower")] == [3, 5, 3]
        assert _row(box, O.CHECKER, impl=impl, conn=4)["components_pred"] == 13


def test_ring_with_island_and_broken_rings():
    hand = O.hand_masks()
    full = np.ones((9, 11), dtype=bool)
    for impl in ("scipy", "numpy"):
        row = _row(full, hand["ring_island"], impl=impl)
        # 7 x 9 ring = 28 pixels, island 2; the island lies in the hole: P is the whole 7 x 9 box
        assert (row["n_pred"], row["components_pred"], row["kept_pred"], row["filled_pred"]) == (30, 2, 28, 63)
        row = _row(np.ones((9, 9), dtype=bool), hand["ring_diagonal_gap"], impl=impl)
        # a 7 x 7 ring without one corner: 23 pixels, still one component, and the 5 x 5 hole stays closed to 4-steps
        assert (row["n_pred"], row["components_pred"], row["filled_pred"]) == (23, 1, 23 + 25)
        assert _row(np.ones((9, 9), dtype=bool), hand["ring_diagonal_gap"], impl=impl, fill_conn=8)["filled_pred"] == 23
        row = _row(np.ones((8, 10), dtype=bool), hand["ring_on_border"], impl=impl)
        assert (row["n_pred"], row["filled_pred"]) == (22, 42)          # 6 x 7 ring on two borders: the hole is enclosed
        row = _row(np.ones((8, 10), dtype=bool), hand["c_open_to_border"], impl=impl)
        assert (row["n_pred"], row["filled_pred"]) == (15, 15)          # open towards the border: nothing to fill


def test_tie_goes_to_the_smallest_index_and_size_beats_order():
    hand = O.hand_masks()
    for impl in ("scipy", "numpy"):
        row = _row(hand["two_equal"], hand["two_equal"], impl=impl)
        assert (row["components_gt"], row["kept_gt"]) == (3, 6)
        assert [row[k] for k in ("gt_x", "gt_y", "gt_w", "gt_h")] == [5, 1, 3, 2]        # the block that starts first
        assert [row[k] for k in ("pred_x", "pred_y", "pred_w", "pred_h")] == [5, 1, 3, 2]
        assert [_row(hand["two_equal"], hand["two_equal"], impl=impl, tie="last")[k] for k in ("gt_x", "gt_y")] == [1, 4]
        row = _row(hand["larger_later"], hand["larger_later"], impl=impl)
        assert (row["components_pred"], row["kept_pred"], row["filled_pred"]) == (3, 14, 20)
        assert [row[k] for k in ("pred_x", "pred_y", "pred_w", "pred_h")] == [3, 4, 5, 4]


def test_widths_are_counts_inside_the_box_of_k():
    u = O.U_SHAPE
    for impl in ("scipy", "numpy"):
        row = _row(u, u, impl=impl)
        # box 7 x 5 at (0, 0); rows 1, 2, 3 hold the two arms: 2 pixels each, not 7
        assert [row[k] for k in ("gt_width_upper", "gt_width_middle", "gt_width_lower")] == [2, 2, 2]
        assert [row[k] for k in ("pred_width_upper", "pred_width_middle", "pred_width_lower")] == [2, 2, 2]
        assert _row(u, u, impl=impl, widths="extent")["gt_width_middle"] == 7
    # the ground-truth side counts G itself, speckle in the box's columns included, but takes the box from K(G)
    g = np.zeros((6, 8), dtype=bool)
    g[1:5, 1:4] = True
    g[3, 7] = True                                                      # outside the box's columns: not counted
    g[0, 2] = False
    row = _row(g, g)
    assert [row[k] for k in ("gt_x", "gt_y", "gt_w", "gt_h")] == [1, 1, 3, 4]
    assert [row[k] for k in ("gt_width_upper", "gt_width_middle", "gt_width_lower")] == [3, 3, 3]
    assert _row(g, g, box="all")["gt_w"] == 7


def test_empty_full_and_single_pixel():
    e, f = np.zeros((6, 5), dtype=bool), np.ones((6, 5), dtype=bool)
    assert O.table_masks(e, e) == [0] * 9 + [-1, -1, 0, 0, -1, -1, 0, 0] + [0] * 7
    assert O.table_masks(f, e) == [30, 0, 1, 0, 30, 0, 0, 0, 30, 0, 0, 5, 6, -1, -1, 0, 0, 5, 5, 5, 0, 0, 0, 0]
    assert O.table_masks(e, f) == [0, 30, 0, 1, 0, 30, 30, 0, 30, -1, -1, 0, 0, 0, 0, 5, 6, 0, 0, 0, 5, 5, 5, 0]
    one = np.ones((1, 1), dtype=bool)
    assert O.table_masks(one, one) == [1] * 9 + [0, 0, 1, 1, 0, 0, 1, 1] + [1] * 6 + [0]


def test_spiral_is_one_long_component_and_stays_open():
    s = O.spiral(31)
    lab4, n4 = O.label_numpy(s, conn=4)
    assert n4 == 1 and s[0].all() and not s[1, :-1].any()
    row = _row(s, s)
    assert row["components_pred"] == 1 and row["kept_pred"] == row["filled_pred"] == int(s.sum())


def test_values_at_the_threshold_are_background():
    t = np.float32(0.2)
    pred = np.array([[t, -t, np.nextafter(t, np.float32(1)), np.nextafter(-t, np.float32(-1)), 0.0]], dtype=np.float32)
    g, r = O.masks(np.zeros_like(pred), pred, t)
    assert r.tolist() == [[False, False, True, True, False]] and not g.any()
    gt, pred = O.images_from_masks(np.ones((9, 9), dtype=bool), np.zeros((9, 9), dtype=bool), seed=3)
    assert (pred == t).any() and (pred == -t).any() and not O.masks(gt, pred)[1].any()


# ---- golden file ------------------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_generator_writes(gold):
    cases = O.golden_cases()
    assert [c[0] for c in cases] == [c[0] for c in gold]
    for (name, g, r), (_, gg, gr, exp) in zip(cases, gold):
        assert np.array_equal(g, gg) and np.array_equal(r, gr), name
        assert O.table_masks(g, r) == exp, name
    assert os.path.getsize(GOLDEN) < 100 * 1024
    shapes = {c[1].shape for c in gold}
    assert {(1, 1), (1, 7), (7, 1), (5, 5), (31, 33), (64, 64), (67, 129), (256, 256), (1024, 3), (3, 1024)} <= shapes


def test_the_two_oracles_agree_on_every_golden_input(gold):
    for name, g, r, exp in gold:
        assert O.table_masks(g, r, impl="numpy") == exp, name
        assert O.table_masks(g, r, impl="scipy") == exp, name


@pytest.mark.parametrize("mutation", O.MUTATIONS, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
def test_golden_cases_tell_each_mistake_from_the_rule(gold, mutation):
    small = [c for c in gold if c[1].size <= 67 * 129]
    changed = [name for name, g, r, exp in small if O.table_masks(g, r, **mutation) != exp]
    assert changed, f"no golden case notices {mutation}"


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------
def _reference_metrics(gt, pred, p, g):
    """metrics.py:170-209, 345-398 restated on the oracle's regions (mask values 0 / 1, float32 flats as there)."""
    pp = np.where(p, pred, np.float32(0))
    mse = float(np.mean((gt.astype(np.float64) - pp.astype(np.float64)) ** 2))
    psnr = float("inf") if mse == 0 else 20 * np.log10(max(np.max(gt), np.max(pp)) / np.sqrt(mse))
    a, b = p.reshape(-1).astype(np.float32), g.reshape(-1).astype(np.float32)
    inter = float(np.sum(a * b))
    dice = (2.0 * inter + 1e-6) / (float(np.sum(a)) + float(np.sum(b)) + 1e-6)
    union = int(np.sum((a + b) > 0))
    return {"MSE": mse, "PSNR": float(psnr), "Dice Coefficient": dice, "Dice Loss": 1 - dice, "IoU": 1.0 if union == 0 else inter / union}


def test_pair_metrics_equal_the_reference_formulas(gold):
    from pti_ldm_vae_amd.utils import compare_metrics as M
    assert M.COLUMNS == O.COLUMNS
    for i, (name, g, r, exp) in enumerate(c for c in gold if c[1].size <= 64 * 64):
        gt, pred = O.images_from_masks(g, r, seed=i)
        counts, sums, ps = O.compare(gt[None], pred[None])
        assert counts[0].tolist() == exp
        (m,) = M.pair_metrics(counts, sums, *g.shape)
        row = dict(zip(O.COLUMNS, exp))
        if row["kept_gt"] == 0 or row["kept_pred"] == 0:
            assert m == (M.NO_GT if row["kept_gt"] == 0 else M.NO_PRED), name
            continue
        assert tuple(m) == M.METRIC_KEYS
        for key, want in _reference_metrics(gt, pred, ps[0], g).items():
            assert m[key] == pytest.approx(want, rel=1e-12, abs=1e-15), (name, key)
        dims = [(row["gt_h"], row["pred_h"]), (row["gt_width_upper"], row["pred_width_upper"]),
                (row["gt_width_middle"], row["pred_width_middle"]), (row["gt_width_lower"], row["pred_width_lower"])]
        ratio_keys = ("Height Metric", "Width Metric Upper", "Width Metric Middle", "Width Metric Lower")
        diff_keys = ("Absolute Height Difference", "Absolute Width Upper Difference", "Absolute Width Middle Difference",
                     "Absolute Width Lower Difference")
        for (a, b), rk, dk in zip(dims, ratio_keys, diff_keys):
            assert m[rk] == (None if max(a, b) == 0 else min(a, b) / max(a, b)) and m[dk] == abs(a - b), (name, rk)
        assert list(M.dimensions(exp).values()) == [row["gt_h"], row["gt_width_upper"], row["gt_width_middle"], row["gt_width_lower"],
                                                    row["pred_h"], row["pred_width_upper"], row["pred_width_middle"],
                                                    row["pred_width_lower"]]


def _counts_row(**kw):
    base = dict.fromkeys(O.COLUMNS, 0)
    base.update(n_gt=10, n_pred=10, components_gt=1, components_pred=1, kept_gt=10, kept_pred=10, filled_pred=10, intersection=5,
                union=15, gt_w=5, gt_h=4, pred_w=5, pred_h=2, gt_width_upper=3, gt_width_middle=3, gt_width_lower=3,
                pred_width_upper=3, pred_width_middle=2, pred_width_lower=3)
    base.update(kw)
    return [base[k] for k in O.COLUMNS]


def test_pair_metrics_none_inf_skip_and_status_rules():
    from pti_ldm_vae_amd.utils import compare_metrics as M
    rows = [_counts_row(), _counts_row(gt_width_upper=0, pred_width_upper=0), _counts_row(kept_gt=0), _counts_row(kept_pred=0),
            _counts_row()]
    sums = [[8.0, 1.0, 0.5], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, -1.0, 0.0]]
    m = M.pair_metrics(rows, sums, 2, 4)
    assert m[0]["MSE"] == 1.0 and m[0]["PSNR"] == 0.0 and m[0]["Height Metric"] == 0.5 and m[0]["Width Metric Middle"] == 2 / 3
    assert m[0]["Dice Coefficient"] == (10 + 1e-6) / (20 + 1e-6) and m[0]["IoU"] == 1 / 3 and m[0]["Absolute Height Difference"] == 2
    assert m[1]["PSNR"] == math.inf and m[1]["Width Metric Upper"] is None and m[1]["Absolute Width Upper Difference"] == 0
    assert m[2] == M.NO_GT and m[3] == M.NO_PRED
    assert m[4]["PSNR"] is None                                         # no positive pixel on either side: no peak
    with pytest.raises(RuntimeError, match="status"):
        M.pair_metrics([_counts_row(status=1)], [[0.0, 0.0, 0.0]], 2, 4)
    with pytest.raises(ValueError):
        M.pair_metrics(rows, sums[:2], 2, 4)


def _reference_aggregate(all_metrics, key):
    """metrics.py:484-541, 733-741 for one key without None entries."""
    data = [m[key] for m in all_metrics]
    n = len(data)
    mean, std = np.mean(data), np.std(data)
    lo, hi = mean - 1.96 * (std / np.sqrt(n)), mean + 1.96 * (std / np.sqrt(n))
    margin = (hi - lo) / 2
    q1, q3 = np.percentile(data, [25, 75])
    iqr = q3 - q1
    return {"mean": mean, "std": std, "ci95": [lo, hi],
            "outliers": {"outside_1_ci": sum(1 for x in data if x < lo or x > hi),
                         "outside_2_ci": sum(1 for x in data if x < mean - 2 * margin or x > mean + 2 * margin),
                         "outside_3_ci": sum(1 for x in data if x < mean - 3 * margin or x > mean + 3 * margin),
                         "outside_iqr": sum(1 for x in data if x < q1 - 1.5 * iqr or x > q3 + 1.5 * iqr),
                         "outside_z": sum(1 for x in data if abs((x - mean) / std) > 3) if std else 0}}


def test_aggregate_and_threshold_counts():
    from pti_ldm_vae_amd.utils import compare_metrics as M
    rs = np.random.RandomState(5)
    all_metrics = []
    for i in range(40):
        m = {k: float(rs.rand()) for k in M.METRIC_KEYS}
        m["Absolute Height Difference"] = int(rs.randint(0, 14))
        m["Absolute Width Middle Difference"] = int(rs.randint(0, 14))
        m["Absolute Width Lower Difference"] = int(rs.randint(0, 14))
        m["Height Metric"] = 0.85 + 0.15 * float(rs.rand())
        m["Width Metric Middle"] = 0.85 + 0.15 * float(rs.rand())
        m["IoU"] = 0.5                                                  # std 0: no z-outliers, no division
        all_metrics.append(m)
    all_metrics[3]["MSE"] = 50.0                                        # an outlier by every rule
    agg = M.aggregate(all_metrics)
    assert list(agg) == list(M.METRIC_KEYS)
    for key in M.METRIC_KEYS:
        want = _reference_aggregate(all_metrics, key)
        a = agg[key]
        assert a["n"] == 40 and a["none"] == 0
        assert a["mean"] == pytest.approx(want["mean"], rel=1e-14) and a["std"] == pytest.approx(want["std"], rel=1e-14, abs=0)
        assert a["ci95"] == pytest.approx(want["ci95"], rel=1e-14)
        assert a["outliers"] == want["outliers"], key
        data = [m[key] for m in all_metrics]
        assert a["worst"] == (min(data) if key in M.HIGHER_IS_BETTER else max(data))
    assert agg["MSE"]["outliers"]["outside_z"] == 1 and agg["MSE"]["worst"] == 50.0
    assert agg["IoU"]["std"] == 0.0 and agg["IoU"]["outliers"]["outside_z"] == 0
    assert M.HIGHER_IS_BETTER == {"PSNR", "Dice Coefficient", "Height Metric", "Width Metric Upper", "Width Metric Middle",
                                  "Width Metric Lower", "IoU"}
    # None entries: left out of the key's statistics and counted
    holes = [dict(m) for m in all_metrics]
    for i in (0, 7, 9):
        holes[i]["Width Metric Upper"] = None
    a = M.aggregate(holes)["Width Metric Upper"]
    want = _reference_aggregate([m for i, m in enumerate(all_metrics) if i not in (0, 7, 9)], "Width Metric Upper")
    assert (a["n"], a["none"]) == (37, 3) and a["mean"] == pytest.approx(want["mean"], rel=1e-14) and a["outliers"] == want["outliers"]
    gone = M.aggregate([dict(m, PSNR=None) for m in all_metrics])["PSNR"]
    assert gone["n"] == 0 and gone["none"] == 40 and gone["mean"] is None and set(gone["outliers"].values()) == {0}
    assert M.aggregate([]) == {}
    # the twelve threshold rows
    rows = M.threshold_counts(holes)
    assert [r[0] for r in rows] == [
        "Exams with Height Metric > 0.95", "Exams with Width Metric > 0.95", "Exams with Height Metric > 0.97",
        "Exams with Width Metric > 0.97", "Exams with Height Metric > 0.90", "Exams with Width Metric > 0.90",
        "Exams with Absolute Height Difference < 5", "Exams with Absolute Middle Width Difference < 5",
        "Exams with Absolute Lower Width Difference < 5", "Exams with Absolute Height Difference < 10",
        "Exams with Absolute Middle Width Difference < 10", "Exams with Absolute Lower Width Difference < 10"]
    want = [sum(m["Height Metric"] > 0.95 for m in holes), sum(m["Width Metric Middle"] > 0.95 for m in holes),
            sum(m["Height Metric"] > 0.97 for m in holes), sum(m["Width Metric Middle"] > 0.97 for m in holes),
            sum(m["Height Metric"] > 0.90 for m in holes), sum(m["Width Metric Middle"] > 0.90 for m in holes)]
    want += [sum(m[k] < lim for m in holes) for lim in (5, 10)
             for k in ("Absolute Height Difference", "Absolute Width Middle Difference", "Absolute Width Lower Difference")]
    assert [r[1] for r in rows] == want and [r[2] for r in rows] == [round(c / 40 * 100, 2) for c in want]
    none_rows = M.threshold_counts([dict(m, **{"Height Metric": None}) for m in holes])
    assert none_rows[0][1] == none_rows[2][1] == none_rows[4][1] == 0
    assert M.threshold_counts([])[0][1:] == (0, 0.0)


def test_csv_rows_have_the_reference_layout(tmp_path):
    from pti_ldm_vae_amd.utils import compare_metrics as M
    ms = M.pair_metrics([_counts_row(), _counts_row(pred_h=4)], [[8.0, 1.0, 0.5], [4.0, 1.0, 0.5]], 2, 4)
    agg, thr = M.aggregate(ms), M.threshold_counts(ms)
    rows = M.metrics_csv_rows(agg, thr, 2)
    assert len(rows) == len(M.METRIC_KEYS) + 12
    M.write_csv(tmp_path / "_metrics.csv", M.METRICS_CSV_COLUMNS, rows)
    lines = (tmp_path / "_metrics.csv").read_text().splitlines()
    assert lines[0] == ("Metric;Average;Worst Value;Confidence Interval Lower (95%);Confidence Interval Upper (95%);"
                        "Number of Images Processed;Outside 1 CI;Outside 2 CI;Outside 3 CI;IQR Outliers;Z-Score Outliers;Count;Percentage")
    assert lines[1] == f"MSE;{round(0.75, 3)};1.0;{round(0.75 - 1.96 * 0.25 / math.sqrt(2), 3)};{round(0.75 + 1.96 * 0.25 / math.sqrt(2), 3)};2;0;0;0;0;0;;"   # 0.5 and 1.0 lie inside 0.404 .. 1.096
    assert lines[len(M.METRIC_KEYS) + 1] == "Exams with Height Metric > 0.95;;;;;;;;;;;1;50.0"
    assert M.DIMENSION_COLUMNS == ("Image Path", "GT Height", "GT Width Upper", "GT Width Middle", "GT Width Lower", "Gen Height",
                                   "Gen Width Upper", "Gen Width Middle", "Gen Width Lower")


def test_distribution_plot_is_written_without_a_display(tmp_path):
    from pti_ldm_vae_amd.utils import compare_metrics as M
    ms = M.pair_metrics([_counts_row(), _counts_row(pred_h=4), _counts_row(pred_h=3)], [[8.0, 1.0, 0.5]] * 3, 2, 4)
    M.save_distributions(tmp_path / "d.png", ms, M.aggregate(ms))
    assert (tmp_path / "d.png").read_bytes()[:4] == b"\x89PNG"


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
def test_ops_mask_compare_refuses_before_a_launch():
    from pti_ldm_vae_amd import ops
    assert ops.MASK_COMPARE_MAX_EDGE == 1024 and ops.MASK_COMPARE_COLUMNS == O.COLUMNS and len(ops.MASK_COMPARE_COLUMNS) == 24
    a = torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="CUDA"):
        ops.mask_compare(a, a)                                          # right dtype, host tensors
    for gt, pred in ((a.double(), a), (a, a.half()), (a.numpy(), a), (a, None), (a.int(), a)):
        with pytest.raises(TypeError, match="float32"):
            ops.mask_compare(gt, pred)


def test_pti_mask_compare_validates_before_launch():
    from pti_ldm_vae_amd import _lib, ops
    h = _lib.lib()
    p = C.c_void_p(64)      # never dereferenced: every call below returns before a launch
    ws = h.pti_mask_compare_ws_bytes

    def call(gt=p, pred=p, n=2, hh=8, w=8, thr=0.2, counts=p, sums=p, wsp=p, ws_bytes=None):
        return h.pti_mask_compare(gt, pred, n, hh, w, thr, counts, sums, wsp, ws(n, hh, w) if ws_bytes is None else ws_bytes, None)

    for kw in ({"gt": None}, {"pred": None}, {"counts": None}, {"sums": None}, {"wsp": None}):
        assert call(**kw) == -1, kw
        assert b"null pointer" in h.pti_last_error_string()
    for kw in ({"n": 0}, {"hh": 0}, {"w": 0}, {"n": -1}):
        assert call(**dict(kw, ws_bytes=1 << 20)) == -1, kw
        assert b"bad shape" in h.pti_last_error_string()
    for kw in ({"hh": 1025}, {"w": 1025}):
        assert call(**dict(kw, ws_bytes=1 << 40)) == -2, kw
        assert b"unsupported shape" in h.pti_last_error_string()
    assert call(hh=1024, w=1024, ws_bytes=8) == -1 and b"workspace" in h.pti_last_error_string()   # the cap itself passes the shape test
    for thr in (-0.1, float("nan")):
        assert call(thr=thr) == -1 and b"threshold" in h.pti_last_error_string()
    for kw in ({"gt": C.c_void_p(66)}, {"pred": C.c_void_p(65)}, {"counts": C.c_void_p(66)}, {"sums": C.c_void_p(68)}):
        assert call(**kw) == -1 and b"misaligned" in h.pti_last_error_string(), kw
    assert call(wsp=C.c_void_p(66)) == -1 and b"4-byte aligned" in h.pti_last_error_string()
    assert call(ws_bytes=ws(2, 8, 8) - 1) == -1 and b"workspace of" in h.pti_last_error_string()
    # the size query: pure host arithmetic, three int32 planes and the fill's extra node per image
    assert ws(1, 1, 1) >= 4 * 4 and ws(2, 8, 8) == 2 * ws(1, 8, 8) and ws(1, 8, 8) >= 4 * (3 * 64 + 1)
    assert ws(64, 1024, 1024) >= 64 * 3 * 4 * 1024 * 1024              # beyond 2^31 bytes: 64-bit arithmetic
    assert ws(0, 8, 8) == ws(1, 0, 8) == ws(1, 8, 0) == ws(1, 1025, 8) == ws(1, 8, 1025) == 0
    with pytest.raises(_lib.PtiError, match="unsupported shape"):
        _lib.check(call(hh=ops.MASK_COMPARE_MAX_EDGE + 1, ws_bytes=1 << 40), "pti_mask_compare")
    text = open(os.path.join(ROOT, "include", "pti_vae.h")).read()
    assert f"#define PTI_MASK_COMPARE_MAX_EDGE {ops.MASK_COMPARE_MAX_EDGE}" in text
    assert f"#define PTI_MASK_COMPARE_COLUMNS {len(ops.MASK_COMPARE_COLUMNS)}" in text


def test_command_argument_refusals(tmp_path, capsys):
    from pti_ldm_vae_amd import compare_images as cli
    a = cli.parse_args(["--gt-dir", "a", "--pred-dir", "b"])
    assert (a.threshold, a.batch_size, a.num_samples, a.output_dir, a.no_plot, a.seed) == (0.2, 64, None, None, False, 0)
    assert cli.parse_args(["--results-dir", "r", "--no-plot", "--num-samples", "3"]).num_samples == 3
    for argv in ([], ["--gt-dir", "a"], ["--pred-dir", "b"], ["--gt-dir", "a", "--pred-dir", "b", "--results-dir", "r"],
                 ["--results-dir", "r", "--threshold", "-1"], ["--results-dir", "r", "--threshold", "nan"],
                 ["--results-dir", "r", "--batch-size", "0"], ["--results-dir", "r", "--num-samples", "0"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    with pytest.raises(FileNotFoundError, match="does not exist"):
        cli.list_pairs(cli.parse_args(["--results-dir", str(tmp_path / "nope")]))
    # pairing by file name, unpaired files reported, other files ignored
    gt_dir, pred_dir = tmp_path / "edente", tmp_path / "edente_synth"
    gt_dir.mkdir()
    pred_dir.mkdir()
    for d, names in ((gt_dir, ("a.tif", "b.TIF", "only_gt.tif", "notes.txt")), (pred_dir, ("a.tif", "b.TIF", "only_pred.tiff"))):
        for name in names:
            (d / name).write_bytes(b"")
    pairs, unpaired = cli.list_pairs(cli.parse_args(["--gt-dir", str(gt_dir), "--pred-dir", str(pred_dir)]))
    assert [p[0] for p in pairs] == ["a.tif", "b.TIF"] and unpaired == {"gt_only": ["only_gt.tif"], "pred_only": ["only_pred.tiff"]}
    # a side-by-side file of odd width is refused, not skipped
    from pti_ldm_vae_amd.data import write_tiff
    write_tiff(str(tmp_path / "odd.tif"), np.zeros((4, 7), dtype=np.float32))
    with pytest.raises(cli.OddWidth, match="odd"):
        cli.load_pair(tmp_path / "odd.tif", None)
    write_tiff(str(tmp_path / "even.tif"), np.arange(24, dtype=np.float32).reshape(4, 6))
    gt, pred = cli.load_pair(tmp_path / "even.tif", None)
    assert gt.shape == pred.shape == (4, 3) and gt[0].tolist() == [0, 1, 2] and pred[0].tolist() == [3, 4, 5]
    assert gt.flags.c_contiguous and pred.dtype == np.float32
    write_tiff(str(tmp_path / "other.tif"), np.zeros((4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="same dimensions"):
        cli.load_pair(tmp_path / "even.tif", tmp_path / "other.tif")

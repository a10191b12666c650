"""CPU tests of the surface-distance feature: the oracle of ``tests/surface_distance_oracle.py`` against scipy's erosion, brute
force and ``distance_transform_edt``; the per-mille rank rule against ``np.percentile``; ``compare_metrics.surface_metrics`` on
hand-made tables; the header's constants; the argument refusals of ``pti_surface_distance`` that return before any launch; the
new options of ``compare_images``; and the golden file against the oracle that wrote it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mask_compare_oracle as MC
import surface_distance_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_masks(count, seed):
    rs = np.random.RandomState(seed)
    for i in range(count):
        h, w = rs.randint(3, 60, size=2)
        kind = i % 4
        if kind == 0:
            yield rs.rand(h, w) < rs.uniform(0.05, 0.9)
        elif kind == 1:
            yield MC.blob_speckle(h, w, seed * 1000 + i, speckle=rs.uniform(0, 0.2), voids=rs.uniform(0, 0.2))
        elif kind == 2:
            yield (rs.rand(h, w) < 0.5) & MC.blob_speckle(h, w, seed * 1000 + i)
        else:
            m = np.zeros((h, w), dtype=bool)
            m[rs.randint(0, h), rs.randint(0, w)] = True
            yield m | (rs.rand(h, w) < 0.01)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_the_edge_rule_is_mask_xor_its_erosion():
    from scipy import ndimage
    for m in list(_random_masks(200, 1)) + list(MC.hand_masks().values()):
        assert np.array_equal(O.edges(m), m ^ ndimage.binary_erosion(m))
    assert O.edges(np.ones((4, 5), dtype=bool)).sum() == 14 and not O.edges(np.zeros((3, 3), dtype=bool)).any()
    assert O.edges(np.ones((1, 1), dtype=bool)).all()


def test_squared_distances_equal_brute_force_and_the_edt():
    from scipy import ndimage
    masks = list(_random_masks(200, 2))
    tested = 0
    for a, b in zip(masks[::2], masks[1::2]):
        h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
        a, b = a[:h, :w], b[:h, :w]
        ea, eb, da, db = O.distances(a, b)
        if da is None:
            continue
        tested += 1
        assert np.array_equal(da, O.brute(ea, eb)) and np.array_equal(db, O.brute(eb, ea))
        assert np.array_equal(da, O.d2_numpy(ea, eb)) and np.array_equal(db, O.d2_numpy(eb, ea))
        dist = ndimage.distance_transform_edt(~eb)                                       # the float map, squared and rounded
        assert np.array_equal(da, np.rint(dist[ea] ** 2).astype(np.int64))
        assert da.min() >= 0 and da.max() <= (h - 1) ** 2 + (w - 1) ** 2
    assert tested >= 90


def test_a_table_lists_what_the_header_says():
    a = np.zeros((9, 12), dtype=bool)
    a[2:7, 2:7] = True                                                                   # a 5 x 5 square: 16 edge pixels
    b = np.roll(a, 3, axis=1)
    rows, sums = O.table(a, b, 950, (0, 1, 3))
    assert rows[0][:3] == [25, 16, 9] and rows[1][:3] == [25, 16, 9]
    assert rows[0][3] == 15 * 950 // 1000 == 14 and rows[0][10] == 0
    d = np.sort(O.distances(a, b)[2])
    assert rows[0][4] == d[14] and rows[0][5] == d[15] and rows[0][6:10] == [int((d <= 0).sum()), int((d <= 1).sum()), int((d <= 9).sum()), 0]
    assert sums[0] == math.fsum(np.sqrt(d.astype(np.float64)))
    empty = np.zeros_like(a)
    for pair in ((a, empty), (empty, a), (empty, empty)):
        rows, sums = O.table(*pair)
        assert [r[2:] for r in rows] == [[-1, 0, -1, -1, 0, 0, 0, 0, 0]] * 2 and sums == [0.0, 0.0]
        assert [r[0] for r in rows] == [int(pair[0].sum()), int(pair[1].sum())]
    assert O.tol_d2((0, 1, 1.5, 2, 1500)) == [0, 1, 2, 4, 2250000]


def test_the_per_mille_rank_rule_reproduces_numpy_percentile():
    rs = np.random.RandomState(3)
    worst = 0.0
    for i in range(200):
        m = int(rs.randint(1, 400))
        d2 = np.sort(rs.randint(0, [4, 50, 3000, 2 * 1023 ** 2][i % 4] + 1, size=m)).astype(np.int64)
        for pm in (950, 0, 500, 999, 1000, 333):
            lo, rem = O.ranks(m, pm)
            d2_lo, d2_hi = int(d2[lo]), int(d2[lo + 1] if rem else d2[lo])
            got = O.percentile_of(d2_lo, d2_hi, m, pm)
            want = float(np.percentile(np.sqrt(d2.astype(np.float64)), pm / 10))
            # numpy's rank (m - 1) * (pm / 10) / 100 is rounded in floating point: m 2^-50 of a step; then the lerp and its operands
            gate = (m * 2.0 ** -50) * (math.sqrt(d2_hi) - math.sqrt(d2_lo)) + 8 * np.spacing(want)
            assert abs(got - want) <= gate, (m, pm, got, want)
            worst = max(worst, abs(got - want) / max(want, 1e-300))
    print(f"largest relative difference from np.percentile: {worst:.2e}")


def test_the_golden_file_holds_the_oracles_answers():
    path = os.path.join(ROOT, "tests", "golden", "surface_distance_golden.npz")
    assert os.path.getsize(path) < 100 * 1024
    with np.load(path) as z:
        cases, pm, tols = O.unpack_cases(z), int(z["pm"]), tuple(float(t) for t in z["tolerances"])
    fresh = O.golden_cases()
    assert [c[0] for c in cases] == [c[0] for c in fresh] and (pm, tols) == (O.GOLDEN_PM, O.GOLDEN_TOLERANCES)
    assert {c[1].shape for c in cases} >= set(O.SHAPES)
    for (name, a, b, counts, sums), (_, fa, fb) in zip(cases, fresh):
        assert np.array_equal(a, fa) and np.array_equal(b, fb), name
        if a.size <= 67 * 129:
            want = O.table(a, b, pm, tols, impl="numpy" if a.size > 2000 else "brute")
            assert counts.tolist() == want[0] and sums.tolist() == want[1], name


# ---- the host arithmetic of the report ---------------------------------------------------------------------------------------------
def _tables(pairs, pm, tols):
    return O.batch(pairs, pm, tols)


def test_surface_metrics_on_hand_made_tables():
    from pti_ldm_vae_amd.utils import compare_metrics as M
    sq = np.zeros((12, 16), dtype=bool)
    sq[3:9, 3:9] = True
    moved = np.roll(sq, 3, axis=1)
    empty = np.zeros_like(sq)
    tols, pm = (1.0, 2.0), 950
    counts, sums = _tables([(sq, sq), (sq, moved), (sq, empty), (empty, empty)], pm, tols)
    same, shifted, none_a, none_b = M.surface_metrics(counts, sums, tols, pm)
    keys = ("Hausdorff Distance", "Hausdorff Distance 95", "Average Surface Distance", "Surface Dice @ 1 px", "Surface Dice @ 2 px")
    assert tuple(same) == keys == M.surface_keys(tols, pm)
    assert list(same.values()) == [0.0, 0.0, 0.0, 1.0, 1.0]
    assert shifted["Hausdorff Distance"] == 3.0 and shifted["Hausdorff Distance 95"] == 3.0
    d = np.sqrt(np.concatenate(O.distances(sq, moved)[2:]).astype(np.float64))
    assert abs(shifted["Average Surface Distance"] - d.mean()) < 1e-12
    assert shifted["Surface Dice @ 1 px"] == float((d <= 1).mean()) and shifted["Surface Dice @ 2 px"] == float((d <= 2).mean())
    assert 0 < shifted["Surface Dice @ 1 px"] < shifted["Surface Dice @ 2 px"] < 1
    assert none_a == dict.fromkeys(keys) == none_b
    # the percentile is numpy's, per side, the larger side reported
    blob_a, blob_b = MC.blob_speckle(31, 33, 1, speckle=0.1), MC.blob_speckle(31, 33, 2, speckle=0.02)
    counts, sums = _tables([(blob_a, blob_b)], 900, ())
    got = M.surface_metrics(counts, sums, (), 900)[0]
    da, db = (np.sqrt(v.astype(np.float64)) for v in O.distances(blob_a, blob_b)[2:])
    assert tuple(got) == ("Hausdorff Distance", "Hausdorff Distance 90", "Average Surface Distance")
    assert abs(got["Hausdorff Distance 90"] - max(np.percentile(da, 90), np.percentile(db, 90))) < 1e-12
    assert got["Hausdorff Distance"] == max(da.max(), db.max())
    blk = M.surface_block(counts[0], sums[0], 900)
    assert blk["edge_pixels_gt"] == len(da) and blk["edge_pixels_pred"] == len(db) and blk["max_gt_to_pred"] == da.max()
    assert abs(blk["mean_pred_to_gt"] - db.mean()) < 1e-12 and abs(blk["percentile_gt_to_pred"] - np.percentile(da, 90)) < 1e-12
    bad = counts.copy()
    bad[0, 1, 10] = 1
    with pytest.raises(RuntimeError, match="status"):
        M.surface_metrics(bad, sums, (), 900)
    with pytest.raises(ValueError):
        M.surface_metrics(counts, sums, (1, 2, 3, 4, 5), 900)


def test_pair_metrics_appends_the_surface_keys_and_is_unchanged_without_them():
    from pti_ldm_vae_amd.utils import compare_metrics as M
    g, r = MC.blob_speckle(31, 33, 5), MC.blob_speckle(31, 33, 6, speckle=0.1)
    gt, pred = MC.images_from_masks(g, r, seed=1)
    counts, sums, ps = MC.compare(gt[None], pred[None])
    plain = M.pair_metrics(counts, sums, 31, 33)
    assert M.pair_metrics(counts, sums, 31, 33, surface=None) == plain and tuple(plain[0]) == M.METRIC_KEYS
    sc, ss = _tables([(g, ps[0])], 950, (1.0,))
    both = M.pair_metrics(counts, sums, 31, 33, surface=(sc, ss, (1.0,), 950))[0]
    extra = M.surface_metrics(sc, ss, (1.0,), 950)[0]
    assert tuple(both) == M.METRIC_KEYS + tuple(extra) and {k: both[k] for k in M.METRIC_KEYS} == plain[0]
    assert {k: both[k] for k in extra} == extra
    with pytest.raises(ValueError):
        M.pair_metrics(counts, sums, 31, 33, surface=(np.concatenate([sc, sc]), np.concatenate([ss, ss]), (1.0,), 950))
    # surface Dice is higher-is-better, the distances are not
    rows = [dict(plain[0], **{"Hausdorff Distance": v, "Surface Dice @ 1 px": 1 - v / 10}) for v in (1.0, 4.0, 2.0)]
    agg = M.aggregate(rows)
    assert agg["Hausdorff Distance"]["worst"] == 4.0 and agg["Surface Dice @ 1 px"]["worst"] == 0.6
    assert "Surface Dice @ 1 px" not in M.HIGHER_IS_BETTER and "Surface Dice @ 1 px" not in M.HIGHER_IS_BETTER_OPTIONAL


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def test_header_constants_equal_their_mirrors():
    from pti_ldm_vae_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "pti_vae.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define (PTI_[A-Z0-9_]+)[ \t]+(\d+)\b", text)}
    assert defines["PTI_SURFACE_COLUMNS"] == len(_lib.SURFACE_COLUMNS) == len(ops.SURFACE_COLUMNS) == len(O.COLUMNS) == 11
    assert defines["PTI_SURFACE_MAX_TOLERANCES"] == _lib.SURFACE_MAX_TOLERANCES == ops.SURFACE_MAX_TOLERANCES == O.MAX_TOLERANCES == 4
    assert ops.SURFACE_COLUMNS is _lib.SURFACE_COLUMNS and tuple(_lib.SURFACE_COLUMNS) == O.COLUMNS
    for name in ("pti_surface_distance", "pti_surface_distance_ws_bytes", "pti_mask_compare_outputs"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)


def test_refusals_that_return_before_any_launch():
    from pti_ldm_vae_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)
    tol = (C.c_int32 * 5)(0, 1, 2, 3, 4)

    def call(a=p, b=p, n=1, h=8, w=8, pm=950, n_tol=2, counts=p, sums=p, ws=p, ws_bytes=1 << 30, a_bits=1, b_bits=2, tols=tol):
        return lib.pti_surface_distance(a, a_bits, b, b_bits, n, h, w, pm, tols, n_tol, counts, sums, ws, ws_bytes, None)

    for kw in (dict(a=None), dict(b=None), dict(counts=None), dict(sums=None), dict(ws=None), dict(tols=None)):
        assert call(**kw) == -1 and b"null pointer" in lib.pti_last_error_string(), kw
    assert call(h=0) == -1 and b"bad shape" in lib.pti_last_error_string()
    assert call(n=0) == -1 and call(w=0) == -1
    assert call(w=1025) == -2 and b"unsupported shape" in lib.pti_last_error_string()
    assert call(h=1025) == -2 and call(n=32768) == -2
    assert call(pm=1001) == -1 and b"per mille" in lib.pti_last_error_string()
    assert call(pm=-1) == -1
    assert call(n_tol=5) == -1 and b"tolerances" in lib.pti_last_error_string()
    assert call(n_tol=-1) == -1
    assert call(tols=(C.c_int32 * 2)(1, -3)) == -1 and b"negative" in lib.pti_last_error_string()
    assert call(a_bits=0) == -1 and call(b_bits=256) == -1
    assert call(ws_bytes=16) == -1 and b"workspace" in lib.pti_last_error_string()
    assert call(ws=C.c_void_p(4100)) == -1 and call(sums=C.c_void_p(4100)) == -1 and call(counts=C.c_void_p(4098)) == -1
    size = lib.pti_surface_distance_ws_bytes
    assert size(1, 1025, 8) == 0 and size(0, 8, 8) == 0 and size(1, 8, 0) == 0 and size(32768, 8, 8) == 0
    assert size(1, 1, 1) > 0 and size(1, 8, 8) % 8 == 0 and size(2, 64, 64) - size(1, 64, 64) == size(1, 64, 64)
    assert 12 * 1024 * 1024 <= size(1, 1024, 1024) <= 12 * 1024 * 1024 + (1 << 16)       # 12 bytes per pixel and a few KB
    # the new entry of the comparison launch refuses aliased outputs before a launch, too
    f = lib.pti_mask_compare_outputs
    assert f(p, C.c_void_p(8192), 1, 8, 8, 0.2, p, p, None, p, p, 1 << 20, None) == -1 and b"alias" in lib.pti_last_error_string()
    assert f(p, C.c_void_p(8192), 1, 8, 8, 0.2, p, p, C.c_void_p(8192), None, p, 1 << 20, None) == -1
    assert f(p, C.c_void_p(8192), 1, 8, 8, 0.2, p, p, C.c_void_p(12288), C.c_void_p(12288), p, 1 << 20, None) == -1
    assert f(None, p, 1, 8, 8, 0.2, p, p, None, None, p, 1 << 20, None) == -1 and b"null pointer" in lib.pti_last_error_string()


def test_ops_argument_conversions_need_no_gpu():
    from pti_ldm_vae_amd import ops
    assert [ops.surface_percentile_pm("t", v) for v in (0, 50, 95.0, 99.9, 100, 12.3)] == [0, 500, 950, 999, 1000, 123]
    for bad in (95.05, -0.1, 100.1, float("nan")):
        with pytest.raises(ValueError):
            ops.surface_percentile_pm("t", bad)
    assert ops.surface_tolerances_d2("t", (0, 1, 1.5, 2)) == [0, 1, 2, 4] == O.tol_d2((0, 1, 1.5, 2))
    assert ops.surface_tolerances_d2("t", (1500, 1e9)) == [2250000, 2 ** 31 - 1] and ops.surface_tolerances_d2("t", ()) == []
    for bad in ((1, 2, 3, 4, 5), (-1,), (float("nan"),)):
        with pytest.raises(ValueError):
            ops.surface_tolerances_d2("t", bad)


def test_the_three_new_options_of_the_command():
    from pti_ldm_vae_amd import compare_images as cli
    base = ["--results-dir", "x"]
    a = cli.parse_args(base)
    assert a.surface is False and a.surface_tolerances is None and a.surface_percentile is None
    a = cli.parse_args(base + ["--surface"])
    assert a.surface is True and a.surface_tolerances == [1.0, 2.0] and a.surface_percentile == 95.0
    a = cli.parse_args(base + ["--surface", "--surface-tolerances", "0", "1.5", "3", "10", "--surface-percentile", "99.9", "--ssim", "--straighten"])
    assert a.surface_tolerances == [0.0, 1.5, 3.0, 10.0] and a.surface_percentile == 99.9 and a.ssim and a.straighten
    for bad in (["--surface-tolerances", "1"], ["--surface-percentile", "90"], ["--surface", "--surface-tolerances", "1", "2", "3", "4", "5"],
                ["--surface", "--surface-tolerances", "-1"], ["--surface", "--surface-percentile", "95.05"],
                ["--surface", "--surface-percentile", "101"], ["--surface", "--surface-tolerances"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert cli.SURFACE_SCRATCH_CAP == 1 << 30

"""CPU tests of the two-sample permutation tests: the oracle's algebra, the labellings, the oracle end to end on fixed seeds,
and the argument checks of the launchers and entry points (no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import two_sample_oracle as O
from pti_ldm_vae_amd.analysis import two_sample as TS


# ---- oracle algebra ---------------------------------------------------------------------------------------------------------
def test_forms_from_the_definition():
    rng = np.random.default_rng(3)
    n = 7
    w = rng.integers(0, 65536, size=(n, n))                 # asymmetric, non-zero diagonal
    w[0, 1], w[5, 2] = 0, 65535
    masks = np.concatenate([rng.integers(0, 2, size=(6, n)), np.zeros((1, n), int), np.ones((1, n), int)]).astype(np.uint8)
    got = O.forms(w, masks)
    assert got.dtype == np.int64 and np.array_equal(got, O.forms_loops(w, masks))
    assert got[-1, 0] == w.sum() and got[-1, 1] == got[-1, 2] == w.sum() and not got[-2].any()


def test_statistics_against_the_unquantised_kernel():
    """The three statistics from the quantised integers against a direct fp64 evaluation from the float kernel.

    Bound.  An entry of the quantised matrix is rint(65535 v) with v in [0, 1], so w / 65535 differs from v by at most
    q = 0.5 / 65535 (the rounding) plus the fp64 error of forming v, below 1e-15 and taken as 1e-12 here.  Each statistic is
    a signed combination of MEANS of entries: MMD^2 = mean_AA + mean_BB - 2 mean_AB, energy = 2 mean_AB - mean_AA' - mean_BB'
    (the primes: means over n^2 entries with a zero diagonal, which is exact in both), so the absolute coefficients sum to 4
    and |quantised - direct| <= 4 (q + 1e-12) in kernel units; the energy statistic is reported in distance units, which
    multiplies the bound by the scale (the matrix maximum).  The neighbour share has no quantisation: its bound is the fp64
    rounding of one division, 2^-52 relative."""
    rng = np.random.default_rng(11)
    n_a, n_b, dim = 5, 6, 3
    z = rng.standard_normal((n_a + n_b, dim)).astype(np.float32)
    z[n_a:] += 0.7
    dist = O.pairwise(z)
    d = dist.astype(np.float64)
    n = n_a + n_b
    ia, ib = np.arange(n_a), np.arange(n_a, n)
    off = ~np.eye(n, dtype=bool)
    ones = np.ones((1, n), dtype=np.uint8)
    masks = np.concatenate([TS.permutation_masks(n_a, n_b, 4, 0), ones])
    q = 0.5 / 65535 + 1e-12

    med = float(O.lower_median(dist))
    k = np.mean([np.exp(-(d * d) / (2.0 * (b * med) ** 2)) for b in (0.5, 1.0, 2.0)], axis=0)
    w, _ = O.kernel_matrix(dist, "gaussian", med)
    for row in range(masks.shape[0] - 1):
        a, b = np.flatnonzero(masks[row]), np.flatnonzero(masks[row] == 0)
        sub = lambda r, c: (k * off)[np.ix_(r, c)].sum()
        direct = sub(a, a) / (n_a * (n_a - 1)) + sub(b, b) / (n_b * (n_b - 1)) - 2 * sub(a, b) / (n_a * n_b)
        got = O.statistics(O.forms(w, masks), n_a, n_b, "mmd")[row] / 65535.0
        assert abs(got - direct) <= 4 * q, (row, got, direct)

    dmax = float(dist.max())
    w, _ = O.kernel_matrix(dist, "energy", dmax)
    for row in range(masks.shape[0] - 1):
        a, b = np.flatnonzero(masks[row]), np.flatnonzero(masks[row] == 0)
        sub = lambda r, c: d[np.ix_(r, c)].sum()
        direct = 2 * sub(a, b) / (n_a * n_b) - sub(a, a) / n_a ** 2 - sub(b, b) / n_b ** 2
        got = O.statistics(O.forms(w, masks), n_a, n_b, "energy")[row] * dmax / 65535.0
        assert abs(got - direct) <= 4 * q * dmax, (row, got, direct)

    kk = 3
    w = O.knn_indicator(O.knn_table(dist, kk + 1), n)
    assert (w.sum(1) == kk).all()
    same = sum(int(w[i, j]) for i in range(n) for j in range(n) if (i < n_a) == (j < n_a))
    got = O.statistics(O.forms(w, masks), n_a, n_b, "knn", kk)[0]
    assert abs(got - same / (n * kk)) <= 2.0 ** -52
    # the module's own evaluation agrees with the oracle's on equal integers, bit for bit
    entry, null = TS.evaluate_forms(O.forms(w, masks), n_a, n_b, "knn", neighbors=kk)
    raw = O.statistics(O.forms(w, masks), n_a, n_b, "knn", kk)
    assert entry["statistic"] == raw[0] and np.array_equal(null, raw[1:]) and entry["levels"] == 2


def test_half_zone_of_the_test_inputs_is_nearly_empty():
    """The inputs the GPU kernel test uses: the entries within 1e-9 of a half-integer are under 0.1 % (here: none or few)."""
    for n, seed in ((4, 0), (5, 1), (64, 2), (301, 3)):
        dist = O.pairwise(np.random.default_rng(seed).standard_normal((n, 6)))
        for kind, scale in (("gaussian", O.lower_median(dist)), ("energy", dist.max())):
            near = O.kernel_matrix(dist, kind, scale)[1]
            assert near.sum() < 0.001 * n * n, (n, kind, int(near.sum()))


# ---- labellings -------------------------------------------------------------------------------------------------------------
def test_permutation_masks_plain():
    m = TS.permutation_masks(7, 5, 300, 4)
    assert m.dtype == np.uint8 and m.shape == (301, 12) and set(np.unique(m)) == {0, 1}
    assert m[0].tolist() == [1] * 7 + [0] * 5
    assert (m.sum(1) == 7).all()
    assert np.array_equal(m, TS.permutation_masks(7, 5, 300, 4))
    assert not np.array_equal(m, TS.permutation_masks(7, 5, 300, 5))
    assert len({row.tobytes() for row in m}) > 100
    # the documented draw: one rng.random(n) per further row, label A to the n_a smallest keys
    rng = np.random.Generator(np.random.PCG64(4))
    for row in range(1, 301):
        keys = rng.random(12)
        want = np.zeros(12, np.uint8)
        want[np.argsort(keys, kind="stable")[:7]] = 1
        assert np.array_equal(m[row], want), row


def test_permutation_masks_stratified():
    strata_a = ["p1", "p1", "p2", "p3", "p3", "p3"]
    strata_b = ["p2", "p2", "p1", "p4", "p4", "p3"]           # p4: rows of B only
    strata = strata_a + strata_b
    m = TS.permutation_masks(6, 6, 200, 9, strata)
    assert m[0].tolist() == [1] * 6 + [0] * 6 and (m.sum(1) == 6).all()
    for key in set(strata):
        idx = [i for i, s in enumerate(strata) if s == key]
        assert (m[:, idx].sum(1) == m[0, idx].sum()).all(), key
    p4 = [i for i, s in enumerate(strata) if s == "p4"]
    assert not m[:, p4].any()
    assert TS.fixed_strata(6, 6, strata) == (1, 2) and TS.fixed_strata(6, 6) == (0, 0)
    assert len({row.tobytes() for row in m}) > 20
    assert np.array_equal(m, TS.permutation_masks(6, 6, 200, 9, strata))
    assert not np.array_equal(m, TS.permutation_masks(6, 6, 200, 10, strata))
    with pytest.raises(ValueError, match="strata"):
        TS.permutation_masks(6, 6, 10, 0, strata[:-1])
    with pytest.raises(ValueError, match="permutations"):
        TS.permutation_masks(6, 6, 0, 0)


# ---- end to end on the oracle -----------------------------------------------------------------------------------------------
# Seeds chosen on the CPU: with DATA_SEED = 5 and PERM_SEED = 0 the same-distribution case gives p > 0.05 in all three tests.
DATA_SEED, PERM_SEED, ROWS, COLS, PERMS = 5, 0, 40, 16, 199


def groups(shift):
    rng = np.random.default_rng(DATA_SEED)
    a = rng.standard_normal((ROWS, COLS)).astype(np.float32)
    b = rng.standard_normal((ROWS, COLS)).astype(np.float32) + np.float32(shift)
    return a, b


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, shift in (("same", 0.0), ("shifted", 2.0)):
        a, b = groups(shift)
        out[name] = O.two_sample(O.pairwise(np.concatenate([a, b])), ROWS, ROWS, permutations=PERMS, seed=PERM_SEED)
    return out


def test_same_distribution_is_not_rejected(cases):
    for kind in TS.TESTS:
        assert cases["same"][kind]["p_value"] > 0.05, (kind, cases["same"][kind]["p_value"])


def test_shifted_group_is_rejected_at_the_floor(cases):
    for kind in TS.TESTS:
        assert cases["shifted"][kind]["exceed"] == 0 and cases["shifted"][kind]["p_value"] == 1 / (PERMS + 1), kind


def test_report_from_oracle_integers_is_json_without_nan(cases):
    import json
    entries = {}
    for kind in TS.TESTS:
        entries[kind], null = TS.evaluate_forms(cases["same"][kind]["forms"], ROWS, ROWS, kind, neighbors=5,
                                                unit={"mmd": 1 / 65535.0, "energy": cases["same"]["max"] / 65535.0, "knn": 1.0}[kind])
        assert entries[kind]["exceed"] == cases["same"][kind]["exceed"] and entries[kind]["p_value"] == cases["same"][kind]["p_value"]
        assert np.array_equal(null, cases["same"][kind]["null"])
    undefined, null = TS.evaluate_forms(np.zeros((PERMS + 2, 3), np.int64), ROWS, ROWS, "mmd", unit=None, scale=0.0)
    assert undefined["statistic"] is None and undefined["p_value"] is None and undefined["scale"] == 0.0 and np.isnan(null).all()
    flat, _ = TS.evaluate_forms(np.zeros((PERMS + 2, 3), np.int64), ROWS, ROWS, "mmd")
    assert flat["z"] is None and flat["p_value"] == 1.0
    doc = TS.build_report(dict(entries, flat=flat, undefined=undefined), ROWS, ROWS, 0, 5, None)
    text = json.dumps(doc, indent=2, allow_nan=False)
    assert "NaN" not in text and list(doc)[:6] == ["n_a", "n_b", "stratified", "fixed_strata", "fixed_rows", "seed"]


# ---- launchers and entry points -----------------------------------------------------------------------------------------------
def test_launchers_refuse_before_touching_the_library(monkeypatch):
    from pti_ldm_vae_amd import ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(ops.L, "lib", no_library)
    w = torch.zeros(8, 8, dtype=torch.int32)
    d = torch.zeros(8, 8)
    masks = torch.zeros(3, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="w: expected torch.int32"):
        ops.permutation_forms(w.long(), masks)
    with pytest.raises(ValueError, match="w: expected a square"):
        ops.permutation_forms(w[:, :7], masks)
    with pytest.raises(ValueError, match="w: unsupported shape"):
        ops.permutation_forms(torch.zeros(3, 3, dtype=torch.int32), masks[:, :3])
    with pytest.raises(ValueError, match="w: unsupported shape"):
        ops.permutation_forms(torch.empty((8193, 8193), dtype=torch.int32), masks)
    with pytest.raises(ValueError):                          # host tensors: no CPU path
        ops.permutation_forms(w, masks)
    for fn in (ops.distance_median, lambda t: ops.two_sample_kernel(t, "energy")):
        with pytest.raises(TypeError, match="dist: expected torch.float32"):
            fn(d.double())
        with pytest.raises(ValueError, match="dist: expected a square"):
            fn(d[:5])
        with pytest.raises(ValueError, match="dist: unsupported shape"):
            fn(d[:3, :3])
        with pytest.raises(ValueError):
            fn(d)
    with pytest.raises(ValueError, match="kind"):
        ops.two_sample_kernel(d, "laplace")
    with pytest.raises(ValueError, match="bandwidths"):
        ops.two_sample_kernel(d, "gaussian", scale=torch.ones(()), bandwidths=())
    with pytest.raises(ValueError, match="bandwidths"):
        ops.two_sample_kernel(d, "gaussian", scale=torch.ones(()), bandwidths=(1.0, -1.0))
    with pytest.raises(ValueError, match="scale"):
        ops.two_sample_kernel(d, "gaussian")
    idx = torch.zeros(8, 3, dtype=torch.int32)
    with pytest.raises(TypeError, match="knn_idx"):
        ops.knn_indicator(idx.long(), 8)
    with pytest.raises(ValueError, match="n: unsupported"):
        ops.knn_indicator(idx, 3)
    with pytest.raises(ValueError, match="knn_idx must be"):
        ops.knn_indicator(idx, 9)
    with pytest.raises(ValueError):
        ops.knn_indicator(idx, 8)


def test_mask_table_checks(monkeypatch):
    from pti_ldm_vae_amd import ops
    monkeypatch.setattr(ops, "_dense_rows", lambda t, name, dtype=None, **k: t)      # let a host matrix pass as w
    monkeypatch.setattr(ops.L, "lib", lambda: pytest.fail("the library was touched"))
    w = torch.zeros(8, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"masks must be \[P, 8\]"):
        ops.permutation_forms(w, torch.zeros(3, 7, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"masks must be \[P, 8\]"):
        ops.permutation_forms(w, torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(TypeError, match="masks: expected torch.uint8"):
        ops.permutation_forms(w, torch.zeros(3, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="masks: unsupported number of labellings 0"):
        ops.permutation_forms(w, torch.zeros(0, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="masks: unsupported number of labellings 65537"):
        ops.permutation_forms(w, torch.zeros(65537, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="masks: expected a CUDA"):
        ops.permutation_forms(w, torch.zeros(3, 8, dtype=torch.uint8))


def test_entry_points_refuse_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(4096)                                     # never dereferenced on these paths
    assert h.pti_distance_median_ws_bytes(3) == 0 and h.pti_distance_median_ws_bytes(8193) == 0
    assert h.pti_distance_median_ws_bytes(4) == 258 * 4
    assert h.pti_permutation_forms_ws_bytes(3, 1) == 0 and h.pti_permutation_forms_ws_bytes(8193, 1) == 0
    assert h.pti_permutation_forms_ws_bytes(8, 0) == 0 and h.pti_permutation_forms_ws_bytes(8, 65537) == 0
    # tight: two planes of n_pad^2 bytes, P n_pad bytes, 8 n bytes, each part rounded up to 256
    assert h.pti_permutation_forms_ws_bytes(65, 3) == 2 * 128 * 128 + 512 + 768
    assert h.pti_permutation_forms_ws_bytes(8192, 65536) == 2 * 8192 * 8192 + 65536 * 8192 + 65536
    assert h.pti_distance_median(None, 8, 8, p, p, 2048, None) == -1 and b"null" in h.pti_last_error_string()
    assert h.pti_distance_median(p, 8, 3, p, p, 2048, None) == -1
    assert h.pti_distance_median(p, 8, 8193, p, p, 2048, None) == -2
    assert h.pti_distance_median(p, 7, 8, p, p, 2048, None) == -1 and b"stride" in h.pti_last_error_string()
    assert h.pti_distance_median(p, 8, 8, p, p, 1028, None) == -1 and b"workspace" in h.pti_last_error_string()
    bw = (C.c_double * 3)(0.5, 1.0, 2.0)
    assert h.pti_two_sample_kernel(p, 8, 8, 2, p, bw, 3, p, p, None) == -1 and b"kind" in h.pti_last_error_string()
    assert h.pti_two_sample_kernel(p, 8, 8, 0, None, bw, 3, p, p, None) == -1 and b"scale" in h.pti_last_error_string()
    assert h.pti_two_sample_kernel(p, 8, 8, 0, p, bw, 9, p, p, None) == -1 and b"bandwidths" in h.pti_last_error_string()
    bad = (C.c_double * 1)(0.0)
    assert h.pti_two_sample_kernel(p, 8, 8, 0, p, bad, 1, p, p, None) == -1 and b"positive" in h.pti_last_error_string()
    assert h.pti_two_sample_kernel(p, 8, 8193, 1, None, None, 0, p, p, None) == -2
    assert h.pti_knn_indicator(p, 8, 0, p, None) == -1 and h.pti_knn_indicator(p, 8, 9, p, None) == -1
    assert h.pti_knn_indicator(p, 3, 2, p, None) == -1 and h.pti_knn_indicator(p, 8193, 2, p, None) == -2
    assert h.pti_permutation_forms(p, 8, 8, None, 1, p, p, 1 << 20, None) == -1
    assert h.pti_permutation_forms(p, 8, 3, p, 1, p, p, 1 << 20, None) == -1
    assert h.pti_permutation_forms(p, 8, 8, p, 65537, p, p, 1 << 40, None) == -2
    assert h.pti_permutation_forms(p, 7, 8, p, 1, p, p, 1 << 20, None) == -1 and b"stride" in h.pti_last_error_string()
    assert h.pti_permutation_forms(p, 8, 8, p, 1, p, p, 100, None) == -1 and b"workspace" in h.pti_last_error_string()
    assert h.pti_permutation_forms(p, 8, 8, p, 1, C.c_void_p(4100), p, 1 << 20, None) == -1 and b"misaligned" in h.pti_last_error_string()


def test_two_sample_tests_argument_checks():
    a = np.zeros((5, 3), np.float32)
    for kwargs, match in ((dict(permutations=0), "permutations"), (dict(permutations=65535), "permutations"),
                          (dict(neighbors=0), "neighbors"), (dict(neighbors=9), "neighbors"), (dict(bandwidths=()), "bandwidths")):
        opts = dict(permutations=10, neighbors=2, bandwidths=(1.0,))
        opts.update(kwargs)
        with pytest.raises(ValueError, match=match):
            TS.check_arguments(5, 5, opts["permutations"], opts["neighbors"], opts["bandwidths"])
    with pytest.raises(ValueError, match="at least 2 rows"):
        TS.check_arguments(1, 5, 10, 2, (1.0,))
    with pytest.raises(ValueError, match="8192"):
        TS.check_arguments(5000, 5000, 10, 2, (1.0,))
    with pytest.raises(ValueError, match="strata"):
        TS.two_sample_tests(a, a, strata_a=["x"] * 5, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="columns"):
        TS.two_sample_tests(a, a[:, :2], device=torch.device("cpu"))


def test_cli_flags_parse_and_need_two_groups():
    from pti_ldm_vae_amd import analyze_static
    base = ["--vae-weights", "w", "--config-file", "c", "--folder-edente", "e"]
    plain = analyze_static.parse_args(base)
    assert "group_test" not in vars(plain) and plain.group_test is False and plain.group_test_permutations == 9999
    args = analyze_static.parse_args(base + ["--group-test", "--group-test-permutations", "99", "--group-test-stratify", "patient",
                                             "--group-test-neighbors", "3", "--group-test-seed", "7"])
    assert (args.group_test, args.group_test_permutations, args.group_test_stratify, args.group_test_neighbors,
            args.group_test_seed) == (True, 99, "patient", 3, 7)
    with pytest.raises(SystemExit, match="--folder-dente"):
        analyze_static.main(base + ["--group-test"])

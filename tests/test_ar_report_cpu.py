"""CPU tests of the attribute-ordering report: the numpy oracle against scipy and against its committed golden file, the
mutations of the oracle that the checks must catch, ``utils.ar_metrics.order_statistics`` on the oracle's counts, the
pieces of both commands that need no GPU, and the refusals of ``pti_rank_agreement`` (they return before any launch)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import ar_report_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports():
    """{case name: (case, oracle report)}: computed once and shared, never modified."""
    return {case.name: (case, O.report(case.z, case.attrs, case.channels, case.deltas)) for case in O.all_cases()}


def test_case_list_is_the_specified_one():
    assert [(n, l, na) for _, n, l, na, *_ in O.CASES[:6]] == [(2, 1, 1), (3, 2, 1), (65, 3, 2), (257, 10, 6), (1030, 16, 16),
                                                                  (2500, 10, 6)]
    assert [n for _, n, *_ in O.CASES[6:]] == [97, 97] and O.CASES[5][6][0] > 0 and O.CASES[5][6][1] > 0


def test_oracle_reproduces_the_golden_file(reports):
    gold = O.load_golden()
    assert sorted(gold) == sorted(f"{name}/{k}" for name in reports for k in ("counts", "ar_loss", "gate"))
    for name, (case, r) in reports.items():
        assert np.array_equal(gold[f"{name}/counts"], r["counts"]) and gold[f"{name}/counts"].dtype == np.int64
        assert np.array_equal(gold[f"{name}/ar_loss"], r["ar_loss"])
        gate = O.gate_of(r["ar_loss"], O.ar_loss_fp32(case.z, case.attrs, case.channels, case.deltas))
        assert gate == float(gold[f"{name}/gate"])          # measured on the CPU, recorded, reproducible
        assert gate < 1e-5


def test_five_classes_partition_the_pairs_and_every_class_is_populated(reports):
    for name, (case, r) in reports.items():
        assert np.all(r["counts"].sum(-1) == case.n * (case.n - 1) // 2), name
        assert np.all(r["counts"] >= 0)
    for name in ("n257", "n1030", "n2500"):
        assert np.all(reports[name][1]["counts"].reshape(-1, 5).min(0) > 0), name   # every tie class occurs


def test_tau_b_equals_scipy(reports):
    from scipy.stats import kendalltau
    for name in ("n65", "n257"):
        case, r = reports[name]
        for q in range(case.na):
            for c in range(case.l):
                want = kendalltau(case.attrs[q], case.z[:, c], variant="b").statistic
                assert abs(r["kendall_tau_b"][q, c] - want) <= 1e-12, (name, q, c)


def test_degenerate_cases(reports):
    case, r = reports["n97_equal_attrs"]
    assert np.all(r["pairs"] == 0) and np.all(r["ar_loss"] == 0.0) and np.all(np.isnan(r["kendall_tau_b"]))
    assert np.all(r["counts"][..., :3] == 0)
    case, r = reports["n97_const_channel"]
    assert np.all(np.isnan(r["kendall_tau_b"][:, 2])) and np.all(r["counts"][:, 2, 0] == 0)   # the constant channel
    assert case.channels[1] == -1 and r["ar_loss"][1] == 0.0 and r["loss_sum"][1] == 0.0 and r["ar_loss"][2] > 0.0
    assert r["ar_loss"][0] == 1.0                                                                # tanh(0) - (+-1), squared


def test_order_statistics_reproduces_the_oracle(reports):
    from pti_ldm_vae_amd.utils.ar_metrics import order_statistics
    for name, (case, r) in reports.items():
        s = order_statistics(r["counts"], r["loss_sum"])
        assert np.array_equal(np.array(s["pairs"]), r["pairs"]), name
        for key in ("concordance", "kendall_tau_b"):
            got = np.array([[np.nan if v is None else v for v in row] for row in s[key]], dtype=np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(r[key])), (name, key)
            np.testing.assert_allclose(got[~np.isnan(got)], r[key][~np.isnan(got)], rtol=1e-14, atol=0)
        np.testing.assert_allclose(np.array(s["ar_loss"]), r["ar_loss"], rtol=1e-15, atol=0)
        json.dumps(s, allow_nan=False)                                                            # null, never NaN
    with pytest.raises(ValueError):
        order_statistics(np.zeros((2, 3, 4)), np.zeros(2))


MUTATIONS = ["ordered", "z_ties_concordant", "tau_a", "mean_over_all", "flip_sign"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_mutated_oracle_is_caught(reports, mutation):
    """Each wrong definition changes a count or moves ar_loss past the gate on at least one case.  tau-a is the exception:
    it changes only the denominator of tau, so it can do neither, and is caught by a third criterion instead -- tau itself
    moves by more than 1e-9 (the oracle agrees with scipy's tau-b to 1e-12, test_tau_b_equals_scipy)."""
    gold = O.load_golden()
    caught = []
    for name in ("n3", "n65", "n257"):
        case, r = reports[name]
        m = O.report(case.z, case.attrs, case.channels, case.deltas, **{mutation: True})
        if not np.array_equal(m["counts"], r["counts"]):
            caught.append((name, "counts"))
        if O.loss_deviation(m["ar_loss"], gold[f"{name}/ar_loss"]) > float(gold[f"{name}/gate"]):
            caught.append((name, "ar_loss"))
        ok = ~np.isnan(r["kendall_tau_b"])
        if np.max(np.abs(m["kendall_tau_b"][ok] - r["kendall_tau_b"][ok])) > 1e-9:
            caught.append((name, "tau"))
    assert caught, mutation
    kinds = {k for _, k in caught}
    assert kinds & ({"tau"} if mutation == "tau_a" else {"counts", "ar_loss"}), (mutation, caught)


def test_pearson_and_best_channel():
    from pti_ldm_vae_amd.utils import ar_metrics as M
    rng = np.random.default_rng(3)
    z = rng.normal(size=(50, 4)).astype(np.float32)
    z[:, 3] = 1.5
    attrs = np.stack([2.0 * z[:, 1] + 0.01 * rng.normal(size=50), rng.normal(size=50), np.full(50, 4.0)]).astype(np.float32)
    r = M.pearson_matrix(z, attrs)
    want = np.corrcoef(np.concatenate([attrs[:2].astype(np.float64), z[:, :3].T.astype(np.float64)]))[:2, 2:]
    np.testing.assert_allclose(np.array(r)[:2, :3].astype(np.float64), want, rtol=1e-10)
    assert r[0][3] is None and r[2] == [None] * 4 and r[0][1] > 0.99
    assert M.best_channel([0.1, -0.7, 0.7, None]) == 1 and M.best_channel([None, None]) is None
    case = O.make_case("t", 40, 4, 2, 5)
    rep = O.report(case.z, case.attrs, case.channels, case.deltas)
    doc = M.attribute_report(["a", "b"], [1, -1], [1.0, 2.0], rep["counts"], rep["loss_sum"], M.pearson_matrix(case.z, case.attrs))
    assert set(doc) == {"attributes", "kendall_tau_b", "concordance", "pearson_r", "counts"}
    assert set(doc["attributes"]["a"]) == {"latent_channel", "delta", "pairs", "concordance", "kendall_tau_b", "pearson_r",
                                           "ar_loss", "best_channel", "mapped_channel_is_best"}
    assert doc["attributes"]["b"]["kendall_tau_b"] is None and doc["attributes"]["b"]["mapped_channel_is_best"] is False
    assert doc["attributes"]["a"]["kendall_tau_b"] == doc["kendall_tau_b"][0][1]
    json.dumps(doc, allow_nan=False)


def test_load_attribute_mapping_errors():
    from pti_ldm_vae_amd.analyze_ar_channels import load_attribute_mapping
    ns = types.SimpleNamespace
    with pytest.raises(ValueError, match="regularized_attributes"):
        load_attribute_mapping(ns())
    with pytest.raises(ValueError, match="regularized_attributes"):
        load_attribute_mapping(ns(regularized_attributes={}))
    with pytest.raises(ValueError, match="empty"):
        load_attribute_mapping(ns(regularized_attributes={"enabled": True}))
    with pytest.raises(ValueError, match="empty"):
        load_attribute_mapping(ns(regularized_attributes={"attribute_latent_mapping": {"_comment": "x"}}))
    got = load_attribute_mapping(ns(regularized_attributes={"attribute_latent_mapping": {
        "_comment": "x", "height_0": {"latent_channel": 0, "delta": 1.0}, "width_0": {"latent_channel": "3"}}}))
    assert got == {"height_0": 0, "width_0": 3}
    from pti_ldm_vae_amd.utils.config import load_vae_config
    real = load_attribute_mapping(load_vae_config(os.path.join(ROOT, "config", "ar_vae_dente_kl1e3.json")))
    assert real == {"height_0": 0, "width_0": 1, "width_1": 2, "width_2": 3, "width_3": 4, "width_4": 5}


def test_normalize_to_unit_edge_cases():
    from pti_ldm_vae_amd.analyze_ar_channels import _normalize_to_unit, channel_titles
    empty = np.zeros((0, 3), np.float32)
    assert _normalize_to_unit(empty) is empty
    const = np.full((4, 5), 2.5, np.float32)
    out = _normalize_to_unit(const)
    assert out.shape == const.shape and out.dtype == const.dtype and not out.any()
    x = np.array([[-2.0, 0.0], [2.0, 6.0]])
    np.testing.assert_array_equal(_normalize_to_unit(x), (x + 2.0) / 8.0)
    assert _normalize_to_unit(np.array([3.0])).tolist() == [0.0]
    assert channel_titles(3, {"h": 2, "w": 0, "far": 9}) == ["ch 0: w (regularized)", "ch 1: unmapped", "ch 2: h (regularized)"]


def test_panel_and_heatmap_writers(tmp_path):
    from PIL import Image
    from pti_ldm_vae_amd.analyze_ar_channels import save_panel
    from pti_ldm_vae_amd.utils.ar_metrics import save_tau_heatmap
    rng = np.random.default_rng(0)
    lat = rng.normal(size=(10, 8, 8)).astype(np.float32)
    lat[4] = 0.0
    p = save_panel(tmp_path / "panel.png", rng.random((1, 32, 32)), rng.random((1, 32, 32)), lat, {"height_0": 0, "width_0": 1})
    with Image.open(p) as im:
        assert im.size[0] > 200 and im.size[1] > 200
    tau = [[0.5, None, -0.25], [None, None, None]]
    h = save_tau_heatmap(tmp_path / "tau.png", tau, ["a", "b"], [0, -1])
    with Image.open(h) as im:
        assert im.format == "PNG"


def test_argument_parsing_of_both_commands():
    from pti_ldm_vae_amd import analyze_ar_channels as A
    from pti_ldm_vae_amd import evaluate_ar_vae as E
    a = E.parse_args(["-c", "cfg.json", "--checkpoint", "w.pth", "--input-dir", "imgs"])
    assert (a.batch_size, a.seed, a.num_samples, a.num_workers, a.attributes_path, a.output_dir, a.random_init_vae) == (
        8, 42, None, 4, None, None, False)
    a = E.parse_args(["-c", "c", "--checkpoint", "w", "--input-dir", "d", "--attributes-path", "a.json", "--output-dir", "o",
                      "--batch-size", "5", "--num-samples", "23", "--num-workers", "2", "--seed", "7", "--random-init-vae"])
    assert (a.attributes_path, a.output_dir, a.batch_size, a.num_samples, a.num_workers, a.seed, a.random_init_vae) == (
        "a.json", "o", 5, 23, 2, 7, True)
    with pytest.raises(SystemExit):
        E.parse_args(["-c", "c", "--checkpoint", "w"])
    b = A.parse_args(["-c", "c", "--checkpoint", "w", "--image-path", "x.tif"])
    assert (b.image_path, b.output_dir, b.random_init_vae) == ("x.tif", None, False)
    for flag in ("--port", "--host", "--debug"):            # no interactive server
        with pytest.raises(SystemExit):
            A.parse_args(["-c", "c", "--checkpoint", "w", "--image-path", "x.tif", flag, "1"])


def test_check_table_refusals():
    import torch
    from pti_ldm_vae_amd.evaluate_ar_vae import check_table
    check_table(torch.zeros(5, 2), ["a", "b"])
    with pytest.raises(SystemExit, match="--num-samples"):
        check_table(torch.zeros(32769, 1), ["a"])
    with pytest.raises(SystemExit, match="at least 2"):
        check_table(torch.zeros(1, 1), ["a"])
    t = torch.zeros(4, 2)
    t[2, 1] = float("nan")
    with pytest.raises(SystemExit, match="'b' of image 2"):
        check_table(t, ["a", "b"])
    t[2, 1] = float("inf")
    with pytest.raises(SystemExit, match="not finite"):
        check_table(t, ["a", "b"])


def test_rank_agreement_refusals_and_size_query():
    """PTI_EINVAL (-1) / PTI_EUNSUPPORTED (-2) before any launch; pointers are never dereferenced on these paths."""
    from pti_ldm_vae_amd import _lib as L
    h = L.lib()
    ws = h.pti_rank_agreement_ws_bytes
    slot = 4 * 8 + 5 * 17 * 2 * 4                      # per workgroup: 4 fp64 loss partials + 5 x 17 {C, D} int32 pairs
    assert ws(2, 1, 1) == slot and ws(256, 16, 4) == slot and ws(257, 10, 6) == 3 * 2 * slot
    assert ws(32768, 16, 16) == 128 * 129 // 2 * 4 * slot
    assert ws(1, 1, 1) == 0 and ws(32769, 1, 1) == 0 and ws(10, 17, 1) == 0 and ws(10, 1, 17) == 0 and ws(10, 0, 1) == 0
    p = C.c_void_p(4096)
    ch, dl = (C.c_int32 * 16)(*([0] * 16)), (C.c_float * 16)(*([1.0] * 16))

    def call(zt=p, ldz=100, attrs=p, lda=100, n=100, l=4, na=2, channels=ch, deltas=dl, counts=p, loss=p, wsp=p, nbytes=1 << 20):
        return h.pti_rank_agreement(zt, ldz, attrs, lda, n, l, na, channels, deltas, counts, loss, wsp, nbytes, None)

    for kw in (dict(zt=None), dict(attrs=None), dict(channels=None), dict(deltas=None), dict(counts=None), dict(loss=None),
               dict(wsp=None)):
        assert call(**kw) == -1 and b"null" in h.pti_last_error_string(), kw
    assert call(n=1) == -1 and call(l=0) == -1 and call(na=0) == -1
    assert call(n=32769, ldz=40000, lda=40000) == -2 and b"unsupported" in h.pti_last_error_string()
    assert call(l=17) == -2 and call(na=17) == -2
    assert call(ldz=99) == -1 and b"stride" in h.pti_last_error_string()
    assert call(lda=99) == -1
    bad = (C.c_int32 * 16)(*([0, 4] + [0] * 14))
    assert call(channels=bad) == -1 and b"channels[1]" in h.pti_last_error_string()
    assert call(wsp=C.c_void_p(4100)) == -1 and b"aligned" in h.pti_last_error_string()
    assert call(counts=C.c_void_p(4100)) == -1 and call(zt=C.c_void_p(4098)) == -1
    assert call(nbytes=ws(100, 4, 2) - 1) == -1 and b"workspace" in h.pti_last_error_string()
    with pytest.raises(L.PtiError):
        L.check(-1, "pti_rank_agreement")


def test_rank_agreement_refuses_an_out_tuple_of_the_wrong_length():
    """The length of ``out=(counts, loss_sum)`` is checked before anything else, so no device is needed."""
    import torch

    from pti_ldm_vae_amd import ops
    z, a = torch.zeros(10, 3), torch.zeros(2, 10)
    for out in ((None,), (None, None, None), ()):
        with pytest.raises(ValueError, match=r"rank_agreement: out must be \(counts, loss_sum\)"):
            ops.rank_agreement(z, a, [0, 1], [1.0, 1.0], out=out)

"""CPU tests of the disentanglement report: the numpy oracle against scipy, sklearn and numpy's own histogram and against its
committed golden file, the mutations of the oracle that the checks must catch, ``utils.disentanglement`` on the oracle's
integer tables, the pieces of the command that need no GPU, and the refusals of ``pti_tied_ranks`` / ``pti_rank_moments`` /
``pti_joint_histogram`` (they return before any launch)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import disentanglement_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports():
    """{case name: (case, oracle report)}: computed once and shared, never modified."""
    return {case.name: (case, O.report(case.z, case.attrs, case.bins)) for case in O.all_cases()}


def _nan(rows):
    return np.array([[np.nan if v is None else v for v in row] for row in rows], dtype=np.float64)


def _close(got, want, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want)) and bool(np.all(np.abs(got - want)[~np.isnan(want)] <= tol))


def test_case_list_is_the_specified_one(reports):
    assert [(n, l, na) for _, n, l, na, *_ in O.CASES[:6]] == [(2, 1, 1), (3, 2, 1), (65, 3, 2), (257, 10, 6), (1030, 16, 16),
                                                                  (2500, 10, 6)]
    assert O.CASES[5][7][0] > 0 and O.CASES[5][7][1] > 0 and [n for _, n, *_ in O.CASES[6:]] == [97, 300]
    assert {spec[6] for spec in O.CASES} == {2, 20, 32}
    case = reports["n97_const"][0]
    assert np.all(case.z[:, 2] == case.z[0, 2]) and np.all(case.attrs[1] == case.attrs[1, 0])
    case = reports["n300_edges"][0]
    assert case.bins == 20 and sorted(set(case.z[:, 0].tolist())) == [float(v) for v in range(21)]   # a value on every edge
    assert np.array_equal(reports["n300_edges"][1]["edges"][0], np.arange(20.0))
    assert np.any(np.signbit(case.z[:, 1]) & (case.z[:, 1] == 0)) and np.any(~np.signbit(case.z[:, 1]) & (case.z[:, 1] == 0))
    assert len(set(case.attrs[0].tolist())) == 5


def test_oracle_reproduces_the_golden_file(reports):
    gold = O.load_golden()
    assert sorted(gold) == sorted(f"{name}/{k}" for name in reports for k in O.TABLES + O.FLOATS)
    assert os.path.getsize(O.GOLDEN) < 1 << 20
    for name, (_, r) in reports.items():
        for k in O.TABLES:
            assert np.array_equal(gold[f"{name}/{k}"], r[k]) and gold[f"{name}/{k}"].dtype == r[k].dtype, (name, k)
        for k in O.FLOATS:
            assert _close(gold[f"{name}/{k}"], r[k]), (name, k)
    assert gold["n1030/rank2"].dtype == np.int32 and gold["n1030/gram"].dtype == np.int64
    assert gold["n1030/bins"].dtype == np.uint8 and gold["n1030/counts"].dtype == np.int32


def test_integer_tables_are_consistent(reports):
    for name, (case, r) in reports.items():
        assert np.all(r["rank2"].astype(np.int64).sum(1) == case.n * (case.n + 1)), name
        assert np.all(r["counts"].sum((2, 3)) == case.n), name
        assert r["bins"].max() < case.bins and np.array_equal(np.diag(r["gram"]) >= r["sums"], np.ones(case.l + case.na, bool))
        for q in range(case.na):                                     # the marginals are the row and column sums
            for c in range(case.l):
                assert np.array_equal(r["counts"][q, c].sum(1), np.bincount(r["bins"][case.l + q], minlength=case.bins))
                assert np.array_equal(r["counts"][q, c].sum(0), np.bincount(r["bins"][c], minlength=case.bins))
    z1 = reports["n300_edges"][0].z[:, 1]
    r1 = reports["n300_edges"][1]["rank2"][1]
    assert len(set(r1[z1 == 0].tolist())) == 1                       # -0.0 ties with 0.0


def test_oracle_ranks_and_spearman_equal_scipy(reports):
    from scipy.stats import rankdata, spearmanr
    for name, (case, r) in reports.items():
        cols = O.columns(case.z, case.attrs)
        assert np.array_equal(r["rank2"], np.stack([np.rint(2 * rankdata(c, method="average")) for c in cols]).astype(np.int32)), name
    for name in ("n65", "n257"):
        case, r = reports[name]
        for q in range(case.na):
            for c in range(case.l):
                want = spearmanr(case.attrs[q], case.z[:, c]).statistic
                assert abs(r["spearman_rho"][q, c] - want) <= 1e-12, (name, q, c)


def test_oracle_bins_and_mi_equal_numpy_and_sklearn(reports):
    from sklearn.metrics import mutual_info_score
    for name, (case, r) in reports.items():
        cols = O.columns(case.z, case.attrs)
        for k, x in enumerate(cols):
            counts, edges = np.histogram(x, case.bins)
            assert np.array_equal(r["edges"][k], edges[:-1].astype(np.float64)), (name, k)
            assert np.array_equal(r["bins"][k], np.digitize(x, edges[:-1]) - 1), (name, k)
            assert np.array_equal(np.bincount(r["bins"][k], minlength=case.bins), counts), (name, k)   # numpy's own histogram
    for name in ("n65", "n257", "n300_edges"):
        case, r = reports[name]
        for q in range(case.na):
            for c in range(case.l):
                want = mutual_info_score(r["bins"][case.l + q], r["bins"][c])
                assert abs(r["mutual_information"][q, c] - want) <= 1e-12, (name, q, c)
            assert abs(r["entropy"][q] - mutual_info_score(r["bins"][case.l + q], r["bins"][case.l + q])) <= 1e-12


@pytest.mark.parametrize("bins", [2, 20, 32])
def test_counting_rule_equals_digitize_on_the_edges(bins):
    """The device's bin rule, #{k: edges[k] <= (double) x} - 1, with values sitting exactly on interior edges."""
    from pti_ldm_vae_amd.utils.disentanglement import bin_edges
    rng = np.random.default_rng(bins)
    for lo, hi in ((0.0, float(bins)), (-1.0, 3.0), (0.3, 0.3)):
        edges = bin_edges(lo, hi, bins)
        assert edges.dtype == np.float64 and edges.shape == (bins,)
        x = np.concatenate([edges.astype(np.float32), rng.uniform(edges[0], edges[-1] + 1.0, 200).astype(np.float32),
                            np.array([lo, hi], np.float32)])
        x = x[x.astype(np.float64) >= edges[0]]
        counted = (edges[None, :] <= x.astype(np.float64)[:, None]).sum(1) - 1
        assert np.array_equal(counted, np.digitize(x, edges) - 1)
        assert counted.min() == 0 and counted.max() == bins - 1
        col = np.array([lo, hi] + [lo] * 3, np.float32)
        assert np.array_equal(edges, np.histogram(col, bins)[1][:-1].astype(np.float64))       # a constant column included


def test_host_arithmetic_reproduces_the_oracle(reports):
    from pti_ldm_vae_amd.utils import disentanglement as D
    from pti_ldm_vae_amd.utils.ar_metrics import pearson_matrix
    for name, (case, r) in reports.items():
        cols = O.columns(case.z, case.attrs)
        assert np.array_equal(D.edge_tables(cols.min(1), cols.max(1), case.bins), r["edges"]), name
        rho = D.spearman_matrix(r["sums"], r["gram"], case.n, case.na, case.l)
        assert _close(_nan(rho), r["spearman_rho"]), name
        mi, h = D.mutual_information(r["counts"])
        assert _close(mi, r["mutual_information"]) and _close(h, r["entropy"]), name
        pearson = pearson_matrix(case.z, case.attrs)
        assert _close(_nan(pearson), r["pearson_r"], 1e-10), name
        names = [f"a{q}" for q in range(case.na)]
        doc = D.disentanglement_report(names, case.channels, case.n, r["sums"], r["gram"], r["counts"], pearson)
        json.dumps(doc, allow_nan=False)                                                         # null, never NaN
        got = np.array([np.nan if doc["scores"][k] is None else doc["scores"][k] for k in O.SCORES])
        assert _close(got, r["scores"], 1e-9), (name, got, r["scores"])
        for q, key in enumerate(names):
            entry = doc["attributes"][key]
            assert set(entry) == {"latent_channel", "spearman_rho", "best_channel_spearman", "mapped_channel_is_best", "mig", "sap"}
            assert entry["spearman_rho"] == rho[q][case.channels[q]]
            ok = ~np.isnan(r["spearman_rho"][q])
            assert entry["best_channel_spearman"] == (int(np.nanargmax(np.abs(r["spearman_rho"][q]))) if ok.any() else None)
            assert _close([np.nan if entry[k] is None else entry[k] for k in ("mig", "sap")], [r["mig"][q], r["sap"][q]], 1e-9)
        for k, labels in (("mig", names), ("sap", names), ("interpretability", names),
                          ("modularity", [f"channel {c}" for c in range(case.l)])):
            assert doc["excluded"][k] == [lab for lab, v in zip(labels, r[k]) if np.isnan(v)], (name, k)
    with pytest.raises(ValueError):
        D.spearman_matrix([1, 2], [[1, 2], [3, 4]], 5, 2, 2)
    with pytest.raises(ValueError):
        D.mutual_information(np.zeros((2, 3, 4)))


MUTATIONS = {"ordinal_ranks": "rank2", "strict_edges": "bins", "open_last_bin": "counts", "log2_mi": "scores",
             "unsorted_top_two": "scores", "modularity_over_na": "scores"}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_mutated_oracle_is_caught(reports, mutation):
    """Each wrong definition changes an exact table or moves a score by more than 1e-9 on at least one case."""
    caught = set()
    for name in ("n65", "n257", "n97_const", "n300_edges"):
        case, r = reports[name]
        m = O.report(case.z, case.attrs, case.bins, **{mutation: True})
        caught |= {k for k in O.TABLES if not np.array_equal(m[k], r[k])}
        ok = ~np.isnan(r["scores"])
        if np.any(np.isnan(m["scores"][ok])) or np.max(np.abs(m["scores"][ok] - r["scores"][ok])) > 1e-9:
            caught.add("scores")
    assert MUTATIONS[mutation] in caught, (mutation, caught)


def test_none_and_excluded_rules():
    from pti_ldm_vae_amd.utils import disentanglement as D
    mi = np.array([[0.5, 0.2, 0.0], [0.0, 0.0, 0.0], [0.1, 0.4, 0.0]])
    h = np.array([1.0, 0.0, 2.0])
    pearson = [[0.9, -0.5, None], [None, None, None], [0.1, None, None]]
    s = D.scores(mi, h, pearson, ["a", "b", "c"])
    assert s["per_attribute"]["mig"] == [pytest.approx(0.3), None, pytest.approx(0.15)]          # H = 0: no MIG
    assert s["per_attribute"]["sap"] == [pytest.approx(0.81 - 0.25), None, None]                 # fewer than two defined r
    assert s["per_attribute"]["interpretability"] == [pytest.approx(0.81), None, None]           # r undefined at argmax MI
    assert s["per_channel"]["modularity"][:2] == [pytest.approx(1 - 0.01 / (0.25 * 2)), pytest.approx(1 - 0.04 / (0.16 * 2))]
    assert s["per_channel"]["modularity"][2] is None                                             # a channel without any MI
    assert s["excluded"] == {"mig": ["b"], "modularity": ["channel 2"], "sap": ["b", "c"], "interpretability": ["b", "c"]}
    assert s["scores"]["mig"] == pytest.approx(0.225) and s["scores"]["sap"] == pytest.approx(0.56)
    json.dumps(s, allow_nan=False)
    one = D.scores(np.array([[0.3, 0.1]]), np.array([1.0]), [[0.5, 0.2]], ["a"])                  # na < 2: no modularity
    assert one["scores"]["modularity"] is None and one["excluded"]["modularity"] == ["channel 0", "channel 1"]
    col = D.scores(np.array([[0.3], [0.2]]), np.array([1.0, 1.0]), [[0.5], [0.2]], ["a", "b"])    # L < 2: no gaps
    assert col["scores"]["mig"] is None and col["scores"]["sap"] is None and col["scores"]["interpretability"] == pytest.approx(0.145)
    assert D.spearman_matrix([6, 6, 6], [[14, 12, 14], [12, 12, 12], [14, 12, 14]], 3, 1, 2) == [[1.0, None]]
    assert D.best_channel([0.1, -0.7, 0.7, None]) == 1 and D.best_channel([None]) is None


def test_argument_parsing():
    from pti_ldm_vae_amd import evaluate_disentanglement as E
    a = E.parse_args(["-c", "cfg.json", "--checkpoint", "w.pth", "--input-dir", "imgs"])
    assert (a.batch_size, a.seed, a.num_samples, a.num_workers, a.attributes_path, a.output_dir, a.random_init_vae, a.bins,
            a.from_npz) == (8, 42, None, 4, None, None, False, 20, None)
    a = E.parse_args(["-c", "c", "--checkpoint", "w", "--input-dir", "d", "--attributes-path", "a.json", "--output-dir", "o",
                      "--batch-size", "5", "--num-samples", "23", "--num-workers", "2", "--seed", "7", "--random-init-vae",
                      "--bins", "32"])
    assert (a.attributes_path, a.output_dir, a.batch_size, a.num_samples, a.num_workers, a.seed, a.random_init_vae, a.bins) == (
        "a.json", "o", 5, 23, 2, 7, True, 32)
    a = E.parse_args(["-c", "c", "--from-npz", "m.npz"])
    assert a.from_npz == "m.npz" and a.checkpoint is None and a.input_dir is None
    for bad in (["-c", "c", "--checkpoint", "w"], ["-c", "c", "--input-dir", "d"], ["--from-npz", "m.npz"],
                ["-c", "c", "--from-npz", "m.npz", "--bins", "1"], ["-c", "c", "--from-npz", "m.npz", "--bins", "33"]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)


def test_from_npz_with_a_stubbed_device_layer(tmp_path, monkeypatch):
    """``--from-npz`` loads no model and no images: with the device layer replaced by the oracle's tables the command runs
    on the CPU and writes what the oracle computes."""
    import torch
    from PIL import Image
    from pti_ldm_vae_amd import evaluate_disentanglement as E
    cfg = json.load(open(os.path.join(ROOT, "config", "ar_vae_dente_kl1e3.json")))
    names = [k for k in cfg["regularized_attributes"]["attribute_latent_mapping"] if not k.startswith("_")]
    cfg["run_dir"] = str(tmp_path / "run")
    cf = tmp_path / "ar.json"
    cf.write_text(json.dumps(cfg))
    case = O.make_case("cli", 40, 10, len(names), 5, "plain", 20)
    files = [f"img_{i:03d}.tif" for i in range(case.n)]
    npz = tmp_path / "channel_means.npz"
    np.savez(npz, z=case.z, attrs=case.attrs, names=np.array(names), files=np.array(files))
    calls = []

    def tables(z, attrs, bins):
        calls.append((tuple(z.shape), tuple(attrs.shape), bins, z.dtype))
        r = O.report(z.numpy(), attrs.numpy(), bins)
        return r["sums"], r["gram"], r["counts"].astype(np.int64), z.numpy()

    monkeypatch.setattr(E, "init_device_and_seed", lambda seed: torch.device("cpu"))
    monkeypatch.setattr(E, "device_tables", tables)
    monkeypatch.setattr(E, "load_model", lambda *a, **k: pytest.fail("--from-npz must not load a model"))
    E.main(["-c", str(cf), "--from-npz", str(npz), "--bins", "8"])
    assert calls == [((40, 10), (len(names), 40), 8, torch.float32)]
    out = tmp_path / "run" / "ar_eval"
    doc = json.loads((out / "disentanglement.json").read_text())
    assert set(doc) == {"scores", "attributes", "spearman_rho", "mutual_information", "pearson_r", "entropy", "bins", "n_images",
                        "excluded", "args", "files"}
    assert doc["bins"] == 8 and doc["n_images"] == 40 and doc["files"] == files and list(doc["attributes"]) == names
    assert doc["args"]["from_npz"] == str(npz) and set(doc["scores"]) == set(O.SCORES)
    r = O.report(case.z, case.attrs, 8)
    assert _close(_nan(doc["spearman_rho"]), r["spearman_rho"]) and _close(doc["mutual_information"], r["mutual_information"])
    assert _close([doc["scores"][k] for k in O.SCORES], r["scores"], 1e-9)
    mapping = cfg["regularized_attributes"]["attribute_latent_mapping"]
    for q, k in enumerate(names):
        ch = int(mapping[k]["latent_channel"])
        assert doc["attributes"][k]["latent_channel"] == ch and doc["attributes"][k]["spearman_rho"] == doc["spearman_rho"][q][ch]
    with Image.open(out / "disentanglement.png") as im:
        assert im.format == "PNG"
    np.savez(npz, z=case.z, attrs=case.attrs, names=np.array(names[::-1]))
    with pytest.raises(SystemExit, match="holds attributes"):
        E.main(["-c", str(cf), "--from-npz", str(npz)])
    np.savez(npz, z=case.z[:, :4], attrs=case.attrs, names=np.array(names))
    with pytest.raises(SystemExit, match="4 channels"):
        E.main(["-c", str(cf), "--from-npz", str(npz)])
    np.savez(npz, z=case.z)
    with pytest.raises(SystemExit, match="lacks"):
        E.main(["-c", str(cf), "--from-npz", str(npz)])


def test_entry_point_refusals_and_size_query():
    """PTI_EINVAL (-1) / PTI_EUNSUPPORTED (-2) before any launch; pointers are never dereferenced on these paths."""
    from pti_ldm_vae_amd import _lib as L
    from pti_ldm_vae_amd import ops
    h = L.lib()
    assert (ops.DISENT_MAX_N, ops.DISENT_MAX_COLS, ops.DISENT_MAX_BINS) == (32768, 32, 32)
    p = C.c_void_p(4096)

    def ranks(cols=p, ld=100, n=100, m=4, rank2=p):
        return h.pti_tied_ranks(cols, ld, n, m, rank2, None)

    assert ranks(cols=None) == -1 and b"null" in h.pti_last_error_string()
    assert ranks(rank2=None) == -1 and b"tied_ranks" in h.pti_last_error_string()
    assert ranks(n=1) == -1 and ranks(m=0) == -1
    assert ranks(n=32769, ld=40000) == -2 and b"unsupported" in h.pti_last_error_string()
    assert ranks(m=33) == -2
    assert ranks(ld=99) == -1 and b"stride" in h.pti_last_error_string()
    assert ranks(cols=C.c_void_p(4098)) == -1 and b"misaligned" in h.pti_last_error_string()
    assert ranks(rank2=C.c_void_p(4097)) == -1

    def moments(rank2=p, n=100, m=4, sums=p, gram=p):
        return h.pti_rank_moments(rank2, n, m, sums, gram, None)

    for kw in (dict(rank2=None), dict(sums=None), dict(gram=None)):
        assert moments(**kw) == -1 and b"null" in h.pti_last_error_string(), kw
    assert moments(n=1) == -1 and moments(m=0) == -1 and b"rank_moments" in h.pti_last_error_string()
    assert moments(n=32769) == -2 and moments(m=33) == -2 and b"unsupported" in h.pti_last_error_string()
    assert moments(rank2=C.c_void_p(4098)) == -1 and moments(sums=C.c_void_p(4100)) == -1
    assert moments(gram=C.c_void_p(4100)) == -1 and b"misaligned" in h.pti_last_error_string()

    ws = h.pti_joint_histogram_ws_bytes
    assert ws(2, 1, 1, 2) == 16 and ws(2048, 10, 6, 20) == 60 * 400 * 4 and ws(2049, 10, 6, 20) == 2 * 60 * 400 * 4
    assert ws(32768, 16, 16, 32) == 16 * 256 * 1024 * 4
    for bad in ((1, 1, 1, 2), (32769, 1, 1, 2), (10, 17, 1, 2), (10, 1, 17, 2), (10, 0, 1, 2), (10, 1, 0, 2), (10, 1, 1, 1),
                (10, 1, 1, 33)):
        assert ws(*bad) == 0, bad

    def hist(zt=p, ldz=100, attrs=p, lda=100, n=100, l=4, na=2, bins=20, ez=p, ea=p, bz=p, ba=p, counts=p, wsp=p, nbytes=1 << 20):
        return h.pti_joint_histogram(zt, ldz, attrs, lda, n, l, na, bins, ez, ea, bz, ba, counts, wsp, nbytes, None)

    for kw in (dict(zt=None), dict(attrs=None), dict(ez=None), dict(ea=None), dict(bz=None), dict(ba=None), dict(counts=None),
               dict(wsp=None)):
        assert hist(**kw) == -1 and b"null" in h.pti_last_error_string(), kw
    assert hist(n=1) == -1 and hist(l=0) == -1 and hist(na=0) == -1 and hist(bins=1) == -1
    assert b"joint_histogram" in h.pti_last_error_string()
    assert hist(n=32769, ldz=40000, lda=40000) == -2 and b"unsupported" in h.pti_last_error_string()
    assert hist(l=17) == -2 and hist(na=17) == -2 and hist(bins=33) == -2
    assert hist(ldz=99) == -1 and b"stride" in h.pti_last_error_string()
    assert hist(lda=99) == -1
    assert hist(zt=C.c_void_p(4098)) == -1 and hist(attrs=C.c_void_p(4098)) == -1 and hist(counts=C.c_void_p(4098)) == -1
    assert hist(ez=C.c_void_p(4100)) == -1 and hist(ea=C.c_void_p(4100)) == -1 and b"misaligned" in h.pti_last_error_string()
    assert hist(wsp=C.c_void_p(4098)) == -1 and b"aligned" in h.pti_last_error_string()
    assert hist(nbytes=ws(100, 4, 2, 20) - 1) == -1 and b"workspace" in h.pti_last_error_string()
    with pytest.raises(L.PtiError):
        L.check(-2, "pti_joint_histogram")


def test_out_tuples_of_the_wrong_length_are_refused():
    """``out=(sums, gram)`` / ``out=(bins_z, bins_a, counts)``: the length is checked before anything else (no device needed)."""
    import torch

    from pti_ldm_vae_amd import ops
    rank2 = torch.ones(2, 10, dtype=torch.int32)
    for out in ((None,), (None, None, None)):
        with pytest.raises(ValueError, match=r"rank_moments: out must be \(sums, gram\)"):
            ops.rank_moments(rank2, out=out)
    z, a, ez, ea = torch.rand(10, 3), torch.rand(2, 10), torch.zeros(3, 4), torch.zeros(2, 4)
    for out in ((None, None), (None, None, None, None)):
        with pytest.raises(ValueError, match=r"joint_histogram: out must be \(bins_z, bins_a, counts\)"):
            ops.joint_histogram(z, a, ez, ea, out=out)

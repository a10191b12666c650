"""GPU tests of the projection-quality report: ``ops.neighbor_ranks`` / ``ops.segment_row_sums`` (csrc/projection_quality.hip)
against the numpy oracle (tests/projection_quality_oracle.py), their locality, reproducibility and refusals,
``analysis.projection_quality`` on the golden cases, and ``analyze_static --quality`` end to end.

Gates.  Ranks and every other integer: equality.  A segment sum: |got - fsum| <= (len - 1) 2^-53 sum |d|, the bound of an
fp64 sum in any order.  The report against the oracle on the device's OWN distance matrices: ratios 1e-13 relative (same
integers, same formula); per-point silhouettes 4 (n - 1) 2^-53 absolute (a and b each carry one such sum, s = (b - a) / max(a,
b) at most doubles their relative errors).  The report against scikit-learn's recorded fp64 values: at most twice the
deviation of the oracle on numpy fp32 distances from the same values, computed here."""
import json
import math
import os

import numpy as np
import pytest
import torch

import projection_quality_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "projection_quality_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _true_distances(n, seed):
    rng = np.random.default_rng(seed)
    return O.pairwise(rng.standard_normal((n, 6)).astype(np.float32), np.float32)


def _planted_ties(n, seed):
    """Duplicate rows, a constant row, -0.0 and +inf entries."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 4)).astype(np.float32)
    x[1] = x[0]                                             # duplicate rows: a zero off the diagonal, two equal rows
    if n > 4:
        x[n - 1] = x[n // 2]
    d = O.pairwise(np.round(x * 4) / 4, np.float32)         # a coarse grid: many equal distances
    d[2 % n, :] = 1.5                                       # a constant row (its diagonal included)
    d[0, n - 1] = -0.0
    d[n - 1, 0] = -0.0
    d[1, 2 % n] = np.inf
    d[n - 1, 1] = np.inf
    if n > 4:
        d[3, 3] = -0.0
        d[4, :3] = np.inf
    return d


def _listed(n, m, seed):
    """Random neighbour lists with the row's own index and repeated entries in them."""
    rng = np.random.default_rng(seed)
    nbr = rng.integers(0, n, size=(n, m)).astype(np.int32)
    nbr[::2, 0] = np.arange(n)[::2]                         # own index
    if m > 1:
        nbr[:, m - 1] = nbr[:, 0]                           # a repeated entry
    return nbr


RANK_CASES = [(n, m) for n in (3, 5, 64, 65, 300) for m in sorted({1, 2, 40, min(n - 1, 256)})]


@pytest.mark.parametrize("n,m", RANK_CASES)
@pytest.mark.parametrize("kind", ["true", "ties"])
def test_neighbor_ranks_equal_the_oracle(dev, n, m, kind):
    from pti_ldm_vae_amd import ops
    d = (_true_distances if kind == "true" else _planted_ties)(n, 100 * n + m)
    nbr = _listed(n, m, 7 * n + m)
    want = O.neighbor_ranks(d, nbr)
    assert (want == 0).any() and (kind == "true" or O.has_row_ties(d))
    dist, idx = torch.from_numpy(d).to(dev), torch.from_numpy(nbr).to(dev)
    got = ops.neighbor_ranks(dist, idx)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, m)
    assert np.array_equal(got.cpu().numpy(), want)
    # a row-strided view of the matrix is used in place; out is written in place and nothing after it
    pad = torch.full((n, n + 5), 9.0, device=dev)
    pad[:, 2:n + 2] = dist
    buf = torch.full((n * m + 64,), -77, dtype=torch.int32, device=dev)
    out = buf[:n * m].view(n, m)
    assert ops.neighbor_ranks(pad[:, 2:n + 2], idx, out=out) is out
    assert torch.equal(out, got) and bool((buf[n * m:] == -77).all())
    # rank <= k is what umap_knn returns without the diagonal
    if kind == "true" and 2 <= m < n - 1 and m + 1 <= 256:
        knn, _ = ops.umap_knn(dist, m + 1)
        ranks = ops.neighbor_ranks(dist, knn.contiguous()).cpu().numpy()
        assert np.array_equal(ranks, np.tile(np.arange(m + 1), (n, 1)))    # distinct distances: self first, then 1 .. m


def test_neighbor_ranks_foreign_indices_are_not_dereferenced(dev):
    from pti_ldm_vae_amd import ops
    d = _true_distances(65, 1)
    nbr = _listed(65, 6, 2)
    nbr[:, 1], nbr[:, 3], nbr[5, 4] = -1, 65, 2 ** 31 - 1
    got = ops.neighbor_ranks(torch.from_numpy(d).to(dev), torch.from_numpy(nbr).to(dev)).cpu().numpy()
    assert np.array_equal(got, O.neighbor_ranks(d, nbr)) and (got[:, 1] == -1).all() and (got[:, 3] == -1).all() and got[5, 4] == -1


def test_neighbor_ranks_at_the_row_cap(dev):
    from pti_ldm_vae_amd import ops
    n, m = 8192, 4
    gen = torch.Generator(device=dev).manual_seed(8192)
    dist = torch.rand(n, n, generator=gen, device=dev)
    nbr = torch.randint(0, n, (n, m), generator=gen, device=dev, dtype=torch.int32)
    got = ops.neighbor_ranks(dist, nbr)
    rows = [0, 1, 63, 64, 255, 256, 1000, 2047, 4095, 4096, 5000, 6001, 7777, 8000, 8190, 8191]
    sel = torch.tensor(rows, device=dev)
    want = O.neighbor_ranks(dist[sel].cpu().numpy(), nbr[sel].cpu().numpy(), rows=rows)
    assert np.array_equal(got[sel].cpu().numpy(), want) and int(got.min()) >= 0 and int(got.max()) <= n - 1


def test_neighbor_ranks_are_local_and_reproducible(dev):
    from pti_ldm_vae_amd import ops
    d = torch.from_numpy(_planted_ties(300, 5)).to(dev)
    nbr = torch.from_numpy(_listed(300, 40, 6)).to(dev)
    first = ops.neighbor_ranks(d, nbr)
    assert torch.equal(ops.neighbor_ranks(d, nbr), first)
    moved = nbr.clone()
    rows = torch.tensor([3, 64, 65, 299], device=dev)
    moved[rows] = nbr[rows].flip(1)
    again = ops.neighbor_ranks(d, moved)
    keep = torch.ones(300, dtype=torch.bool, device=dev)
    keep[rows] = False
    assert torch.equal(again[keep], first[keep]) and torch.equal(again[rows], first[rows].flip(1))


def _segments(n, g):
    """g segments over n columns with empty ones first, last and in the middle where g allows."""
    if g == 1:
        return [0, n]
    if g == n:
        return list(range(n + 1))
    if g == 2:
        return [0, 0, n]
    assert g == 7
    a, b, c = max(1, n // 4), max(2, n // 2), max(3, 3 * n // 4)
    return [0, 0, a, b, b, c, n, n]


SUM_CASES = [(n, g) for n in (3, 65, 300) for g in sorted({1, 2, 7, n})]


@pytest.mark.parametrize("n,g", SUM_CASES)
def test_segment_row_sums_values(dev, n, g):
    from pti_ldm_vae_amd import ops
    seg = _segments(n, g)
    assert len(seg) == g + 1 and seg[0] == 0 and seg[-1] == n and all(b >= a for a, b in zip(seg, seg[1:]))
    if g == 7:
        assert seg[1] == 0 and seg[-2] == n and any(a == b for a, b in zip(seg[2:-2], seg[3:-1]))   # empty: first, last, middle
    d = _true_distances(n, n + g) * 37.0
    got = ops.segment_row_sums(torch.from_numpy(d).to(dev), seg)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, g)
    got = got.cpu().numpy()
    d64 = d.astype(np.float64)
    worst = 0.0
    for i in range(n):
        for s in range(g):
            vals = d64[i, seg[s]:seg[s + 1]]
            want, bound = math.fsum(vals), max(len(vals) - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(vals))
            assert abs(got[i, s] - want) <= bound, (i, s, got[i, s], want, bound)
            if len(vals) == 0:
                assert got[i, s] == 0.0
            worst = max(worst, abs(got[i, s] - want) / max(want, 1e-300))
    print(f"n={n} G={g}: largest relative deviation from fsum {worst:.2e}")
    # a device table, a row-strided matrix and an out buffer with canaries
    pad = torch.full((n, n + 3), 5.0, device=dev)
    pad[:, 1:n + 1] = torch.from_numpy(d).to(dev)
    buf = torch.full((n * g + 64,), -3.0, dtype=torch.float64, device=dev)
    out = buf[:n * g].view(n, g)
    assert ops.segment_row_sums(pad[:, 1:n + 1], torch.tensor(seg, dtype=torch.int32, device=dev), out=out) is out
    assert np.array_equal(out.cpu().numpy(), got) and bool((buf[n * g:] == -3.0).all())


def test_segment_row_sums_bits_depend_on_the_segment_alone(dev):
    from pti_ldm_vae_amd import ops
    big = torch.from_numpy(_true_distances(300, 9) * 11.0).to(dev)
    seg_big = [0, 17, 17, 80, 293, 300]
    first = ops.segment_row_sums(big, seg_big)
    assert torch.equal(ops.segment_row_sums(big, seg_big), first)
    small = torch.zeros(65, 65, device=dev)
    small[:, 2:65] = big[100:165, 17:80]                   # the 63 values of segment 2, rows 100 .. 164, elsewhere in a 65-row call
    small[:, :2] = 3.25
    got = ops.segment_row_sums(small, [0, 2, 65])
    assert torch.equal(got[:, 1].view(torch.int64), first[100:165, 2].view(torch.int64))
    wide = torch.zeros(65, 65, device=dev)
    wide[:7, :] = 1.0
    wide[:7, 30:37] = big[:7, 293:300]                     # segment 4 (7 values) of rows 0 .. 6
    got = ops.segment_row_sums(wide, [0] + [30] * 20 + [37, 65])
    assert torch.equal(got[:7, 20].view(torch.int64), first[:7, 4].view(torch.int64))


def test_refusals_come_before_any_launch(dev):
    from pti_ldm_vae_amd import ops
    d = torch.rand(8, 8, device=dev)
    nbr = torch.zeros(8, 3, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        ops.neighbor_ranks(d.double(), nbr)
    with pytest.raises(TypeError):
        ops.neighbor_ranks(d, nbr.long())
    with pytest.raises(TypeError):
        ops.neighbor_ranks(d, nbr, out=torch.zeros(8, 3, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        ops.neighbor_ranks(d, torch.zeros(3, 8, dtype=torch.int32, device=dev).t())
    with pytest.raises(ValueError):
        ops.neighbor_ranks(d, nbr[:7])
    with pytest.raises(ValueError, match="3 <= n"):
        ops.neighbor_ranks(d[:2, :2], nbr[:2])
    with pytest.raises(ValueError, match="8192"):
        ops.neighbor_ranks(torch.empty(8193, 8193, device=dev), torch.zeros(8193, 1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="256"):
        ops.neighbor_ranks(torch.rand(300, 300, device=dev), torch.zeros(300, 257, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.segment_row_sums(d.double(), [0, 8])
    with pytest.raises(TypeError):
        ops.segment_row_sums(d, torch.tensor([0, 8], device=dev))
    with pytest.raises(ValueError, match="2048"):
        ops.segment_row_sums(torch.rand(2100, 2100, device=dev), [0] * 2049 + [2100])
    for bad in ([0, 7], [1, 8], [0, 5, 4, 8], [0, 9]):
        with pytest.raises(ValueError, match="ascend"):
            ops.segment_row_sums(d, bad)
    with pytest.raises(ValueError, match="ascend"):
        ops.segment_row_sums(d, torch.tensor([0, 4, 7], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="3 <= n"):
        ops.segment_row_sums(d[:2, :2], [0, 2])


@pytest.mark.parametrize("n,d", [(1, 1), (3, 2), (65, 2), (300, 2), (257, 3), (64, 8)])
def test_projection_distances_are_fp64_rounded_once(dev, n, d):
    """Gate: at most ONE fp32 unit in the last place from the fp32 nearest numpy's fp64 distance -- the device's fp64 value is
    within a few 2^-53 of numpy's (exact differences, a sum of at most 8 squares, a root), so the two can round to different
    fp32 only when they straddle a rounding boundary, and then to neighbours."""
    from pti_ldm_vae_amd import ops
    rng = np.random.default_rng(10 * n + d)
    y = (rng.standard_normal((n, d)) * 7.0).astype(np.float32)
    if n > 2:
        y[2] = y[0]                                         # a duplicate row: exact zeros off the diagonal
    want = O.pairwise(y).astype(np.float32)
    t = torch.from_numpy(y).to(dev)
    got = ops.projection_distances(t)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, n)
    assert torch.equal(got, got.t()) and float(got.diagonal().abs().max()) == 0.0
    g = got.cpu().numpy()
    off = np.abs(g.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"n={n} d={d}: entries that differ from fp32(numpy fp64) {int((off > 0).sum())} of {n * n}, by at most {int(off.max())} ulp")
    assert off.max() <= 1 and (n < 3 or g[0, 2] == 0.0)
    assert torch.equal(ops.projection_distances(t), got)
    pad = torch.full((n, d + 3), 2.5, device=dev)
    pad[:, 1:d + 1] = t
    buf = torch.full((n + 2, n + 5), -7.0, device=dev)
    view = buf[1:n + 1, 2:n + 2]
    assert ops.projection_distances(pad[:, 1:d + 1], out=view) is view and torch.equal(view, got)
    buf[1:n + 1, 2:n + 2] = -7.0
    assert float((buf + 7.0).abs().max()) == 0.0            # nothing outside the view was written


def test_projection_distances_refusals(dev):
    from pti_ldm_vae_amd import ops
    with pytest.raises(ValueError, match="1 <= d <= 8"):
        ops.projection_distances(torch.zeros(5, 9, device=dev))
    with pytest.raises(ValueError, match="8192"):
        ops.projection_distances(torch.zeros(8193, 2, device=dev))
    with pytest.raises(TypeError):
        ops.projection_distances(torch.zeros(5, 2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.projection_distances(torch.zeros(5, 2))
    with pytest.raises(ValueError):
        ops.projection_distances(torch.zeros(5, 2, device=dev), out=torch.zeros(5, 4, device=dev))


# ---- the report ----------------------------------------------------------------------------------------------------------------
def _flat(report):
    """The report's numbers as {path: value}."""
    out = {}
    for key in ("trustworthiness", "continuity", "neighborhood_preservation"):
        out.update({f"{key}/{k}": v for k, v in report[key].items()})
    for name, entry in report["labels"].items():
        for key, val in entry.items():
            if isinstance(val, dict):
                out.update({f"{name}/{key}/{k}": v for k, v in val.items()})
            elif key != "classes":
                out[f"{name}/{key}"] = val
    return out


def _assert_reports_agree(got, want, got_points, want_points, n):
    assert {k: got[k] for k in ("n", "high_dims", "neighbors", "excluded")} == {k: want[k] for k in ("n", "high_dims", "neighbors", "excluded")}
    assert {name: e["classes"] for name, e in got["labels"].items()} == {name: e["classes"] for name, e in want["labels"].items()}
    a, b = _flat(got), _flat(want)
    assert sorted(a) == sorted(b)
    for key in a:
        assert (a[key] is None) == (b[key] is None), key
        if a[key] is not None:
            assert not math.isnan(a[key]) and abs(a[key] - b[key]) <= 1e-13 * abs(b[key]), (key, a[key], b[key])
    assert sorted(got_points) == sorted(want_points)
    for key in got_points:
        if key.endswith("_local"):                          # the same integers under the same expression: the same bits
            assert np.array_equal(got_points[key], want_points[key]), key
        else:
            assert np.abs(got_points[key] - want_points[key]).max() <= 4 * (n - 1) * 2.0 ** -53, key


@pytest.mark.parametrize("case", ["main", "small"])
def test_projection_quality_on_the_golden_cases(gold, dev, case):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.analysis import projection_quality
    high, low = gold[f"{case}/high"], gold[f"{case}/low"]
    n = len(high)
    labels = {name: list(gold[f"{case}/labels_{name}"]) for name in ("group", "patient")}
    got, got_points = projection_quality(high, low, neighbors=(5, 15, 40), labels=labels, device=dev)
    again, again_points = projection_quality(torch.from_numpy(high).to(dev), torch.from_numpy(low).to(dev), neighbors=(5, 15, 40),
                                             labels=labels, device=dev)
    assert json.dumps(got, sort_keys=True) == json.dumps(again, sort_keys=True)
    assert all(np.array_equal(got_points[k], again_points[k]) for k in got_points)
    # against the oracle on the device's own distance matrices
    dh = ops.latent_pairwise(torch.from_numpy(high).to(dev)).cpu().numpy()
    dl = ops.projection_distances(torch.from_numpy(low).to(dev)).cpu().numpy()
    want, want_points = O.report_from_distances(dh, dl, high.shape[1], (5, 15, 40), labels)
    _assert_reports_agree(got, want, got_points, want_points, n)
    assert got["neighbors"] == [int(k) for k in gold[f"{case}/neighbors"]]
    for c, k in enumerate(got["neighbors"]):
        assert abs(got_points["trustworthiness_local"][:, c].mean() - got["trustworthiness"][k]) <= 1e-13


@pytest.mark.parametrize("case", ["main", "small"])
def test_deviation_from_sklearn_is_that_of_fp32_distances(gold, dev, case):
    """The device report against scikit-learn's recorded fp64 values: at most twice the deviation of the oracle on numpy fp32
    distances from the same values, per family of figures (the rank figures; the silhouette samples).

    Measured on MI355X: ``main`` rank figures 0 against 0 for numpy fp32 (every integer of the report equals the one from
    fp64 distances), silhouette samples 1.372e-07 against 1.225e-07; ``small`` 0 against 0 and 7.469e-08 against 7.750e-08.
    The rank figures are quantised (one unit of one integer sum is 5.8e-07 at k = 40 here) and the numpy fp32 reference
    deviates by 0, so this asks for exactly the fp64 integers.  With the projection's distances accumulated in fp32
    (``latent_pairwise``, up to 1.7 ulp here) the continuity sum at k = 40 was 257102 against 257103: two entries of row 231
    that differ by 1.2e-8 relative in fp64, a fifth of an fp32 unit in the last place, came out in the other order.  The
    report now takes those distances from ``projection_distances`` (fp64, rounded once), which keeps the true order wherever
    two entries do not round to the same fp32."""
    from pti_ldm_vae_amd.analysis import projection_quality
    high, low = gold[f"{case}/high"], gold[f"{case}/low"]
    labels = {name: list(gold[f"{case}/labels_{name}"]) for name in ("group", "patient")}
    got, got_points = projection_quality(high, low, neighbors=(5, 15, 40), labels=labels, device=dev)
    fp32, fp32_points = O.report(high, low, (5, 15, 40), labels, dtype=np.float32)

    def deviation(report, points):
        ranks = max(abs(report[key][k] - float(gold[f"{case}/{key}"][c])) for key in ("trustworthiness", "continuity")
                    for c, k in enumerate(report["neighbors"]))
        sil = max(np.abs(points[f"silhouette_{space}_{name}"] - gold[f"{case}/silhouette_{space}_{name}"]).max()
                  for space in ("latent", "projection") for name in ("group", "patient"))
        return ranks, sil

    (dev_rank, dev_sil), (ref_rank, ref_sil) = deviation(got, got_points), deviation(fp32, fp32_points)
    print(f"{case}: deviation from scikit-learn's fp64 values: rank figures {dev_rank:.3e} (numpy fp32 {ref_rank:.3e}), "
          f"silhouette samples {dev_sil:.3e} (numpy fp32 {ref_sil:.3e})")
    assert dev_rank <= 2.0 * ref_rank and dev_sil <= 2.0 * ref_sil


def test_projection_quality_edge_inputs(dev):
    from pti_ldm_vae_amd.analysis import projection_quality
    rng = np.random.default_rng(4)
    x = rng.standard_normal((40, 2)).astype(np.float32)
    x[7] = x[3]                                             # duplicate rows: the own index need not come first
    x[8] = x[3]
    report, points = projection_quality(x, x, neighbors=(3, 19, 20), labels={"one": [0] * 40, "each": list(range(40))}, device=dev)
    assert report["neighbors"] == [3, 19] and list(report["excluded"]) == [20]
    for k in (3, 19):
        assert report["trustworthiness"][k] == 1.0 and report["continuity"][k] == 1.0 and report["neighborhood_preservation"][k] == 1.0
        assert report["labels"]["one"]["knn_agreement_latent"][k] == 1.0 and report["labels"]["each"]["knn_agreement_projection"][k] == 0.0
    assert report["labels"]["one"]["silhouette_latent"] is None and report["labels"]["each"]["silhouette_projection"] == 0.0
    assert (points["silhouette_latent_each"] == 0.0).all() and "silhouette_latent_one" not in points
    want, _ = O.report(x, x, (3, 19, 20), {"one": [0] * 40, "each": list(range(40))}, dtype=np.float32)
    assert _flat(report) == _flat(want)
    tiny, _ = projection_quality(x[:4], x[:4], neighbors=(1, 2), device=dev)
    assert tiny["neighbors"] == [1] and tiny["trustworthiness"][1] == 1.0
    with pytest.raises(ValueError, match="non-finite"):
        projection_quality(torch.full((6, 2), float("inf"), device=dev), x[:6], device=dev)


# ---- analyze_static --quality end to end -------------------------------------------------------------------------------------
def _write_group(folder, patients, per_patient, seed):
    from pti_ldm_vae_amd.data import write_tiff
    rng = np.random.default_rng(seed)
    folder.mkdir(parents=True)
    k = 0
    for patient in patients:
        for _ in range(per_patient):
            h, w = 96 + 8 * (k % 3), 120 - 4 * (k % 5)
            img = rng.standard_normal((h, w)).astype(np.float32) * 300 + 900 + 40 * int(patient)
            yy, xx = np.mgrid[0:h, 0:w]
            img[((xx - w / 2) / (0.4 * w)) ** 2 + ((yy - h / 2) / (0.32 * h)) ** 2 > 1.0] = 0.0
            write_tiff(str(folder / f"{k:03d}_HA_2021_02_{patient}.tif"), img)
            k += 1


def test_analyze_static_quality_end_to_end(dev, tmp_path, capsys):
    import matplotlib.image

    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import analyze_static, ops
    _write_group(tmp_path / "edente", ["11", "12", "13", "14", "15", "16"], 4, seed=1)     # 24 + 24 images, six patients
    _write_group(tmp_path / "dente", ["12", "13", "11", "16", "15", "14"], 4, seed=2)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64])
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)
    base = ["--vae-weights", str(ck), "--config-file", str(tmp_path / "cfg.json"), "--folder-edente", str(tmp_path / "edente"),
            "--folder-dente", str(tmp_path / "dente"), "--patch-size", "64", "64", "--cache-dir", str(tmp_path / "cache"),
            "--batch-size", "8", "--dpi", "40"]
    runs = (("pca", ["--method", "pca", "--quality", "--quality-neighbors", "3", "5"], [3, 5], []),
            ("umap", ["--method", "umap", "--umap-backend", "hip", "--quality"], [5, 15], ["40"]))
    for method, extra, ks, excluded in runs:
        out = tmp_path / f"out_{method}"
        analyze_static.main(base + extra + ["--output-dir", str(out)])
        printed = capsys.readouterr().out
        for k in ks:
            assert f"Projection quality k={k}: trustworthiness " in printed
        for name in ("projection_quality.json", "projection_quality.npz", f"{method}_projection_quality.png", "latents.npz"):
            assert (out / name).is_file() and (out / name).stat().st_size > 0, name
        assert matplotlib.image.imread(str(out / f"{method}_projection_quality.png")).ndim == 3
        raw = (out / "projection_quality.json").read_bytes()
        doc = json.loads(raw)
        assert list(doc) == ["method", "n", "high_dims", "neighbors", "excluded", "trustworthiness", "continuity",
                             "neighborhood_preservation", "labels", "args"]
        assert doc["method"] == method and doc["n"] == 48 and doc["high_dims"] == 256 and doc["neighbors"] == ks
        assert list(doc["excluded"]) == excluded and sorted(doc["labels"]) == ["group", "patient"]
        assert doc["args"]["quality"] is True and doc["args"]["method"] == method and doc["args"]["quality_neighbors"] == (ks if method == "pca" else [5, 15, 40])
        # the oracle's report on latents.npz, from the distances the device makes of those rows
        z = np.load(out / "latents.npz")
        high = np.concatenate([z["latents_edente"], z["latents_dente"]])
        low = np.concatenate([z["projection_edente"], z["projection_dente"]]).astype(np.float32)
        ids = list(z["ids_edente"]) + list(z["ids_dente"])
        labels = {"group": ["edente"] * 24 + ["dente"] * 24, "patient": ids}
        dh = ops.latent_pairwise(torch.from_numpy(high).to(dev)).cpu().numpy()
        dl = ops.projection_distances(torch.from_numpy(low).to(dev)).cpu().numpy()
        want, want_points = O.report_from_distances(dh, dl, 256, doc["args"]["quality_neighbors"], labels)
        got = dict(doc, excluded={int(k): v for k, v in doc["excluded"].items()})
        for key in ("trustworthiness", "continuity", "neighborhood_preservation"):
            got[key] = {int(k): v for k, v in doc[key].items()}
        got["labels"] = {name: {key: ({int(k): v for k, v in val.items()} if isinstance(val, dict) else val)
                                for key, val in entry.items()} for name, entry in doc["labels"].items()}
        pts = np.load(out / "projection_quality.npz")
        got_points = {k: pts[k] for k in want_points}
        _assert_reports_agree(got, want, got_points, want_points, 48)
        assert list(pts["ids"]) == ids and list(pts["paths"]) == list(z["paths_edente"]) + list(z["paths_dente"])
        assert np.array_equal(pts["projection"], np.concatenate([z["projection_edente"], z["projection_dente"]]))
        assert list(pts["neighbors"]) == ks and pts["trustworthiness_local"].shape == (48, len(ks))
        # a second run writes the same bytes
        analyze_static.main(base + extra + ["--output-dir", str(out)])
        assert (out / "projection_quality.json").read_bytes() == raw
    # without --quality the file set is what it has always been
    plain = tmp_path / "plain"
    analyze_static.main(base + ["--method", "pca", "--output-dir", str(plain)])
    assert sorted(os.listdir(plain)) == ["distance_metrics.txt", "exams_sorted_by_distance.txt", "latents.npz", "pca_projection.png"]
    for name in ("distance_metrics.txt", "exams_sorted_by_distance.txt"):
        assert (plain / name).read_bytes() == (tmp_path / "out_pca" / name).read_bytes()

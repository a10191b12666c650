"""GPU tests of the surface distances: ``ops.surface_distance`` (csrc/surface_distance.hip) against the scipy oracle of
``tests/surface_distance_oracle.py`` and the tables recorded in ``tests/golden/surface_distance_golden.npz``, the mask output of
``ops.mask_compare``, and ``compare_images --surface`` end to end.

Every integer column is held to equality.  The gate on a side's fp64 sum is ``(n_edge + 4) * 2^-52`` relative to ``math.fsum``
over the oracle's correctly rounded roots: the bound of any summation order of ``n_edge`` non-negative terms plus a 2-ulp root.

Every launch goes through ``_run``: the masks sit inside larger buffers of 0xFF bytes (foreground, were they read), the outputs
and the workspace are followed by canary words that must survive, and all three are filled with NaN bits first."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import mask_compare_oracle as MC
import mask_register_oracle as R
import surface_distance_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_distance_golden.npz")
CANARY_I, NAN_BITS = 0x5A5A5A5A, 0x7FC00000
NCOL = len(O.COLUMNS)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return O.unpack_cases(z), int(z["pm"]), tuple(float(t) for t in z["tolerances"])


def _poisoned(dev, a, lead):
    buf = torch.full((lead + a.size + 64,), 0xFF, dtype=torch.uint8, device=dev)
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _run(dev, a, b=None, percentile=O.GOLDEN_PM / 10, tolerances=O.GOLDEN_TOLERANCES, fill=NAN_BITS):
    """One call -> (int32 ``[n, 2, 11]``, float64 ``[n, 2]``) as numpy; checks the canaries.  ``a`` alone: the packed form (bit 0
    and bit 1 of one uint8 batch); with ``b``: two boolean batches, passed as 0 / 1 bytes.  ``fill``: the 32-bit word the
    workspace and the outputs hold before the call (NaN bits by default: nothing may depend on them)."""
    from pti_ldm_vae_amd import _lib, ops
    a = np.ascontiguousarray(a, dtype=np.uint8)
    n, h, w = a.shape
    d_a = _poisoned(dev, a, 16)
    d_b = None if b is None else _poisoned(dev, np.ascontiguousarray(b, dtype=np.uint8), 8)
    nc, ns = n * 2 * NCOL, n * 4
    flat_c = torch.full((nc + 64,), fill, dtype=torch.int32, device=dev)
    flat_s = torch.full((ns + 64,), fill, dtype=torch.int32, device=dev)
    flat_c[nc:] = CANARY_I
    flat_s[ns:] = CANARY_I
    words = (_lib.lib().pti_surface_distance_ws_bytes(n, h, w) + 3) // 4
    key = ("surface_distance", dev.index, ops._stream(), n, h, w)
    flat_w = ops._SCRATCH.get(("canaried",) + key)
    if flat_w is None:                              # the scratch ops.surface_distance will find: a view with canaries behind it
        flat_w = ops._SCRATCH[("canaried",) + key] = torch.empty(words + 64, dtype=torch.int32, device=dev)
        ops._SCRATCH[key] = flat_w[:words].view(torch.float32)
    flat_w[:words] = fill
    flat_w[words:] = CANARY_I
    counts, sums = ops.surface_distance(d_a, d_b, percentile=percentile, tolerances=tolerances,
                                        out=(flat_c[:nc].view(n, 2, NCOL), flat_s[:ns].view(torch.float64).view(n, 2)))
    torch.cuda.synchronize()
    assert bool((flat_c[nc:] == CANARY_I).all()), "canary behind counts was overwritten"
    assert bool((flat_s[ns:] == CANARY_I).all()), "canary behind sums was overwritten"
    assert bool((flat_w[words:] == CANARY_I).all()), "canary behind the workspace was overwritten"
    return counts.cpu().numpy(), sums.cpu().numpy()


def _packed(pairs):
    return np.stack([a.astype(np.uint8) | (b.astype(np.uint8) << 1) for a, b in pairs])


def _check(got, want, names):
    """Integers equal, sums within the bound; prints each sum's error as a share of its gate."""
    (gc, gs), (wc, ws) = got, want
    worst = 0.0
    for i, name in enumerate(names):
        assert gc[i].tolist() == np.asarray(wc[i]).tolist(), name
        for side in range(2):
            gate = O.sum_bound(int(wc[i][side][1])) * ws[i][side]
            err = abs(gs[i][side] - ws[i][side])
            assert err <= gate, (name, side, gs[i][side], ws[i][side])
            worst = max(worst, err / gate if gate else 0.0)
    print(f"{len(names)} case(s): integers equal, largest sum error as a share of its gate {worst:.3f}")


# ---- golden and generated cases ------------------------------------------------------------------------------------------------
def test_every_golden_case_has_the_oracles_integers(dev, gold):
    cases, pm, tols = gold
    by_shape = {}
    for c in cases:
        by_shape.setdefault(c[1].shape, []).append(c)
    assert set(O.SHAPES) <= set(by_shape)
    for shape, group in by_shape.items():
        got = _run(dev, _packed([(c[1], c[2]) for c in group]), percentile=pm / 10, tolerances=tols)
        _check(got, (np.stack([c[3] for c in group]), np.stack([c[4] for c in group])), [c[0] for c in group])
    kinds = {c[0].split("/")[1] for c in cases if c[0].startswith("67x129/")}
    assert {"corner_vs_checker", "identical", "empty_vs_blob", "both_empty", "full_vs_full", "spiral_vs_comb", "ring_vs_blob"} <= kinds


def test_special_pairs_mean_what_they_should(dev):
    h, w = 67, 129
    named = dict((c[0].split("/")[1], (c[1], c[2])) for c in O.shape_cases(h, w))
    counts, sums = _run(dev, _packed(list(named.values())))
    got = dict(zip(named, zip(counts, sums)))
    c, s = got["identical"]
    assert c[0].tolist() == c[1].tolist() and c[0][2] == c[0][4] == c[0][5] == 0 and c[0][6] == c[0][7] == c[0][1] > 0 and s.tolist() == [0.0, 0.0]
    for name in ("empty_vs_blob", "blob_vs_empty", "both_empty"):
        c, s = got[name]
        a, b = named[name]
        assert c[:, 2:].tolist() == [[-1, 0, -1, -1, 0, 0, 0, 0, 0]] * 2 and s.tolist() == [0.0, 0.0]
        assert c[:, 0].tolist() == [int(a.sum()), int(b.sum())] and c[:, 1].tolist() == [int(O.edges(a).sum()), int(O.edges(b).sum())]
    c, s = got["corner_vs_checker"]                       # every checkerboard pixel looks for the one pixel in the corner
    assert c[0][1] == 1 and c[1][1] == (h * w + 1) // 2 and c[1][2] == (h - 1) ** 2 + (w - 1) ** 2 and c[0][2] in (1, 0)
    c, s = got["full_vs_full"]                            # the outline of a full image is its border
    assert c[0][0] == h * w and c[0][1] == 2 * (h + w) - 4 and c[0][2] == 0


def test_one_pair_at_the_cap(dev):
    h = w = 1024
    a, b = O.sparse_blobs(h, w, 5), O.sparse_blobs(h, w, 6)
    a[0, 0] = a[h - 1, w - 1] = True                      # the largest index and the largest distance the kernel can meet
    b[0, w - 1] = True
    want = O.batch([(a, b)])
    _check(_run(dev, _packed([(a, b)])), want, ["1024x1024"])
    assert want[0][0, :, 2].max() > 1 << 17


# ---- percentiles and tolerances ------------------------------------------------------------------------------------------------
def _small_m_pairs():
    h, w = 7, 80
    one, two, far = (np.zeros((h, w), dtype=bool) for _ in range(3))
    one[3, 0] = True
    two[3, 1] = two[3, 60] = True                         # d2 = 1 and 3600: two different coarse bins of d2 >> 10
    far[0, 79] = far[6, 79] = far[3, 40] = True
    blob = MC.blob_speckle(h, w, 5, speckle=0.05)
    return {"m1_vs_m2_across_bins": (one, two), "m2_vs_m1": (two, one), "m1_vs_blob": (one, blob), "three_vs_two": (far, two),
            "blob_vs_m2": (blob, two)}


@pytest.mark.parametrize("percentile", [0.0, 50.0, 95.0, 99.9, 100.0])
def test_percentile_edges(dev, percentile):
    pm = round(percentile * 10)
    small = _small_m_pairs()
    want = O.batch(list(small.values()), pm)
    _check(_run(dev, _packed(list(small.values())), percentile=percentile), want, list(small))
    lo_hi = want[0][0, 1, 4:6].tolist()                   # side 1 of (one, two): m = 2, distances 1 and 60
    assert lo_hi == {0: [1, 1], 500: [1, 3600], 950: [1, 3600], 999: [1, 3600], 1000: [3600, 3600]}[pm]
    blobs = [(MC.blob_speckle(31, 33, 40 + i, speckle=0.1), MC.blob_speckle(31, 33, 50 + i, speckle=0.2, voids=0.1)) for i in range(4)]
    _check(_run(dev, _packed(blobs), percentile=percentile), O.batch(blobs, pm), [f"blobs_{i}" for i in range(4)])


@pytest.mark.parametrize("tolerances", [(0, 1, 1.5, 2), (1500,), ()])
def test_tolerances(dev, tolerances):
    pairs = [(MC.blob_speckle(67, 129, 60 + i, speckle=0.05), MC.blob_speckle(67, 129, 70 + i, speckle=0.1, voids=0.1)) for i in range(3)]
    want = O.batch(pairs, tolerances=tolerances)
    got = _run(dev, _packed(pairs), tolerances=tolerances)
    _check(got, want, [f"pair_{i}" for i in range(3)])
    if tolerances == (0, 1, 1.5, 2):                      # floor(1.5^2) = 2: d2 <= 2 is more than d2 <= 1 and less than d2 <= 4 here
        w = got[0][:, :, 6:10].sum(axis=(0, 1))
        assert w[0] < w[1] < w[2] < w[3]
    if tolerances == (1500,):
        assert (got[0][:, :, 6] == got[0][:, :, 1]).all() and (got[0][:, :, 7:10] == 0).all()
    if tolerances == ():
        assert (got[0][:, :, 6:10] == 0).all()


# ---- independence, stale memory, reproducibility -------------------------------------------------------------------------------
def test_rows_do_not_depend_on_batch_position_neighbours_stale_memory_or_form(dev):
    h, w = 67, 129
    others = [(MC.blob_speckle(h, w, 900 + i, speckle=0.05), MC.blob_speckle(h, w, 950 + i, speckle=0.1)) for i in range(9)]
    probe = (MC.blob_speckle(h, w, 77, speckle=0.02), MC.spiral(31).repeat(3, axis=0)[:h, :].repeat(5, axis=1)[:, :w])
    alone = _run(dev, _packed([probe]))
    for pos in (0, 4, 9):
        order = others[:pos] + [probe] + others[pos:]
        got = _run(dev, _packed(order))
        assert got[0][pos].tobytes() == alone[0][0].tobytes() and got[1][pos].tobytes() == alone[1][0].tobytes()
        assert got[0][(pos + 1) % 10].tobytes() != alone[0][0].tobytes()
    a, b, c = _run(dev, _packed(others)), _run(dev, _packed(others)), _run(dev, _packed(others), fill=0)
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
    assert np.isfinite(a[1]).all() and (a[0][:, :, 10] == 0).all()
    two = _run(dev, np.stack([p[0] for p in others]), np.stack([p[1] for p in others]))
    assert two[0].tobytes() == a[0].tobytes() and two[1].tobytes() == a[1].tobytes()


# ---- the masks of the comparison launch ----------------------------------------------------------------------------------------
def test_mask_compare_writes_the_two_regions_and_the_same_numbers(dev):
    from pti_ldm_vae_amd import ops
    for h, w, n in ((31, 33, 5), (67, 129, 3)):
        pairs = [MC.images_from_masks(MC.blob_speckle(h, w, 300 + i, speckle=0.1), MC.blob_speckle(h, w, 400 + i, speckle=0.25, voids=0.1), seed=i)
                 for i in range(n)]
        pairs.append((pairs[0][0], np.zeros((h, w), dtype=np.float32)))                  # no prediction at all
        hole_g = MC.ring(h, w, 3, 3, h - 4, w - 4)
        gt_hole, pred_hole = MC.images_from_masks(hole_g, hole_g, seed=9)
        pred_hole[~hole_g] = 0.0                                                         # a filled hole of zero-valued pixels
        pairs.append((gt_hole, pred_hole))
        gt, pred = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        counts, sums, cleaned = ops.mask_compare(d_gt, d_pred, cleaned=True)
        buf = torch.full((gt.size + 64,), 0xA5, dtype=torch.uint8, device=dev)
        c2, s2, m2 = ops.mask_compare(d_gt, d_pred, masks=buf[:gt.size].view(gt.shape))
        c3, s3, cl3, m3 = ops.mask_compare(d_gt, d_pred, cleaned=True, masks=True)
        torch.cuda.synchronize()
        assert bool((buf[gt.size:] == 0xA5).all())
        for c, s in ((c2, s2), (c3, s3)):
            assert counts.cpu().numpy().tobytes() == c.cpu().numpy().tobytes() and sums.cpu().numpy().tobytes() == s.cpu().numpy().tobytes()
        assert cleaned.cpu().numpy().tobytes() == cl3.cpu().numpy().tobytes()
        want_c, _, ps = MC.compare(gt, pred)
        assert counts.cpu().numpy().tolist() == want_c.tolist()
        want = np.stack([MC.masks(g, r)[0].astype(np.uint8) | (p.astype(np.uint8) << 1) for g, r, p in zip(gt, pred, ps)])
        assert m2.dtype == torch.uint8 and m2.cpu().numpy().tobytes() == want.tobytes() == m3.cpu().numpy().tobytes()
        hole = (want[-1] & 2) != 0
        assert ((cleaned[-1].cpu().numpy() != 0) != hole).any() and hole.sum() == (h - 6) * (w - 6)   # cleaned != 0 is not P
        assert (want[-2] & 2).sum() == 0
        for bad in (buf[:gt.size].view(gt.shape)[:, :, :-1], torch.zeros(gt.shape, dtype=torch.int32, device=dev),
                    torch.zeros((len(pairs), h, w + 1), dtype=torch.uint8, device=dev), d_pred.view(torch.uint8).reshape(-1)[:gt.size].view(gt.shape)):
            with pytest.raises((ValueError, TypeError)):
                ops.mask_compare(d_gt, d_pred, masks=bad)
        alias = torch.zeros(gt.size * 4, dtype=torch.uint8, device=dev)
        with pytest.raises(ValueError, match="must not be"):
            ops.mask_compare(d_gt, d_pred, cleaned=alias.view(torch.float32).view(gt.shape), masks=alias[:gt.size].view(gt.shape))
        # the surface distances of those bits are the oracle's on G and P
        got = ops.surface_distance(m2, percentile=95.0, tolerances=(1, 2))
        torch.cuda.synchronize()
        _check((got[0].cpu().numpy(), got[1].cpu().numpy()), O.batch([((m & 1) != 0, (m & 2) != 0) for m in want]), [f"{h}x{w}_{i}" for i in range(len(pairs))])


# ---- layouts and refusals --------------------------------------------------------------------------------------------------------
def test_layouts_out_and_refusals_on_the_device(dev):
    import ctypes as C

    from pti_ldm_vae_amd import _lib, ops
    a, b = MC.blob_speckle(8, 13, 3), MC.blob_speckle(8, 13, 4)
    m = torch.from_numpy(_packed([(a, b)])).to(dev)
    want = O.batch([(a, b)], 950, ())
    counts = torch.zeros(1, 2, NCOL, dtype=torch.int32, device=dev)
    sums = torch.zeros(1, 2, dtype=torch.float64, device=dev)
    got = ops.surface_distance(m, out=(counts, sums))
    assert got[0] is counts and got[1] is sums and counts.cpu().numpy().tolist() == want[0].tolist()
    fresh = ops.surface_distance(torch.from_numpy(a[None]).to(dev), torch.from_numpy(b[None]).to(dev))      # bool tensors, fresh outputs
    assert fresh[0].dtype == torch.int32 and tuple(fresh[0].shape) == (1, 2, NCOL) and fresh[1].dtype == torch.float64
    assert fresh[0].cpu().numpy().tolist() == want[0].tolist()
    for kw in (dict(out=(counts.long(), sums)), dict(out=(counts, sums.float())), dict(out=(counts[:, :1], sums)), dict(out=(counts,)),
               dict(out=(counts.cpu(), sums)), dict(percentile=95.05), dict(percentile=101), dict(tolerances=(1, 2, 3, 4, 5)),
               dict(tolerances=(-1,))):
        with pytest.raises((ValueError, TypeError)):
            ops.surface_distance(m, **kw)
    for bad in (m.float(), m[0], m[:, :, ::2], m.cpu(), m[:0]):
        with pytest.raises((ValueError, TypeError)):
            ops.surface_distance(bad)
    with pytest.raises(ValueError):
        ops.surface_distance(m, m[:, :, :5].contiguous())
    ws = torch.zeros(1 << 16, device=dev)
    for hh, ww in ((1025, 2), (2, 1025)):
        z = torch.zeros(1, hh, ww, dtype=torch.uint8, device=dev)
        with pytest.raises(ValueError, match="unsupported shape"):
            ops.surface_distance(z)
        rc = _lib.lib().pti_surface_distance(ops._ptr(z), 1, ops._ptr(z), 2, 1, hh, ww, 950, (C.c_int32 * 1)(0), 0, ops._ptr(counts),
                                             ops._ptr(sums), ops._ptr(ws), ws.numel() * 4, ops._stream())
        assert rc == -2 and b"unsupported shape" in _lib.lib().pti_last_error_string()
    torch.cuda.synchronize()
    for hh, ww in ((1, 1024), (1024, 1), (1, 1)):                                        # edges 1 and 1024 are served
        z = torch.full((1, hh, ww), 3, dtype=torch.uint8, device=dev)
        c, s = ops.surface_distance(z, tolerances=(0,))
        assert c.cpu().numpy().tolist() == [[[hh * ww, hh * ww, 0, (hh * ww - 1) * 950 // 1000, 0, 0, hh * ww, 0, 0, 0, 0]] * 2]
        assert s.cpu().tolist() == [[0.0, 0.0]]


# ---- the command -----------------------------------------------------------------------------------------------------------------
def _e2e_pairs():
    pairs = {}
    for i in range(5):
        g, r = R.ellipse(40, 36, 0.0, 16, 8, cy=22, cx=18), R.ellipse(40, 36, 0.0, 15 - i % 2, 7 + i % 2, cy=22, cx=18 + i % 3)
        if i == 3:
            r[10:14, 17:20] = False                                                      # a hole the cleaning fills
        if i == 4:
            r[22, 26:33] = True                                                          # a thin spur: Dice barely moves, Hausdorff does
        pairs[f"a{i}.tif"] = R.images(g, r, ("textured", "signed", "flat")[i % 3], 50 + i)
    for i in range(5):
        g, r = R.ellipse(33, 47, 20.0 * (i % 2), 14, 9, cy=18), np.roll(R.ellipse(33, 47, 20.0 * (i % 2), 13, 10, cy=18), i, axis=1)
        pairs[f"b{i}.tif"] = R.images(g, r, ("textured", "signed")[i % 2], 60 + i)
    return pairs


def _read_csv(path):
    with open(path, newline="", encoding="utf-8") as fh:
        return list(csv.reader(fh, delimiter=";"))


def test_compare_images_surface_end_to_end(dev, tmp_path, capsys):
    from pti_ldm_vae_amd import compare_images as cli
    from pti_ldm_vae_amd.data import write_tiff
    from pti_ldm_vae_amd.data.tiff import read_tiff
    from pti_ldm_vae_amd.utils import compare_metrics as M
    pairs = _e2e_pairs()
    gt_dir, pred_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pred_dir.mkdir()
    for name, (gt, pred) in pairs.items():
        write_tiff(str(gt_dir / name), gt)
        write_tiff(str(pred_dir / name), pred)
    common = ["--gt-dir", str(gt_dir), "--pred-dir", str(pred_dir), "--no-plot", "--batch-size", "3"]

    def run(tag, extra):
        out_dir = tmp_path / f"report_{tag}"
        cli.main(common + ["--output-dir", str(out_dir)] + extra)
        return out_dir, json.loads((out_dir / "compare_metrics.json").read_text())

    reg_dir = tmp_path / "registered"
    tols, pm = (1.0, 2.5), 900
    flags = ["--surface", "--surface-tolerances", "1", "2.5", "--surface-percentile", "90"]
    plain_dir, plain = run("plain", [])
    surf_dir, surf = run("surface", flags)
    straight_dir, straight = run("straight", ["--straighten"])
    both_dir, both = run("both", ["--straighten", "--write-registered", str(reg_dir)] + flags)
    _, ssim = run("ssim", ["--ssim"])
    ssim_dir, ssim_surf = run("ssim_surface", ["--ssim"] + flags)
    capsys.readouterr()
    keys = M.surface_keys(tols, pm)
    assert keys == ("Hausdorff Distance", "Hausdorff Distance 90", "Average Surface Distance", "Surface Dice @ 1 px", "Surface Dice @ 2.5 px")

    def regions(report, name):
        """G and P of the pair the run measured, by the oracle."""
        if report is both:
            img = np.asarray(read_tiff(str(reg_dir / name)))
            gt, pred = np.ascontiguousarray(img[:, :img.shape[1] // 2]), np.ascontiguousarray(img[:, img.shape[1] // 2:])
        else:
            gt, pred = pairs[name]
        return MC.masks(gt, pred)[0], MC.compare(gt[None], pred[None])[2][0]

    for report, out_dir, without in ((surf, surf_dir, plain), (both, both_dir, straight), (ssim_surf, ssim_dir, ssim)):
        assert report["arguments"]["surface"] is True and report["arguments"]["surface_tolerances"] == [1.0, 2.5]
        assert report["arguments"]["surface_percentile"] == 90.0
        assert list(report["images"]) == list(without["images"]) and len(report["images"]) >= 10
        for name, img in report["images"].items():
            before = without["images"][name]
            assert tuple(img["metrics"]) == tuple(before["metrics"]) + keys
            g, p = regions(report, name)
            wc, ws = O.batch([(g, p)], pm, tols)
            want = M.surface_metrics(wc, ws, tols, pm)[0]
            got = img["metrics"]
            for k in keys:
                if k == "Average Surface Distance":
                    m = int(wc[0, :, 1].sum())
                    assert abs(got[k] - want[k]) <= O.sum_bound(m) * want[k], (name, k)
                else:
                    assert got[k] == want[k], (name, k, got[k], want[k])
            print(f"{name}: " + ", ".join(f"{k} {got[k]:.4f}" for k in keys))
            assert {k: v for k, v in got.items() if k not in keys} == before["metrics"] and img["counts"] == before["counts"]
            assert img["sums"] == before["sums"]
            blk = img["surface"]
            assert blk["edge_pixels_gt"] == int(O.edges(g).sum()) and blk["edge_pixels_pred"] == int(O.edges(p).sum()) and blk["percentile"] == 90.0
            assert max(blk["max_gt_to_pred"], blk["max_pred_to_gt"]) == got["Hausdorff Distance"]
            assert max(blk["percentile_gt_to_pred"], blk["percentile_pred_to_gt"]) == got["Hausdorff Distance 90"]
            assert blk["mean_gt_to_pred"] > 0 and blk["mean_pred_to_gt"] > 0
        values = [v["metrics"] for v in report["images"].values()]
        agg = M.aggregate(values)
        assert report["aggregates"] == json.loads(json.dumps(agg))
        assert agg["Surface Dice @ 1 px"]["worst"] == min(v["Surface Dice @ 1 px"] for v in values)      # higher is better
        assert agg["Hausdorff Distance"]["worst"] == max(v["Hausdorff Distance"] for v in values)
        rows = _read_csv(out_dir / "_metrics.csv")
        assert [r[0] for r in rows[1 + len(before["metrics"]):1 + len(before["metrics"]) + len(keys)]] == list(keys)
        assert rows[1 + len(before["metrics"])][1] == str(round(float(np.mean([v["Hausdorff Distance"] for v in values])), 3))
    if True:                                              # the spur: a long way for the outline, next to nothing for the overlap
        assert surf["images"]["a4.tif"]["metrics"]["Hausdorff Distance"] >= 5 and surf["images"]["a4.tif"]["metrics"]["Dice Coefficient"] > 0.85
    # the same folder without the flag: no trace of the feature
    for report, out_dir in ((plain, plain_dir), (straight, straight_dir)):
        text = (out_dir / "_metrics.csv").read_text() + json.dumps([report["aggregates"], report["images"], sorted(report["arguments"])])
        assert "urface" not in text and "Hausdorff" not in text
        assert len(_read_csv(out_dir / "_metrics.csv")) == 1 + len(M.METRIC_KEYS) + 12
        for img in report["images"].values():
            assert tuple(img["metrics"]) == M.METRIC_KEYS and "surface" not in img

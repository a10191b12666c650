"""GPU tests of the image-comparison path: ``ops.mask_compare`` (csrc/mask_compare.hip) against the oracle of
``tests/mask_compare_oracle.py`` and the recorded tables of ``tests/golden/mask_compare_golden.npz`` -- every comparison of
the integer table is exact equality, both maxima are exact, the squared-error sum is held to twice the deviation an
fp32-accumulating restatement shows on the same input -- and ``compare_images`` end to end on folders of TIF files.

Every launch goes through ``_run``: the images sit inside larger buffers with foreground-valued poison before and behind
them (a read outside an image changes a result), both outputs and the workspace are followed by 64 canary words that must
survive the launch, and the workspace is filled with random words first (nothing may depend on what it held)."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import mask_compare_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mask_compare_golden.npz")
CANARY_I, CANARY_F, POISON = 0x5A5A5A5A, -12345.678, 7.5


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return O.unpack_cases(z)


def _poisoned(dev, a, lead):
    """The batch inside a larger buffer: ``lead`` poison floats in front, 64 behind; -> contiguous view of the batch."""
    buf = torch.full((lead + a.size + 64,), POISON, dtype=torch.float32, device=dev)
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _run(dev, gt, pred, threshold=O.THRESHOLD, stale=None):
    """One launch -> (counts int32 [n, 24], sums float64 [n, 3]) as numpy; checks all canaries.  ``stale``: seed of the
    random words the workspace holds before the launch (None: leave what the last launch on this shape left)."""
    from pti_ldm_vae_amd import _lib, ops
    gt, pred = np.ascontiguousarray(gt, dtype=np.float32), np.ascontiguousarray(pred, dtype=np.float32)
    n, h, w = gt.shape[0], gt.shape[-2], gt.shape[-1]
    d_gt, d_pred = _poisoned(dev, gt, 17), _poisoned(dev, pred, 5)
    flat_c = torch.full((n * 24 + 64,), CANARY_I, dtype=torch.int32, device=dev)
    flat_s = torch.full((n * 3 + 64,), CANARY_F, dtype=torch.float64, device=dev)
    words = (_lib.lib().pti_mask_compare_ws_bytes(n, h, w) + 3) // 4
    key = ("mask_compare", dev.index, ops._stream(), n, h, w)
    flat_w = ops._SCRATCH.get(("canaried",) + key)
    if flat_w is None:                              # the scratch ops.mask_compare will find: a view with canaries behind it
        flat_w = ops._SCRATCH[("canaried",) + key] = torch.empty(words + 64, dtype=torch.int32, device=dev)
        flat_w[:words] = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int64, device=dev).to(torch.int32)
        ops._SCRATCH[key] = flat_w[:words].view(torch.float32)
    if stale is not None:
        gen = torch.Generator(device=dev).manual_seed(stale)
        flat_w[:words] = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    flat_w[words:] = CANARY_I
    counts, sums = ops.mask_compare(d_gt, d_pred, threshold=float(threshold),
                                    out=(flat_c[:n * 24].view(n, 24), flat_s[:n * 3].view(n, 3)))
    torch.cuda.synchronize()
    assert bool((flat_c[n * 24:] == CANARY_I).all()), "canary behind counts was overwritten"
    assert bool((flat_s[n * 3:] == CANARY_F).all()), "canary behind sums was overwritten"
    assert bool((flat_w[words:] == CANARY_I).all()), "canary behind the workspace was overwritten"
    return counts.cpu().numpy(), sums.cpu().numpy()


def _check(dev, gt, pred, threshold=O.THRESHOLD, stale=0):
    """Run and hold against the scipy oracle -> (counts, sums, worst ratio of the sum's deviation to its gate)."""
    counts, sums = _run(dev, gt, pred, threshold, stale)
    gt3, pred3 = gt.reshape(-1, *gt.shape[-2:]), pred.reshape(-1, *pred.shape[-2:])
    want_c, want_s, ps = O.compare(gt3, pred3, threshold)
    assert counts.tolist() == want_c.tolist()
    assert sums[:, 1].tolist() == want_s[:, 1].tolist() and sums[:, 2].tolist() == want_s[:, 2].tolist()   # maxima: exact
    worst = 0.0
    for i, p in enumerate(ps):
        gate = 2.0 * abs(O.sq_err_sum_fp32(gt3[i], pred3[i], p) - want_s[i, 0])
        dev_ = abs(sums[i, 0] - want_s[i, 0])
        print(f"sq_err_sum image {i} {gt3[i].shape}: fp64 oracle {want_s[i, 0]!r} device {sums[i, 0]!r} deviation {dev_:.3e} gate {gate:.3e}")
        assert dev_ <= gate
        worst = max(worst, dev_ / want_s[i, 0] if want_s[i, 0] else 0.0)
    print(f"largest relative deviation of the fp64 sum: {worst:.3e}")
    return counts, sums


# ---- the golden cases: hand-built masks and every tested shape ----------------------------------------------------------------
def _golden_batches(gold):
    by_shape = {}
    for i, (name, g, r, exp) in enumerate(gold):
        by_shape.setdefault(g.shape, []).append((name, *O.images_from_masks(g, r, seed=100 + i), exp))
    return by_shape


@pytest.fixture(scope="module")
def batches(gold):
    return _golden_batches(gold)


def test_every_golden_case_equals_the_recorded_table(dev, batches):
    shapes = set()
    for shape, cases in batches.items():
        gt, pred = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
        counts, _ = _check(dev, gt, pred)
        for (name, _, _, exp), row in zip(cases, counts.tolist()):
            assert row == exp, name
        shapes.add(shape)
    assert {(1, 1), (1, 7), (7, 1), (5, 5), (31, 33), (64, 64), (67, 129), (256, 256), (1024, 3), (3, 1024)} <= shapes


def test_hand_built_answers(dev, batches):
    """The same numbers tests/test_mask_compare_cpu.py works out by hand, from the device."""
    got = {}
    for shape, cases in batches.items():
        if max(shape) > 31:
            continue
        counts, _ = _run(dev, np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]))
        got.update({c[0]: dict(zip(O.COLUMNS, row)) for c, row in zip(cases, counts.tolist())})
    r = got["checker_5/pred_vs_box"]
    assert (r["n_pred"], r["components_pred"], r["kept_pred"], r["filled_pred"], r["intersection"], r["union"]) == (13, 1, 13, 17, 9, 17)
    r = got["ring_island/pred_vs_box"]
    assert (r["components_pred"], r["kept_pred"], r["filled_pred"]) == (2, 28, 63)
    assert got["ring_diagonal_gap/pred_vs_box"]["filled_pred"] == 48 and got["ring_on_border/pred_vs_box"]["filled_pred"] == 42
    assert got["c_open_to_border/pred_vs_box"]["filled_pred"] == 15
    r = got["two_equal/gt_vs_turned"]
    assert [r[k] for k in ("gt_x", "gt_y", "gt_w", "gt_h")] == [5, 1, 3, 2] and r["kept_gt"] == 6 and r["components_gt"] == 3
    r = got["larger_later/pred_vs_box"]
    assert [r[k] for k in ("pred_x", "pred_y", "pred_w", "pred_h")] == [3, 4, 5, 4] and (r["kept_pred"], r["filled_pred"]) == (14, 20)
    r = got["spiral_31/gt_vs_turned"]
    assert r["components_gt"] == r["components_pred"] == 1 and r["kept_pred"] == r["filled_pred"] == r["n_pred"]
    r = got["u_shape/gt_vs_turned"]
    assert [r[k] for k in ("gt_width_upper", "gt_width_middle", "gt_width_lower")] == [2, 2, 2]
    assert list(got["empty_6x5/gt_vs_turned"].values()) == [0] * 9 + [-1, -1, 0, 0, -1, -1, 0, 0] + [0] * 7
    assert all(r["status"] == 0 for r in got.values())


def test_values_at_the_threshold_and_odd_floats(dev):
    t = O.THRESHOLD
    up, down = np.nextafter(t, np.float32(1)), np.nextafter(-t, np.float32(-1))
    pred = np.zeros((3, 5, 6), dtype=np.float32)
    pred[0, 1:4, 1:5] = t                           # exactly at the threshold: background, R is empty
    pred[0, 2, 2] = -t
    pred[1, 1:4, 1:5] = up                          # one step beyond: foreground
    pred[1, 2, 2] = down
    pred[2] = pred[1]
    gt = np.zeros_like(pred)
    gt[:, 1:4, 1:5] = 1.0
    gt[1, 0, 0] = np.float32(1e-45)                 # the smallest subnormal and -0.0: != 0 holds for the first only
    gt[1, 4, 5] = np.float32(-0.0)
    gt[2, 1:4, 1:5] = -3.0                          # a negative ground truth is foreground too
    counts, _ = _check(dev, gt, pred)
    rows = [dict(zip(O.COLUMNS, r)) for r in counts.tolist()]
    assert rows[0]["n_pred"] == 0 and rows[0]["filled_pred"] == 0 and rows[0]["pred_x"] == -1
    assert rows[1]["n_pred"] == 12 and rows[1]["n_gt"] == 13 and rows[1]["intersection"] == 12
    assert rows[2]["n_gt"] == 12
    # another threshold, and threshold 0 (every non-zero prediction is foreground)
    g, r = O.hand_masks()["ring_island"], O.hand_masks()["two_equal"]
    for thr in (0.0, 0.5, 3.0):
        gt, pred = O.images_from_masks(g, np.pad(r, ((1, 1), (1, 1))), seed=9, threshold=thr)
        _check(dev, gt[None], pred[None], threshold=thr)


def test_layouts_out_and_refusals_on_the_device(dev, batches):
    from pti_ldm_vae_amd import ops
    cases = batches[(5, 5)]
    gt, pred = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    want = _run(dev, gt, pred)[0]
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    counts, sums = ops.mask_compare(d_gt[:, None], d_pred[:, None])                # [n, 1, h, w], fresh outputs, default threshold
    assert counts.dtype == torch.int32 and sums.dtype == torch.float64 and tuple(sums.shape) == (len(cases), 3)
    assert counts.cpu().numpy().tolist() == want.tolist()
    big = torch.zeros(1, 1025, 2, device=dev)
    for a, b in ((big, big), (big.transpose(1, 2).contiguous(), big.transpose(1, 2).contiguous()), (d_gt, d_pred[:, :4]),
                 (d_gt[0], d_pred[0]), (d_gt[:, :, ::2], d_pred[:, :, ::2]), (d_gt[:0], d_pred[:0])):
        with pytest.raises(ValueError):
            ops.mask_compare(a, b)
    for kw in (dict(threshold=-0.1), dict(threshold=float("nan")), dict(out=(counts,)), dict(out=(counts[:1], sums)),
               dict(out=(counts, sums.float()))):
        with pytest.raises((ValueError, TypeError)):
            ops.mask_compare(d_gt, d_pred, **kw)
    edge = torch.zeros(1, 1024, 2, device=dev)                                     # the cap itself is served
    assert ops.mask_compare(edge, edge)[0][0, :9].cpu().tolist() == [0] * 9


# ---- independence, stale workspace, reproducibility -----------------------------------------------------------------------------
def test_rows_do_not_depend_on_batch_position_or_neighbours(dev):
    h, w = 31, 33
    pairs = [O.images_from_masks(O.blob_speckle(h, w, 300 + i, speckle=0.1), O.blob_speckle(h, w, 400 + i, speckle=0.25), seed=i)
             for i in range(9)]
    probe = O.images_from_masks(np.pad(O.spiral(31), ((0, 0), (1, 1))), O.blob_speckle(h, w, 77, speckle=0.3, voids=0.2), seed=50)
    alone = _check(dev, probe[0][None], probe[1][None])
    for pos in (0, 4, 9):
        order = pairs[:pos] + [probe] + pairs[pos:]
        counts, sums = _check(dev, np.stack([p[0] for p in order]), np.stack([p[1] for p in order]), stale=pos)
        assert counts[pos].tolist() == alone[0][0].tolist()
        assert sums[pos].tobytes() == alone[1][0].tobytes()
    twice = _run(dev, np.stack([probe[0]] * 5), np.stack([probe[1]] * 5))
    for i in range(5):
        assert twice[0][i].tolist() == alone[0][0].tolist() and twice[1][i].tobytes() == alone[1][0].tobytes()


def test_a_dense_call_leaves_nothing_behind_for_a_sparse_one(dev):
    h, w = 64, 64
    dense = O.images_from_masks(np.ones((h, w), dtype=bool), np.random.RandomState(1).rand(h, w) < 0.7, seed=1)
    sparse_g, sparse_r = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    sparse_g[10:12, 50:53] = sparse_r[40, 3] = sparse_r[41, 4] = True
    sparse_r[5:9, 5:9] = True
    sparse_r[6:8, 6:8] = False
    sparse = O.images_from_masks(sparse_g, sparse_r, seed=2)
    _check(dev, np.stack([dense[0]] * 3), np.stack([dense[1]] * 3), stale=3)
    counts, _ = _check(dev, np.stack([sparse[0]] * 3), np.stack([sparse[1]] * 3), stale=None)   # the dense call's leftovers
    row = dict(zip(O.COLUMNS, counts[1].tolist()))
    assert (row["components_pred"], row["kept_pred"], row["filled_pred"]) == (2, 12, 16)


def test_two_calls_are_bitwise_equal(dev, batches):
    cases = batches[(67, 129)] + batches[(67, 129)]
    gt, pred = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    a, b = _run(dev, gt, pred, stale=11), _run(dev, gt, pred, stale=12)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[1][0].tobytes() == a[1][len(cases) // 2].tobytes()


# ---- the command ------------------------------------------------------------------------------------------------------------------
def _exact_images(g, r, seed):
    """Images on a grid of eighths: every squared difference and every partial sum is exact in fp64, so the device's sum
    equals the oracle's bit for bit whatever the order, and the report can be compared with ``==``."""
    rs = np.random.RandomState(seed)
    gt = np.where(g, rs.choice([0.5, 0.75, 1.0, -0.5], g.shape), 0.0).astype(np.float32)
    pred = np.where(r, rs.choice([0.25, 0.5, 0.875, -0.375], r.shape), rs.choice([0.0, 0.125, -0.125], r.shape)).astype(np.float32)
    assert np.array_equal(O.masks(gt, pred)[0], g) and np.array_equal(O.masks(gt, pred)[1], r)
    return gt, pred


def _expected_report(named_pairs):
    """name -> (gt, pred) in report order -> (images, skipped, aggregates, thresholds) from the oracle and compare_metrics."""
    from pti_ldm_vae_amd.utils import compare_metrics as M
    images, skipped = {}, []
    for name, (gt, pred) in named_pairs.items():
        if isinstance(gt, str):
            skipped.append({"image": name, "reason": gt})
            continue
        counts, sums, _ = O.compare(gt[None], pred[None])
        (m,) = M.pair_metrics(counts, sums, *gt.shape)
        if isinstance(m, str):
            skipped.append({"image": name, "reason": m})
        else:
            images[name] = {"metrics": m, "dimensions": M.dimensions(counts[0]), "counts": dict(zip(O.COLUMNS, counts[0].tolist())),
                            "sums": dict(zip(("sq_err_sum", "max_gt", "max_pred"), sums[0].tolist()))}
    ms = [v["metrics"] for v in images.values()]
    return images, skipped, M.aggregate(ms), [{"name": n, "count": c, "percentage": p} for n, c, p in M.threshold_counts(ms)]


def _read_csv(path):
    with open(path, newline="", encoding="utf-8") as fh:
        return list(csv.reader(fh, delimiter=";"))


def _check_outputs(out_dir, named_pairs, plot):
    from pti_ldm_vae_amd.utils import compare_metrics as M
    images, skipped, aggregates, thresholds = _expected_report(named_pairs)
    report = json.loads((out_dir / "compare_metrics.json").read_text())
    want = json.loads(json.dumps({"images": images, "skipped": skipped, "aggregates": aggregates, "thresholds": thresholds}))
    for key, value in want.items():
        assert report[key] == value, key
    assert report["images_processed"] == len(images) and list(report["images"]) == list(images)
    dims = _read_csv(out_dir / "_dimensions.csv")
    assert dims[0] == list(M.DIMENSION_COLUMNS)
    assert dims[1:] == [[name] + [str(v) for v in img["dimensions"].values()] for name, img in images.items()]
    rows = M.metrics_csv_rows(aggregates, [(t["name"], t["count"], t["percentage"]) for t in thresholds], len(images))
    got = _read_csv(out_dir / "_metrics.csv")
    assert got[0] == list(M.METRICS_CSV_COLUMNS) and len(got) == 1 + len(M.METRIC_KEYS) + 12
    assert got[1:] == [[str(r.get(c, "")) for c in M.METRICS_CSV_COLUMNS] for r in rows]
    assert (out_dir / "_metrics_distribution.png").exists() == plot
    return report


def test_compare_images_end_to_end(dev, tmp_path, capsys):
    from pti_ldm_vae_amd import compare_images as cli
    from pti_ldm_vae_amd.data import write_tiff
    pairs = {}
    for i, (h, w) in enumerate([(40, 36), (40, 36), (40, 36), (33, 47), (40, 36)]):
        pairs[f"img{i:02d}.tif"] = _exact_images(O.blob_speckle(h, w, 500 + i, speckle=0.01), O.blob_speckle(h, w, 600 + i, speckle=0.05), i)
    blank = np.zeros((40, 36), dtype=bool)
    pairs["img05_no_pred.tif"] = _exact_images(O.blob_speckle(40, 36, 9, speckle=0.0), blank, 7)
    pairs["img06_no_gt.tif"] = _exact_images(blank, O.blob_speckle(40, 36, 10), 8)
    # ---- a folder pair ----
    gt_dir, pred_dir, out_dir = tmp_path / "edente", tmp_path / "edente_synth", tmp_path / "report"
    gt_dir.mkdir()
    pred_dir.mkdir()
    for name, (gt, pred) in pairs.items():
        write_tiff(str(gt_dir / name), gt)
        write_tiff(str(pred_dir / name), pred)
    write_tiff(str(gt_dir / "img07_sizes.tif"), np.zeros((8, 8), dtype=np.float32))
    write_tiff(str(pred_dir / "img07_sizes.tif"), np.zeros((8, 9), dtype=np.float32))
    write_tiff(str(gt_dir / "only_gt.tif"), np.zeros((8, 8), dtype=np.float32))
    (pred_dir / "notes.txt").write_text("not an image")
    cli.main(["--gt-dir", str(gt_dir), "--pred-dir", str(pred_dir), "--output-dir", str(out_dir), "--batch-size", "2"])
    printed = capsys.readouterr().out
    assert "Unpaired: only_gt.tif is in the ground truth folder only" in printed and "5 pair(s) compared, 3 skipped" in printed
    named = dict(pairs)
    named["img07_sizes.tif"] = ("Images do not have the same dimensions: (8, 8) and (8, 9)", None)
    report = _check_outputs(out_dir, named, plot=True)
    assert [s["image"] for s in report["skipped"]] == ["img05_no_pred.tif", "img06_no_gt.tif", "img07_sizes.tif"]
    assert report["unpaired"] == {"gt_only": ["only_gt.tif"], "pred_only": []}
    assert report["arguments"]["threshold"] == 0.2 and report["arguments"]["batch_size"] == 2
    assert report["aggregates"]["Dice Coefficient"]["n"] == 5
    # ---- side-by-side files, as inference_vae writes them; default output folder; no plot ----
    res_dir = tmp_path / "results_tif"
    res_dir.mkdir()
    for name, (gt, pred) in pairs.items():
        write_tiff(str(res_dir / name), np.concatenate([gt, pred], axis=1))
    cli.main(["--results-dir", str(res_dir), "--no-plot"])
    capsys.readouterr()
    again = _check_outputs(res_dir / "compare", pairs, plot=False)
    assert again["images"] == report["images"]
    write_tiff(str(res_dir / "odd.tif"), np.zeros((4, 7), dtype=np.float32))
    with pytest.raises(cli.OddWidth):
        cli.main(["--results-dir", str(res_dir), "--no-plot"])

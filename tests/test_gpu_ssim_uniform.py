"""GPU tests of the uniform-window SSIM: ``ops.ssim_uniform`` (csrc/ssim_uniform.hip) against the fp64 oracle of
``tests/ssim_uniform_oracle.py`` and the values recorded in ``tests/golden/ssim_uniform_golden.npz``, the cleaned-prediction
output of ``ops.mask_compare``, and ``compare_images --ssim`` end to end.

The gate on ``|kernel - fp64 oracle|`` of an image is ``8 * max(D_ref(image), D_ref at offset 0, 2^-24)``: ``D_ref`` is the
distance of the oracle file's fp32 restatement from its fp64 oracle on the same image, worked out on the CPU here and never
taken from the kernel; the second term is the ``D_ref`` of an offset golden case's twin without the offset; the third is fp32's
unit roundoff (``ssim_uniform_oracle.gates`` says why).  The data range is held to equality.

Every launch goes through ``_run``: the images sit inside larger buffers with poison before and behind them, the output and the
workspace are followed by canary words that must survive, and both are filled with NaN bits first."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import mask_compare_oracle as MC
import mask_register_oracle as R
import ssim_uniform_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ssim_uniform_golden.npz")
CANARY_I, CANARY_F, POISON, NAN_BITS = 0x5A5A5A5A, -12345.678, 7.5e3, 0x7FC00000


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return O.unpack_cases(z)


def _gate(x, y, data_range=None):
    return O.gate_of(abs(O.ssim_fp32(x, y, data_range)[0] - O.ssim_valid(x, y, data_range)[0]))


def _poisoned(dev, a, lead):
    buf = torch.full((lead + a.size + 64,), POISON, dtype=torch.float32, device=dev)
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _run(dev, x, y, data_range=None, fill=NAN_BITS):
    """One call -> float64 ``[n, 2]`` as numpy; checks the canaries.  ``fill``: the 32-bit word the workspace and the output hold
    before the call (NaN bits by default: nothing may depend on them)."""
    from pti_ldm_vae_amd import _lib, ops
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    n, h, w = x.shape
    d_x, d_y = _poisoned(dev, x, 16), _poisoned(dev, y, 6)
    flat_o = torch.full((n * 4 + 64,), fill, dtype=torch.int32, device=dev)
    flat_o[n * 4:] = CANARY_I
    words = (_lib.lib().pti_ssim_uniform_ws_bytes(n, h, w) + 3) // 4
    key = ("ssim_uniform", dev.index, ops._stream(), n, h, w)
    flat_w = ops._SCRATCH.get(("canaried",) + key)
    if flat_w is None:                              # the scratch ops.ssim_uniform will find: a view with canaries behind it
        flat_w = ops._SCRATCH[("canaried",) + key] = torch.empty(words + 64, dtype=torch.int32, device=dev)
        ops._SCRATCH[key] = flat_w[:words].view(torch.float32)
    flat_w[:words] = fill
    flat_w[words:] = CANARY_I
    out = ops.ssim_uniform(d_x, d_y, data_range=data_range, out=flat_o[:n * 4].view(torch.float64).view(n, 2))
    torch.cuda.synchronize()
    assert bool((flat_o[n * 4:] == CANARY_I).all()), "canary behind out was overwritten"
    assert bool((flat_w[words:] == CANARY_I).all()), "canary behind the workspace was overwritten"
    return out.cpu().numpy()


def _pairs(cases):
    pairs = [O.case_pair(c) for c in cases]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ---- the golden cases --------------------------------------------------------------------------------------------------------------
def test_every_golden_case_is_within_its_gate(dev, gold):
    cases, expected = gold
    gates, d = O.gates(cases), O.d_ref(cases)
    by_shape = {}
    for c, e in zip(cases, expected):
        by_shape.setdefault((c["h"], c["w"]), []).append((c, e))
    assert set(by_shape) == set(O.SHAPES)
    worst = 0.0
    for shape, group in by_shape.items():
        x, y = _pairs([c for c, _ in group])
        got = _run(dev, x, y)
        for (c, e), row in zip(group, got):
            err = abs(row[0] - e[0])
            print(f"{c['name']:22s} oracle {e[0]:.12f} device {row[0]:.12f} error {err:.3e} D_ref {d[c['name']]:.3e} gate {gates[c['name']]:.3e}")
            assert row[1] == e[1], c["name"]                                      # the data range: exact
            assert err <= gates[c["name"]], c["name"]
            if c["variant"] == "flat_gt":
                assert row.tolist() == [0.0, 0.0]
            worst = max(worst, err / gates[c["name"]])
    print(f"largest error as a share of its gate: {worst:.3f}")


def test_an_explicit_data_range_is_used_as_given(dev, gold):
    cases = [c for c in gold[0] if (c["h"], c["w"]) == (45, 71) and c["variant"] == "noisy"]
    x, y = _pairs(cases)
    for rng in (2.5, 0.3):
        got = _run(dev, x, y, data_range=rng)
        for i, c in enumerate(cases):
            want = O.ssim_valid(x[i], y[i], data_range=rng)
            gate = _gate(x[i], y[i], rng)
            print(f"{c['name']:22s} range {rng}: error {abs(got[i, 0] - want[0]):.3e} gate {gate:.3e}")
            assert got[i, 1] == rng and abs(got[i, 0] - want[0]) <= gate
    assert _run(dev, x, y, data_range=0.0).tolist() == [[0.0, 0.0]] * len(cases)      # a zero range: {0, 0}, no launch is skipped


def test_a_flat_ground_truth_reports_zero_and_zero(dev, gold):
    c = next(c for c in gold[0] if c["name"] == "64x64_flat_gt")
    probe = next(c for c in gold[0] if c["name"] == "64x64")
    x, y = _pairs([probe, c, probe])
    got = _run(dev, x, y)
    assert got[1].tolist() == [0.0, 0.0] and got[0, 1] > 0 and got[0].tobytes() == got[2].tobytes()


# ---- independence, stale memory, reproducibility -----------------------------------------------------------------------------------
def test_rows_do_not_depend_on_batch_position_neighbours_or_stale_memory(dev):
    h, w = 45, 71
    others = [O.make_pair(h, w, 900 + i, noise=0.1, offset=float(i))[:2] for i in range(9)]
    probe = O.make_pair(h, w, 77, noise=0.05)[:2]
    alone = _run(dev, probe[0][None], probe[1][None])
    for pos in (0, 4, 9):
        order = others[:pos] + [probe] + others[pos:]
        got = _run(dev, np.stack([p[0] for p in order]), np.stack([p[1] for p in order]))
        assert got[pos].tobytes() == alone[0].tobytes()
        assert got[(pos + 1) % 10, 1] != alone[0, 1]                                     # the neighbours have ranges of their own
    # two calls, and a third over a zeroed workspace and output: the same bits
    x, y = np.stack([p[0] for p in others]), np.stack([p[1] for p in others])
    a, b, c = _run(dev, x, y), _run(dev, x, y), _run(dev, x, y, fill=0)
    assert a.tobytes() == b.tobytes() == c.tobytes() and np.isfinite(a).all()
    given = [_run(dev, x, y, data_range=1.25, fill=f) for f in (NAN_BITS, 0)]
    assert given[0].tobytes() == given[1].tobytes() and np.isfinite(given[0]).all()


def test_layouts_out_and_refusals_on_the_device(dev):
    from pti_ldm_vae_amd import _lib, ops
    x, y = (torch.from_numpy(a[None]).to(dev) for a in O.make_pair(8, 13, 3)[:2])
    want = O.ssim_valid(x[0].cpu().numpy(), y[0].cpu().numpy())
    got = ops.ssim_uniform(x[:, None], y[:, None])                                       # [n, 1, h, w], a fresh output
    assert got.dtype == torch.float64 and tuple(got.shape) == (1, 2) and abs(float(got[0, 0]) - want[0]) < 1e-5 and float(got[0, 1]) == want[1]
    for hh, ww in ((6, 13), (13, 6), (1025, 8), (8, 1025)):                              # an edge of 6 and of 1025, either way
        z = torch.zeros(1, hh, ww, device=dev)
        with pytest.raises(ValueError, match="unsupported shape"):
            ops.ssim_uniform(z, z)
        ws = torch.zeros(1 << 16, device=dev)
        rc = _lib.lib().pti_ssim_uniform(ops._ptr(z), ops._ptr(z), 1, hh, ww, -1.0, ops._ptr(got), ops._ptr(ws), ws.numel() * 4, ops._stream())
        assert rc == -2 and b"unsupported shape" in _lib.lib().pti_last_error_string()
    for a, b in ((x, y[:, :7]), (x[0], y[0]), (x[:, :, ::2], y[:, :, ::2]), (x[:0], y[:0])):
        with pytest.raises(ValueError):
            ops.ssim_uniform(a, b)
    for kw in (dict(out=got.float()), dict(out=got[:, :1]), dict(out=torch.zeros(2, 2, dtype=torch.float64, device=dev)), dict(data_range=-2.0)):
        with pytest.raises((ValueError, TypeError)):
            ops.ssim_uniform(x, y, **kw)
    torch.cuda.synchronize()
    edge = torch.zeros(1, 1024, 7, device=dev)                                           # both caps are served
    assert ops.ssim_uniform(edge, edge).cpu().tolist() == [[0.0, 0.0]]


# ---- the cleaned prediction of the comparison launch -------------------------------------------------------------------------------
def test_mask_compare_writes_the_cleaned_prediction_and_the_same_numbers(dev):
    from pti_ldm_vae_amd import ops
    for h, w, n in ((31, 33, 5), (67, 129, 3)):
        pairs = [MC.images_from_masks(MC.blob_speckle(h, w, 300 + i, speckle=0.1), MC.blob_speckle(h, w, 400 + i, speckle=0.25, voids=0.1), seed=i)
                 for i in range(n)]
        pairs.append((pairs[0][0], np.zeros((h, w), dtype=np.float32)))                  # no prediction at all: all background
        gt, pred = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        counts, sums = ops.mask_compare(d_gt, d_pred)
        buf = torch.full((gt.size + 64,), POISON, dtype=torch.float32, device=dev)
        c2, s2, cleaned = ops.mask_compare(d_gt, d_pred, cleaned=buf[:gt.size].view(gt.shape))
        torch.cuda.synchronize()
        assert bool((buf[gt.size:] == POISON).all())
        assert counts.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes() and sums.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
        want_c, _, ps = MC.compare(gt, pred)
        assert counts.cpu().numpy().tolist() == want_c.tolist()
        want = np.stack([np.where(p, r, np.float32(0)) for p, r in zip(ps, pred)]).astype(np.float32)
        assert (want != pred).any() and cleaned.cpu().numpy().tobytes() == want.tobytes()
        fresh = ops.mask_compare(d_gt, d_pred, cleaned=True)[2]
        assert fresh.cpu().numpy().tobytes() == want.tobytes()
        for bad in (d_pred, d_gt, buf[:gt.size].view(gt.shape)[:, :, :-1], torch.zeros(gt.shape, dtype=torch.float64, device=dev)):
            with pytest.raises((ValueError, TypeError)):
                ops.mask_compare(d_gt, d_pred, cleaned=bad)


# ---- the command -------------------------------------------------------------------------------------------------------------------
def _e2e_pairs():
    pairs = {}
    for i in range(5):
        g, r = R.ellipse(40, 36, 0.0, 16, 8, cy=22, cx=18), R.ellipse(40, 36, 0.0, 15 - i % 2, 7 + i % 2, cy=22, cx=18)
        pairs[f"a{i}.tif"] = R.images(g, r, ("textured", "signed", "flat")[i % 3], 50 + i)
    for i in range(4):
        g, r = R.ellipse(33, 47, 20.0 * (i % 2), 14, 9, cy=18), np.roll(R.ellipse(33, 47, 20.0 * (i % 2), 13, 10, cy=18), i, axis=1)
        pairs[f"b{i}.tif"] = R.images(g, r, ("textured", "signed")[i % 2], 60 + i)
    flat = R.images(np.ones((40, 36), dtype=bool), R.ellipse(40, 36, 0.0, 15, 7, cy=22, cx=18), "flat", 70)
    pairs["c_flat_gt.tif"] = flat                                                        # a constant ground truth: range 0
    low = np.zeros((6, 20), dtype=bool)
    low[0:6, 9:12] = True
    pairs["d_low.tif"] = R.images(low, low, "textured", 71)                              # 6 rows: no 7 x 7 window fits (an upright bar)
    return pairs


def _read_csv(path):
    with open(path, newline="", encoding="utf-8") as fh:
        return list(csv.reader(fh, delimiter=";"))


def test_compare_images_ssim_end_to_end(dev, tmp_path, capsys):
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
    plain_dir, plain = run("plain", [])
    ssim_dir, with_ssim = run("ssim", ["--ssim"])
    _, straight = run("straight", ["--straighten"])
    both_dir, both = run("both", ["--straighten", "--ssim", "--write-registered", str(reg_dir)])
    capsys.readouterr()

    def measured(report, name):
        """The pair the run measured, the prediction cleaned by the oracle's P."""
        if report is both:
            img = np.asarray(read_tiff(str(reg_dir / name)))
            gt, pred = np.ascontiguousarray(img[:, :img.shape[1] // 2]), np.ascontiguousarray(img[:, img.shape[1] // 2:])
        else:
            gt, pred = pairs[name]
        p = MC.compare(gt[None], pred[None])[2][0]
        return gt, np.where(p, pred, np.float32(0)).astype(np.float32)

    for report, out_dir, without in ((with_ssim, ssim_dir, plain), (both, both_dir, straight)):
        assert report["arguments"]["ssim"] is True and list(report["images"]) == list(without["images"]) and len(report["images"]) >= 10
        for name, img in report["images"].items():
            assert list(img["metrics"])[:3] == ["MSE", "SSIM", "PSNR"]
            gt, cleaned = measured(report, name)
            got = img["metrics"]["SSIM"]
            if name in ("c_flat_gt.tif", "d_low.tif"):                                   # no SSIM, every other metric stays
                assert got is None and img["sums"]["ssim_data_range"] == (0.0 if name == "c_flat_gt.tif" else None)
            else:
                want, gate = O.ssim_valid(gt, cleaned), _gate(gt, cleaned)
                print(f"{name} ({'registered' if report is both else 'as read'}): oracle {want[0]:.9f} report {got:.9f} error {abs(got - want[0]):.3e} gate {gate:.3e}")
                assert abs(got - want[0]) <= gate and img["sums"]["ssim_data_range"] == want[1]
                if report is with_ssim:                                                  # the raw prediction would not pass: the pair is (gt, cleaned)
                    assert abs(O.ssim_valid(gt, pairs[name][1])[0] - want[0]) > gate
            rest = {k: v for k, v in img["metrics"].items() if k != "SSIM"}
            assert rest == without["images"][name]["metrics"] and img["counts"] == without["images"][name]["counts"]
        values = [v["metrics"] for v in report["images"].values()]
        agg = M.aggregate(values)
        assert report["aggregates"] == json.loads(json.dumps(agg)) and agg["SSIM"]["none"] == 2 and agg["SSIM"]["n"] == len(values) - 2
        rows = M.metrics_csv_rows(agg, [(t["name"], t["count"], t["percentage"]) for t in report["thresholds"]], len(values))
        got_rows = _read_csv(out_dir / "_metrics.csv")
        assert got_rows[2][0] == "SSIM" and got_rows[2] == [str(rows[1].get(c, "")) for c in M.METRICS_CSV_COLUMNS]
        assert got_rows[2][1] == str(round(float(np.mean([v["SSIM"] for v in values if v["SSIM"] is not None])), 3))
        assert len(got_rows) == 1 + len(M.METRIC_KEYS) + 1 + 12
    # the same folder without the flag: no key anywhere, and the files of a run before the flag existed
    assert all(r[0] != "SSIM" for r in _read_csv(plain_dir / "_metrics.csv")) and len(_read_csv(plain_dir / "_metrics.csv")) == 1 + len(M.METRIC_KEYS) + 12
    for report in (plain, straight):
        assert "ssim" not in report["arguments"] and "SSIM" not in report["aggregates"]
        for img in report["images"].values():
            assert tuple(img["metrics"]) == M.METRIC_KEYS and tuple(img["sums"]) == ("sq_err_sum", "max_gt", "max_pred")

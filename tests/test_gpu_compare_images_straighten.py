"""``compare_images --straighten`` end to end on a temporary folder of small TIFs: upright pairs measure as they did, a
prediction moved sideways is forgiven, a tilted pair's report and written files are what ``ops.register_pairs`` returns, and
pairs that cannot be registered are skipped with the reason."""
import json

import numpy as np
import pytest
import torch

import mask_register_oracle as R

pytestmark = pytest.mark.gpu

H, W = 40, 36


def _pairs():
    """name -> (gt, pred) fp32 images; values on both sides are textured, the prediction's background is inside the threshold."""
    up_g, up_r = R.ellipse(H, W, 0.0, 16, 8, cy=22, cx=18), R.ellipse(H, W, 0.0, 15, 7, cy=22, cx=18)
    pairs = {}
    for i in range(2):                               # upright and centred: symmetric about column 18
        pairs[f"a_upright{i}.tif"] = R.images(up_g, up_r, "textured", 70 + i)
    for i in range(2):                               # the same pairs, the prediction moved 3 columns to the left
        gt, pred = pairs[f"a_upright{i}.tif"]
        pairs[f"b_moved{i}.tif"] = (gt, np.roll(pred, -3, axis=1))
    pairs["c_tilted.tif"] = R.images(R.ellipse(H, W, 25.0, 15, 6, cy=21), np.roll(R.ellipse(H, W, 21.0, 14, 7, cy=21), 2, axis=1), "signed", 80)
    top = R.ellipse(H, W, 0.0, 10, 6, cy=14, cx=18)  # nothing below row 24: the bottom fifth (rows 32 ..) is empty
    pairs["d_top_only.tif"] = R.images(top, top, "flat", 81)
    low = np.zeros((4, 8), dtype=bool)
    low[1:3, 2:6] = True
    pairs["e_low.tif"] = R.images(low, low, "flat", 82)
    return pairs


def _run(cli, tmp_path, pairs, tag, extra):
    from pti_ldm_vae_amd.data import write_tiff
    gt_dir, pred_dir, out_dir = tmp_path / "gt", tmp_path / "pred", tmp_path / f"report_{tag}"
    if not gt_dir.exists():
        gt_dir.mkdir()
        pred_dir.mkdir()
        for name, (gt, pred) in pairs.items():
            write_tiff(str(gt_dir / name), gt)
            write_tiff(str(pred_dir / name), pred)
    cli.main(["--gt-dir", str(gt_dir), "--pred-dir", str(pred_dir), "--output-dir", str(out_dir), "--no-plot", "--batch-size", "3"] + extra)
    return json.loads((out_dir / "compare_metrics.json").read_text())


def test_compare_images_straighten_end_to_end(dev, tmp_path, capsys):
    from pti_ldm_vae_amd import compare_images as cli
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.data.tiff import read_tiff
    pairs = _pairs()
    plain = _run(cli, tmp_path, pairs, "plain", [])
    reg_dir = tmp_path / "registered"
    report = _run(cli, tmp_path, pairs, "straight", ["--straighten", "--write-registered", str(reg_dir)])
    capsys.readouterr()
    assert plain["arguments"]["straighten"] is False and report["arguments"]["straighten"] is True
    assert report["arguments"]["write_registered"] == str(reg_dir.resolve())
    assert all("registration" not in v for v in plain["images"].values())
    assert list(report["images"]) == ["a_upright0.tif", "a_upright1.tif", "b_moved0.tif", "b_moved1.tif", "c_tilted.tif"]
    # upright, centred: nothing is turned or moved, and the figures are those of the run without the flag
    for i in range(2):
        got, was = report["images"][f"a_upright{i}.tif"], plain["images"][f"a_upright{i}.tif"]
        assert got["metrics"] == was["metrics"] and got["dimensions"] == was["dimensions"]
        reg = got["registration"]
        assert reg["angle_gt_deg"] == reg["angle_pred_deg"] == 0.0 and reg["shift"] == 0 and reg["centre_gt"] == reg["centre_pred"] == 18
    # moved sideways: found, undone, and forgiven in Dice and IoU -- without the flag it is charged
    for i in range(2):
        got, ref = report["images"][f"b_moved{i}.tif"], report["images"][f"a_upright{i}.tif"]
        assert got["registration"]["shift"] == 3 and got["registration"]["centre_pred"] == 15
        assert got["metrics"]["Dice Coefficient"] == ref["metrics"]["Dice Coefficient"] and got["metrics"]["IoU"] == ref["metrics"]["IoU"]
        assert plain["images"][f"b_moved{i}.tif"]["metrics"]["Dice Coefficient"] < ref["metrics"]["Dice Coefficient"]
    # the tilted pair: the report's block and the written files are ops.register_pairs' own answers
    gt, pred = pairs["c_tilted.tif"]
    rot_gt, aligned, info = ops.register_pairs(torch.from_numpy(gt[None]).to(dev), torch.from_numpy(pred[None]).to(dev), threshold=0.2)
    host = {k: v.cpu().numpy()[0] for k, v in info.items()}
    block = report["images"]["c_tilted.tif"]["registration"]
    assert block == json.loads(json.dumps(cli.registration_block(host["moments"], host["coeffs"], host["align"])))
    assert 15.0 < block["angle_gt_deg"] < 35.0 and set(block) == {"angle_gt_deg", "angle_pred_deg", "moments_gt", "moments_pred",
                                                                  "centre_gt", "centre_pred", "shift"}
    assert block["moments_gt"]["m00"] == int(R.moments_stage(gt, pred)[1][0][0])
    both = np.asarray(read_tiff(str(reg_dir / "c_tilted.tif")))
    assert both.shape == (H, 2 * W) and both.dtype == np.float32
    assert both[:, :W].tobytes() == rot_gt.cpu().numpy()[0].tobytes() and both[:, W:].tobytes() == aligned.cpu().numpy()[0].tobytes()
    assert sorted(p.name for p in reg_dir.iterdir()) == list(report["images"])       # skipped pairs are not written
    # the written folder is a --results-dir: measuring it as it is gives the figures of the registered pair
    again_args = cli.parse_args(["--results-dir", str(reg_dir), "--no-plot"])
    again = cli.run(again_args, dev)
    assert again["images"]["c_tilted.tif"]["counts"]["intersection"] == report["images"]["c_tilted.tif"]["counts"]["intersection"]
    # what cannot be registered is skipped with its reason
    assert report["skipped"] == [
        {"image": "d_top_only.tif", "reason": "no foreground in the bottom 20 % of the ground truth and the prediction"},
        {"image": "e_low.tif", "reason": "image height 4 is below 5 pixels: there is no bottom fifth to align by"}]
    assert plain["skipped"] == [] and plain["images_processed"] == 7 and report["images_processed"] == 5

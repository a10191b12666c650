#!/usr/bin/env python3
"""Does a generated or reconstructed image have the same SHAPE as its ground truth?  The counterpart of the reference's
``analysis/metrics.py::ImageComparison.process_all_images``: Dice and IoU of the foreground masks, the object's height and
its width at three levels, MSE / PSNR against the cleaned prediction, their aggregates with outlier counts, and the share
of exams within 5 / 10 pixels or above 90 / 95 / 97 %.

    python -m pti_ldm_vae_amd.compare_images --gt-dir edente --pred-dir edente_synth [--output-dir DIR]
    python -m pti_ldm_vae_amd.compare_images --results-dir inference_vae_<checkpoint>/results_tif
    python -m pti_ldm_vae_amd.compare_images --results-dir ... --straighten [--write-registered DIR]
    python -m pti_ldm_vae_amd.compare_images --results-dir ... --ssim
    python -m pti_ldm_vae_amd.compare_images --results-dir ... --surface [--surface-tolerances 1 2] [--surface-percentile 95]

``--gt-dir`` / ``--pred-dir`` pair the ``.tif`` / ``.tiff`` files of two folders by file name (files present in one folder
only are reported); ``--results-dir`` takes the ``[input | reconstruction]`` files ``inference_vae`` writes: the left half is
the ground truth, the right half the prediction, and a file of odd width is refused.

The ground-truth mask is ``pixel != 0``; the prediction's is ``|pixel| > --threshold``, cleaned to its largest 8-connected
component with the holes filled -- the per-pixel work of a batch is one ``ops.mask_compare`` launch (csrc/mask_compare.hip)
and one copy back; images are grouped by size.  A pair whose sides differ in size, cannot be read, is larger than the
kernel's 1024-pixel edge or has no foreground on a side is skipped and listed with the reason.

Written to ``--output-dir`` (default ``<input folder>/compare``): ``_metrics.csv`` and ``_dimensions.csv`` in the reference's
layout (``;``-separated), ``compare_metrics.json`` (per-image rows, aggregates, thresholds, skipped pairs, resolved
arguments) and, unless ``--no-plot``, ``_metrics_distribution.png``.  Not computed: the VGG16 feature distances.

``--ssim`` adds the reference's ``"SSIM"`` row: ``skimage.metrics.structural_similarity`` with its defaults and ``data_range =
max(gt) - min(gt)`` -- a 7 x 7 uniform window, sample covariance, the mean with a 3-pixel border cropped off -- between the
ground truth and the cleaned prediction (the pair the MSE is formed from; with ``--straighten`` the registered pair).  The
``mask_compare`` launch writes the cleaned prediction, ``ops.ssim_uniform`` (csrc/ssim_uniform.hip) adds up to three launches,
and the two doubles per image travel in the same copy back.  Each metric dictionary then carries ``"SSIM"`` right after
``"MSE"``, ``_metrics.csv`` gains the row, and an image's ``"sums"`` block gains ``"ssim_data_range"``.  The value is ``None``
for a constant ground truth (data range 0) and for an image with an edge below 7 pixels; such a pair keeps its other metrics
(the reference drops it).  This is NOT ``evaluate_vae``'s SSIM (Gaussian window, zero padding, fixed range, raw reconstruction).
Without ``--ssim`` every output is what it was.

``--surface`` adds how far the outlines are apart, in pixels: ``"Hausdorff Distance"``, ``"Hausdorff Distance 95"`` (the
``--surface-percentile`` of the directed distances, the larger side), ``"Average Surface Distance"`` (the pooled symmetric mean)
and one ``"Surface Dice @ t px"`` per ``--surface-tolerances`` value (edge pixels within ``t``, pixel counts, not surfel
lengths), between exactly the two regions the Dice is formed from: the ground-truth mask and the prediction's filled largest
component (with ``--straighten`` those of the registered pair).  The ``mask_compare`` launch writes both regions as bits,
``ops.surface_distance`` (csrc/surface_distance.hip, an exact Euclidean distance transform, three launches) follows on the same
stream and its 13 doubles per image travel in the same copy back.  The keys come after the existing ones, an image gains a
``"surface"`` block (both directed maxima, percentile values, means and edge counts) and all values are ``None`` when a side has
no outline.  Without ``--surface`` every output is what it was.

``--straighten`` registers every pair before it is measured, as the reference does: both sides are turned until the object's
major axis is vertical (orientation from the second moments of the filled largest component, 4 x 4 cubic rotation about
``(w // 2, h // 2)``, replicate border), then the prediction is moved sideways until the centres of the non-zero pixels in the
bottom fifth agree -- ``ops.register_pairs``, three more launches per batch, still one copy back.  Each image of
``compare_metrics.json`` then carries a ``"registration"`` block (both angles in degrees, the six moments per side, both
centres, the shift); a pair lower than 5 pixels, or with nothing in the bottom fifth of a side, is skipped with the reason.
``--write-registered DIR`` writes ``[rotated ground truth | aligned prediction]`` per compared pair, in the layout
``--results-dir`` reads.  Without ``--straighten`` the report is what it was."""
from __future__ import annotations

import argparse
import json
import random
from pathlib import Path

import numpy as np

WHO = "compare_images"


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="Shape comparison of ground-truth / prediction image pairs (Dice, IoU, object "
                                                 "height and widths); MI355X, HIP labelling kernel.")
    parser.add_argument("--gt-dir", type=Path, default=None, help="folder of ground-truth TIFs (with --pred-dir)")
    parser.add_argument("--pred-dir", type=Path, default=None, help="folder of predicted TIFs, paired with --gt-dir by file name")
    parser.add_argument("--results-dir", type=Path, default=None,
                        help="folder of inference_vae results_tif files: [input | reconstruction] side by side")
    parser.add_argument("--threshold", type=float, default=0.2, help="a predicted pixel is foreground when |pixel| > this (default: 0.2)")
    parser.add_argument("--batch-size", type=int, default=64, help="image pairs per kernel launch (default: 64)")
    parser.add_argument("--num-samples", type=int, default=None, help="compare a random sample of this many pairs (default: all)")
    parser.add_argument("--output-dir", type=Path, default=None, help="where the report goes (default: <input folder>/compare)")
    parser.add_argument("--no-plot", action="store_true", help="do not write _metrics_distribution.png")
    parser.add_argument("--seed", type=int, default=0, help="seed of the --num-samples draw (default: 0)")
    parser.add_argument("--straighten", action="store_true",
                        help="straighten both sides and align the prediction by the bottom fifth before measuring")
    parser.add_argument("--write-registered", type=Path, default=None, metavar="DIR",
                        help="with --straighten: write [rotated ground truth | aligned prediction] TIFs of the compared pairs here")
    parser.add_argument("--ssim", action="store_true",
                        help="also report skimage's uniform-window SSIM of the ground truth and the cleaned prediction")
    parser.add_argument("--surface", action="store_true",
                        help="also report Hausdorff, its percentile form, the average surface distance and surface Dice of the two "
                             "masks' outlines, in pixels; a batch is cut so that the distance kernel's scratch stays under 1 GiB")
    parser.add_argument("--surface-tolerances", type=float, nargs="+", default=None, metavar="T",
                        help="with --surface: up to 4 surface Dice tolerances in pixels (default: 1 2)")
    parser.add_argument("--surface-percentile", type=float, default=None,
                        help="with --surface: the percentile of the robust Hausdorff distance, a multiple of 0.1 (default: 95)")
    args = parser.parse_args(argv)
    if not args.surface and (args.surface_tolerances is not None or args.surface_percentile is not None):
        parser.error("--surface-tolerances and --surface-percentile need --surface")
    if args.surface:
        args.surface_tolerances = [1.0, 2.0] if args.surface_tolerances is None else args.surface_tolerances
        args.surface_percentile = 95.0 if args.surface_percentile is None else args.surface_percentile
        if len(args.surface_tolerances) > 4 or any(not t >= 0.0 for t in args.surface_tolerances):
            parser.error(f"--surface-tolerances takes at most 4 values >= 0, got {args.surface_tolerances}")
        pm = round(args.surface_percentile * 10.0)
        if not 0 <= pm <= 1000 or abs(args.surface_percentile * 10.0 - pm) > 1e-9:
            parser.error(f"--surface-percentile must be a multiple of 0.1 in 0 .. 100, got {args.surface_percentile}")
    if args.write_registered is not None and not args.straighten:
        parser.error("--write-registered needs --straighten")
    pair_mode = args.gt_dir is not None or args.pred_dir is not None
    if pair_mode and args.results_dir is not None:
        parser.error("give either --gt-dir with --pred-dir, or --results-dir, not both")
    if not pair_mode and args.results_dir is None:
        parser.error("give --gt-dir with --pred-dir, or --results-dir")
    if pair_mode and (args.gt_dir is None or args.pred_dir is None):
        parser.error("--gt-dir and --pred-dir go together")
    if not args.threshold >= 0.0:
        parser.error(f"--threshold must be >= 0, got {args.threshold}")
    if args.batch_size < 1:
        parser.error(f"--batch-size must be >= 1, got {args.batch_size}")
    if args.num_samples is not None and args.num_samples < 1:
        parser.error(f"--num-samples must be >= 1, got {args.num_samples}")
    return args


def list_tif_files(path: Path) -> dict[str, Path]:
    """file name -> file of every ``.tif`` / ``.tiff`` (any letter case) in ``path``, sorted."""
    if not path.is_dir():
        raise FileNotFoundError(f"{WHO}: folder does not exist: {path}")
    return {p.name: p for p in sorted(path.iterdir()) if p.is_file() and p.suffix.lower() in {".tif", ".tiff"}}


def list_pairs(args) -> tuple[list, dict]:
    """-> (``[(name, gt file, pred file or None)]`` in sorted order, ``{"gt_only": [...], "pred_only": [...]}``); a pred
    file of ``None`` means the one file holds both halves."""
    if args.results_dir is not None:
        files = list_tif_files(args.results_dir)
        return [(name, p, None) for name, p in files.items()], {"gt_only": [], "pred_only": []}
    gt, pred = list_tif_files(args.gt_dir), list_tif_files(args.pred_dir)
    unpaired = {"gt_only": sorted(set(gt) - set(pred)), "pred_only": sorted(set(pred) - set(gt))}
    return [(name, gt[name], pred[name]) for name in sorted(set(gt) & set(pred))], unpaired


class OddWidth(Exception):
    """A --results-dir file that cannot be split in two halves: the run is refused, not the file skipped."""


def load_pair(gt_file: Path, pred_file: Path | None):
    """-> (gt, pred) as 2-D float32 arrays.  ValueError: unreadable, not 2-D or sides of different size (the pair is
    skipped); OddWidth: a side-by-side file that cannot be halved (the run is refused)."""
    from .data.tiff import read_tiff
    if pred_file is None:
        both = np.asarray(read_tiff(str(gt_file)))
        if both.ndim != 2:
            raise ValueError(f"{gt_file.name}: expected a 2-D image, got shape {both.shape}")
        if both.shape[1] % 2:
            raise OddWidth(f"{WHO}: {gt_file}: width {both.shape[1]} is odd: not an [input | reconstruction] file")
        half = both.shape[1] // 2
        gt, pred = both[:, :half], both[:, half:]
    else:
        gt, pred = np.asarray(read_tiff(str(gt_file))), np.asarray(read_tiff(str(pred_file)))
    if gt.ndim != 2 or pred.ndim != 2:
        raise ValueError(f"expected 2-D images, got shapes {gt.shape} and {pred.shape}")
    if gt.shape != pred.shape:
        raise ValueError(f"Images do not have the same dimensions: {gt.shape} and {pred.shape}")
    return np.ascontiguousarray(gt, dtype=np.float32), np.ascontiguousarray(pred, dtype=np.float32)


NO_BOTTOM = "no foreground in the bottom 20 % of the "
TOO_LOW = "image height {} is below 5 pixels: there is no bottom fifth to align by"


def registration_block(moments, coeffs, align) -> dict:
    """The ``"registration"`` entry of one image from its rows of ``ops.register_pairs``' info (host arrays: int64
    ``[2, 10]``, float64 ``[2, 3]``, int32 ``[6]``)."""
    from . import ops
    a = dict(zip(ops.ALIGN_BOTTOM_COLUMNS, (int(v) for v in align)))
    out = {}
    for side, name in enumerate(("gt", "pred")):
        out[f"angle_{name}_deg"] = float(np.degrees(coeffs[side][0]))
        out[f"moments_{name}"] = dict(zip(ops.MASK_MOMENTS_COLUMNS[:6], (int(v) for v in moments[side][:6])))
    out.update(centre_gt=a["centre_gt"], centre_pred=a["centre_pred"], shift=a["shift"])
    return out


def registration_skip(moments, align):
    """The reason a registered pair is not measured, or None."""
    from . import ops
    from .utils import compare_metrics as M
    status = ops.MASK_MOMENTS_COLUMNS.index("status")
    if moments[0][status] or moments[1][status]:
        raise RuntimeError(f"{WHO}: mask_moments reported status {int(moments[0][status])} / {int(moments[1][status])} (label loop overrun)")
    if moments[0][0] == 0 or moments[1][0] == 0:
        return M.NO_GT if moments[0][0] == 0 else M.NO_PRED
    bad = int(align[ops.ALIGN_BOTTOM_COLUMNS.index("status")])
    return NO_BOTTOM + {1: "ground truth", 2: "prediction", 3: "ground truth and the prediction"}[bad] if bad else None


SURFACE_SCRATCH_CAP = 1 << 30   # bytes of ops.surface_distance's scratch a --surface batch may ask for


def _measure(gt, pred, threshold, counts, sums, ssim_out, surface=None):
    """``ops.mask_compare`` of a pair of device batches; with ``ssim_out`` (the ``[n, 2]`` tail of the batch's buffer) the launch
    also writes the cleaned prediction and ``ops.ssim_uniform`` of (gt, cleaned) follows on the same stream.  A batch with an
    edge below 7 pixels has no window: its rows are zeroed instead (range 0: ``pair_metrics`` reports ``None``).

    ``surface = (counts view, sums view, tolerances, percentile)``: the launch also writes the two regions as bits and
    ``ops.surface_distance`` of them follows on the same stream, into those views of the batch's buffer."""
    from . import ops
    more = {} if surface is None else {"masks": True}
    if ssim_out is None:
        got = ops.mask_compare(gt, pred, threshold=threshold, out=(counts, sums), **more)
    elif min(gt.shape[-2:]) < ops.SSIM_UNIFORM_MIN_EDGE:
        got = ops.mask_compare(gt, pred, threshold=threshold, out=(counts, sums), **more)
        ssim_out.zero_()
    else:
        got = ops.mask_compare(gt, pred, threshold=threshold, out=(counts, sums), cleaned=True, **more)
        ops.ssim_uniform(gt, got[2], out=ssim_out)
    if surface is not None:
        ops.surface_distance(got[-1], percentile=surface[3], tolerances=surface[2], out=(surface[0], surface[1]))


def compare_batch(gts: list, preds: list, threshold: float, device, straighten: bool = False, images: bool = False,
                  ssim: bool = False, surface=None):
    """One launch and ONE copy back for a batch of one shape -> (counts int32 ``[n, 24]``, sums float64 ``[n, 3]``) on the
    host.  Both outputs are views of one device buffer (3 doubles, then 24 int32 = 12 doubles per image).

    ``straighten``: ``ops.register_pairs`` first (three more launches, no synchronisation), the measurement is of the
    registered pair, and a third value is returned: ``{"moments", "coeffs", "align"}`` as host arrays -- they travel in the
    same buffer (29 more doubles per image) and the same copy; with ``images`` also ``"rotated_gt"`` and ``"aligned_pred"``.

    ``ssim``: ``ops.ssim_uniform`` of the measured ground truth and the cleaned prediction after ``mask_compare`` (up to three
    more launches), and one more value is returned LAST: float64 ``[n, 2]`` = ``{ssim, data range}`` -- two more doubles per
    image at the end of the same buffer, the same copy.

    ``surface = (tolerances, percentile)``: ``ops.surface_distance`` of the measured pair's two regions after that (three more
    launches), and one more value is returned after all others: ``(counts int32 [n, 2, 11], sums float64 [n, 2])`` -- 13 more
    doubles per image at the very end of the same buffer, the same copy."""
    import torch

    from . import ops
    n = len(gts)
    gt = torch.from_numpy(np.stack(gts)).to(device)
    pred = torch.from_numpy(np.stack(preds)).to(device)
    base, tail_ssim = n * (44 if straighten else 15), 2 * n if ssim else 0
    tail = tail_ssim + (13 * n if surface is not None else 0)
    cols = len(ops.SURFACE_COLUMNS)

    def surface_views(buf):
        at = base + tail_ssim
        return (buf[at + 2 * n:at + 13 * n].view(torch.int32).view(n, 2, cols), buf[at:at + 2 * n].view(n, 2)) + tuple(surface)

    def surface_host(host):
        at = base + tail_ssim
        return (host[at + 2 * n:at + 13 * n].view(np.int32).reshape(n, 2, cols).copy(), host[at:at + 2 * n].reshape(n, 2).copy())
    if straighten:
        buf = torch.empty(n * 44 + tail, dtype=torch.float64, device=device)
        parts, at = [], 0
        for per_image in (3, 12, 20, 6, 3):          # sums, counts, moments, coeffs, align
            parts.append(buf[at:at + per_image * n])
            at += per_image * n
        sums, counts = parts[0].view(n, 3), parts[1].view(torch.int32).view(n, len(ops.MASK_COMPARE_COLUMNS))
        moments, coeffs = parts[2].view(torch.int64).view(n, 2, 10), parts[3].view(n, 2, 3)
        align = parts[4].view(torch.int32).view(n, len(ops.ALIGN_BOTTOM_COLUMNS))
        rot_gt, aligned, _ = ops.register_pairs(gt, pred, threshold=threshold, out=(None, None, moments, coeffs, align))
        _measure(rot_gt, aligned, threshold, counts, sums, buf[at:at + 2 * n].view(n, 2) if ssim else None,
                 surface_views(buf) if surface is not None else None)
        host = buf.cpu().numpy()
        cut = np.cumsum([0, 3 * n, 12 * n, 20 * n, 6 * n, 3 * n])
        reg = {"moments": host[cut[2]:cut[3]].view(np.int64).reshape(n, 2, 10).copy(), "coeffs": host[cut[3]:cut[4]].reshape(n, 2, 3).copy(),
               "align": host[cut[4]:cut[5]].view(np.int32).reshape(n, -1).copy()}
        if images:
            reg["rotated_gt"], reg["aligned_pred"] = rot_gt.cpu().numpy(), aligned.cpu().numpy()
        res = (host[cut[1]:cut[2]].view(np.int32).reshape(n, -1).copy(), host[:3 * n].reshape(n, 3).copy(), reg)
        res = res + (host[cut[5]:cut[5] + 2 * n].reshape(n, 2).copy(),) if ssim else res
        return res + (surface_host(host),) if surface is not None else res
    buf = torch.empty(n * 15 + tail, dtype=torch.float64, device=device)
    sums = buf[:3 * n].view(n, 3)
    counts = buf[3 * n:15 * n].view(torch.int32).view(n, len(ops.MASK_COMPARE_COLUMNS))
    _measure(gt, pred, threshold, counts, sums, buf[15 * n:17 * n].view(n, 2) if ssim else None,
             surface_views(buf) if surface is not None else None)
    host = buf.cpu().numpy()
    res = (host[3 * n:15 * n].view(np.int32).reshape(n, -1).copy(), host[:3 * n].reshape(n, 3).copy())
    res = res + (host[15 * n:17 * n].reshape(n, 2).copy(),) if ssim else res
    return res + (surface_host(host),) if surface is not None else res


def run(args, device) -> dict:
    """The whole report as a dictionary (what ``compare_metrics.json`` holds), files not yet written."""
    from . import ops
    from .utils import compare_metrics as M
    pairs, unpaired = list_pairs(args)
    if not pairs:
        raise FileNotFoundError(f"{WHO}: no .tif / .tiff " + ("file in " + str(args.results_dir) if args.results_dir is not None
                                else f"file name is present in both {args.gt_dir} and {args.pred_dir}"))
    if args.num_samples is not None and args.num_samples < len(pairs):
        pairs = sorted(random.Random(args.seed).sample(pairs, args.num_samples))
    results, buckets = {}, {}
    straighten = getattr(args, "straighten", False)
    with_ssim = getattr(args, "ssim", False)
    surface = (tuple(args.surface_tolerances), args.surface_percentile) if getattr(args, "surface", False) else None
    surface_pm = ops.surface_percentile_pm(WHO, surface[1]) if surface is not None else None

    def batch_limit(shape):
        """Pairs of this shape per launch: --batch-size, cut so that the distance kernel's scratch stays under the cap."""
        if surface is None:
            return args.batch_size
        from . import _lib
        return max(1, min(args.batch_size, SURFACE_SCRATCH_CAP // max(_lib.lib().pti_surface_distance_ws_bytes(1, *shape), 1)))

    def flush(shape):
        names, gts, preds = buckets.pop(shape)
        reg = ssim_rows = surf = None
        got = compare_batch(gts, preds, args.threshold, device, straighten, straighten and args.write_registered is not None, with_ssim,
                            surface)
        if surface is not None:
            got, surf = got[:-1], got[-1]
        if with_ssim:
            got, ssim_rows = got[:-1], got[-1]
        if straighten:
            counts, sums, reg = got
        else:
            counts, sums = got
        for i, (name, row, s, m) in enumerate(zip(names, counts, sums, M.pair_metrics(counts, sums, *shape, ssim=ssim_rows, surface=surf and surf + (surface[0], surface_pm)))):
            if reg is not None:
                m = registration_skip(reg["moments"][i], reg["align"][i]) or m
            results[name] = m if isinstance(m, str) else {"metrics": m, "dimensions": M.dimensions(row),
                                                          "counts": dict(zip(ops.MASK_COMPARE_COLUMNS, (int(v) for v in row))),
                                                          "sums": dict(zip(ops.MASK_COMPARE_SUMS, (float(v) for v in s)))}
            if with_ssim and not isinstance(m, str):
                results[name]["sums"]["ssim_data_range"] = float(ssim_rows[i][1]) if min(shape) >= ops.SSIM_UNIFORM_MIN_EDGE else None
            if surf is not None and not isinstance(m, str):
                results[name]["surface"] = M.surface_block(surf[0][i], surf[1][i], surface_pm)
            if reg is not None and not isinstance(m, str):
                results[name]["registration"] = registration_block(reg["moments"][i], reg["coeffs"][i], reg["align"][i])
                if args.write_registered is not None:
                    from .data.tiff import write_tiff
                    args.write_registered.mkdir(parents=True, exist_ok=True)
                    write_tiff(str(args.write_registered / name), np.concatenate([reg["rotated_gt"][i], reg["aligned_pred"][i]], axis=1))

    for name, gt_file, pred_file in pairs:
        try:
            gt, pred = load_pair(gt_file, pred_file)
            if max(gt.shape) > ops.MASK_COMPARE_MAX_EDGE or min(gt.shape) < 1:
                raise ValueError(f"image size {gt.shape} is not supported (1 .. {ops.MASK_COMPARE_MAX_EDGE} pixels per edge)")
            if straighten and gt.shape[0] < ops.ALIGN_BOTTOM_MIN_HEIGHT:
                raise ValueError(TOO_LOW.format(gt.shape[0]))
        except (FileNotFoundError, ValueError) as exc:
            results[name] = str(exc)
            continue
        bucket = buckets.setdefault(gt.shape, ([], [], []))
        for lst, v in zip(bucket, (name, gt, pred)):
            lst.append(v)
        if len(bucket[0]) >= batch_limit(gt.shape):
            flush(gt.shape)
    for shape in list(buckets):
        flush(shape)

    names = [p[0] for p in pairs]
    images = {name: results[name] for name in names if not isinstance(results[name], str)}
    skipped = [{"image": name, "reason": results[name]} for name in names if isinstance(results[name], str)]
    all_metrics = [v["metrics"] for v in images.values()]
    # (a run without --ssim or --surface writes the file it wrote before the flag existed: the keys appear only when it is set)
    hidden = (() if with_ssim else ("ssim",)) + (() if surface is not None else ("surface", "surface_tolerances", "surface_percentile"))
    return {"arguments": {k: (str(v) if isinstance(v, Path) else v) for k, v in sorted(vars(args).items()) if k not in hidden},
            "images_processed": len(images), "images": images, "aggregates": M.aggregate(all_metrics),
            "thresholds": [{"name": n_, "count": c, "percentage": p} for n_, c, p in M.threshold_counts(all_metrics)],
            "skipped": skipped, "unpaired": unpaired}


def write_report(report: dict, out_dir: Path, plot: bool) -> list:
    from .utils import compare_metrics as M
    out_dir.mkdir(parents=True, exist_ok=True)
    written = [out_dir / "_metrics.csv", out_dir / "_dimensions.csv", out_dir / "compare_metrics.json"]
    thresholds = [(t["name"], t["count"], t["percentage"]) for t in report["thresholds"]]
    M.write_csv(written[0], M.METRICS_CSV_COLUMNS, M.metrics_csv_rows(report["aggregates"], thresholds, report["images_processed"]))
    M.write_csv(written[1], M.DIMENSION_COLUMNS, [dict(v["dimensions"], **{"Image Path": name}) for name, v in report["images"].items()])
    with written[2].open("w", encoding="utf-8") as fh:
        json.dump(report, fh, indent=2)
    if plot and report["images"]:
        written.append(out_dir / "_metrics_distribution.png")
        M.save_distributions(written[-1], [v["metrics"] for v in report["images"].values()], report["aggregates"])
    return written


def main(argv=None) -> None:
    from . import _lib
    from .utils.cli_common import init_device_and_seed
    _lib.refuse_wrong_result_env("compare_images.py")
    args = parse_args(argv)
    for key in ("gt_dir", "pred_dir", "results_dir", "output_dir", "write_registered"):
        if getattr(args, key) is not None:
            setattr(args, key, getattr(args, key).expanduser().resolve())
    if args.output_dir is None:
        args.output_dir = (args.results_dir if args.results_dir is not None else args.gt_dir) / "compare"
    list_pairs(args)                                   # a missing folder is reported before the device is touched
    device = init_device_and_seed(None)
    report = run(args, device)
    written = write_report(report, args.output_dir, plot=not args.no_plot)
    for side, label in (("gt_only", "ground truth"), ("pred_only", "prediction")):
        for name in report["unpaired"][side]:
            print(f"Unpaired: {name} is in the {label} folder only")
    for s in report["skipped"]:
        print(f"Skipping {s['image']}: {s['reason']}")
    print(f"{report['images_processed']} pair(s) compared, {len(report['skipped'])} skipped")
    for key in ("Dice Coefficient", "IoU", "Height Metric", "Width Metric Middle"):
        a = report["aggregates"].get(key)
        if a and a["n"]:
            print(f"   {key}: {a['mean']:.4f} (worst {a['worst']:.4f}, n = {a['n']})")
    for path in written:
        print(f"   written: {path}")


if __name__ == "__main__":
    main()

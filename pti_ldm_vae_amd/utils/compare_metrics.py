"""Host arithmetic of the image-comparison report (reference src/pti_ldm_vae/analysis/metrics.py: ``ImageComparison``):
from the integer table and the three fp64 sums of ``ops.mask_compare`` to the per-pair metrics, their aggregates with the
reference's five outlier counts, the twelve threshold counts and the rows of its two CSV files.  No torch, fp64 throughout.

``pair_metrics(..., ssim=...)`` adds the reference's ``"SSIM"`` row from ``ops.ssim_uniform``'s two numbers per pair (skimage's
uniform-window SSIM of the ground truth and the cleaned prediction); without the argument nothing changes.

``surface_metrics`` turns the integer table and the sums of ``ops.surface_distance`` into the boundary distances of a pair
(Hausdorff, its percentile form, the average symmetric surface distance, surface Dice), and
``pair_metrics(..., surface=...)`` appends them; without the argument nothing changes.

What is not here: the VGG16 cosine similarity and Euclidean distance; the straighten / align step that the
reference runs before measuring happens on the device before these numbers are taken."""
from __future__ import annotations

import math

import numpy as np

from .._lib import MASK_COMPARE_COLUMNS as COLUMNS
from .._lib import SURFACE_COLUMNS

METRIC_KEYS = ("MSE", "PSNR", "Dice Coefficient", "Dice Loss", "IoU", "Height Metric", "Width Metric Upper",
               "Width Metric Middle", "Width Metric Lower", "Absolute Height Difference", "Absolute Width Upper Difference",
               "Absolute Width Middle Difference", "Absolute Width Lower Difference")
# higher is better (metrics.py:465-475); for every other key the worst value is the largest
HIGHER_IS_BETTER = frozenset(("PSNR", "Dice Coefficient", "Height Metric", "Width Metric Upper", "Width Metric Middle",
                              "Width Metric Lower", "IoU"))
# the optional row of ``pair_metrics(..., ssim=...)`` is higher-is-better too; kept apart so that the set above stays the
# flagless report's
HIGHER_IS_BETTER_OPTIONAL = frozenset(("SSIM",))
# ... and so is every optional key that starts with one of these (``surface_metrics``: one key per tolerance)
HIGHER_IS_BETTER_OPTIONAL_PREFIXES = ("Surface Dice @ ",)
SSIM_MIN_EDGE = 7   # the uniform window of ``ops.ssim_uniform``: a smaller image has no SSIM
OUTLIER_KEYS = ("outside_1_ci", "outside_2_ci", "outside_3_ci", "outside_iqr", "outside_z")
DIMENSION_COLUMNS = ("Image Path", "GT Height", "GT Width Upper", "GT Width Middle", "GT Width Lower", "Gen Height",
                     "Gen Width Upper", "Gen Width Middle", "Gen Width Lower")
METRICS_CSV_COLUMNS = ("Metric", "Average", "Worst Value", "Confidence Interval Lower (95%)", "Confidence Interval Upper (95%)",
                       "Number of Images Processed", "Outside 1 CI", "Outside 2 CI", "Outside 3 CI", "IQR Outliers",
                       "Z-Score Outliers", "Count", "Percentage")
NO_GT = "no foreground component in the ground truth"
NO_PRED = "no foreground component in the prediction"
SMOOTH = 1e-6


def _ratio(a: int, b: int):
    """min / max, ``None`` when the larger term is 0 (the reference divides by zero there)."""
    hi = max(a, b)
    return None if hi == 0 else min(a, b) / hi


def dimensions(row) -> dict:
    """One row of the integer table -> the eight measured sizes under the names of ``_dimensions.csv``."""
    c = dict(zip(COLUMNS, (int(v) for v in row)))
    return {"GT Height": c["gt_h"], "GT Width Upper": c["gt_width_upper"], "GT Width Middle": c["gt_width_middle"],
            "GT Width Lower": c["gt_width_lower"], "Gen Height": c["pred_h"], "Gen Width Upper": c["pred_width_upper"],
            "Gen Width Middle": c["pred_width_middle"], "Gen Width Lower": c["pred_width_lower"]}


def surface_keys(tolerances, percentile_pm: int) -> tuple:
    """The keys of ``surface_metrics`` in order: ``"Hausdorff Distance"``, ``"Hausdorff Distance 95"`` (the percentile as given),
    ``"Average Surface Distance"``, then ``"Surface Dice @ {t} px"`` per tolerance."""
    return ("Hausdorff Distance", f"Hausdorff Distance {percentile_pm / 10:g}", "Average Surface Distance") \
        + tuple(f"Surface Dice @ {float(t):g} px" for t in tolerances)


def _surface_sides(counts, sums, percentile_pm: int):
    """One image's two rows -> per side ``{n_edge, max, percentile, mean}`` in pixels; the last three ``None`` on an empty side
    (the kernel marks both rows then).  A non-zero status column raises."""
    out = []
    for row, total in zip(counts, sums):
        c = dict(zip(SURFACE_COLUMNS, (int(v) for v in row)))
        if c["status"] != 0:
            raise RuntimeError(f"surface_metrics: surface_distance reported status {c['status']}")
        m = c["n_edge"]
        if m == 0 or c["max_d2"] < 0:
            out.append({"n_edge": m, "max": None, "percentile": None, "mean": None, "within": None})
            continue
        lo, hi = math.sqrt(c["d2_lo"]), math.sqrt(c["d2_hi"])
        frac = (((m - 1) * percentile_pm) % 1000) / 1000.0
        out.append({"n_edge": m, "max": math.sqrt(c["max_d2"]), "percentile": lo + frac * (hi - lo), "mean": float(total) / m,
                    "within": [c[f"within_{j}"] for j in range(4)], "sum": float(total)})
    return out


def surface_block(counts, sums, percentile_pm: int) -> dict:
    """The ``"surface"`` entry of one image in ``compare_metrics.json``: both directed maxima, percentile values and means (side
    0 from the ground truth's outline to the prediction's, side 1 the other way) and both edge counts, in pixels."""
    g, p = _surface_sides(counts, sums, percentile_pm)
    return {"percentile": percentile_pm / 10, "edge_pixels_gt": g["n_edge"], "edge_pixels_pred": p["n_edge"],
            "max_gt_to_pred": g["max"], "max_pred_to_gt": p["max"], "percentile_gt_to_pred": g["percentile"],
            "percentile_pred_to_gt": p["percentile"], "mean_gt_to_pred": g["mean"], "mean_pred_to_gt": p["mean"]}


def surface_metrics(counts, sums, tolerances, percentile_pm: int) -> list:
    """Per pair the boundary distances, in pixels, from ``ops.surface_distance``'s ``counts`` int ``[n, 2, 11]`` and ``sums``
    float64 ``[n, 2]`` (host arrays); ``tolerances`` are the pixel distances the launch was given, ``percentile_pm`` its
    percentile in per-mille.  With ``m_s`` the edge pixels of side ``s``:

    * ``"Hausdorff Distance"``: ``sqrt(max(max_d2 of both sides))``;
    * ``"Hausdorff Distance 95"``: per side ``sqrt(d2_lo) + frac (sqrt(d2_hi) - sqrt(d2_lo))``, ``frac = (((m - 1) pm) % 1000) /
      1000`` -- numpy's linear percentile of the side's distances -- and the larger of the two sides;
    * ``"Average Surface Distance"``: ``(sum_0 + sum_1) / (m_0 + m_1)``, the pooled symmetric mean;
    * ``"Surface Dice @ {t} px"``: ``(within_0j + within_1j) / (m_0 + m_1)`` -- edge PIXELS within the tolerance, not surfel
      lengths.

    All of them are ``None`` when a side has no edge pixel."""
    counts = np.asarray(counts).reshape(-1, 2, len(SURFACE_COLUMNS))
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    if len(counts) != len(sums):
        raise ValueError(f"surface_metrics: {len(counts)} count rows but {len(sums)} sum rows")
    tolerances = list(tolerances)
    if len(tolerances) > 4:
        raise ValueError(f"surface_metrics: at most 4 tolerances, got {len(tolerances)}")
    keys = surface_keys(tolerances, percentile_pm)
    out = []
    for c, s in zip(counts, sums):
        a, b = _surface_sides(c, s, percentile_pm)
        if a["max"] is None or b["max"] is None:
            out.append(dict.fromkeys(keys))
            continue
        m = a["n_edge"] + b["n_edge"]
        values = [max(a["max"], b["max"]), max(a["percentile"], b["percentile"]), (a["sum"] + b["sum"]) / m]
        values += [(a["within"][j] + b["within"][j]) / m for j in range(len(tolerances))]
        out.append(dict(zip(keys, values)))
    return out


def pair_metrics(counts, sums, h: int, w: int, ssim=None, surface=None) -> list:
    """Per image either the metric dictionary (``METRIC_KEYS`` in order) or, for a pair that is skipped, the reason as a
    string: a side without any foreground component has no box to measure (the reference's ``except`` drops such a pair).

    ``ssim``: float64 ``[n, 2]`` = ``{ssim, data range}`` as ``ops.ssim_uniform`` returns them (host array); every dictionary
    then carries ``"SSIM"`` right after ``"MSE"`` (the reference's order).  It is ``None`` when the data range is 0 (a constant
    ground truth: 0 / 0) or when an edge is below ``SSIM_MIN_EDGE`` (no 7 x 7 window fits); such a pair keeps its other metrics.

    ``surface``: ``(counts, sums, tolerances, percentile_pm)`` as ``surface_metrics`` takes them; its keys are appended after
    the existing ones.

    ``counts`` int ``[n, 24]`` / ``sums`` float64 ``[n, 3]`` as ``ops.mask_compare`` returns them (host arrays), ``h, w`` the
    image size.  PSNR is ``inf`` at MSE 0 and ``None`` when neither image has a positive pixel; a ratio is ``None`` when
    its larger term is 0.  A non-zero status column raises: the kernel reported an overrun of its bounded loops."""
    counts = np.asarray(counts).reshape(-1, len(COLUMNS))
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    if len(counts) != len(sums):
        raise ValueError(f"pair_metrics: {len(counts)} count rows but {len(sums)} sum rows")
    npix = int(h) * int(w)
    if npix < 1:
        raise ValueError(f"pair_metrics: bad image size {h} x {w}")
    if ssim is not None:
        ssim = np.asarray(ssim, dtype=np.float64).reshape(-1, 2)
        if len(ssim) != len(counts):
            raise ValueError(f"pair_metrics: {len(counts)} count rows but {len(ssim)} ssim rows")
    if surface is not None:
        surface = surface_metrics(*surface)
        if len(surface) != len(counts):
            raise ValueError(f"pair_metrics: {len(counts)} count rows but {len(surface)} surface rows")
    out = []
    for i, (row, (sq, max_gt, max_pred)) in enumerate(zip(counts, sums)):
        c = dict(zip(COLUMNS, (int(v) for v in row)))
        if c["status"] != 0:
            raise RuntimeError(f"pair_metrics: image {i}: mask_compare reported status {c['status']} (label loop overrun)")
        if c["kept_gt"] == 0 or c["kept_pred"] == 0:
            out.append(NO_GT if c["kept_gt"] == 0 else NO_PRED)
            continue
        mse = float(sq) / npix
        peak = max(float(max_gt), float(max_pred))
        psnr = math.inf if mse == 0 else (None if peak <= 0 else 20.0 * math.log10(peak / math.sqrt(mse)))
        dice = (2.0 * c["intersection"] + SMOOTH) / (c["filled_pred"] + c["n_gt"] + SMOOTH)
        d = dimensions(row)
        m = {"MSE": mse, "PSNR": psnr, "Dice Coefficient": dice, "Dice Loss": 1.0 - dice,
             "IoU": 1.0 if c["union"] == 0 else c["intersection"] / c["union"],
             "Height Metric": _ratio(d["GT Height"], d["Gen Height"]),
             "Width Metric Upper": _ratio(d["GT Width Upper"], d["Gen Width Upper"]),
             "Width Metric Middle": _ratio(d["GT Width Middle"], d["Gen Width Middle"]),
             "Width Metric Lower": _ratio(d["GT Width Lower"], d["Gen Width Lower"]),
             "Absolute Height Difference": abs(d["GT Height"] - d["Gen Height"]),
             "Absolute Width Upper Difference": abs(d["GT Width Upper"] - d["Gen Width Upper"]),
             "Absolute Width Middle Difference": abs(d["GT Width Middle"] - d["Gen Width Middle"]),
             "Absolute Width Lower Difference": abs(d["GT Width Lower"] - d["Gen Width Lower"])}
        assert tuple(m) == METRIC_KEYS
        if ssim is not None:
            value = None if (ssim[i][1] == 0 or min(int(h), int(w)) < SSIM_MIN_EDGE) else float(ssim[i][0])
            m = {"MSE": m.pop("MSE"), "SSIM": value, **m}
        if surface is not None:
            m.update(surface[i])
        out.append(m)
    return out


def aggregate(all_metrics: list) -> dict:
    """key -> ``{n, none, mean, std, ci95, worst, outliers}`` over a list of metric dictionaries.

    ``None`` entries are left out of a key's statistics and counted in ``none``; ``n`` is what is left.  ``std`` is the
    population value, ``ci95 = mean -+ 1.96 std / sqrt(n)``, ``worst`` the smallest value of a ``HIGHER_IS_BETTER`` key and
    the largest of any other, ``outliers`` the five counts of the reference's ``count_outliers``: outside 1 / 2 / 3 half-widths
    of the confidence interval round the mean, outside the 1.5 IQR fences, ``|z| > 3`` (0 when ``std`` is 0).  A key without
    any value has ``None`` statistics and zero counts."""
    keys = list(all_metrics[0]) if all_metrics else []
    out = {}
    for key in keys:
        data = np.array([m[key] for m in all_metrics if m[key] is not None], dtype=np.float64)
        n, none = len(data), len(all_metrics) - len(data)
        if n == 0:
            out[key] = {"n": 0, "none": none, "mean": None, "std": None, "ci95": None, "worst": None,
                        "outliers": dict.fromkeys(OUTLIER_KEYS, 0)}
            continue
        with np.errstate(invalid="ignore"):
            mean, std = float(np.mean(data)), float(np.std(data))
            half = 1.96 * (std / math.sqrt(n))
            lo, hi = mean - half, mean + half
            margin = (hi - lo) / 2
            q1, q3 = np.percentile(data, [25, 75])
            iqr = q3 - q1
            outliers = {
                "outside_1_ci": int(np.sum((data < lo) | (data > hi))),
                "outside_2_ci": int(np.sum((data < mean - 2 * margin) | (data > mean + 2 * margin))),
                "outside_3_ci": int(np.sum((data < mean - 3 * margin) | (data > mean + 3 * margin))),
                "outside_iqr": int(np.sum((data < q1 - 1.5 * iqr) | (data > q3 + 1.5 * iqr))),
                "outside_z": 0 if std == 0 else int(np.sum(np.abs((data - mean) / std) > 3)),
            }
        higher = key in HIGHER_IS_BETTER or key in HIGHER_IS_BETTER_OPTIONAL or key.startswith(HIGHER_IS_BETTER_OPTIONAL_PREFIXES)
        worst = float(data.min() if higher else data.max())
        out[key] = {"n": n, "none": none, "mean": mean, "std": std, "ci95": [lo, hi], "worst": worst, "outliers": outliers}
    return out


def threshold_counts(all_metrics: list) -> list:
    """The twelve ``(name, count, percentage)`` rows of metrics.py:770-783 over the processed pairs; a ``None`` metric passes
    no threshold; the percentage is of all processed pairs, rounded to two places."""
    n = len(all_metrics)

    def count(key, test):
        return sum(1 for m in all_metrics if m[key] is not None and test(m[key]))

    rows = []
    for level in (0.95, 0.97, 0.90):
        rows.append((f"Exams with Height Metric > {level:.2f}", count("Height Metric", lambda v: v > level)))
        rows.append((f"Exams with Width Metric > {level:.2f}", count("Width Metric Middle", lambda v: v > level)))
    for limit in (5, 10):
        rows.append((f"Exams with Absolute Height Difference < {limit}", count("Absolute Height Difference", lambda v: v < limit)))
        rows.append((f"Exams with Absolute Middle Width Difference < {limit}",
                     count("Absolute Width Middle Difference", lambda v: v < limit)))
        rows.append((f"Exams with Absolute Lower Width Difference < {limit}",
                     count("Absolute Width Lower Difference", lambda v: v < limit)))
    return [(name, c, round(c / n * 100, 2) if n else 0.0) for name, c in rows]


def metrics_csv_rows(aggregates: dict, thresholds: list, n_images: int) -> list:
    """Rows of ``_metrics.csv`` as dictionaries over ``METRICS_CSV_COLUMNS`` (missing cells stay empty): one row per metric
    with its rounded statistics, then the threshold rows with ``Count`` and ``Percentage``."""
    rows = []
    r3 = lambda v: "" if v is None else round(v, 3)   # noqa: E731
    for key, a in aggregates.items():
        ci = a["ci95"] or (None, None)
        rows.append({"Metric": key, "Average": r3(a["mean"]), "Worst Value": r3(a["worst"]),
                     "Confidence Interval Lower (95%)": r3(ci[0]), "Confidence Interval Upper (95%)": r3(ci[1]),
                     "Number of Images Processed": n_images, "Outside 1 CI": a["outliers"]["outside_1_ci"],
                     "Outside 2 CI": a["outliers"]["outside_2_ci"], "Outside 3 CI": a["outliers"]["outside_3_ci"],
                     "IQR Outliers": a["outliers"]["outside_iqr"], "Z-Score Outliers": a["outliers"]["outside_z"]})
    for name, c, pct in thresholds:
        rows.append({"Metric": name, "Count": c, "Percentage": pct})
    return rows


def write_csv(path, columns, rows) -> None:
    """``;``-separated file with a header line; ``rows`` are dictionaries, a missing cell is left empty."""
    import csv
    with open(path, "w", newline="", encoding="utf-8") as fh:
        writer = csv.DictWriter(fh, fieldnames=list(columns), delimiter=";", restval="")
        writer.writeheader()
        writer.writerows(rows)


def save_distributions(path, all_metrics: list, aggregates: dict) -> None:
    """One histogram per key with the mean (dashed), the IQR fences and the +-3 sigma lines, as the reference's
    ``plot_metric_distributions_with_ci`` draws them; written to ``path``, never shown."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    keys = [k for k, a in aggregates.items() if a["n"] > 0]
    cols = 3
    rows = max((len(keys) + cols - 1) // cols, 1)
    fig, axes = plt.subplots(rows, cols, figsize=(15, rows * 4), squeeze=False)
    axes = axes.flatten()
    for ax, key in zip(axes, keys):
        data = np.array([m[key] for m in all_metrics if m[key] is not None], dtype=np.float64)
        data = data[np.isfinite(data)]
        a = aggregates[key]
        if len(data):
            ax.hist(data, bins=20, color="lightblue", edgecolor="black", alpha=0.7)
            q1, q3 = np.percentile(data, [25, 75])
            mean, std = float(np.mean(data)), float(np.std(data))
            ax.axvline(mean, color="red", linestyle="--", label="Mean", lw=2)
            ax.axvline(q1 - 1.5 * (q3 - q1), color="orange", linestyle="-", label="IQR Lower", lw=2)
            ax.axvline(q3 + 1.5 * (q3 - q1), color="orange", linestyle="-", label="IQR Upper", lw=2)
            ax.axvline(mean - 3 * std, color="red", linestyle="-", label="Z-Score -3", lw=2)
            ax.axvline(mean + 3 * std, color="red", linestyle="-", label="Z-Score +3", lw=2)
            ax.legend(loc="upper left", fontsize=8)
        ax.set_title(f"Distribution of {key} (n = {a['n']})", fontsize=12)
        ax.set_xlabel(f"{key} values", fontsize=10)
        ax.set_ylabel("Frequency", fontsize=10)
    for ax in axes[len(keys):]:
        fig.delaxes(ax)
    fig.tight_layout()
    fig.savefig(path)
    plt.close(fig)

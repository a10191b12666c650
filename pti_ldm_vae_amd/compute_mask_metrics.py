#!/usr/bin/env python3
"""Geometric attributes of dental mask pairs -- the counterpart of the reference's ``vae_scripts/compute_mask_metrics.py``:
the per-image JSON files that ``regularized_attributes.attribute_file`` of an AR-VAE config names.

    python -m pti_ldm_vae_amd.compute_mask_metrics --edente-dir DIR --dente-dir DIR [--output-edente F --output-dente F]

Same options, defaults, outputs and skip messages, plus ``--batch-size``: the ``.tif`` / ``.tiff`` stems present in both
folders are processed in sorted order, ``--batch-size`` pairs per kernel launch.  Every mask is binarised as
``pixel > 0``; the edente mask gives ``height_0`` (height of the bounding box of all its foreground pixels) and
``--edente-width-samples`` widths inside the box, lowest row first; the dente mask gives one width per
``--dente-heights-mm`` entry, measured that far above its last row, and carries the edente ``height_0``.  A pair whose
edente mask is empty, or whose files cannot be read, is skipped with a message and appears in neither file.

TIFF files are decoded by ``data.tiff.read_tiff``; the geometry runs on the HIP device (``data.mask_metrics``)."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

DEFAULT_HEIGHTS_MM = (5.0, 10.0, 14.0, 18.0, 22.0)


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="AR-VAE attribute files (bounding-box height, row widths) from mask TIFs; "
                                                 "MI355X, HIP mask kernel.")
    parser.add_argument("--edente-dir", type=Path, default=Path("./data/edente"), help="folder of edente masks")
    parser.add_argument("--dente-dir", type=Path, default=Path("./data/dente"),
                        help="folder of dente masks; a pair is the same file stem in both folders")
    parser.add_argument("--output-edente", type=Path, default=Path("./data/metrics/attributes_edente.json"),
                        help="JSON written for the edente masks")
    parser.add_argument("--output-dente", type=Path, default=Path("./data/metrics/attributes_dente.json"),
                        help="JSON written for the dente masks")
    parser.add_argument("--pixel-size-mm", type=float, default=0.15, help="millimetres per pixel (default: 0.15)")
    parser.add_argument("--dente-heights-mm", type=float, nargs="+", default=DEFAULT_HEIGHTS_MM,
                        help="distances above the last row of a dente mask at which its width is taken, in mm "
                             "(default: 5 10 14 18 22)")
    parser.add_argument("--edente-width-samples", type=int, default=5,
                        help="widths taken at evenly spread rows of the edente bounding box (default: 5)")
    parser.add_argument("--batch-size", type=int, default=64, help="mask pairs per kernel launch (default: 64)")
    return parser.parse_args(argv)


def list_tif_files(path: Path) -> dict[str, Path]:
    """stem -> file of every ``.tif`` / ``.tiff`` (any letter case) in ``path``."""
    return {p.stem: p for p in sorted(path.iterdir()) if p.suffix.lower() in {".tif", ".tiff"}}


def process_dataset(edente_dir: Path, dente_dir: Path, *, pixel_size_mm: float, dente_heights_mm, edente_width_samples: int,
                    batch_size: int, device) -> tuple[dict[str, dict[str, int]], dict[str, dict[str, int]]]:
    """-> (attributes_edente, attributes_dente), keyed by file name, in sorted stem order."""
    from .data.mask_metrics import mask_attributes, pixel_offsets_mm
    from .data.tiff import read_tiff
    for name, folder in (("Edente", edente_dir), ("Dente", dente_dir)):
        if not folder.is_dir():
            raise FileNotFoundError(f"{name} mask folder does not exist: {folder}")
    edente_files, dente_files = list_tif_files(edente_dir), list_tif_files(dente_dir)
    stems = sorted(set(edente_files) & set(dente_files))
    if not stems:
        raise FileNotFoundError(f"no .tif / .tiff stem is present in both {edente_dir} and {dente_dir}")
    offsets = pixel_offsets_mm(dente_heights_mm, pixel_size_mm)
    attributes_edente, attributes_dente, skipped = {}, {}, 0
    batch_size = max(int(batch_size), 1)
    for start in range(0, len(stems), batch_size):
        batch = stems[start:start + batch_size]
        results, readable, masks = {}, [], ([], [])
        for stem in batch:
            try:
                pair = read_tiff(str(edente_files[stem])), read_tiff(str(dente_files[stem]))
            except (FileNotFoundError, ValueError) as exc:
                results[stem] = str(exc)
                continue
            readable.append(stem)
            masks[0].append(pair[0])
            masks[1].append(pair[1])
        results.update(zip(readable, mask_attributes(masks[0], masks[1], samples=edente_width_samples, bottom_offsets=offsets,
                                                     device=device)))
        for stem in batch:
            if isinstance(results[stem], str):
                skipped += 1
                print(f"Skipping {stem}: {results[stem]}")
            else:
                attributes_edente[edente_files[stem].name], attributes_dente[dente_files[stem].name] = results[stem]
    if skipped:
        print(f"{skipped} pair(s) skipped (listed above); they are in neither output file")
    return attributes_edente, attributes_dente


def save_json(data: dict, path: Path) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    with path.open("w", encoding="utf-8") as fh:
        json.dump(data, fh, indent=4)


def main(argv=None) -> None:
    from . import _lib
    from .utils.cli_common import init_device_and_seed
    _lib.refuse_wrong_result_env("compute_mask_metrics.py")
    args = parse_args(argv)
    edente_dir, dente_dir, output_edente, output_dente = (p.expanduser().resolve() for p in (
        args.edente_dir, args.dente_dir, args.output_edente, args.output_dente))
    heights = tuple(float(v) for v in args.dente_heights_mm)
    device = init_device_and_seed(None)
    attributes_edente, attributes_dente = process_dataset(
        edente_dir, dente_dir, pixel_size_mm=float(args.pixel_size_mm), dente_heights_mm=heights,
        edente_width_samples=int(args.edente_width_samples), batch_size=args.batch_size, device=device)
    save_json(attributes_edente, output_edente)
    save_json(attributes_dente, output_dente)
    summary = {
        "config": {"edente_dir": str(edente_dir), "dente_dir": str(dente_dir), "output_edente": str(output_edente),
                   "output_dente": str(output_dente), "pixel_size_mm": float(args.pixel_size_mm),
                   "dente_heights_mm": list(heights), "edente_width_samples": int(args.edente_width_samples)},
        "generated": [str(output_edente), str(output_dente)],
        "edente_entries": len(attributes_edente),
        "dente_entries": len(attributes_dente),
    }
    print(json.dumps(summary, indent=2))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Predict with a trained regression head on frozen VAE latents -- the counterpart of the reference's
``reg_scripts/inference_regression.py``.

Same options and defaults (``-c --checkpoint --input-dir --output-dir --batch-size --num-workers --num-samples
--seed 42``), same output: ``<output dir>/predictions.json`` = ``{"predictions": {file name: {target: value}}}``
(de-normalised when the run saved ``trained_weights/target_norm_stats.json``); the output directory defaults to
``<run_dir>/inference`` (inference_regression.py:81-120).

``--head hip`` (default): encoder on the HIP engine, then one fused HIP head forward per batch; the predictions of the
whole set stay on the device and are moved once (``utils.regression_utils.predict_on_device``).  ``--head torch``: the
reference's loop with the ``nn.Linear`` head.  ``--random-init-vae`` as in ``train_regression``.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import torch

from .data import create_regression_inference_dataloader
from .evaluate_regression import build_model, load_optional_normalizer
from .utils import regression_utils as R
from .utils.cli_common import init_device_and_seed, load_json_config, resolve_run_dir


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Run inference with a regression head on VAE latents (HIP encoder and head).")
    p.add_argument("-c", "--config-file", required=True, help="Path to regression config JSON.")
    p.add_argument("--checkpoint", required=True, help="Checkpoint of the trained head.")
    p.add_argument("--input-dir", required=True, help="Directory containing images.")
    p.add_argument("--output-dir", default=None, help="Directory to write predictions.json (default: <run_dir>/inference).")
    p.add_argument("--batch-size", type=int, default=None, help="Override batch size.")
    p.add_argument("--num-workers", type=int, default=None, help="Override dataloader workers.")
    p.add_argument("--num-samples", type=int, default=None, help="Limit number of images.")
    p.add_argument("--seed", type=int, default=42, help="Seed for determinism.")
    p.add_argument("--random-init-vae", action="store_true",
                   help="seeded random VAE weights instead of vae.checkpoint (throughput / smoke runs)")
    p.add_argument("--head", choices=("hip", "torch"), default="hip",
                   help="hip: fused HIP head (default); torch: the nn.Linear head")
    return p.parse_args(argv)


def save_predictions(output_dir: Path, target_names: list[str], files: list[str], preds: torch.Tensor) -> None:
    """inference_regression.py:37-47 (``preds``: [N, T] on the host)."""
    rows = preds.tolist()
    payload = {"predictions": {Path(path).name: {name: float(rows[i][j]) for j, name in enumerate(target_names)}
                               for i, path in enumerate(files)}}
    output_dir.mkdir(parents=True, exist_ok=True)
    with (output_dir / "predictions.json").open("w", encoding="utf-8") as handle:
        json.dump(payload, handle, indent=2)


def normalize_configs(config: dict, args: argparse.Namespace):
    """inference_regression.py:58-78."""
    data_cfg = R.extract_regression_data_config(config)
    train_cfg = R.extract_regression_train_config(config)
    if args.batch_size is not None:
        train_cfg["batch_size"] = args.batch_size
    if args.num_workers is not None:
        data_cfg["num_workers"] = args.num_workers
    config["data"], config["regression_train"] = data_cfg, train_cfg
    return data_cfg, train_cfg


def predict_torch(model, dataloader, normalizer, device) -> torch.Tensor:
    """The reference's loop (inference_regression.py:105-116) with the predictions gathered on the device."""
    preds = []
    model.eval()
    with torch.no_grad():
        for images in dataloader:
            out = model(images.to(device))
            preds.append(normalizer.denormalize(out) if normalizer is not None else out)
    return torch.cat(preds)


def main(argv=None) -> None:
    args = parse_args(argv)
    config = load_json_config(args.config_file)
    data_cfg, train_cfg = normalize_configs(config, args)
    run_dir = resolve_run_dir(config, args.config_file)
    device = init_device_and_seed(args.seed)
    targets: list[str] = list(config["targets"])
    model = build_model(config, targets, device, args.random_init_vae)
    R.load_regression_checkpoint(Path(args.checkpoint), model, targets)
    dataloader, image_paths = create_regression_inference_dataloader(
        input_dir=args.input_dir, patch_size=tuple(data_cfg["patch_size"]), batch_size=int(train_cfg["batch_size"]),
        num_samples=args.num_samples, num_workers=data_cfg.get("num_workers", 4), device=device)
    normalizer = load_optional_normalizer(run_dir, targets)
    if args.head == "hip":
        preds = R.predict_on_device(model, dataloader, normalizer)
    else:
        preds = predict_torch(model, dataloader, normalizer, device)
    output_dir = Path(args.output_dir) if args.output_dir is not None else run_dir / "inference"
    save_predictions(output_dir, targets, image_paths, preds.cpu())
    print("Inference complete")
    print(f"   Predictions written to {output_dir / 'predictions.json'}")


if __name__ == "__main__":
    main()

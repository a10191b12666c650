#!/usr/bin/env python3
"""Evaluate a trained regression head on frozen VAE latents -- the counterpart of the reference's
``reg_scripts/evaluate_regression.py``.

Same options and defaults (``-c --checkpoint --input-dir --attributes-path --output-dir --batch-size --num-workers
--num-samples --seed 42``), same config schema as ``train_regression`` plus the optional ``evaluation`` block, same output:
``<output dir>/metrics.json`` = ``{"metrics": {"val_loss", "mae", "mse", "mae_<target>", "mse_<target>", ...}, "args",
"files"}`` with ``resolved_input_dir`` / ``resolved_attributes_path`` among the args; the output directory defaults to
``<run_dir>/eval`` and the target normaliser is read from ``<run_dir>/trained_weights/target_norm_stats.json`` when that
file exists (evaluate_regression.py:92-131).

The encoder forward runs on the HIP engine under ``no_grad``.  ``--head hip`` (default) runs the head, the
de-normalisation and the loss as one fused HIP forward per batch and folds the whole set on the device, with one host
synchronisation per run (``utils.regression_utils.evaluate_on_device``); ``--head torch`` is the reference's
``validate_one_epoch``.  ``--random-init-vae`` builds the VAE of ``vae.config_file`` with seeded random weights when no
checkpoint exists, as ``train_regression`` has it (never silently).
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

from .data import create_regression_eval_dataloader
from .models import VAEModel
from .utils import regression_utils as R
from .utils.cli_common import init_device_and_seed, load_json_config, resolve_run_dir
from .utils.config import load_vae_config

NORM_STATS_FILENAME = "target_norm_stats.json"


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Evaluate a regression head on VAE latents (HIP encoder and head).")
    p.add_argument("-c", "--config-file", required=True, help="Path to regression config JSON.")
    p.add_argument("--checkpoint", required=True, help="Checkpoint of the trained head.")
    p.add_argument("--input-dir", required=False, default=None,
                   help="Directory containing validation/test images (default: evaluation.data_base_dir).")
    p.add_argument("--attributes-path", required=False, default=None,
                   help="Attributes JSON for evaluation targets (default: evaluation.attributes_path).")
    p.add_argument("--output-dir", default=None, help="Directory to write metrics.json (default: <run_dir>/eval).")
    p.add_argument("--batch-size", type=int, default=None, help="Override batch size.")
    p.add_argument("--num-workers", type=int, default=None, help="Override dataloader workers.")
    p.add_argument("--num-samples", type=int, default=None, help="Evaluate only first N samples.")
    p.add_argument("--seed", type=int, default=42, help="Seed for determinism.")
    p.add_argument("--random-init-vae", action="store_true",
                   help="seeded random VAE weights instead of vae.checkpoint (throughput / smoke runs)")
    p.add_argument("--head", choices=("hip", "torch"), default="hip",
                   help="hip: fused HIP head and on-device metrics (default); torch: the reference's validate_one_epoch")
    return p.parse_args(argv)


def save_metrics(output_dir: Path, metrics: dict, args: argparse.Namespace, files: list[str]) -> None:
    """evaluate_regression.py:47-53."""
    payload = {"metrics": metrics, "args": vars(args).copy(), "files": files}
    output_dir.mkdir(parents=True, exist_ok=True)
    with (output_dir / "metrics.json").open("w", encoding="utf-8") as handle:
        json.dump(payload, handle, indent=2)


def load_optional_normalizer(run_dir: Path, target_names: list[str]):
    """evaluate_regression.py:56-61: the training run's normaliser when it saved one."""
    path = run_dir / "trained_weights" / NORM_STATS_FILENAME
    return R.load_target_normalizer(path, target_names) if path.exists() else None


def normalize_configs(config: dict, args: argparse.Namespace):
    """evaluate_regression.py:64-89: data / train / evaluation blocks with the CLI values applied."""
    data_cfg = R.extract_regression_data_config(config)
    train_cfg = R.extract_regression_train_config(config)
    eval_cfg = R.extract_regression_eval_config(config, data_cfg)
    if args.batch_size is not None:
        train_cfg["batch_size"] = args.batch_size
    if args.num_workers is not None:
        data_cfg["num_workers"] = eval_cfg["num_workers"] = args.num_workers
    if args.attributes_path is not None:
        eval_cfg["attributes_path"] = args.attributes_path
    config["data"], config["regression_train"], config["evaluation"] = data_cfg, train_cfg, eval_cfg
    return data_cfg, train_cfg, eval_cfg


def build_model(config: dict, targets: list[str], device, random_init_vae: bool):
    """The frozen VAE + head of the config (``--random-init-vae``: seeded random encoder, said out loud)."""
    if random_init_vae:
        print("[WARN] --random-init-vae: the VAE encoder has seeded random weights, not vae.checkpoint")
        vae = VAEModel.from_config(load_vae_config(config["vae"]["config_file"]).autoencoder_def).to(device).eval()
        return R.build_regression_model(vae, config, targets, device)[0]
    return R.build_regression_model_from_config(config, targets, device)[0]


def main(argv=None) -> None:
    args = parse_args(argv)
    config = load_json_config(args.config_file)
    data_cfg, train_cfg, eval_cfg = normalize_configs(config, args)
    run_dir = resolve_run_dir(config, args.config_file)
    device = init_device_and_seed(args.seed)
    targets: list[str] = list(config["targets"])
    model = build_model(config, targets, device, args.random_init_vae)
    R.load_regression_checkpoint(Path(args.checkpoint), model, targets)
    batch_size = int(train_cfg["batch_size"])
    input_dir = args.input_dir or eval_cfg["data_base_dir"]
    attributes_path = eval_cfg["attributes_path"]
    dataloader, image_paths = create_regression_eval_dataloader(
        input_dir=input_dir, attributes_path=attributes_path, targets=targets, patch_size=tuple(eval_cfg["patch_size"]),
        batch_size=batch_size, num_workers=eval_cfg.get("num_workers", 4), num_samples=args.num_samples,
        data_source=eval_cfg.get("data_source", "edente"), normalize_attributes=eval_cfg.get("normalize_attributes"),
        device=device)
    normalizer = load_optional_normalizer(run_dir, targets)
    loss_name = train_cfg.get("loss", "mse")
    if args.head == "hip":
        val_loss, metrics = R.evaluate_on_device(model, dataloader, loss_name, targets, normalizer, batch_size)
    else:
        val_loss, metrics = R.validate_one_epoch(model, dataloader, R.build_loss_fn(loss_name), device, targets, normalizer)
    resolved = vars(args).copy()
    resolved["resolved_input_dir"], resolved["resolved_attributes_path"] = input_dir, attributes_path
    output_dir = Path(args.output_dir) if args.output_dir is not None else run_dir / "eval"
    save_metrics(output_dir, {"val_loss": val_loss, **metrics}, argparse.Namespace(**resolved), image_paths)
    print("Evaluation complete")
    print(f"   Metrics written to {output_dir / 'metrics.json'}")


if __name__ == "__main__":
    main()

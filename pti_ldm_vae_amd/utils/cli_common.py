"""Shared pieces of the inference and evaluation commands (reference ``src/pti_ldm_vae/utils/cli_common.py:16-134``):
same option names and defaults, same default directory names.  ``init_device_and_seed`` does what the reference's does
without its MONAI calls (``print_config`` / ``set_determinism``)."""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Any

import torch

from .vae_loader import default_eval_output_dir, load_vae_config, load_vae_model


def add_shared_io_args(parser: argparse.ArgumentParser, output_help: str) -> None:
    """``-c/--config-file``, ``--checkpoint``, ``--input-dir`` (required), ``--output-dir``, ``--num-samples``,
    ``--batch-size 8``, ``--num-workers 4``, ``--seed 42``."""
    parser.add_argument("-c", "--config-file", required=True, help="Config json file")
    parser.add_argument("--checkpoint", type=str, required=True,
                        help="Checkpoint file: a bare state dict (autoencoder_epoch73.pth) or a training checkpoint "
                             "(checkpoint_epoch73.pth)")
    parser.add_argument("--input-dir", type=str, required=True, help="Directory containing input TIF images")
    parser.add_argument("--output-dir", type=str, default=None, help=output_help)
    parser.add_argument("--num-samples", type=int, default=None, help="Number of samples to process (default: all)")
    parser.add_argument("--batch-size", type=int, default=8, help="Batch size (default: 8)")
    parser.add_argument("--num-workers", type=int, default=4, help="Number of TIFF decoding threads (default: 4)")
    parser.add_argument("--seed", type=int, default=42, help="Random seed for determinism (default: 42)")


def init_device_and_seed(seed: int | None) -> torch.device:
    """Select the device and seed torch's generators (``None``: leave them).  The commands run on the HIP device only."""
    if not torch.cuda.is_available():
        raise RuntimeError("pti_ldm_vae_amd: the HIP engine needs an MI355X (there is no CPU/PyTorch fallback)")
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    print(f"Using device: {device}")
    if seed is not None:
        torch.manual_seed(seed)
    return device


def load_config_and_model(config_file: str, checkpoint_path: str, device: torch.device) -> tuple[Any, Any]:
    """-> (parsed config, eval-mode ``VAEModel`` with the checkpoint's weights)."""
    config = load_vae_config(config_file)
    return config, load_vae_model(config, checkpoint_path, device)


def build_inference_dataloader(input_dir: str, config: Any, batch_size: int, num_samples: int | None, num_workers: int,
                               device="cuda"):
    """-> (loader, image paths) with the training pipeline's preprocessing at ``autoencoder_train.patch_size``."""
    from ..data import create_vae_inference_dataloader
    return create_vae_inference_dataloader(input_dir=input_dir, patch_size=tuple(config.autoencoder_train["patch_size"]),
                                           batch_size=batch_size, num_samples=num_samples, num_workers=num_workers,
                                           device=device)


def resolve_inference_output_dirs(checkpoint_path: str, output_dir: str | None) -> tuple[Path, Path, Path]:
    """-> (root, root/results_tif, root/results_png), created; root defaults to ``inference_vae_<checkpoint stem>``."""
    root = Path(output_dir) if output_dir is not None else Path(f"inference_vae_{Path(checkpoint_path).stem}")
    out_tif, out_png = root / "results_tif", root / "results_png"
    for d in (out_tif, out_png):
        d.mkdir(parents=True, exist_ok=True)
    return root, out_tif, out_png


def resolve_eval_output_dir(config_file: str, output_dir: str | None) -> Path:
    """-> the evaluation's output directory, created; defaults to ``evals/<config stem>``."""
    out = Path(output_dir) if output_dir is not None else default_eval_output_dir(config_file)
    out.mkdir(parents=True, exist_ok=True)
    return out


def load_json_config(config_file: str) -> dict[str, Any]:
    """The parsed JSON configuration file (reference cli_common.py:137-147)."""
    import json
    with open(config_file, encoding="utf-8") as handle:
        return json.load(handle)


def resolve_run_dir(config: dict[str, Any], config_file: str) -> Path:
    """-> ``config["run_dir"]``, or ``runs/<config stem>`` (stored back into ``config``) when it is missing; created
    (reference cli_common.py:150-166)."""
    if config.get("run_dir"):
        run_dir = Path(config["run_dir"])
    else:
        run_dir = Path("runs") / Path(config_file).stem
        config["run_dir"] = str(run_dir)
    run_dir.mkdir(parents=True, exist_ok=True)
    return run_dir

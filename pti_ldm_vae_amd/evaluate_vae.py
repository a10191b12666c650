#!/usr/bin/env python3
"""Evaluate a trained VAE on a folder of TIF images -- the counterpart of the reference's ``vae_scripts/evaluate_vae.py``.

Same CLI (``-c/--config-file --checkpoint --input-dir --output-dir --num-samples --batch-size --num-workers --seed``),
same ``<output-dir>/metrics.json`` (``{"args", "metrics", "files"}``; default directory ``evals/<config name>/``), same
metrics: mean and standard deviation of ``recon_loss``, ``kl_loss``, ``perceptual_loss``, ``loss_total`` (one value per
batch) and ``psnr``, ``ssim``, ``mse``, ``mae`` (one value per image, on the images clamped to [0, 1]).

Per batch, all on the device (evaluate_vae.py:82-109): one SAMPLED forward (the reference calls ``autoencoder(images)``),
``pti_vae_loss`` for the L1-or-L2 intensity term and the KL term on the unclamped tensors, ``pti_image_metrics`` for the
four per-image numbers in one fused pass (clamp to [0, 1] applied as the images are loaded), the perceptual term on the
perceptual engine, and ONE device-to-host copy of all of it.  ``loss_total = intensity + kl + perceptual_weight *
perceptual`` with KL unweighted, as the reference has it.

Different on purpose: the perceptual term needs pretrained weights that cannot be fetched here.  ``--perceptual-weights
SQUEEZENET_PTH LPIPS_SQUEEZE_PTH`` (local files, as in ``train_vae``) makes it part of the evaluation; without them a
config with a non-zero ``perceptual_weight`` is refused, or, with ``--ignore-unavailable-terms``, evaluated without the
term after a warning: the ``perceptual_loss_*`` keys are then left out and nothing is added to ``loss_total``.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from . import ops
from .utils.cli_common import (add_shared_io_args, build_inference_dataloader, init_device_and_seed, load_config_and_model,
                               resolve_eval_output_dir)
from .utils.eval_metrics import serialize_args

PER_BATCH = ("recon_loss", "kl_loss", "perceptual_loss", "loss_total")
PER_IMAGE = ("mse", "mae", "psnr", "ssim")        # column order of ops.image_metrics


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="Evaluate a trained VAE on a test set (MI355X, HIP engine).")
    add_shared_io_args(parser, output_help="Output directory for metrics (default: evals/<config_name>/)")
    parser.add_argument("--ignore-unavailable-terms", action="store_true",
                        help="evaluate without the perceptual term when its weight files are not given")
    parser.add_argument("--perceptual-weights", nargs=2, metavar=("SQUEEZENET_PTH", "LPIPS_SQUEEZE_PTH"), default=None,
                        help="local weight files of the perceptual loss: torchvision squeezenet1_1 state_dict and lpips v0.1 squeeze.pth")
    return parser.parse_args(argv)


def select_intensity_loss(config) -> str:
    """"l2" when the config trains with it, else "l1" (evaluate_vae.py:36-47)."""
    return "l2" if config.autoencoder_train.get("recon_loss") == "l2" else "l1"


@torch.no_grad()
def evaluate(autoencoder, dataloader, device, recon_loss: str = "l1", perceptual=None, perceptual_weight: float = 0.0,
             on_batch=None) -> dict[str, float]:
    """Run the evaluation -> ``{"<metric>_mean", "<metric>_std"}`` (population standard deviation, as ``np.std``).

    ``recon_loss``: "l1" or "l2".  ``perceptual``: a module ``loss(input, target) -> scalar`` or None (the
    ``perceptual_loss`` keys are then left out).  ``on_batch(images, reconstruction, z_mu, z_third)``: optional observer,
    called with the device tensors of each batch (copy what you keep: the loader reuses its buffers)."""
    if recon_loss not in ("l1", "l2"):
        raise ValueError(f"recon_loss must be 'l1' or 'l2', got {recon_loss!r}")
    values: dict[str, list[float]] = {k: [] for k in PER_BATCH + PER_IMAGE}
    for batch in dataloader:
        images = batch.to(device).float().contiguous()
        reconstruction, z_mu, z_third = autoencoder(images)
        reconstruction = reconstruction.float().contiguous()
        b = images.shape[0]
        # everything the host needs of this batch in one buffer: [intensity, kl, perceptual, b x (mse, mae, psnr, ssim)]
        pack = torch.zeros(3 + 4 * b, dtype=torch.float32, device=images.device)
        ops.vae_loss(reconstruction, images, z_mu.contiguous(), z_third.contiguous(), pack[:2], None, None, None,
                     l2=recon_loss == "l2", third_mode=0, kl_weight=0.0)
        ops.image_metrics(reconstruction, images, clamp=(0.0, 1.0), out=pack[3:].view(b, 4))
        if perceptual is not None:
            pack[2].copy_(perceptual(reconstruction, images).reshape(()))
        if on_batch is not None:
            on_batch(images, reconstruction, z_mu, z_third)
        host = pack.cpu().double()                      # the batch's one device-to-host copy (and its one sync)
        intensity, kl, perc = host[0].item(), host[1].item(), host[2].item()
        values["recon_loss"].append(intensity)
        values["kl_loss"].append(kl)
        if perceptual is not None:
            values["perceptual_loss"].append(perc)
        values["loss_total"].append(intensity + kl + perceptual_weight * perc)
        per_image = host[3:].view(b, 4)
        for col, key in enumerate(PER_IMAGE):
            values[key].extend(per_image[:, col].tolist())
    summary: dict[str, float] = {}
    for key in ("recon_loss", "kl_loss", "perceptual_loss", "psnr", "ssim", "loss_total", "mse", "mae"):
        if values[key]:
            summary[f"{key}_mean"] = float(np.mean(values[key]))
            summary[f"{key}_std"] = float(np.std(values[key]))
    return summary


def save_metrics(output_dir: Path, summary: dict[str, float], image_paths: list[str], args: argparse.Namespace) -> None:
    """``<output_dir>/metrics.json`` = {"args": the CLI arguments, "metrics": summary, "files": the evaluated paths}."""
    payload = {"args": serialize_args(args), "metrics": summary, "files": list(image_paths)}
    with open(Path(output_dir) / "metrics.json", "w", encoding="utf-8") as f:
        json.dump(payload, f, indent=2)


def main(argv=None) -> None:
    from . import _lib
    from .models import PerceptualLoss
    _lib.refuse_wrong_result_env("evaluate_vae.py")
    args = parse_args(argv)
    device = init_device_and_seed(args.seed)
    config, autoencoder = load_config_and_model(args.config_file, args.checkpoint, device)
    if config.autoencoder_def["in_channels"] != 1:
        raise SystemExit("evaluate_vae: the TIFF pipeline produces single-channel images (in_channels must be 1)")
    perceptual_weight = float(config.autoencoder_train.get("perceptual_weight", 0.0))
    perceptual = None
    if args.perceptual_weights:
        perceptual = PerceptualLoss(spatial_dims=2, network_type="squeeze", weights=tuple(args.perceptual_weights)).to(device)
    elif perceptual_weight != 0.0:
        msg = (f"terms not available in the native evaluation: perceptual_weight={perceptual_weight} (the pretrained "
               "SqueezeNet/LPIPS weights are not available offline: supply them with --perceptual-weights)")
        if not args.ignore_unavailable_terms:
            raise SystemExit(msg + " — set it to 0 or pass --ignore-unavailable-terms")
        print("[WARN] " + msg + " — evaluating without it: no perceptual_loss keys, nothing added to loss_total")
        perceptual_weight = 0.0
    output_dir = resolve_eval_output_dir(args.config_file, args.output_dir)
    dataloader, image_paths = build_inference_dataloader(input_dir=args.input_dir, config=config, batch_size=args.batch_size,
                                                         num_samples=args.num_samples, num_workers=args.num_workers,
                                                         device=device)
    print(f"[INFO] Found {len(image_paths)} images in {args.input_dir}")
    summary = evaluate(autoencoder, dataloader, device, select_intensity_loss(config), perceptual=perceptual,
                       perceptual_weight=perceptual_weight)
    save_metrics(output_dir, summary, image_paths, args)
    print("\n=== Evaluation Summary ===")
    for key, value in summary.items():
        print(f"{key}: {value:.4f}")
    print(f"\nMetrics saved to {output_dir / 'metrics.json'}")


if __name__ == "__main__":
    main()

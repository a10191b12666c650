#!/usr/bin/env python3
"""Did the attribute regularisation work?  For a trained AR-VAE and a directory of images with an attribute file, report
how well latent channel ``c_q`` orders the images the way attribute ``q`` does -- and whether it does so better than the
other channels -- over ALL image pairs, not the 56 ordered pairs of a training batch of 8.

The reference answers this by eye only (``vae_scripts/analyze_ar_channels.py``: one image, a Dash server; its panel is
``analyze_ar_channels`` here).  This command has no counterpart there.

Per batch the graph-replayed encoder (``encode_deterministic``) gives ``z_mu``; the per-image code is
``z_mu.double().mean((2, 3)).float()``, collected in one preallocated ``[N, L]`` device matrix.  ONE ``ops.rank_agreement``
call then classifies every image pair for every (attribute, channel) on the device and adds up the full-set value of the
term the training minimises; the results come to the host in one copy.

Outputs in ``--output-dir`` (default ``<run_dir>/ar_eval``):

* ``ar_metrics.json``: ``attributes`` (by name: ``latent_channel, delta, pairs, concordance, kendall_tau_b, pearson_r, ar_loss,
  best_channel`` = argmax |tau_b| over the channels, ``mapped_channel_is_best``), the ``[na][L]`` matrices ``kendall_tau_b``,
  ``concordance``, ``pearson_r``, the exact ``counts`` ``[na][L][5]`` (concordant, discordant, z-tied, a-tied, both-tied),
  ``n_images``, ``args``, ``files``.  An undefined ratio is ``null``.
* ``channel_means.npz``: ``z`` [N, L], ``attrs`` [na, N], ``names``, ``files``.
* ``ar_matrix.png``: the tau-b heat map with the mapped cells outlined.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from . import ops
from .data import create_regression_eval_dataloader
from .models import VAEModel
from .trainer import ARSettings
from .utils import ar_metrics
from .utils.cli_common import init_device_and_seed, resolve_run_dir
from .utils.vae_loader import load_vae_config, load_vae_model


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Attribute-ordering report of an AR-VAE over all image pairs (HIP pair kernel).")
    p.add_argument("-c", "--config-file", required=True, help="AR-VAE config JSON.")
    p.add_argument("--checkpoint", required=True, help="VAE checkpoint (bare state dict or training checkpoint).")
    p.add_argument("--input-dir", required=True, help="Directory containing the images.")
    p.add_argument("--attributes-path", default=None,
                   help="Attributes JSON (default: regularized_attributes.attribute_file of the config).")
    p.add_argument("--output-dir", default=None, help="Where to write the report (default: <run_dir>/ar_eval).")
    p.add_argument("--batch-size", type=int, default=8, help="Encoder batch size (default: 8).")
    p.add_argument("--num-samples", type=int, default=None, help="Use only the first N images.")
    p.add_argument("--num-workers", type=int, default=4, help="TIFF decoding threads (default: 4).")
    p.add_argument("--seed", type=int, default=42, help="Seed for determinism.")
    p.add_argument("--random-init-vae", action="store_true",
                   help="seeded random VAE weights instead of --checkpoint (throughput / smoke runs)")
    return p.parse_args(argv)


def load_model(config, checkpoint: str, device, random_init_vae: bool) -> VAEModel:
    if random_init_vae:
        print("[WARN] --random-init-vae: the VAE has seeded random weights, not --checkpoint")
        return VAEModel.from_config(config.autoencoder_def).to(device).eval()
    return load_vae_model(config, checkpoint, device)


def check_table(table: torch.Tensor, names: list[str]) -> None:
    """Refuse what the pair kernel does not define: non-finite attribute values, more than 32768 images, fewer than 2."""
    n = table.shape[0]
    if n > ops.RANK_AGREEMENT_MAX_N:
        raise SystemExit(f"evaluate_ar_vae: {n} images, the pair kernel takes at most {ops.RANK_AGREEMENT_MAX_N}: "
                         "pass --num-samples")
    if n < 2:
        raise SystemExit(f"evaluate_ar_vae: {n} image(s); an ordering needs at least 2")
    bad = ~torch.isfinite(table)
    if bool(bad.any()):
        row, col = (int(v) for v in bad.nonzero()[0])
        raise SystemExit(f"evaluate_ar_vae: attribute {names[col]!r} of image {row} is not finite ({float(table[row, col])})")


@torch.no_grad()
def channel_means(model: VAEModel, loader, n: int, latent_channels: int, device) -> torch.Tensor:
    """-> ``[N, L]`` fp32 device matrix: ``encode_deterministic(batch).double().mean((2, 3)).float()`` of every batch."""
    z = torch.empty((n, latent_channels), dtype=torch.float32, device=device)
    row = 0
    for images, _ in loader:
        z_mu = model.encode_deterministic(images)
        z[row:row + z_mu.shape[0]] = z_mu.double().mean((2, 3)).float()
        row += z_mu.shape[0]
    if row != n:
        raise RuntimeError(f"evaluate_ar_vae: the loader gave {row} images, {n} expected")
    return z


def main(argv=None) -> None:
    args = parse_args(argv)
    config = load_vae_config(args.config_file)
    ra = getattr(config, "regularized_attributes", None) or {}
    latent_channels = int(config.autoencoder_def["latent_channels"])
    settings = ARSettings.from_config(ra, gamma=0.0, latent_channels=latent_channels)
    if latent_channels > ops.RANK_AGREEMENT_MAX_L or len(settings.names) > ops.RANK_AGREEMENT_MAX_NA:
        raise SystemExit(f"evaluate_ar_vae: {len(settings.names)} attributes x {latent_channels} channels; the pair kernel "
                         f"takes at most {ops.RANK_AGREEMENT_MAX_NA} x {ops.RANK_AGREEMENT_MAX_L}")
    attributes_path = args.attributes_path if args.attributes_path is not None else ra.get("attribute_file")
    if attributes_path is None:
        raise SystemExit("evaluate_ar_vae: no --attributes-path and no regularized_attributes.attribute_file in the config")
    device = init_device_and_seed(args.seed)
    model = load_model(config, args.checkpoint, device, args.random_init_vae)
    loader, paths = create_regression_eval_dataloader(
        input_dir=args.input_dir, attributes_path=attributes_path, targets=settings.names,
        patch_size=tuple(config.autoencoder_train["patch_size"]), batch_size=args.batch_size, num_workers=args.num_workers,
        num_samples=args.num_samples, data_source=getattr(config, "data_source", "edente"),
        normalize_attributes=ra.get("normalize_attributes"), device=device)
    table = loader.stacked_targets()                                   # host [N, na]
    check_table(table, settings.names)
    n = table.shape[0]
    attrs = table.t().contiguous().to(device)                          # [na, N]
    z = channel_means(model, loader, n, latent_channels, device)
    counts, loss_sum = ops.rank_agreement(z, attrs, settings.channels, settings.deltas)
    packed = torch.cat([counts.reshape(-1).double(), loss_sum, z.reshape(-1).double()]).cpu()   # one copy to the host
    k = counts.numel()
    counts_h = packed[:k].to(torch.int64).reshape(counts.shape).numpy()   # < 2^53: exact through fp64
    loss_h = packed[k:k + loss_sum.numel()].numpy()
    z_h = packed[k + loss_sum.numel():].float().reshape(z.shape).numpy()
    attrs_h = table.t().contiguous().numpy()

    report = ar_metrics.attribute_report(settings.names, settings.channels, settings.deltas, counts_h, loss_h,
                                         ar_metrics.pearson_matrix(z_h, attrs_h))
    files = [Path(p).name for p in paths]
    resolved = vars(args).copy()
    resolved["resolved_attributes_path"] = attributes_path
    report.update(n_images=n, args=resolved, files=files)
    out_dir = Path(args.output_dir) if args.output_dir is not None else resolve_run_dir(vars(config), args.config_file) / "ar_eval"
    out_dir.mkdir(parents=True, exist_ok=True)
    with (out_dir / "ar_metrics.json").open("w", encoding="utf-8") as handle:
        json.dump(report, handle, indent=2)
    np.savez(out_dir / "channel_means.npz", z=z_h, attrs=attrs_h, names=np.array(settings.names), files=np.array(files))
    ar_metrics.save_tau_heatmap(out_dir / "ar_matrix.png", report["kendall_tau_b"], settings.names, settings.channels)
    for name, entry in report["attributes"].items():
        tau = entry["kendall_tau_b"]
        print(f"   {name}: channel {entry['latent_channel']} tau_b {'n/a' if tau is None else format(tau, '+.4f')} "
              f"ar_loss {entry['ar_loss']:.6f} best channel {entry['best_channel']}")
    print("Evaluation complete")
    print(f"   Report written to {out_dir / 'ar_metrics.json'}")


if __name__ == "__main__":
    main()

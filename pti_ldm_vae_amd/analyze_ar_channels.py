#!/usr/bin/env python3
"""Every latent channel of ONE image next to the image and its reconstruction -- the content of the reference's
``vae_scripts/analyze_ar_channels.py`` as files instead of a Dash server (no interactive server, hence no
``--port`` / ``--host`` / ``--debug``).

Same steps: the training pipeline's preprocessing at ``autoencoder_train.patch_size``, ``encode_deterministic``,
``decode_stage_2_outputs``; every tile is min-max normalised to [0, 1] on its own (a constant map becomes zeros) and the
channel tiles are titled ``ch k: <attribute> (regularized)`` or ``ch k: unmapped`` from the config's
``regularized_attributes.attribute_latent_mapping``.

Outputs in ``--output-dir`` (default ``<run_dir>/ar_channels``): ``ar_channels_<stem>.png`` (Input, Reconstruction, then one
tile per latent channel) and ``ar_channels_<stem>.npz`` (``original``: the image as stored, ``input``: the preprocessed image
the encoder saw, ``reconstruction``, ``latents`` [L, h, w]).
"""
from __future__ import annotations

import argparse
import math
from pathlib import Path
from typing import Any

import numpy as np
import torch

from .utils.cli_common import init_device_and_seed, resolve_run_dir
from .utils.vae_loader import load_vae_config, load_vae_model


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Panel of the AR-VAE latent channels of a single image.")
    p.add_argument("-c", "--config-file", required=True, help="AR-VAE config (JSON) whose attribute_latent_mapping names the channels.")
    p.add_argument("--checkpoint", required=True, help="Weights of the trained VAE: a bare state dict or a training checkpoint.")
    p.add_argument("--image-path", required=True, help="The one TIFF image to encode and decode.")
    p.add_argument("--output-dir", default=None, help="Where to write the panel (default: <run_dir>/ar_channels).")
    p.add_argument("--random-init-vae", action="store_true",
                   help="seeded random VAE weights instead of --checkpoint (throughput / smoke runs)")
    return p.parse_args(argv)


def load_attribute_mapping(config: Any) -> dict[str, int]:
    """attribute name -> latent channel from ``regularized_attributes.attribute_latent_mapping``; keys that start with
    ``_`` are comments.  ``ValueError`` when the block or the mapping is missing or empty."""
    block = getattr(config, "regularized_attributes", None)
    if not block:
        raise ValueError("the config has no regularized_attributes block")
    named = {key: meta for key, meta in block.get("attribute_latent_mapping", {}).items() if not str(key).startswith("_")}
    if not named:
        raise ValueError("regularized_attributes.attribute_latent_mapping is missing or empty")
    return {key: int(meta["latent_channel"]) for key, meta in named.items()}


def _normalize_to_unit(data: np.ndarray) -> np.ndarray:
    """Min-max map to [0, 1]; an empty array is returned as it is, a constant one as zeros."""
    if data.size == 0:
        return data
    lo, hi = float(data.min()), float(data.max())
    if hi <= lo:
        return np.zeros_like(data)
    return (data - lo) / (hi - lo)


def channel_titles(latent_channels: int, attr_to_channel: dict[str, int]) -> list[str]:
    titles = []
    for k in range(latent_channels):
        name = next((attr for attr, ch in attr_to_channel.items() if ch == k), None)
        titles.append(f"ch {k}: {name} (regularized)" if name else f"ch {k}: unmapped")
    return titles


def save_panel(path, original: np.ndarray, reconstruction: np.ndarray, latents: np.ndarray,
               attr_to_channel: dict[str, int], image_name: str = "") -> Path:
    """Input, Reconstruction and one tile per latent channel, each min-max normalised on its own (matplotlib, Agg)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    tiles = [(np.squeeze(original), "Input", "gray"), (np.squeeze(reconstruction), "Reconstruction", "gray")]
    tiles += [(latents[k], title, "viridis") for k, title in enumerate(channel_titles(latents.shape[0], attr_to_channel))]
    cols = min(4, len(tiles))
    rows = math.ceil(len(tiles) / cols)
    fig, axes = plt.subplots(rows, cols, figsize=(3.4 * cols, 3.4 * rows), squeeze=False)
    for ax in axes.ravel():
        ax.set_axis_off()
    for ax, (data, title, cmap) in zip(axes.ravel(), tiles):
        ax.imshow(_normalize_to_unit(np.asarray(data, dtype=np.float64)), cmap=cmap, vmin=0.0, vmax=1.0)
        ax.set_title(title, fontsize=9)
        ax.set_axis_on()
        ax.set_xticks([])
        ax.set_yticks([])
    if image_name:
        fig.suptitle(f"AR-VAE channels: {image_name}")
    fig.tight_layout()
    path = Path(path)
    fig.savefig(path, dpi=110)
    plt.close(fig)
    return path


@torch.no_grad()
def encode_image(image_path: str, model, patch_size, device):
    """-> (preprocessed image [1, Hp, Wp], reconstruction [1, Hp, Wp], latent means [L, h, w]) as numpy arrays."""
    from .data import DeviceImageLoader
    batch = next(iter(DeviceImageLoader([image_path], 1, patch_size, device, shuffle=False, num_workers=1)))
    z_mu = model.encode_deterministic(batch)
    reconstruction = model.decode_stage_2_outputs(z_mu)
    if z_mu.dim() != 4:
        raise ValueError(f"Unexpected latent shape: {tuple(z_mu.shape)}")
    return batch[0].cpu().numpy(), reconstruction[0].cpu().numpy(), z_mu[0].cpu().numpy()


def main(argv=None) -> None:
    args = parse_args(argv)
    config = load_vae_config(args.config_file)
    attr_to_channel = load_attribute_mapping(config)
    device = init_device_and_seed(42)
    if args.random_init_vae:
        from .models import VAEModel
        print("[WARN] --random-init-vae: the VAE has seeded random weights, not --checkpoint")
        model = VAEModel.from_config(config.autoencoder_def).to(device).eval()
    else:
        model = load_vae_model(config, args.checkpoint, device)
    from .data import read_tiff
    original = np.asarray(read_tiff(args.image_path), dtype=np.float32)
    image, reconstruction, latents = encode_image(args.image_path, model, tuple(config.autoencoder_train["patch_size"]), device)
    out_dir = Path(args.output_dir) if args.output_dir is not None else resolve_run_dir(vars(config), args.config_file) / "ar_channels"
    out_dir.mkdir(parents=True, exist_ok=True)
    stem = Path(args.image_path).stem
    np.savez(out_dir / f"ar_channels_{stem}.npz", original=original, input=image, reconstruction=reconstruction, latents=latents)
    png = save_panel(out_dir / f"ar_channels_{stem}.png", original, reconstruction, latents, attr_to_channel,
                     Path(args.image_path).name)
    print(f"Panel written to {png}")


if __name__ == "__main__":
    main()

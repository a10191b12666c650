#!/usr/bin/env python3
"""Reconstruct a folder of TIF images with a trained VAE -- the counterpart of the reference's
``vae_scripts/inference_vae.py``.

Same CLI as ``evaluate_vae``; per image ``<output-dir>/results_tif/imageNNNN.tif`` (float32, ``[input |
reconstruction]`` side by side: the preprocessed input the model saw and ``reconstruct_deterministic`` of it) and
``<output-dir>/results_png/imageNNNN.png`` (8-bit, each half through ``normalize_batch_for_display``).  The default
output directory is ``inference_vae_<checkpoint name>``.  TIFs are written with this package's ``write_tiff``.

``--display host`` (default) normalises the PNG halves on the host, plane by plane, as the reference does; ``--display
hip`` takes the PNGs of a whole batch from one ``ops.display_planes`` launch and one uint8 copy (same arithmetic, the
percentile interpolation and the map in fp64 instead of fp32: at most one grey level apart on a few pixels).
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

from .data import write_tiff
from .utils.cli_common import (add_shared_io_args, build_inference_dataloader, init_device_and_seed, load_config_and_model,
                               resolve_inference_output_dirs)
from .utils.visualization import normalize_batch_for_display


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="VAE inference (MI355X, HIP engine)")
    add_shared_io_args(parser, output_help="Output directory (default: inference_vae_<checkpoint_name>)")
    parser.add_argument("--display", choices=("host", "hip"), default="host",
                        help="where the PNG halves are normalised: numpy on the host, or one HIP launch per batch")
    return parser.parse_args(argv)


def save_results(idx: int, input_img: torch.Tensor, recon_img: torch.Tensor, out_tif: Path, out_png: Path,
                 png: np.ndarray | None = None) -> None:
    """One result: ``input_img`` / ``recon_img`` are host tensors ``[1, H, W]``; ``png``: the finished 8-bit
    ``[H, 2 W]`` picture when it was made on the device, else it is made here."""
    from PIL import Image
    write_tiff(str(Path(out_tif) / f"image{idx:04d}.tif"),
               np.concatenate([input_img[0].numpy(), recon_img[0].numpy()], axis=1).astype(np.float32))
    if png is None:
        halves = [normalize_batch_for_display(t.unsqueeze(0))[0, 0].numpy() for t in (input_img, recon_img)]
        png = (np.concatenate(halves, axis=1) * 255).astype(np.uint8)
    Image.fromarray(png).save(Path(out_png) / f"image{idx:04d}.png")


@torch.no_grad()
def run_inference(autoencoder, dataloader, device, out_tif: Path, out_png: Path, display: str = "host") -> int:
    """-> number of images written."""
    from . import ops
    idx = 0
    for batch in dataloader:
        images = batch.to(device)
        reconstruction = autoencoder.reconstruct_deterministic(images).float()
        pngs = None
        if display == "hip":    # [b, H, 2 W] uint8: both halves of every image of the batch from one launch
            pngs = ops.display_planes(images.float().contiguous(), reconstruction.contiguous(), nsrc=2, rot90=0,
                                      dtype=torch.uint8)[0].cpu().numpy()
        images, reconstruction = images.cpu(), reconstruction.cpu()
        for i in range(images.shape[0]):
            save_results(idx, images[i], reconstruction[i], out_tif, out_png, None if pngs is None else pngs[i])
            idx += 1
    return idx


def main(argv=None) -> None:
    from . import _lib
    _lib.refuse_wrong_result_env("inference_vae.py")
    args = parse_args(argv)
    device = init_device_and_seed(args.seed)
    config, autoencoder = load_config_and_model(args.config_file, args.checkpoint, device)
    print(f"[INFO] Loaded config from {args.config_file}")
    if config.autoencoder_def["in_channels"] != 1:
        raise SystemExit("inference_vae: the TIFF pipeline produces single-channel images (in_channels must be 1)")
    output_dir, out_tif, out_png = resolve_inference_output_dirs(args.checkpoint, args.output_dir)
    print(f"[INFO] Output directory: {output_dir}")
    dataloader, image_paths = build_inference_dataloader(input_dir=args.input_dir, config=config, batch_size=args.batch_size,
                                                         num_samples=args.num_samples, num_workers=args.num_workers,
                                                         device=device)
    print(f"[INFO] Found {len(image_paths)} images in {args.input_dir}")
    print(f"[INFO] Loaded checkpoint from {args.checkpoint}")
    n = run_inference(autoencoder, dataloader, device, out_tif, out_png, display=args.display)
    print(f"Inference complete: {n} images. Results saved in: {output_dir}")
    print(f"   - TIF files: {out_tif}")
    print(f"   - PNG files: {out_png}")


if __name__ == "__main__":
    main()

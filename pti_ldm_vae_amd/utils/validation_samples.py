"""Validation pictures of a training run (reference ``vae_scripts/train_vae.py:536-549,610-626``): the first image of every
validation batch, its reconstruction and their absolute difference as float32 TIFs under
``<run_dir>/validation_samples/epoch_E/{originale,reconstruction,diff}/stepNNN.tif`` (from epoch 10 on, every 5th epoch,
turned by ``rot90(k=3)``), and one 8-bit ``[input | reconstruction | |difference|]`` triplet per 20th epoch under
``<run_dir>/triplets/`` (the reference logs it to W&B; here it is a PNG).

Nothing here synchronises inside the validation loop: ``add`` only queues device work (three ``rot90`` and, for the
triplet, one ``ops.display_planes`` launch) and keeps the results on the device; ``flush`` copies them to the host once,
after the loop's own synchronisation, and writes the files."""
from __future__ import annotations

from pathlib import Path

import torch

TIF_DIRS = ("originale", "reconstruction", "diff")      # the reference's folder names (sic)


class ValidationSampleWriter:
    def __init__(self, run_dir, start: int = 10, every: int = 5, triplet_every: int = 20):
        self.run_dir = Path(run_dir)
        self.start, self.every, self.triplet_every = int(start), int(every), int(triplet_every)
        self._tifs, self._triplet = [], None
        self._want_tifs = self._want_triplet = False

    def wants_tifs(self, epoch: int) -> bool:
        return self.every > 0 and epoch >= self.start and epoch % self.every == 0

    def wants_triplet(self, epoch: int) -> bool:
        return self.triplet_every > 0 and epoch % self.triplet_every == 0

    def begin(self, epoch: int) -> bool:
        """Start the validation pass of ``epoch`` -> whether ``add`` will keep anything."""
        self._tifs, self._triplet = [], None
        self._want_tifs, self._want_triplet = self.wants_tifs(epoch), self.wants_triplet(epoch)
        return self._want_tifs or self._want_triplet

    def add(self, step: int, images: torch.Tensor, recon: torch.Tensor) -> None:
        """``images`` / ``recon``: one validation batch ``[b, 1, h, w]`` on the device; its first image is kept."""
        if not (self._want_tifs or (self._want_triplet and self._triplet is None)):
            return
        img, rec = images[0, 0].float().contiguous(), recon[0, 0].float().contiguous()
        if self._want_tifs:
            planes = (img, rec, torch.abs(img - rec))
            self._tifs.append((step, torch.stack([torch.rot90(p, k=3, dims=[0, 1]) for p in planes])))
        if self._want_triplet and self._triplet is None:      # the reference keeps one triplet per epoch: the first step's
            from .. import ops
            canvas, _ = ops.display_planes(img[None], rec[None], nsrc=3, rot90=3, dtype=torch.uint8)
            self._triplet = (step, canvas)

    def flush(self, epoch: int) -> None:
        """Copy what ``add`` kept (one transfer per kind) and write the files."""
        from ..data import write_tiff
        parts = []
        if self._tifs:
            host = torch.stack([t for _, t in self._tifs]).cpu().numpy()
            dirs = [self.run_dir / "validation_samples" / f"epoch_{epoch}" / d for d in TIF_DIRS]
            for d in dirs:
                d.mkdir(parents=True, exist_ok=True)
            for (step, _), planes in zip(self._tifs, host):
                for d, plane in zip(dirs, planes):
                    write_tiff(str(d / f"step{step:03}.tif"), plane)
            parts.append(f"{len(self._tifs)} validation samples in {dirs[0].parent}")
        if self._triplet is not None:
            from PIL import Image
            step, canvas = self._triplet
            path = self.run_dir / "triplets" / f"val_epoch{epoch:03}_step{step:03}.png"
            path.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(canvas[0].cpu().numpy()).save(path)
            parts.append(f"triplet {path}")
        if parts:
            print(f"[INFO] Epoch {epoch}: wrote " + " and ".join(parts))
        self._tifs, self._triplet = [], None

"""Per-image cache of encoded latents on disk, byte-compatible with the reference's
(``src/pti_ldm_vae/analysis/latent_cache.py``), so that cache directories can be exchanged between the two:

    <root>/<md5("{absolute weights path}_{patch_size}")[:8]>/
        _metadata.json                                  {"images": {abs path: {"cache_key", "patient_id"}}, "model", "patch_size"}
        <md5("{absolute image path}_{mtime}")[:12]>.npz  arrays "latent" and "patient_id"

An image whose modification time changes gets a new key and is encoded again; an unreadable cache file is re-encoded.
Beyond the reference: ``get_or_encode_batch`` accepts ``encode_many(paths) -> (latents, ids)``; every miss of the call is
then gathered first and encoded in batches, instead of one image per encoder call."""
from __future__ import annotations

import hashlib
import json
import shutil
from pathlib import Path

import numpy as np


class LatentCache:
    def __init__(self, cache_root: Path = Path("cache/latents")) -> None:
        self.cache_root = Path(cache_root)
        self.cache_root.mkdir(parents=True, exist_ok=True)

    # ---- names ----
    def _get_model_signature(self, vae_weights: str, patch_size: tuple[int, int]) -> str:
        text = f"{Path(vae_weights).resolve()}_{patch_size}"
        return hashlib.md5(text.encode()).hexdigest()[:8]

    def _get_image_cache_key(self, image_path: str) -> str:
        path = Path(image_path).resolve()
        mtime = path.stat().st_mtime if path.exists() else 0
        return hashlib.md5(f"{path}_{mtime}".encode()).hexdigest()[:12]

    def _get_cache_file_path(self, image_path: str, model_signature: str) -> Path:
        folder = self.cache_root / model_signature
        folder.mkdir(parents=True, exist_ok=True)
        return folder / f"{self._get_image_cache_key(image_path)}.npz"

    def _get_metadata_path(self, model_signature: str) -> Path:
        return self.cache_root / model_signature / "_metadata.json"

    def _load_metadata(self, model_signature: str) -> dict:
        path = self._get_metadata_path(model_signature)
        if not path.exists():
            return {"images": {}}
        with open(path) as f:
            return json.load(f)

    def _save_metadata(self, model_signature: str, metadata: dict) -> None:
        with open(self._get_metadata_path(model_signature), "w") as f:
            json.dump(metadata, f, indent=2)

    # ---- lookup ----
    def get_or_encode_batch(self, image_paths: list[str], encoder_fn, vae_weights: str, patch_size: tuple[int, int],
                            group_name: str, encode_many=None) -> tuple[np.ndarray, list[str], list[str]]:
        """-> (latents ``[n, D]``, patient ids, paths) in the order of ``image_paths``; only images without a valid cache
        entry are encoded, and their entries written.  ``encoder_fn(path) -> (latent, patient_id)`` encodes one image;
        ``encode_many(paths) -> (latents, ids)``, when given, encodes all misses of this call instead."""
        signature = self._get_model_signature(vae_weights, patch_size)
        metadata = self._load_metadata(signature)
        print(f"📂 Processing {group_name} ({len(image_paths)} images)")
        print(f"   Model: {Path(vae_weights).name} (cache sig: {signature})")

        n = len(image_paths)
        latents: list = [None] * n
        ids: list = [None] * n
        misses: list[tuple[int, Path, str | None]] = []      # (position, cache file, key to record | None: keep the metadata)
        for pos, image_path in enumerate(image_paths):
            cache_file = self._get_cache_file_path(image_path, signature)
            key = self._get_image_cache_key(image_path)
            entry = metadata["images"].get(str(Path(image_path).resolve()), {})
            if cache_file.exists() and entry.get("cache_key") == key:
                try:
                    data = np.load(cache_file)
                    latents[pos], ids[pos] = data["latent"], str(data["patient_id"])
                except Exception as e:
                    print(f"   ⚠️  Cache corrupted for {Path(image_path).name}, re-encoding: {e}")
                    misses.append((pos, cache_file, None))
            else:
                misses.append((pos, cache_file, key))

        if misses:
            miss_paths = [image_paths[pos] for pos, _, _ in misses]
            if encode_many is not None:
                new_latents, new_ids = encode_many(miss_paths)
                if len(new_latents) != len(miss_paths) or len(new_ids) != len(miss_paths):
                    raise ValueError(f"encode_many returned {len(new_latents)} latents / {len(new_ids)} ids for "
                                     f"{len(miss_paths)} images")
            else:
                pairs = [encoder_fn(p) for p in miss_paths]
                new_latents, new_ids = [p[0] for p in pairs], [p[1] for p in pairs]
            for (pos, cache_file, key), latent, patient_id in zip(misses, new_latents, new_ids):
                latent, patient_id = np.asarray(latent), str(patient_id)
                np.savez(cache_file, latent=latent, patient_id=patient_id)
                if key is not None:
                    metadata["images"][str(Path(image_paths[pos]).resolve())] = {"cache_key": key, "patient_id": patient_id}
                latents[pos], ids[pos] = latent, patient_id
            metadata["model"] = str(Path(vae_weights).name)
            metadata["patch_size"] = list(patch_size)
            self._save_metadata(signature, metadata)

        print(f"   ✅ {n - len(misses)} from cache, 🔄 {len(misses)} newly encoded")
        return np.array(latents), ids, list(image_paths)

    # ---- housekeeping ----
    def clear_cache(self, model_signature: str | None = None) -> None:
        """Remove one model's cache directory, or (``None``) everything under the root."""
        if model_signature is None:
            if self.cache_root.exists():
                shutil.rmtree(self.cache_root)
                self.cache_root.mkdir(parents=True, exist_ok=True)
            print(f"🗑️  Cleared all cache in {self.cache_root}")
            return
        folder = self.cache_root / model_signature
        if folder.exists():
            shutil.rmtree(folder)
        print(f"🗑️  Cleared cache for model {model_signature}")

    def get_cache_stats(self) -> dict[str, dict]:
        """-> {model signature: {"model", "patch_size", "num_images", "cache_size_mb"}}."""
        stats: dict[str, dict] = {}
        if not self.cache_root.exists():
            return stats
        for folder in self.cache_root.iterdir():
            if not folder.is_dir():
                continue
            metadata = self._load_metadata(folder.name)
            size = sum(f.stat().st_size for f in folder.glob("*.npz") if f.is_file())
            stats[folder.name] = {"model": metadata.get("model", "unknown"), "patch_size": metadata.get("patch_size", []),
                                  "num_images": len(metadata.get("images", {})), "cache_size_mb": size / (1024 * 1024)}
        return stats

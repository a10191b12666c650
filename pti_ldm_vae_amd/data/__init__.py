"""Input pipeline of the VAE training path: TIFF files -> device batches."""
from .loader import (DeviceImageLoader, create_regression_dataloaders, create_vae_dataloaders, create_vae_inference_dataloader,
                     list_inference_paths, list_tif_paths, shard_indices, split_paths)
from .tiff import read_tiff, write_tiff

__all__ = ["DeviceImageLoader", "create_regression_dataloaders", "create_vae_dataloaders", "create_vae_inference_dataloader",
           "list_inference_paths", "list_tif_paths", "shard_indices", "split_paths", "read_tiff", "write_tiff"]

# evaluation / inference of the regression head (appended: the two factories of dataloaders.py:725-795)
from .loader import create_regression_eval_dataloader, create_regression_inference_dataloader  # noqa: E402

__all__ += ["create_regression_eval_dataloader", "create_regression_inference_dataloader"]

# train-time augmentation
from .augment import AugmentPolicy, draw_params  # noqa: E402

__all__ += ["AugmentPolicy", "draw_params"]

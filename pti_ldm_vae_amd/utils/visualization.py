"""Display helpers of the inference script (reference ``src/pti_ldm_vae/utils/visualization.py:6-40``).  I/O-side code:
it runs on the host in numpy, once per written image, not on the evaluation's hot path."""
from __future__ import annotations

import numpy as np
import torch


def normalize_batch_for_display(tensor: torch.Tensor, low: int = 2, high: int = 98) -> torch.Tensor:
    """``[B, C, H, W]`` -> fp32 ``[B, C, H, W]`` in [0, 1] on the host, plane by plane: the NON-ZERO pixels are mapped
    linearly from their ``low`` .. ``high`` percentiles to 0 .. 1 (``(v - p_low) / (p_high - p_low + 1e-8)``, clipped),
    exact zeros (the background) stay 0, and results below 1e-3 are set to 0.  A plane without a non-zero pixel is all 0."""
    planes = tensor.detach().cpu().numpy()
    out = np.zeros(planes.shape, dtype=planes.dtype)
    for b in range(planes.shape[0]):
        for c in range(planes.shape[1]):
            plane = planes[b, c]
            foreground = plane != 0
            if not foreground.any():
                continue
            values = plane[foreground]
            p_low, p_high = np.percentile(values, low), np.percentile(values, high)
            out[b, c][foreground] = np.clip((values - p_low) / (p_high - p_low + 1e-8), 0, 1)
    out[out < 1e-3] = 0.0
    return torch.from_numpy(out)

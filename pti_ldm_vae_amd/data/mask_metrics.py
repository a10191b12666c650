"""Geometric attributes of edente / dente mask pairs -- the arithmetic of the reference's
``vae_scripts/compute_mask_metrics.py`` (``compute_bbox`` :38-45, ``compute_edente_widths`` :48-61,
``compute_dente_width`` :64-68, ``pixel_offsets_mm`` :76-78, the pairing in ``process_dataset`` :171-196) on the device:
the per-pixel work of a whole batch of masks is one ``ops.mask_geometry`` launch per side.

Both masks are binarised as ``pixel > 0``.  The edente mask gives the bounding box of ALL its foreground pixels (the
reference's docstring speaks of the largest connected component, its code takes none) and ``samples`` widths at rows
spread over the box, lowest row first; the dente mask gives one width per offset counted up from its last row.  A width
is ``last foreground column - first + 1`` of the row, gaps included, 0 for an empty row.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from .. import ops

EMPTY_MASK = "Mask does not contain any foreground pixels"   # the reference's ValueError text (compute_bbox)
_PASS_THROUGH = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}   # dtype -> `elem` of the kernel


def pixel_offsets_mm(heights_mm, pixel_size_mm: float) -> list[int]:
    """Millimetres above the last row -> pixel rows; Python ``round`` (half to even), as the reference."""
    return [int(round(h / pixel_size_mm)) for h in heights_mm]


@functools.lru_cache(maxsize=8)
def _sample_row_table(max_h: int, samples: int) -> np.ndarray:
    table = np.zeros((max_h + 1, max(samples, 0)), dtype=np.int32)
    if samples > 0:
        for h in range(max_h + 1):
            table[h] = np.linspace(0, h, samples + 2, dtype=int)[1:-1][::-1]
    table.setflags(write=False)
    return table


def sample_row_table(max_h: int, samples: int) -> np.ndarray:
    """int32 ``[max_h + 1, samples]``: row ``h`` holds the sampled rows of a bounding box of height ``h``, relative to the
    box's first row and already reversed (entry 0 is the lowest row) -- literally the reference's
    ``np.linspace(0, h, samples + 2, dtype=int)[1:-1][::-1]``.  numpy truncates a float64 product there, which is NOT
    ``i * h // (samples + 1)`` (samples 13, h 122: 60 against 61), so the expression is tabulated on the host with numpy
    itself and the kernel only looks rows up.  ``samples <= 0`` gives a table without columns.  Read-only, cached."""
    if max_h < 0:
        raise ValueError(f"sample_row_table: max_h must be >= 0, got {max_h}")
    return _sample_row_table(int(max_h), int(samples))


def pack_masks(masks) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """2-D arrays of any sizes -> ``(buffer, offsets, hw, elem)``: the flat concatenation, the int64 element offset and
    int32 ``{H, W}`` of every mask, and the kernel's element code.  A batch that is uint8, uint16 or float32 throughout
    is passed through untouched (the kernel thresholds it); any other dtype, or a mixed batch, is binarised here as
    ``a > 0`` in the array's own dtype (so a tiny float64 cannot underflow through a cast) to uint8."""
    arrays = [np.asarray(m) for m in masks]
    for a in arrays:
        if a.ndim != 2:
            raise ValueError(f"pack_masks: expected 2-D masks, got shape {a.shape}")
    kinds = {a.dtype.newbyteorder("=") for a in arrays}
    if len(kinds) == 1 and next(iter(kinds)) in _PASS_THROUGH:
        dtype = next(iter(kinds))
    else:
        dtype = np.dtype(np.uint8)
        arrays = [(a > 0).astype(np.uint8) for a in arrays]
    sizes = np.array([a.size for a in arrays], dtype=np.int64)
    offsets = np.zeros(len(arrays), dtype=np.int64)
    np.cumsum(sizes[:-1], out=offsets[1:])
    hw = np.array([a.shape for a in arrays], dtype=np.int32).reshape(len(arrays), 2)
    buffer = np.empty(int(sizes.sum()), dtype=dtype)
    for a, o in zip(arrays, offsets):
        buffer[o:o + a.size] = a.reshape(-1)
    return buffer, offsets, hw, _PASS_THROUGH[dtype]


def _geometry(masks, samples: int, bottom_offsets, device):
    """One launch over ``masks`` -> host int32 arrays ``(bbox [b, 4], bbox_widths [b, samples], bottom_widths)``."""
    buffer, offsets, hw, elem = pack_masks(masks)
    # the table of a larger bound contains that of a smaller one: round up so that batches share the cached table
    max_h = min(ops.MASK_ROW_CAP, -(-max(int(hw[:, 0].max()), 1) // 256) * 256)
    if buffer.size == 0:
        buffer = np.zeros(1, dtype=buffer.dtype)   # only masks without pixels: the kernel reads none of it

    def dev(a):
        return torch.from_numpy(np.array(a)).to(device)   # a copy: the cached table is read-only

    out = ops.mask_geometry(dev(buffer), dev(offsets), dev(hw), elem=elem, max_h=max_h,
                            sample_rows=dev(sample_row_table(max_h, samples)),
                            bottom_offsets=dev(np.asarray(bottom_offsets, dtype=np.int32).reshape(-1)))
    return tuple(t.cpu().numpy() for t in out)


def _clamp_i32(offsets) -> list[int]:
    """Offsets as int32: anything beyond a mask's height clamps to its first / last row anyway."""
    return [max(-(2 ** 31) + 1, min(2 ** 31 - 1, int(o))) for o in offsets]


def mask_attributes(edente_masks, dente_masks, *, samples: int = 5, bottom_offsets=(33, 67, 93, 120, 147), device="cuda"):
    """Attributes of mask pairs: ``edente_masks[i]`` and ``dente_masks[i]`` are the two 2-D arrays of pair ``i``.
    -> one entry per pair: ``(attrs_edente, attrs_dente)``, two dicts ``{"height_0": h, "width_0": ..}`` in the
    reference's key order (both carry the EDENTE bounding-box height), or a ``str`` saying why the pair is skipped
    (an edente mask without foreground: the reference's message).  One ``ops.mask_geometry`` launch per side."""
    edente_masks, dente_masks = list(edente_masks), list(dente_masks)
    if len(edente_masks) != len(dente_masks):
        raise ValueError(f"mask_attributes: {len(edente_masks)} edente masks for {len(dente_masks)} dente masks")
    if not edente_masks:
        return []
    samples = max(int(samples), 0)
    ed_box, ed_widths, _ = _geometry(edente_masks, samples, (), device)
    de_box, _, de_widths = _geometry(dente_masks, 0, _clamp_i32(bottom_offsets), device)
    out = []
    for i, (ed, de) in enumerate(zip(edente_masks, dente_masks)):
        bad = next((m for m, box in ((ed, ed_box[i]), (de, de_box[i])) if box[0] == -2), None)
        if bad is not None:
            out.append(f"Mask of shape {tuple(np.shape(bad))} is not supported (1..{ops.MASK_ROW_CAP} rows, 1 or more columns)")
        elif ed_box[i, 0] < 0:
            out.append(EMPTY_MASK)
        else:
            height = int(ed_box[i, 3])
            attrs_edente, attrs_dente = {"height_0": height}, {"height_0": height}
            attrs_edente.update((f"width_{k}", int(v)) for k, v in enumerate(ed_widths[i]))
            attrs_dente.update((f"width_{k}", int(v)) for k, v in enumerate(de_widths[i]))
            out.append((attrs_edente, attrs_dente))
    return out

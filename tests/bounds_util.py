"""Helpers of the memory-extent tests (tests/test_gpu_wgrad_workspace.py, tests/test_gpu_kernel_bounds.py): inputs inside
poisoned buffers, outputs and workspaces with canaries round them, and the extent a kernel really wrote.

A kernel that reads outside a tensor handed to it through ``guarded`` picks up poison, so its result differs from the run on
plain tensors; one that writes outside a ``with_canary`` view destroys a canary word.  Every byte such a slip could reach
(4096 bytes either side, or whatever ``extra_bytes`` asks for behind the view) belongs to the helper's own allocation.

Plain torch, no GPU needed: tests/test_bounds_util_cpu.py runs everything here on CPU tensors.
"""
from collections import namedtuple

import torch

PAD_BYTES = 4096                 # poison / canary bytes in front of every view (a multiple of 256: an allocator-fresh
                                 # tensor's alignment is kept; misaligned pointers are not what these tests are about)
CANARY_I, CANARY_F = 0x5A5A5A5A, -12345.678
POISON_NAN, POISON_BIG = float("nan"), 16384.0      # 2^14 is bf16- and fp16-representable; it is written with both signs
POISONS = (POISON_NAN, POISON_BIG)                  # the finite pass: max-style instructions drop a NaN operand

Canary = namedtuple("Canary", "view flat lead count value")


def _fill_poison(flat, poison):
    if not flat.dtype.is_floating_point:           # fixed-point statistics: a huge word for NaN, the value itself otherwise
        flat.fill_(CANARY_I << 24 if poison != poison else int(poison) << 16)
        return
    flat.fill_(poison)
    if poison == poison:
        flat[1::2] = -poison


def guarded(dev, t, poison):
    """``t`` copied into the middle of a larger flat buffer of its dtype with PAD_BYTES of ``poison`` in front and behind
    (NaN, or +/-``poison`` alternating) -> the contiguous view of t's shape."""
    item = t.element_size()
    lead = PAD_BYTES // item
    flat = torch.empty(2 * lead + t.numel(), dtype=t.dtype, device=dev)
    _fill_poison(flat, poison)
    view = flat[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def canary_value(dtype):
    return CANARY_F if dtype.is_floating_point else CANARY_I


def with_canary(dev, shape, dtype, fill, extra_bytes=PAD_BYTES):
    """An output or workspace view of ``shape`` pre-filled with ``fill``, with PAD_BYTES of canary words in front and
    ``extra_bytes`` of them behind -> Canary handle (``.view`` goes to the kernel; ``intact(handle)`` afterwards)."""
    item = torch.empty(0, dtype=dtype).element_size()
    if extra_bytes < item or extra_bytes % item:
        raise ValueError("with_canary: extra_bytes must be a positive multiple of the element size")
    count = 1
    for s in shape:
        count *= int(s)
    lead = PAD_BYTES // item
    flat = torch.empty(lead + count + extra_bytes // item, dtype=dtype, device=dev)
    value = canary_value(dtype)
    flat.fill_(value)
    view = flat[lead:lead + count].view(tuple(shape))
    view.fill_(fill)
    return Canary(view, flat, lead, count, value)


def intact(handle, end=None):
    """Whether every canary word round the view still holds its value.  ``end``: treat only the first ``end`` elements of
    the view as the view (everything behind them must then be canary too)."""
    end = handle.count if end is None else int(end)
    ref = torch.tensor(handle.value, dtype=handle.flat.dtype, device=handle.flat.device)
    front, back = handle.flat[:handle.lead], handle.flat[handle.lead + end:]
    return bool((front == ref).all()) and bool((back == ref).all())


def extent(ws_flat, sentinel):
    """1 + the index of the last element of the flat tensor that differs from ``sentinel`` (0: none does).  A NaN sentinel
    matches any NaN."""
    flat = ws_flat.reshape(-1)
    if sentinel != sentinel:
        diff = ~torch.isnan(flat)
    else:
        diff = flat != torch.tensor(sentinel, dtype=flat.dtype, device=flat.device)
    idx = torch.nonzero(diff)
    return 0 if idx.numel() == 0 else int(idx[-1]) + 1

"""Host-side launchers: validate torch tensors, hand raw pointers to the C-ABI.

Every function launches on ``torch.cuda.current_stream()`` of the calling thread (so the
autograd engine's backward thread and side streams are respected) and never synchronises.
Shapes are checked HERE, before any pointer reaches a kernel.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import namedtuple

import torch

from . import _lib as L
from ._lib import (PTI_CONV_S1, PTI_CONV_S2PAD, PTI_CONV_UP2, PTI_CONV_ZINS, PTI_PRO_GN, PTI_PRO_GN_SILU,
                   PTI_PRO_NONE, ConvDesc)

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
I64 = torch.int64
I32 = torch.int32
I16 = torch.int16
STAT_SCALE = 65536.0   # GroupNorm statistics are Q47.16 fixed-point int64 {sum, sum of squares} (pti_common.h)
ACT16 = (BF16, F16)   # storage formats of a forward activation (flag derived from the tensor's dtype)
LATENT_BWD_MAX_BLOCKS = 512   # PTI_LATENT_BWD_MAX_BLOCKS / PTI_VAE_LOSS_MAX_BLOCKS / PTI_POST_QUANT_BWD_MAX_BLOCKS of
VAE_LOSS_MAX_BLOCKS = 1024    # include/pti_vae.h
POST_QUANT_BWD_MAX_BLOCKS = 256


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """hipStream_t of torch's current stream on the current device.  The public route (torch.cuda.current_stream()
    builds a Stream object, resolves the device index through several Python layers) cost ~8 us per call x ~280 calls
    per training step = a quarter of the step's host time; the two C entry points behind it cost ~0.3 us."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype, name, dims=None):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA(HIP) tensor")
    if (t.dtype not in dtype) if isinstance(dtype, tuple) else (t.dtype != dtype):
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name}: expected {dims} dims, got {tuple(t.shape)}")


def _out(out, shape, dtype, device, name, chk_name=None, rank=True, msg=None):
    """The caller-supplied output ``out`` checked (contiguous ``dtype`` of ``shape`` on ``device``), or a new tensor when
    there is none.  ``chk_name`` / ``rank`` / ``msg``: the site's own name in _chk's errors, whether _chk sees the rank, and
    the text of the shape / device error, where a site's differ from the common ones."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _chk(out, dtype, chk_name or name, len(shape) if rank else None)
    if tuple(out.shape) != tuple(shape) or out.device != device:
        raise ValueError(msg or f"{name} must be {list(shape)} on {device}")
    return out


_SCRATCH = {}


def _scratch(kind, shape, floats, device, stream):
    """fp32 scratch of ``floats`` elements, cached per (kind, device, stream, shape): launches on one stream are ordered,
    so they can share it; two streams never do."""
    key = (kind, device.index, stream) + tuple(shape)
    ws = _SCRATCH.get(key)
    if ws is None:
        ws = _SCRATCH[key] = torch.empty(floats, dtype=F32, device=device)
    return ws


def conv_out_hw(h, w, mode):
    if mode == PTI_CONV_S1:
        return h, w
    if mode == PTI_CONV_S2PAD:
        return (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1
    return 2 * h, 2 * w


def pack_conv_weight(ws, ksize, mode=PTI_CONV_S1, flip=False, out=None, f16=False):
    """fp32 [cout,cin,k,k] (or nn.Linear [cout,cin]) master weight(s) -> MFMA-packed bf16 (``f16``: IEEE fp16, the
    operand of forward launches with ``w_f16``)."""
    ws = list(ws) if isinstance(ws, (list, tuple)) else [ws]
    w0 = ws[0]
    cout, cin = w0.shape[0], w0.shape[1]
    for w in ws:
        _chk(w, F32, "weight")
        if w.shape[0] != cout or w.shape[1] != cin or w.numel() != cout * cin * ksize * ksize:
            raise ValueError("pack_conv_weight: inconsistent weight shapes")
    nbytes = L.lib().pti_conv_packed_bytes(cout * len(ws), cin, ksize, mode)
    if nbytes == 0:
        raise ValueError(f"pack_conv_weight: unsupported cout={cout} cin={cin} k={ksize}")
    if out is None:
        out = torch.empty(nbytes // 2, dtype=F16 if f16 else BF16, device=w0.device)
    elif out.numel() * 2 != nbytes or out.dtype != (F16 if f16 else BF16):
        raise ValueError("pack_conv_weight: bad out size")
    arr = (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
    L.check(L.lib().pti_conv_pack_weights(arr, len(ws), _ptr(out), cout, cin, ksize, mode, int(flip), int(f16), _stream()),
            "pti_conv_pack_weights")
    return out


class DirectRepack:
    """The derived operands of up to DIRECT_REPACK_MAX degenerate-channel convs as ONE launch (csrc/conv_direct.hip,
    ``pti_direct_repack``).  ``entries``: dicts with w (fp32 [cout,cin,3,3]) and optionally b, w_tck, w_tck_t, wpad (zeroed
    fp32 [cout', pad_cin, 3, 3], cout' >= cout), bpad.  Every tensor lives at a fixed address (parameter arena views /
    buffers allocated once), so the table is built once."""

    def __init__(self, entries):
        if not 1 <= len(entries) <= L.DIRECT_REPACK_MAX:
            raise ValueError(f"DirectRepack: 1..{L.DIRECT_REPACK_MAX} entries")
        self.table = L.DirectRepackTable()
        self.table.n = len(entries)
        self._keep = entries
        for i, e in enumerate(entries):
            w = e["w"]
            _chk(w, F32, "w", 4)
            cout, cin = w.shape[0], w.shape[1]
            if w.shape[2] != 3 or w.shape[3] != 3:
                raise ValueError("DirectRepack: 3x3 weights")
            for k in ("b", "w_tck", "w_tck_t", "wpad", "bpad"):
                if e.get(k) is not None:
                    _chk(e[k], F32, k)
            wpad = e.get("wpad")
            pad_cin = 0
            if wpad is not None:
                pad_cin = wpad.shape[1]
                if wpad.dim() != 4 or wpad.shape[0] < cout or pad_cin < cin or wpad.shape[2:] != w.shape[2:]:
                    raise ValueError("DirectRepack: wpad shape")
            for k, size in (("w_tck", cout * cin * 9), ("w_tck_t", cout * cin * 9), ("bpad", cout)):
                if e.get(k) is not None and e[k].numel() < size:
                    raise ValueError(f"DirectRepack: {k} too small")
            if e.get("bpad") is not None and (e.get("b") is None or e["b"].numel() != cout):
                raise ValueError("DirectRepack: bpad needs b")
            self.table.e[i] = L.DirectRepackEntry(_ptr(w), _ptr(e.get("b")), _ptr(e.get("w_tck")), _ptr(e.get("w_tck_t")),
                                                  _ptr(wpad), _ptr(e.get("bpad")), cout, cin, pad_cin, 0)

    def run(self):
        L.check(L.lib().pti_direct_repack(C.byref(self.table), _stream()), "pti_direct_repack")


def _chk_stats(t, count, name):
    _chk(t, I64, name)
    if t.numel() != count:
        raise ValueError(f"{name}: expected {count} fixed-point sums, got {t.numel()}")


def _chk_prologue(who, in_stats, gamma, beta, n, groups, cin):
    _chk_stats(in_stats, n * groups * 2, "in_stats")
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        _chk(t, F32, nm)
        if t.numel() != cin:
            raise ValueError(f"{who}: {nm} size")


# Set to a list to make the MFMA conv / weight-gradient launchers record (kernel name, algorithmic flops, bytes, start
# event, end event, shape) per launch on the current stream -- used by bench.py for the roofline line and its per-shape
# table; None costs nothing.  The kernel name is the symbol the HIP runtime reports for the launch
# (pti_last_kernel_name), shortened the way tools/pmc_traffic.py shortens rocprofv3's Kernel_Name column.
KERNEL_PROFILE = None
_MODE_NAME = {PTI_CONV_S1: "s1", PTI_CONV_S2PAD: "s2", PTI_CONV_UP2: "up2", PTI_CONV_ZINS: "zins"}


def last_kernel_name() -> str:
    name = (L.lib().pti_last_kernel_name() or b"").decode()
    name = name.replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):       # drop the trailing argument list, keep template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i].strip()
    return name.strip()


def _prof_begin(prof):
    """Open a KERNEL_PROFILE record: the start event goes onto the current stream right before the launch to be timed.
    The launchers call this only when profiling is on (``prof`` is the list)."""
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    return prof, e0, e1


def _prof_end(rec, flops, nbytes, shape):
    """Close it right after that launch, before any further pti_* call replaces the kernel name."""
    prof, e0, e1 = rec
    e1.record()
    prof.append((last_kernel_name(), flops, nbytes, e0, e1, shape))


def stats_to_float(stats):
    """Fixed-point {sum, sumsq} -> float64 tensor of the same shape (tests, diagnostics)."""
    return stats.double() / STAT_SCALE


def gn_stats(x, groups, stats=None):
    """x: [N,H,W,C] bf16|fp16 -> stats [N,G,2] int64 Q47.16 {sum, sumsq} (accumulated into ``stats`` if given)."""
    _chk(x, ACT16, "x", 4)
    n, h, w, c = x.shape
    if stats is None:
        stats = torch.zeros(n, groups, 2, dtype=I64, device=x.device)
    else:
        _chk_stats(stats, n * groups * 2, "stats")
    L.check(L.lib().pti_gn_stats(_ptr(x), _ptr(stats), n, h * w, c, groups, int(x.dtype == F16), _stream()),
            "pti_gn_stats")
    return stats


def conv_mfma(x, w_packed, bias, y, *, cout, ksize=3, mode=PTI_CONV_S1, prologue=PTI_PRO_NONE, in_stats=None,
              gamma=None, beta=None, groups=0, eps=1e-6, residual=None, out_stats=None, out_groups=0, act_out=None,
              pool2=False, relu=False):
    """``act_out`` (optional, bf16, x's shape): also write prologue(x) for the weight-gradient pass to reuse.
    ``pool2``: y is [n, ho/2, wo/2, cout], the 2x2 sum pool of the conv output (fused nearest-2x up-sampling backward).
    ``relu``: y = max(conv + bias, 0) (plain fp16 forward launches: the perceptual network's Fire modules)."""
    _chk(x, ACT16, "x", 4)
    _chk(y, ACT16, "y", 4)
    n, h, w, cin = x.shape
    if act_out is not None:
        _chk(act_out, BF16, "act_out", 4)
        if act_out.shape != x.shape:
            raise ValueError("conv_mfma: act_out shape")
    ho, wo = conv_out_hw(h, w, mode)
    yshape = (n, ho // 2, wo // 2, cout) if pool2 else (n, ho, wo, cout)
    if tuple(y.shape) != yshape:
        raise ValueError(f"conv_mfma: y shape {tuple(y.shape)} != {yshape}")
    if w_packed.numel() != cout * cin * ksize * ksize or w_packed.dtype not in (BF16, F16):
        raise ValueError("conv_mfma: packed weight size/dtype mismatch")
    w_f16 = w_packed.dtype == F16   # fp16-packed weights: the MFMA multiplies fp16 operands (forward, fp16 storage)
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() != cout:
            raise ValueError("conv_mfma: bias size")
    if prologue != PTI_PRO_NONE:
        _chk_prologue("conv_mfma", in_stats, gamma, beta, n, groups, cin)
    if residual is not None:
        _chk(residual, ACT16, "residual", 4)
        if residual.shape != y.shape or pool2:
            raise ValueError("conv_mfma: residual shape")
    if out_stats is not None:
        _chk_stats(out_stats, n * out_groups * 2, "out_stats")
    d = ConvDesc(n=n, h=h, w=w, cin=cin, ho=ho, wo=wo, cout=cout, ksize=ksize, mode=mode, prologue=prologue,
                 groups=groups, add_residual=int(residual is not None), accum_stats=int(out_stats is not None),
                 out_groups=out_groups, eps=eps, in_f16=int(x.dtype == F16),
                 res_f16=int(residual is not None and residual.dtype == F16), out_f16=int(y.dtype == F16),
                 pool2x2_out=int(pool2), w_f16=int(w_f16), relu_out=int(relu))
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    if act_out is not None:
        L.check(L.lib().pti_conv2d_mfma_saveact(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(in_stats), _ptr(gamma),
                                                _ptr(beta), _ptr(residual), _ptr(y), _ptr(out_stats), _ptr(act_out),
                                                C.byref(d), _stream()), "pti_conv2d_mfma_saveact")
    else:
        L.check(L.lib().pti_conv2d_mfma(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(in_stats), _ptr(gamma), _ptr(beta),
                                        _ptr(residual), _ptr(y), _ptr(out_stats), C.byref(d), _stream()),
                "pti_conv2d_mfma")
    if rec is not None:
        # algorithmic work; the zero-insert data gradient only has 1/4 useful taps per output pixel
        flops = 2.0 * n * ho * wo * cout * cin * ksize * ksize * (0.25 if mode == PTI_CONV_ZINS else 1.0)
        # algorithmic bytes: read the input once (16-bit), write the output once (+ residual read, + side output)
        nbytes = 2.0 * (x.numel() * (2 if act_out is not None else 1) + y.numel() * (2 if residual is not None else 1))   # (pooled y counted as stored)
        kind = "conv fwd" if x.dtype == F16 or prologue != PTI_PRO_NONE else "conv dgrad"
        _prof_end(rec, flops, nbytes, (kind, cin, cout, ho, wo, ksize, _MODE_NAME[mode], n))
    return y


def _strides4(t, layout):
    """element strides (n,h,w,c) of a 4-D tensor given as 'nchw' or 'nhwc'."""
    s = t.stride()
    return (s[0], s[2], s[3], s[1]) if layout == "nchw" else (s[0], s[1], s[2], s[3])


def conv_direct(x, w_tck, bias, y, *, n, h, w, cin, cout, ksize=3, x_layout="nhwc", y_layout="nhwc",
                prologue=PTI_PRO_NONE, in_stats=None, gamma=None, beta=None, groups=0, eps=1e-6):
    """Degenerate-channel stride-1 conv.  ``w_tck`` fp32 [k*k, cin, cout].  The narrow side may be
    fp32 (any strides, e.g. the user's NCHW tensor); the wide side is dense NHWC bf16."""
    _chk(w_tck, F32, "w_tck")
    if w_tck.numel() != ksize * ksize * cin * cout:
        raise ValueError("conv_direct: weight size")
    if x.numel() != n * h * w * cin or y.numel() != n * h * w * cout:
        raise ValueError("conv_direct: tensor sizes do not match n,h,w,cin,cout")
    if prologue != PTI_PRO_NONE:
        _chk_stats(in_stats, n * groups * 2, "in_stats")
    d = ConvDesc(n=n, h=h, w=w, cin=cin, ho=h, wo=w, cout=cout, ksize=ksize, mode=PTI_CONV_S1, prologue=prologue,
                 groups=groups, eps=eps, in_f32=int(x.dtype == F32), out_f32=int(y.dtype == F32),
                 in_f16=int(x.dtype == F16), out_f16=int(y.dtype == F16))
    d.in_stride = (C.c_int64 * 4)(*_strides4(x, x_layout))
    d.out_stride = (C.c_int64 * 4)(*_strides4(y, y_layout))
    if cout % 32 == 0 and cin <= 16:
        if y.dtype not in ACT16 or not y.is_contiguous() or y_layout != "nhwc":
            raise ValueError("conv_direct: wide output must be dense NHWC bf16/fp16")
    else:
        if x.dtype not in ACT16 or not x.is_contiguous() or x_layout != "nhwc":
            raise ValueError("conv_direct: wide input must be dense NHWC bf16/fp16")
    L.check(L.lib().pti_conv2d_direct(_ptr(x), _ptr(w_tck), _ptr(bias), _ptr(in_stats), _ptr(gamma), _ptr(beta),
                                      _ptr(y), C.byref(d), _stream()), "pti_conv2d_direct")
    return y


def wgrad_direct(wide, narrow, dw, *, n, h, w, cw, cn, ksize, sgn, narrow_layout, dw_strides, dbias_wide=None,
                 dbias_narrow=None, prologue=PTI_PRO_NONE, in_stats=None, gamma=None, beta=None, groups=0, eps=1e-6,
                 workspace=None):
    """dw[tap,cw,k] += sum_p narrow[p,k] * T(wide)[p + sgn*tap, cw]; dw_strides = (tap, cw, k) element
    strides into the fp32 OIHW gradient ``dw`` (must be zero-initialised or hold a running sum)."""
    _chk(wide, ACT16, "wide", 4)
    _chk(dw, F32, "dw")
    if prologue != PTI_PRO_NONE:
        _chk_stats(in_stats, n * groups * 2, "in_stats")
    ns = (C.c_int64 * 4)(*_strides4(narrow, narrow_layout))
    ws = workspace if workspace is not None else wgrad_workspace(wide.device)
    L.check(L.lib().pti_wgrad_direct(_ptr(wide), _ptr(narrow), _ptr(dw), _ptr(dbias_wide), _ptr(dbias_narrow),
                                     _ptr(in_stats), _ptr(gamma), _ptr(beta), n, h, w, cw, cn, ksize, sgn, prologue,
                                     groups, eps, int(narrow.dtype == F32), int(wide.dtype == F16), ns, dw_strides[0],
                                     dw_strides[1],
                                     dw_strides[2], _ptr(ws), ws.numel() * 4, _stream()), "pti_wgrad_direct")
    return dw


_WS = {}


def wgrad_workspace(device, nbytes=int(os.environ.get("PTI_WGRAD_WORKSPACE_MB", "256")) << 20):
    """One reusable split-K workspace per device (slabs of fp32 partial weight gradients).  256 MB by default: a 256 -> 256
    layer's slab is 2.4 MB per pixel split, and a batched launch of 16 such layers that can afford only one or two splits
    per layer has fewer workgroups than the chip has CUs (round 2's 48 MB did that to the AR model's batches)."""
    key = (device.index if device.index is not None else torch.cuda.current_device())
    ws = _WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(nbytes // 4, dtype=F32, device=device)
        _WS[key] = ws
    return ws


def conv_wgrad_mfma(x, dy, dw, dbias, *, ksize=3, mode=PTI_CONV_S1, prologue=PTI_PRO_NONE, in_stats=None, gamma=None,
                    beta=None, groups=0, eps=1e-6, accumulate=False, workspace=None):
    _chk(x, ACT16, "x", 4)
    _chk(dy, BF16, "dy", 4)
    _chk(dw, F32, "dw")
    n, h, w, cin = x.shape
    ho, wo = conv_out_hw(h, w, mode)
    cout = dy.shape[3]
    if tuple(dy.shape) != (n, ho, wo, cout):
        raise ValueError(f"conv_wgrad_mfma: dy shape {tuple(dy.shape)} != {(n, ho, wo, cout)}")
    if dw.numel() != cout * cin * ksize * ksize:
        raise ValueError("conv_wgrad_mfma: dw size")
    if dbias is not None:
        _chk(dbias, F32, "dbias")
        if dbias.numel() != cout:
            raise ValueError("conv_wgrad_mfma: dbias size")
    if prologue != PTI_PRO_NONE:
        _chk_prologue("conv_wgrad_mfma", in_stats, gamma, beta, n, groups, cin)
    ws = workspace if workspace is not None else wgrad_workspace(x.device)
    d = ConvDesc(n=n, h=h, w=w, cin=cin, ho=ho, wo=wo, cout=cout, ksize=ksize, mode=mode, prologue=prologue,
                 groups=groups, eps=eps, in_f16=int(x.dtype == F16))
    prof = KERNEL_PROFILE
    if prof is None:
        L.check(L.lib().pti_conv_wgrad_mfma(_ptr(x), _ptr(dy), _ptr(in_stats), _ptr(gamma), _ptr(beta), _ptr(dw),
                                            _ptr(dbias), _ptr(ws), ws.numel() * 4, int(accumulate), C.byref(d),
                                            _stream()), "pti_conv_wgrad_mfma")
        return dw
    # profiling: the same two launches through the two-call form, with events around the partial (MFMA) kernel only
    splits = C.c_int(0)
    rec = _prof_begin(prof)
    L.check(L.lib().pti_conv_wgrad_mfma_partials(_ptr(x), _ptr(dy), _ptr(in_stats), _ptr(gamma), _ptr(beta), _ptr(ws),
                                                 ws.numel() * 4, C.byref(d), C.byref(splits), _stream()),
            "pti_conv_wgrad_mfma_partials")
    # algorithmic bytes: x and dy read once (16-bit); dw itself is negligible (the split-K slabs are not algorithmic)
    _prof_end(rec, 2.0 * n * ho * wo * cout * cin * ksize * ksize, 2.0 * (x.numel() + dy.numel()),
              ("conv wgrad", cin, cout, ho, wo, ksize, _MODE_NAME[mode], n))
    L.check(L.lib().pti_conv_wgrad_reduce(_ptr(ws), splits.value, _ptr(dw), _ptr(dbias), int(accumulate), C.byref(d),
                                          _stream()), "pti_conv_wgrad_reduce")
    return dw


def wgrad_batch_eligible(x, dy, ksize, mode, prologue):
    """Whether pti_conv_wgrad_mfma_batched can take this weight gradient: plain stride-1 3x3, bf16 x without prologue."""
    return (ksize == 3 and mode == PTI_CONV_S1 and prologue == PTI_PRO_NONE and x.dtype == BF16 and dy.dtype == BF16
            and x.shape[3] % 32 == 0 and dy.shape[3] % 32 == 0 and x.numel() * 2 < (1 << 31) and dy.numel() * 2 < (1 << 31))


def conv_wgrad_mfma_batched(jobs, workspace=None, accumulate=True):
    """``jobs``: up to WGRAD_BATCH_MAX tuples (x [n,h,w,cin] bf16, dy [n,h,w,cout] bf16, dw fp32 [cout*cin*9], dbias fp32
    [cout] | None) of plain stride-1 3x3 convs -> ONE partial launch + ONE reduction launch on the current stream."""
    if not 1 <= len(jobs) <= L.WGRAD_BATCH_MAX:
        raise ValueError(f"conv_wgrad_mfma_batched: 1..{L.WGRAD_BATCH_MAX} jobs, got {len(jobs)}")
    arr = (L.WgradJob * len(jobs))()
    for i, (x, dy, dw, db) in enumerate(jobs):
        _chk(x, BF16, "x", 4)
        _chk(dy, BF16, "dy", 4)
        _chk(dw, F32, "dw")
        n, h, w, cin = x.shape
        cout = dy.shape[3]
        if tuple(dy.shape) != (n, h, w, cout) or dw.numel() != cout * cin * 9 or (db is not None and db.numel() != cout):
            raise ValueError(f"conv_wgrad_mfma_batched: job {i}: shapes")
        if db is not None:
            _chk(db, F32, "dbias")
        arr[i] = L.WgradJob(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), n, h, w, cin,
                            cout, int(accumulate))
    ws = workspace if workspace is not None else wgrad_workspace(jobs[0][0].device)
    prof = KERNEL_PROFILE
    if prof is None:
        L.check(L.lib().pti_conv_wgrad_mfma_batched(arr, len(jobs), _ptr(ws), ws.numel() * 4, _stream()),
                "pti_conv_wgrad_mfma_batched")
        return
    # profiling: the library launches one kernel per mode (pti_conv_wgrad_batched_mode: the v6 kernel's two shapes, two
    # output-channel blocks per workgroup for Cout % 64 == 0, tile pairs otherwise); issue the groups as separate calls,
    # in the library's order, so that each kernel gets its own record (its own algorithmic work, its own duration =
    # partial launch + the <1 % reduction launch) under its own name.  A job the library refuses (mode < 0) goes last.
    groups = {}
    for i, j in enumerate(arr):
        groups.setdefault(L.lib().pti_conv_wgrad_batched_mode(j.n, j.h, j.w, j.cin, j.cout), []).append(i)
    for mode in sorted(groups, reverse=True):
        idx = groups[mode]
        sub = (L.WgradJob * len(idx))(*[arr[i] for i in idx])
        rec = _prof_begin(prof)
        L.check(L.lib().pti_conv_wgrad_mfma_batched(sub, len(idx), _ptr(ws), ws.numel() * 4, _stream()),
                "pti_conv_wgrad_mfma_batched")
        _prof_end(rec, sum(2.0 * arr[i].n * arr[i].h * arr[i].w * arr[i].cout * arr[i].cin * 9 for i in idx),
                  sum(2.0 * (jobs[i][0].numel() + jobs[i][1].numel()) for i in idx),
                  ("conv wgrad (batched)", 0, 0, 0, 0, 3, "s1", len(idx)))


def gn_bwd(x, da, dx, stats, gamma, beta, sums, dgamma, dbeta, *, groups, eps=1e-6, silu=True, dres=None):
    """dx <- backward of act(GroupNorm(x)); ``sums`` is an fp32 [n,c,2] scratch (written; no zeroing needed)."""
    _chk(x, ACT16, "x", 4)
    _chk(da, BF16, "da", 4)
    _chk(dx, BF16, "dx", 4)
    n, h, w, c = x.shape
    if da.shape != x.shape or dx.shape != x.shape or (dres is not None and dres.shape != x.shape):
        raise ValueError("gn_bwd: shape mismatch")
    _chk_stats(stats, n * groups * 2, "stats")
    if sums.numel() != n * c * 2:
        raise ValueError("gn_bwd: scratch sizes")
    blocks = L.lib().pti_gn_bwd_blocks(n, h * w, c)
    if blocks <= 0:
        raise ValueError(f"gn_bwd: unsupported channel count {c}")
    part = torch.empty(n * blocks * c * 2, dtype=torch.float32, device=x.device)
    L.check(L.lib().pti_gn_bwd(_ptr(x), _ptr(da), _ptr(dres), _ptr(dx), _ptr(stats), _ptr(gamma), _ptr(beta),
                               _ptr(sums), _ptr(part), _ptr(dgamma), _ptr(dbeta), n, h * w, c, groups, eps, int(silu),
                               int(x.dtype == F16), _stream()), "pti_gn_bwd")
    return dx


def conv_mfma_gnbwd(dy_in, w_packed_t, gx, gstats, ggamma, gbeta, dy_out, gsums, *, cout, ksize=3, mode=PTI_CONV_S1,
                    groups=0, eps=1e-6, silu=True):
    """Data-gradient conv with the GroupNorm(+SiLU) backward reduction fused into its epilogue:
    dy_out = conv^T(dy_in) * act'(GN(gx)); gsums[n,c] = {sum dy_out, sum dy_out*xhat} (one partial row per pixel tile
    from the conv, added up in a fixed order by pti_gn_sums_finalize: no float atomics, bitwise reproducible)."""
    _chk(dy_in, BF16, "dy_in", 4)
    _chk(gx, ACT16, "gx", 4)
    _chk(dy_out, BF16, "dy_out", 4)
    n, h, w, cin = dy_in.shape
    ho, wo = conv_out_hw(h, w, mode)
    if tuple(dy_out.shape) != (n, ho, wo, cout) or gx.shape != dy_out.shape:
        raise ValueError("conv_mfma_gnbwd: shapes")
    _chk_stats(gstats, n * groups * 2, "gstats")
    if gsums.numel() != n * cout * 2 or ggamma.numel() != cout:
        raise ValueError("conv_mfma_gnbwd: GroupNorm buffers")
    d = ConvDesc(n=n, h=h, w=w, cin=cin, ho=ho, wo=wo, cout=cout, ksize=ksize, mode=mode, groups=groups, eps=eps,
                 res_f16=int(gx.dtype == F16))
    tiles = L.lib().pti_conv_gnbwd_tiles(C.byref(d))
    if tiles <= 0:
        raise ValueError("conv_mfma_gnbwd: unsupported shape")
    part = torch.empty(n * tiles * cout * 2, dtype=torch.float32, device=dy_in.device)
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_conv2d_mfma_gnbwd(_ptr(dy_in), _ptr(w_packed_t), _ptr(gx), _ptr(gstats), _ptr(ggamma),
                                          _ptr(gbeta), _ptr(dy_out), _ptr(part), C.byref(d), int(silu), _stream()),
            "pti_conv2d_mfma_gnbwd")
    if rec is not None:     # (the finalize launch is not part of the record)
        _prof_end(rec, 2.0 * n * ho * wo * cout * cin * ksize * ksize * (0.25 if mode == PTI_CONV_ZINS else 1.0),
                  2.0 * (dy_in.numel() + 2 * dy_out.numel()),
                  ("conv dgrad+GN bwd", cin, cout, ho, wo, ksize, "zins" if mode == PTI_CONV_ZINS else "s1", n))
    L.check(L.lib().pti_gn_sums_finalize(_ptr(part), _ptr(gsums), n, tiles, 2 * cout, _stream()), "pti_gn_sums_finalize")
    return dy_out


def gnbwd_chain_supported(cin, cout, ksize, x_dtype, groups=16):
    """Whether conv_mfma_gnbwd_chain covers a data-gradient launch with ``cin`` input / ``cout`` output channels whose
    epilogue GroupNorm input is stored as ``x_dtype`` (the chained GroupNorm needs at least 8 channels per group: one
    16-byte piece of the loader lies inside one group)."""
    return (x_dtype == F16 and groups > 0 and cin % groups == 0 and cin // groups >= 8
            and bool(L.lib().pti_conv_gnbwd_chain_supported(int(cin), int(cout), int(ksize))))


def conv_mfma_gnbwd_chain(g_in, x_in, in_stats, in_gamma, in_sums, dx_in, w_packed_t, gx, gstats, ggamma, gbeta, dy_out, gsums,
                          *, cout, groups, eps=1e-6, silu=True, in_dgamma=None, in_dbeta=None):
    """conv_mfma_gnbwd whose INPUT is the un-applied GroupNorm backward of the layer above: ``g_in`` = dA * act'(GN(x_in)),
    ``x_in`` that GroupNorm's input, ``in_sums`` its finalized sums; the loader applies rstd*(gamma*g - c1 - xhat*c2) on the
    way in and writes that tensor to ``dx_in`` (bf16) for the weight gradient of the conv in between -- the
    pti_gn_bwd_apply launch of that GroupNorm disappears.  Its affine gradients are added to ``in_dgamma`` / ``in_dbeta`` by
    the finalize launch of this call when given (otherwise: gn_affine_grads)."""
    _chk(g_in, BF16, "g_in", 4)
    _chk(x_in, ACT16, "x_in", 4)
    _chk(dx_in, BF16, "dx_in", 4)
    _chk(gx, ACT16, "gx", 4)
    _chk(dy_out, BF16, "dy_out", 4)
    n, h, w, cin = g_in.shape
    if x_in.shape != g_in.shape or dx_in.shape != g_in.shape or tuple(dy_out.shape) != (n, h, w, cout) or gx.shape != dy_out.shape:
        raise ValueError("conv_mfma_gnbwd_chain: shapes")
    _chk_stats(in_stats, n * groups * 2, "in_stats")
    _chk_stats(gstats, n * groups * 2, "gstats")
    if in_sums.numel() != n * cin * 2 or gsums.numel() != n * cout * 2 or in_gamma.numel() != cin or ggamma.numel() != cout:
        raise ValueError("conv_mfma_gnbwd_chain: GroupNorm buffers")
    d = ConvDesc(n=n, h=h, w=w, cin=cin, ho=h, wo=w, cout=cout, ksize=3, mode=PTI_CONV_S1, groups=groups, eps=eps,
                 res_f16=int(gx.dtype == F16))
    tiles = L.lib().pti_conv_gnbwd_tiles(C.byref(d))
    if tiles <= 0:
        raise ValueError("conv_mfma_gnbwd_chain: unsupported shape")
    part = torch.empty(n * tiles * cout * 2, dtype=torch.float32, device=g_in.device)
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_conv2d_mfma_gnbwd_chain(_ptr(g_in), _ptr(x_in), int(x_in.dtype == F16), _ptr(in_stats), _ptr(in_gamma),
                                                _ptr(in_sums), _ptr(dx_in), _ptr(w_packed_t), _ptr(gx), _ptr(gstats),
                                                _ptr(ggamma), _ptr(gbeta), _ptr(dy_out), _ptr(part), C.byref(d), int(silu),
                                                _stream()), "pti_conv2d_mfma_gnbwd_chain")
    if rec is not None:     # reads g, x_in, gx; writes dx_in and dy_out (the finalize launch is not part of the record)
        _prof_end(rec, 2.0 * n * h * w * cout * cin * 9, 2.0 * (3 * g_in.numel() + 2 * dy_out.numel()),
                  ("conv dgrad+GN bwd (chained)", cin, cout, h, w, 3, "s1", n))
    if in_dgamma is not None or in_dbeta is not None:
        L.check(L.lib().pti_gn_sums_finalize_affine(_ptr(part), _ptr(gsums), n, tiles, 2 * cout, _ptr(in_sums), _ptr(in_dgamma),
                                                    _ptr(in_dbeta), cin, _stream()), "pti_gn_sums_finalize_affine")
    else:
        L.check(L.lib().pti_gn_sums_finalize(_ptr(part), _ptr(gsums), n, tiles, 2 * cout, _stream()), "pti_gn_sums_finalize")
    return dy_out


def gn_affine_grads(sums, dgamma, dbeta, n, c):
    """dgamma[c] += sum_n sums[n][c][1]; dbeta[c] += sum_n sums[n][c][0] (the affine gradients pti_gn_bwd_apply would add)."""
    L.check(L.lib().pti_gn_affine_grads(_ptr(sums), _ptr(dgamma), _ptr(dbeta), int(n), int(c), _stream()), "pti_gn_affine_grads")


def gn_bwd_apply(x, dy, dx, stats, gamma, beta, sums, dgamma, dbeta, *, groups, eps=1e-6, dres=None):
    _chk(x, ACT16, "x", 4)
    _chk(dy, BF16, "dy", 4)
    _chk(dx, BF16, "dx", 4)
    n, h, w, c = x.shape
    if dy.shape != x.shape or dx.shape != x.shape or (dres is not None and dres.shape != x.shape):
        raise ValueError("gn_bwd_apply: shape mismatch")
    _chk_stats(stats, n * groups * 2, "stats")
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_gn_bwd_apply(_ptr(x), _ptr(dy), _ptr(dres), _ptr(dx), _ptr(stats), _ptr(gamma), _ptr(beta),
                                     _ptr(sums), _ptr(dgamma), _ptr(dbeta), n, h * w, c, groups, eps,
                                     int(x.dtype == F16), _stream()), "pti_gn_bwd_apply")
    if rec is not None:   # pure HBM pass: reads x, dy (+ dres), writes dx; ~8 flops per element
        _prof_end(rec, 8.0 * x.numel(), 2.0 * x.numel() * (4 if dres is not None else 3),
                  ("GroupNorm bwd apply", c, c, h, w, 0, "-", n))
    return dx


def pool2x2_sum(x, y):
    _chk(x, BF16, "x", 4)
    _chk(y, BF16, "y", 4)
    n, h2, w2, c = x.shape
    if tuple(y.shape) != (n, h2 // 2, w2 // 2, c) or h2 % 2 or w2 % 2:
        raise ValueError("pool2x2_sum: shapes")
    L.check(L.lib().pti_pool2x2_sum(_ptr(x), _ptr(y), n, h2 // 2, w2 // 2, c, _stream()), "pti_pool2x2_sum")
    return y


def latent_head_fwd(h, eps, wm, bm, wl, bl, wp, bp, mu, sigma, logvar, zq):
    b, hw, l = h.shape
    for t, nm in ((h, "h"), (wm, "wm"), (bm, "bm"), (wl, "wl"), (bl, "bl"), (wp, "wp"), (bp, "bp"), (mu, "mu"),
                  (sigma, "sigma"), (zq, "zq")):
        _chk(t, F32, nm)
    if mu.numel() != b * hw * l or sigma.numel() != b * hw * l or zq.numel() != b * hw * l:
        raise ValueError("latent_head_fwd: output sizes")
    if eps is not None and (eps.numel() != b * hw * l or eps.dtype != F32 or not eps.is_contiguous()):
        raise ValueError("latent_head_fwd: eps must be contiguous fp32 of the latent shape")
    L.check(L.lib().pti_latent_head_fwd(_ptr(h), _ptr(eps), _ptr(wm), _ptr(bm), _ptr(wl), _ptr(bl), _ptr(wp), _ptr(bp),
                                        _ptr(mu), _ptr(sigma), _ptr(logvar), _ptr(zq), b, hw, l, _stream()),
            "pti_latent_head_fwd")


def post_quant(z_nchw, wp, bp, zq):
    b, l = z_nchw.shape[0], z_nchw.shape[1]
    hw = z_nchw.numel() // (b * l)
    _chk(z_nchw, F32, "z")
    L.check(L.lib().pti_post_quant(_ptr(z_nchw), _ptr(wp), _ptr(bp), _ptr(zq), b, hw, l, _stream()), "pti_post_quant")


def post_quant_bwd(dzq, z_nchw, wp, dz, gwp, gbp):
    b, l = z_nchw.shape[0], z_nchw.shape[1]
    hw = z_nchw.numel() // (b * l)
    _chk(dzq, F32, "dzq")
    _chk(z_nchw, F32, "z")
    if dzq.numel() != z_nchw.numel() or (dz is not None and dz.numel() != z_nchw.numel()):
        raise ValueError("post_quant_bwd: sizes")
    ws = torch.empty(POST_QUANT_BWD_MAX_BLOCKS * (l * l + l), dtype=torch.float32, device=dzq.device)
    L.check(L.lib().pti_post_quant_bwd(_ptr(dzq), _ptr(z_nchw), _ptr(wp), _ptr(dz), _ptr(gwp), _ptr(gbp), _ptr(ws), b, hw, l,
                                       _stream()), "pti_post_quant_bwd")


def latent_head_bwd(h, eps, wm, bm, wl, bl, wp, bp, dzq, dmu, dsigma, dh, gwm, gbm, gwl, gbl, gwp, gbp):
    b, hw, l = h.shape
    for t in (dzq, dmu, dsigma):
        if t is not None and (t.dtype != F32 or not t.is_contiguous() or t.numel() != b * hw * l):
            raise ValueError("latent_head_bwd: gradient inputs must be contiguous fp32 of the latent size")
    ws = torch.empty(LATENT_BWD_MAX_BLOCKS * 3 * (l * l + l), dtype=torch.float32, device=h.device)
    L.check(L.lib().pti_latent_head_bwd(_ptr(h), _ptr(eps), _ptr(wm), _ptr(bm), _ptr(wl), _ptr(bl), _ptr(wp), _ptr(bp),
                                        _ptr(dzq), _ptr(dmu), _ptr(dsigma), _ptr(dh), _ptr(gwm), _ptr(gbm), _ptr(gwl),
                                        _ptr(gbl), _ptr(gwp), _ptr(gbp), _ptr(ws), b, hw, l, _stream()),
            "pti_latent_head_bwd")


def vae_loss(recon, images, mu, third, out2, d_recon, d_mu, d_third, *, l2=False, third_mode=0, kl_weight=1e-3):
    for t, nm in ((recon, "recon"), (images, "images"), (mu, "mu"), (third, "third"), (out2, "out2")):
        _chk(t, F32, nm)
    if recon.shape != images.shape or mu.shape != third.shape or out2.numel() < 2:
        raise ValueError("vae_loss: shapes")
    ws = torch.empty(2 * VAE_LOSS_MAX_BLOCKS, dtype=torch.float32, device=recon.device)
    L.check(L.lib().pti_vae_loss(_ptr(recon), _ptr(images), recon.numel(), _ptr(mu), _ptr(third), mu.numel(),
                                 recon.shape[0], _ptr(out2), _ptr(d_recon), _ptr(d_mu), _ptr(d_third), _ptr(ws), int(l2),
                                 third_mode, kl_weight, _stream()), "pti_vae_loss")


def ar_vae_loss(mu, attrs, channels, deltas, per_attr, counts, *, gamma=0.0, d_mu=None, pair_mask=None):
    """AR-VAE term on the device (``pti_ar_vae_loss``): mu [b,l,h,w] fp32, attrs [na,b] fp32, channels int32 [na],
    deltas fp32 [na] -> per_attr fp32 [na], counts int32 [na]; ``d_mu`` (same shape as mu) += gamma * gradient."""
    _chk(mu, F32, "mu", 4)
    _chk(attrs, F32, "attrs", 2)
    _chk(deltas, F32, "deltas")
    _chk(per_attr, F32, "per_attr")
    b, l, h, w = mu.shape
    na = attrs.shape[0]
    if attrs.shape[1] != b or channels.numel() != na or deltas.numel() != na or per_attr.numel() != na or counts.numel() != na:
        raise ValueError("ar_vae_loss: attrs must be [na, b]; channels / deltas / per_attr / counts [na]")
    if channels.dtype != torch.int32 or counts.dtype != torch.int32 or not (channels.is_cuda and counts.is_cuda):
        raise TypeError("ar_vae_loss: channels / counts must be int32 device tensors")
    if d_mu is not None:
        _chk(d_mu, F32, "d_mu", 4)
        if d_mu.shape != mu.shape:
            raise ValueError("ar_vae_loss: d_mu shape")
    if pair_mask is not None:
        if pair_mask.dtype != torch.uint8 or tuple(pair_mask.shape) != (na, b, b) or not pair_mask.is_cuda or not pair_mask.is_contiguous():
            raise ValueError("ar_vae_loss: pair_mask must be a contiguous uint8 device tensor [na, b, b]")
    L.check(L.lib().pti_ar_vae_loss(_ptr(mu), b, l, h * w, _ptr(attrs), _ptr(channels), _ptr(deltas), na, _ptr(pair_mask),
                                    float(gamma), _ptr(per_attr), _ptr(counts), _ptr(d_mu), _stream()), "pti_ar_vae_loss")


def adam_step(p, g, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0):
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, F32, nm)
        if t.numel() != p.numel():
            raise ValueError("adam_step: size mismatch")
    L.check(L.lib().pti_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, step,
                                  grad_scale, _stream()), "pti_adam_step")


# ---- guarded optimiser step (csrc/optim_guard.hip; include/pti_vae.h "guarded optimiser step") ---------------------------
GRAD_GUARD_COLUMNS = L.GRAD_GUARD_COLUMNS                    # the fp64 columns of the control record, in order
GRAD_GUARD_HOST_COLUMNS = L.GRAD_GUARD_HOST_COLUMNS          # the first 64 bytes: what a host reads back
GRAD_GUARD_PARTIALS_CAP = L.GRAD_GUARD_PARTIALS_CAP          # PTI_GRAD_GUARD_PARTIALS_CAP


def grad_guard_ctl(device):
    """A zeroed control record for one optimiser: fp64 [len(GRAD_GUARD_COLUMNS)]."""
    return torch.zeros(len(GRAD_GUARD_COLUMNS), dtype=torch.float64, device=device)


def _chk_ctl(who, ctl, device):
    if not isinstance(ctl, torch.Tensor):
        raise ValueError(f"{who}: ctl: expected a CUDA(HIP) tensor")
    _chk(ctl, torch.float64, "ctl", 1)
    if ctl.numel() != len(GRAD_GUARD_COLUMNS) or ctl.device != device:
        raise ValueError(f"{who}: ctl must be fp64 [{len(GRAD_GUARD_COLUMNS)}] on {device}")


def grad_guard(g, *, ctl, grad_scale=1.0, max_norm=None, skip_nonfinite=False, betas=(0.9, 0.999), ema_decay=None):
    """Norm pass + decision of a guarded step (``pti_grad_guard``, two launches on the current stream, no host sync):
    ``ctl`` (``grad_guard_ctl``) then holds the fp64 sum of squares of ``g`` (flat fp32, 4-byte alignment suffices), the
    norm ``grad_scale * sqrt(sumsq)``, the clip coefficient for ``max_norm`` (None: no clipping), whether the step is
    skipped (a non-finite gradient with ``skip_nonfinite``), and the step counters, bias corrections and EMA decay
    (``ema_decay`` None: no EMA) that ``adam_step_guarded`` reads.  -> the partials buffer (cached per stream and size)."""
    _chk(g, F32, "g", 1)
    _chk_ctl("grad_guard", ctl, g.device)
    n = g.numel()
    nparts = L.lib().pti_grad_guard_partials(n)
    stream = _stream()
    ws, _ = _scratch_bytes("grad_guard", "grad_guard", (n,), 16 * nparts, (n,), g.device, stream)
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_grad_guard(_ptr(g), n, float(grad_scale), 0.0 if max_norm is None else float(max_norm),
                                   int(bool(skip_nonfinite)), betas[0], betas[1], 0.0 if ema_decay is None else float(ema_decay),
                                   _ptr(ws), _ptr(ctl), stream), "pti_grad_guard")
    if rec is not None:     # both launches; the name is the decision kernel's
        _prof_end(rec, 2.0 * n, 4.0 * n + 32.0 * nparts, ("grad_guard", n))
    return ws


def adam_step_guarded(p, g, m, v, *, ctl, lr, betas=(0.9, 0.999), eps=1e-8, ema=None):
    """``adam_step`` as ``grad_guard`` left it in ``ctl``: nothing on a skipped step, else Adam on ``g * (grad_scale * coef)``
    at ``t = applied_steps``, and with ``ema`` (an arena like ``p``) ``ema += (1 - decay) * (p_new - ema)`` in the same pass
    (``pti_adam_step_guarded``)."""
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")) + (((ema, "ema"),) if ema is not None else ()):
        _chk(t, F32, nm)
        if t.numel() != p.numel():
            raise ValueError("adam_step_guarded: size mismatch")
    _chk_ctl("adam_step_guarded", ctl, p.device)
    n = p.numel()
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_adam_step_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), n, lr, betas[0], betas[1], eps,
                                          _ptr(ctl), _stream()), "pti_adam_step_guarded")
    if rec is not None:
        _prof_end(rec, 12.0 * n, (28.0 if ema is None else 36.0) * n, ("adam_step_guarded", n, ema is not None))


def cast_nchw_f32_to_nhwc_bf16(x, y):
    n, c = x.shape[0], x.shape[1]
    _chk(x, F32, "x")
    _chk(y, BF16, "y")
    L.check(L.lib().pti_cast_nchw_f32_to_nhwc_bf16(_ptr(x), _ptr(y), n, c, x.numel() // (n * c), _stream()), "cast")
    return y


def cast_nhwc_bf16_to_nchw_f32(x, y):
    n, c = y.shape[0], y.shape[1]
    _chk(x, BF16, "x")
    _chk(y, F32, "y")
    L.check(L.lib().pti_cast_nhwc_bf16_to_nchw_f32(_ptr(x), _ptr(y), n, c, y.numel() // (n * c), _stream()), "cast")
    return y


def attention_fwd(qkv, o, lse2):
    """qkv [B,L,3C] bf16 -> o [B,L,C] bf16, lse2 [B,L] fp32."""
    _chk(qkv, BF16, "qkv", 3)
    _chk(o, BF16, "o", 3)
    _chk(lse2, F32, "lse2")
    b, l, c3 = qkv.shape
    c = c3 // 3
    if tuple(o.shape) != (b, l, c) or lse2.numel() != b * l or c3 != 3 * c:
        raise ValueError("attention_fwd: shapes")
    L.check(L.lib().pti_attention_fwd(_ptr(qkv), _ptr(o), _ptr(lse2), b, l, c, _stream()), "pti_attention_fwd")
    return o


def attention_bwd(qkv, o, dout, lse2, delta, dqkv):
    _chk(qkv, BF16, "qkv", 3)
    _chk(o, BF16, "o", 3)
    _chk(dout, BF16, "dout", 3)
    _chk(dqkv, BF16, "dqkv", 3)
    b, l, c3 = qkv.shape
    c = c3 // 3
    if o.shape != dout.shape or tuple(o.shape) != (b, l, c) or dqkv.shape != qkv.shape:
        raise ValueError("attention_bwd: shapes")
    if lse2.numel() != b * l or delta.numel() != b * l:
        raise ValueError("attention_bwd: lse/delta sizes")
    L.check(L.lib().pti_attention_bwd(_ptr(qkv), _ptr(o), _ptr(dout), _ptr(lse2), _ptr(delta), _ptr(dqkv), b, l, c,
                                      _stream()), "pti_attention_bwd")
    return dqkv


class BatchedPacker:
    """All MFMA weight packs of a model as ONE kernel launch (the per-layer form costs ~110 launches per
    optimiser step).  Entries are (fp32 weight view [cout,cin,k,k], ksize, mode, flip[, f16]); the packed outputs are
    allocated here and live at fixed addresses, as do the weights (views of the parameter arena)."""

    def __init__(self, entries, device):
        lib = L.lib()
        esz = lib.pti_conv_pack_entry_bytes()
        host = bytearray(esz * len(entries))
        hbuf = (C.c_char * len(host)).from_buffer(host)
        first, total, self.outputs = [], 0, []
        for i, (w, ksize, mode, flip, *rest) in enumerate(entries):
            f16 = bool(rest[0]) if rest else False
            _chk(w, F32, "weight")
            cout, cin = w.shape[0], w.shape[1]
            out = torch.empty(w.numel(), dtype=F16 if f16 else BF16, device=device)
            nb = C.c_int64(0)
            L.check(lib.pti_conv_pack_table_fill(C.byref(hbuf, i * esz), _ptr(w), _ptr(out), cout, cin, ksize, mode,
                                                 int(flip), int(f16), C.byref(nb)), "pti_conv_pack_table_fill")
            first.append(total)
            total += nb.value
            self.outputs.append(out)
        self.n, self.total_blocks = len(entries), total
        self.table = torch.frombuffer(host, dtype=torch.uint8).clone().to(device)
        self.first = torch.tensor(first, dtype=torch.int32, device=device)
        self._keep = [e[0] for e in entries]

    def run(self):
        L.check(L.lib().pti_conv_pack_weights_batched(_ptr(self.table), _ptr(self.first), self.n, self.total_blocks,
                                                      _stream()), "pti_conv_pack_weights_batched")


def preprocess_batch(src, offsets, hw, out, stats=None):
    """Resize(area) + LocalNormalizeByMask of a batch of raw fp32 images (see include/pti_vae.h).
    src: flat fp32 device tensor; offsets int64 [B]; hw int32 [B,2]; out fp32 [B,1,Hp,Wp]."""
    _chk(src, F32, "src")
    _chk(out, F32, "out", 4)
    b, _, hp, wp = out.shape
    if offsets.dtype != torch.int64 or hw.dtype != torch.int32 or offsets.numel() != b or hw.numel() != 2 * b:
        raise ValueError("preprocess_batch: offsets must be int64 [B], hw int32 [B,2]")
    if not (offsets.is_cuda and hw.is_cuda and offsets.is_contiguous() and hw.is_contiguous()):
        raise ValueError("preprocess_batch: descriptor tables must be contiguous device tensors")
    if stats is None:
        stats = torch.empty(3 * b, dtype=torch.float64, device=out.device)
    L.check(L.lib().pti_preprocess_batch(_ptr(src), _ptr(offsets), _ptr(hw), b, hp, wp, _ptr(out), _ptr(stats), _stream()),
            "pti_preprocess_batch")
    return out


# ---- argument checks shared by the analysis and evaluation launchers below ------------------------------------------------
# Their callers hand in arrays, None and views of larger buffers, so these say more than _chk / _out / _scratch; the
# training launchers above never come through here.
def _tensor(t, dtype, name, dims=None):
    """_chk for an argument that may not be a tensor at all."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a CUDA(HIP) tensor")
    _chk(t, dtype, name, dims)


def _dense_rows(t, name, dtype=F32, *, square=False, copy=False):
    """-> ``t`` as a device matrix of ``dtype`` whose rows are dense (column stride 1, row stride >= columns), a
    row-strided slice included.  It is used in place and anything else is refused (a copy would hide the caller's
    buffer), unless ``copy``: then any non-empty floating-point matrix is taken and cast / copied once where it has to be."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA(HIP) tensor")
    if copy and not t.is_floating_point():
        raise TypeError(f"{name}: expected a floating-point matrix, got {t.dtype}")
    if not copy and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    want = (f"{name}: expected {'a square [n, n]' if square else 'an [m, n]'} matrix {'that is not empty' if copy else 'with dense rows'}, "
            f"got {tuple(t.shape)}")
    if t.dim() != 2 or (square and t.shape[0] != t.shape[1]) or (copy and 0 in t.shape):
        raise ValueError(want)
    if copy and t.dtype != dtype:
        t = t.to(dtype)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        if not copy:
            raise ValueError(want)
        t = t.contiguous()
    return t


def _rows_out(out, shape, dtype, device, name):
    """Not _out: a view with a row stride is written in place, so the rule is dense rows, not contiguity."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _dense_rows(out, f"{name}: out", dtype)
    if tuple(out.shape) != tuple(shape) or out.device != device:
        raise ValueError(f"{name}: out must be {list(shape)} on {device}")
    return out


def _outs(who, out, names):
    """The tuple of caller-owned outputs ``out=(a, b, ...)``, or as many ``None``."""
    if out is None:
        return (None,) * len(names)
    if len(out) != len(names):
        raise ValueError(f"{who}: out must be ({', '.join(names)})")
    return tuple(out)


def _scratch_bytes(who, kind, shape, nbytes, what, device, stream):
    """_scratch for a launcher whose workspace the library sizes in bytes (``nbytes`` from its ``pti_*_ws_bytes``; none
    for a shape it does not serve) -> (buffer, its size in bytes)."""
    if nbytes <= 0:
        raise ValueError(f"{who}: unsupported shape {what}")
    ws = _scratch(kind, shape, (nbytes + 3) // 4, device, stream)
    return ws, ws.numel() * 4


def _offsets(who, name, seg, device, what, host=False):
    """An int32 vector of ``what`` + 1 row offsets on ``device`` (``host``: or in host memory)."""
    if not isinstance(seg, torch.Tensor) or (seg.device != device and (seg.is_cuda or not host)):
        raise ValueError(f"{who}: {name} must be a CUDA(HIP) tensor on {device}")
    if seg.dtype != I32:
        raise TypeError(f"{who}: {name} must be int32, got {seg.dtype}")
    if seg.dim() != 1 or seg.numel() < 2 or not seg.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous vector of {what} + 1 offsets")


def _latent_attrs(who, z, attrs):
    """The latent table ``z`` [N, L] in any layout and the attribute table ``attrs`` [na, N] -> (zt, attrs, n, l, na, ldz,
    lda): both as fp32 with dense rows of ``n`` values, ``zt`` = ``z`` transposed (the kernels read channel-major rows)
    -- a transposed view of a channel-major buffer is used in place, anything else is copied once -- and their row
    strides."""
    for name, t in (("z", z), ("attrs", attrs)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{who}: {name}: expected a CUDA(HIP) tensor")
        if not t.is_floating_point():
            raise TypeError(f"{who}: {name}: expected a floating-point matrix, got {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"{who}: {name}: expected a matrix, got {tuple(t.shape)}")
    n, l = z.shape
    na = attrs.shape[0]
    if attrs.shape[1] != n or attrs.device != z.device:
        raise ValueError(f"{who}: z {tuple(z.shape)} needs attrs [na, {n}] on {z.device}, got {tuple(attrs.shape)} on {attrs.device}")
    zt, attrs = _dense_rows(z.t(), f"{who}: z", copy=True), _dense_rows(attrs, f"{who}: attrs", copy=True)
    return zt, attrs, n, l, na, (zt.stride(0) if l > 1 else n), (attrs.stride(0) if na > 1 else n)   # a single row's stride means nothing
SSIM_WINDOW, SSIM_SIGMA = 11, 1.5
_ssim_taps = None


def ssim_taps() -> torch.Tensor:
    """The 11 fp32 taps of the SSIM window, built on the host the way the reference's ``compute_ssim`` builds them
    (eval_metrics.py:37-41): fp32 ``exp`` of -(i-5)^2 / (2 sigma^2), divided by their fp32 sum."""
    global _ssim_taps
    if _ssim_taps is None:
        coords = torch.arange(SSIM_WINDOW) - SSIM_WINDOW // 2
        g = torch.exp(-(coords ** 2) / (2 * SSIM_SIGMA * SSIM_SIGMA))
        _ssim_taps = (g / g.sum()).to(F32).contiguous()
    return _ssim_taps


def image_metrics(pred, target, *, clamp=None, data_range=1.0, k1=0.01, k2=0.03, out=None):
    """Per-sample ``[mse, mae, psnr, ssim]`` of two fp32 ``[n, c, h, w]`` device batches in one fused pass
    (``pti_image_metrics``) -> fp32 ``[n, 4]`` device tensor.

    ``clamp=(lo, hi)`` clamps both inputs as they are loaded (evaluate_vae.py clamps to [0, 1] first).  PSNR and SSIM follow
    the reference's ``compute_psnr`` / ``compute_ssim``: 11x11 Gaussian window (sigma 1.5), zero padding without border
    renormalisation.  The reference function only runs for ``c == 1``; for ``c > 1`` the same window is applied to each
    channel on its own (depthwise) and SSIM is the mean over all channels.  Non-contiguous or non-fp32 inputs are copied
    to contiguous fp32 first.  Runs on the current stream, no host sync; the scratch buffer is cached per (stream, shape)."""
    if not (pred.is_cuda and target.is_cuda):
        raise ValueError("image_metrics: expected CUDA(HIP) tensors")
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"image_metrics: expected two [n, c, h, w] tensors of one shape, got {tuple(pred.shape)} / {tuple(target.shape)}")
    if not (pred.is_floating_point() and target.is_floating_point()):
        raise TypeError("image_metrics: expected floating-point images")
    pred, target = pred.to(F32).contiguous(), target.to(F32).contiguous()
    n, c, h, w = pred.shape
    floats = L.lib().pti_image_metrics_ws_floats(n, c, h, w)
    if floats <= 0:
        raise ValueError(f"image_metrics: unsupported shape {tuple(pred.shape)}")
    out = _out(out, (n, 4), F32, pred.device, "image_metrics: out", chk_name="out")
    stream = _stream()
    ws = _scratch("metrics", (n, c, h, w), floats, pred.device, stream)
    lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    L.check(L.lib().pti_image_metrics(_ptr(pred), _ptr(target), n, c, h, w, int(clamp is not None), lo, hi, float(data_range),
                                      float(k1), float(k2), C.c_void_p(ssim_taps().data_ptr()), _ptr(out), _ptr(ws), stream),
            "pti_image_metrics")
    return out


# ---- latent-space analysis (csrc/latent_stats.hip; include/pti_vae.h "latent-space analysis") -------------------------
def latent_pairwise(a, b=None, *, mode="dist", center=None, out=None):
    """``out[i, j]`` = Euclidean distance (``mode="dist"``) or dot product (``mode="dot"``) of row ``i`` of ``a`` [n1, d]
    and row ``j`` of ``b`` [n2, d] (``b=None``: ``a`` against itself) -> fp32 ``[n1, n2]`` device tensor
    (``pti_latent_pairwise``).  ``center`` [d] is subtracted from both as they are loaded: ``mode="dot"`` with the column
    mean is the centred Gram matrix.  Distances are accumulated as sum (a - b)^2 in fp32 in a fixed order: bitwise
    reproducible, and an entry depends on its two rows only.  Row-strided views and an ``out`` view with a row stride
    are used in place.  Runs on the current stream, no host sync; the scratch buffer is cached per (stream, shape)."""
    if mode not in ("dist", "dot"):
        raise ValueError(f"latent_pairwise: mode must be 'dist' or 'dot', got {mode!r}")
    a = _dense_rows(a, "latent_pairwise: a", copy=True)
    b = a if b is None else _dense_rows(b, "latent_pairwise: b", copy=True)
    if b.shape[1] != a.shape[1] or b.device != a.device:
        raise ValueError(f"latent_pairwise: a {tuple(a.shape)} and b {tuple(b.shape)} must share columns and device")
    n1, d = a.shape
    n2 = b.shape[0]
    if center is not None:
        if not isinstance(center, torch.Tensor) or not center.is_cuda:
            raise ValueError("latent_pairwise: center must be a CUDA(HIP) tensor")
        if not center.is_floating_point():
            raise TypeError("latent_pairwise: center must be floating-point")
        if center.numel() != d or center.device != a.device:
            raise ValueError(f"latent_pairwise: center must hold {d} values on {a.device}")
        center = center.reshape(-1).to(F32).contiguous()
    floats = L.lib().pti_latent_pairwise_ws_floats(n1, n2, d)
    if floats <= 0:
        raise ValueError(f"latent_pairwise: unsupported shape a {tuple(a.shape)} b {tuple(b.shape)}")
    out = _rows_out(out, (n1, n2), F32, a.device, "latent_pairwise")
    stream = _stream()
    ws = _scratch("pair", (n1, n2, d), floats, a.device, stream)
    L.check(L.lib().pti_latent_pairwise(_ptr(a), a.stride(0), n1, _ptr(b), b.stride(0), n2, d, _ptr(center),
                                        int(mode == "dot"), _ptr(out), out.stride(0), _ptr(ws), stream), "pti_latent_pairwise")
    return out


def latent_group_stats(a, seg_a, b, seg_b, *, out=None):
    """Per-patient distance statistics of two groups of rows (``pti_latent_group_stats``) -> fp32 ``[patients, 4]``:
    (centre distance, mean population std of the ``a`` rows, the same for ``b``, mean cross distance), the reference's
    ``compute_distance_metrics`` for every patient at once.  ``a`` [n1, d] / ``b`` [n2, d] hold each patient's rows
    consecutively; ``seg_a`` / ``seg_b`` are int32 device vectors of ``patients + 1`` ascending row offsets.  A patient
    without rows on one side gets a NaN row.  Runs on the current stream, no host sync."""
    a = _dense_rows(a, "latent_group_stats: a", copy=True)
    b = _dense_rows(b, "latent_group_stats: b", copy=True)
    if b.shape[1] != a.shape[1] or b.device != a.device:
        raise ValueError(f"latent_group_stats: a {tuple(a.shape)} and b {tuple(b.shape)} must share columns and device")
    _offsets("latent_group_stats", "seg_a", seg_a, a.device, "patients")
    _offsets("latent_group_stats", "seg_b", seg_b, a.device, "patients")
    if seg_a.numel() != seg_b.numel():
        raise ValueError("latent_group_stats: seg_a and seg_b must describe the same patients")
    e = seg_a.numel() - 1
    (n1, d), n2 = a.shape, b.shape[0]
    floats = L.lib().pti_latent_group_stats_ws_floats(n1, n2, e, d)
    if floats <= 0:
        raise ValueError(f"latent_group_stats: unsupported shape a {tuple(a.shape)} b {tuple(b.shape)} patients {e}")
    out = _rows_out(out, (e, 4), F32, a.device, "latent_group_stats")
    if out.stride(0) != 4:
        raise ValueError("latent_group_stats: out must be contiguous")
    stream = _stream()
    ws = _scratch("group", (n1, n2, e, d), floats, a.device, stream)
    L.check(L.lib().pti_latent_group_stats(_ptr(a), a.stride(0), n1, _ptr(seg_a), _ptr(b), b.stride(0), n2, _ptr(seg_b), e, d,
                                           _ptr(out), _ptr(ws), stream), "pti_latent_group_stats")
    return out


# ---- exact t-SNE (csrc/tsne.hip; include/pti_vae.h "exact t-SNE") -------------------------------------------------------
def tsne_affinities(d2, perplexity, *, out=None):
    """Joint probabilities of exact t-SNE (``pti_tsne_affinities``) from the fp32 matrix ``d2`` [n, n] of SQUARED Euclidean
    distances -> ``(P, sums)``: ``P`` fp32 [n, n], symmetric bit for bit with a zero diagonal (sklearn's
    ``_joint_probabilities`` in dense form: the per-row perplexity search in fp64, then ``max((p_j|i + p_i|j) / S, eps)``),
    and ``sums`` = the fp64 device pair ``{sum P log P, sum P}`` that ``tsne_step`` needs for the KL value.
    2 <= n <= 8192, 0 < perplexity < n.  Runs on the current stream, no host sync."""
    d2 = _dense_rows(d2, "tsne_affinities: d2", square=True)
    n = d2.shape[0]
    perplexity = float(perplexity)
    if not 0.0 < perplexity < n:
        raise ValueError(f"tsne_affinities: perplexity ({perplexity:g}) must be positive and < n ({n})")
    floats = L.lib().pti_tsne_affinities_ws_floats(n)
    if floats <= 0:
        raise ValueError(f"tsne_affinities: unsupported shape {tuple(d2.shape)} (2 <= n <= 8192)")
    out = _rows_out(out, (n, n), F32, d2.device, "tsne_affinities")
    if out.data_ptr() == d2.data_ptr():
        raise ValueError("tsne_affinities: out must not be d2")
    sums = torch.empty(2, dtype=torch.float64, device=d2.device)
    stream = _stream()
    ws = _scratch("tsne_aff", (n,), floats, d2.device, stream)
    L.check(L.lib().pti_tsne_affinities(_ptr(d2), d2.stride(0), n, perplexity, _ptr(out), out.stride(0), _ptr(sums), _ptr(ws),
                                        stream), "pti_tsne_affinities")
    return out, sums


def tsne_step(p, y_in, y_out, update, gains, record, *, sums, exaggeration, momentum, lr, with_record=True):
    """One iteration of exact t-SNE's gradient descent (``pti_tsne_step``: sklearn's ``_kl_divergence`` gradient and
    ``_gradient_descent`` update).  ``p`` fp32 [n, n] and ``sums`` from ``tsne_affinities``; ``y_in`` -> ``y_out`` (two
    distinct contiguous fp32 [n, 2] buffers), ``update`` / ``gains`` fp32 [n, 2] in place; ``record``: fp64 [2] device
    tensor that receives ``{KL(exaggeration * P || Q) at y_in, |gain * grad|_2}`` when ``with_record`` (an iteration
    without a record skips the fp64 work behind the KL value).
    Runs on the current stream, no host sync; bitwise reproducible."""
    p = _dense_rows(p, "tsne_step: p", square=True)
    n = p.shape[0]
    for name, t in (("y_in", y_in), ("y_out", y_out), ("update", update), ("gains", gains)):
        _tensor(t, F32, f"tsne_step: {name}", 2)
        if t.shape[0] != n or t.device != p.device:
            raise ValueError(f"tsne_step: {name} must be [{n}, 2] on {p.device}, got {tuple(t.shape)}")
        if t.shape[1] != 2:
            raise ValueError(f"tsne_step: {name} has {t.shape[1]} columns; only n_components = 2 is built")
    for name, t in (("record", record), ("sums", sums)):
        _tensor(t, torch.float64, f"tsne_step: {name}", 1)
        if t.numel() != 2 or t.device != p.device:
            raise ValueError(f"tsne_step: {name} must hold 2 doubles on {p.device}")
    if y_in.data_ptr() == y_out.data_ptr():
        raise ValueError("tsne_step: y_out must not be y_in")
    floats = L.lib().pti_tsne_step_ws_floats(n, 2)
    if floats <= 0:
        raise ValueError(f"tsne_step: unsupported shape {tuple(p.shape)} (2 <= n <= 8192)")
    stream = _stream()
    ws = _scratch("tsne_step", (n,), floats, p.device, stream)
    L.check(L.lib().pti_tsne_step(_ptr(p), p.stride(0), n, 2, _ptr(y_in), _ptr(y_out), _ptr(update), _ptr(gains), _ptr(sums),
                                  float(exaggeration), float(momentum), float(lr), _ptr(record), int(bool(with_record)),
                                  _ptr(ws), stream), "pti_tsne_step")


# ---- UMAP (csrc/umap.hip; include/pti_vae.h "UMAP of the latent-space analysis") -----------------------------------------
UmapGraph = namedtuple("UmapGraph", "indptr indices weights rate rho sigma nnz")
UmapGraph.__doc__ = """The fuzzy graph of ``umap_graph`` as device CSR: ``indptr`` int32 [n + 1]; ``indices`` int32 (ascending
within a row), ``weights`` fp32 and ``rate`` int32, allocated for min(2 n k, n^2) entries of which the first ``nnz`` are
written; ``rho`` / ``sigma`` fp32 [n]; ``nnz`` = ``indptr[n]``, a 0-d DEVICE tensor (reading it is a host sync)."""


def umap_knn(dist, k, *, out=None):
    """The ``k`` nearest neighbours of every row of the fp32 distance matrix ``dist`` [n, n] (``pti_umap_knn``) ->
    ``(knn_idx int32 [n, k], knn_dist fp32 [n, k])``, ascending by (distance, column): the diagonal competes like any other
    entry and equal distances go by the lower column.  Exact.  ``out``: a pair of tensors to write into.
    3 <= n <= 8192, 2 <= k <= 256, k < n.  Runs on the current stream, no host sync."""
    idx, kd = _outs("umap_knn", out, ("knn_idx", "knn_dist"))
    dist = _dense_rows(dist, "umap_knn: dist", square=True)
    n, k = dist.shape[0], int(k)
    if not (3 <= n <= 8192 and 2 <= k <= 256 and k < n):
        raise ValueError(f"umap_knn: unsupported shape {tuple(dist.shape)} with k={k} (3 <= n <= 8192, 2 <= k <= 256, k < n)")
    idx = _out(idx, (n, k), I32, dist.device, "umap_knn: knn_idx")
    kd = _out(kd, (n, k), F32, dist.device, "umap_knn: knn_dist")
    L.check(L.lib().pti_umap_knn(_ptr(dist), dist.stride(0), n, k, _ptr(idx), _ptr(kd), _stream()), "pti_umap_knn")
    return idx, kd


def umap_graph(knn_idx, knn_dist, n_epochs):
    """UMAP's fuzzy graph from the neighbours of ``umap_knn`` (``pti_umap_graph``: umap-learn's ``smooth_knn_dist`` with the
    search in fp64, ``compute_membership_strengths``, the union ``w = a + a^T - a o a^T``, entries below
    ``wmax / n_epochs`` dropped) -> ``UmapGraph``.  ``rate = floor(w 2^20 / wmax)`` is the integer form of umap-learn's
    ``epochs_per_sample``.  The CSR arrays are allocated for the upper bound min(2 n k, n^2), so nothing comes back to the
    host.  1 <= n_epochs <= 2000.  Runs on the current stream, no host sync; bitwise reproducible."""
    for name, t, dtype in (("knn_idx", knn_idx, I32), ("knn_dist", knn_dist, F32)):
        _tensor(t, dtype, f"umap_graph: {name}", 2)
    n, k = knn_idx.shape
    if tuple(knn_dist.shape) != (n, k) or knn_dist.device != knn_idx.device:
        raise ValueError(f"umap_graph: knn_dist must be [{n}, {k}] on {knn_idx.device}, got {tuple(knn_dist.shape)}")
    n_epochs = int(n_epochs)
    floats, cap = L.lib().pti_umap_graph_ws_floats(n, k), L.lib().pti_umap_graph_capacity(n, k)
    if floats <= 0 or not 1 <= n_epochs <= 2000:
        raise ValueError(f"umap_graph: unsupported shape {tuple(knn_idx.shape)} with n_epochs={n_epochs} "
                         f"(3 <= n <= 8192, 2 <= k <= 256, k < n, 1 <= n_epochs <= 2000)")
    dev = knn_idx.device
    indptr = torch.empty(n + 1, dtype=I32, device=dev)
    indices, rate = torch.empty(cap, dtype=I32, device=dev), torch.empty(cap, dtype=I32, device=dev)
    weights = torch.empty(cap, dtype=F32, device=dev)
    rho, sigma = torch.empty(n, dtype=F32, device=dev), torch.empty(n, dtype=F32, device=dev)
    stream = _stream()
    ws = _scratch("umap_graph", (n, k), floats, dev, stream)
    L.check(L.lib().pti_umap_graph(_ptr(knn_idx), _ptr(knn_dist), n, k, n_epochs, _ptr(indptr), _ptr(indices), _ptr(weights),
                                   _ptr(rate), cap, _ptr(rho), _ptr(sigma), _ptr(ws), stream), "pti_umap_graph")
    return UmapGraph(indptr, indices, weights, rate, rho, sigma, indptr[n])


def umap_epoch(graph, y_in, y_out, *, a, b, alpha, epoch, seed, negative_sample_rate=5):
    """One layout epoch of UMAP as a Jacobi sweep (``pti_umap_epoch``): ``y_in`` -> ``y_out``, two distinct contiguous fp32
    [n, 2] buffers.  ``graph``: an ``UmapGraph`` (only ``indptr``, ``indices`` and ``rate`` are read).  An edge fires in the
    epochs its ``rate`` selects; a fired edge attracts its vertex (twice: the mirrored edge fires in the same epoch) and
    repels it from ``negative_sample_rate`` vertices drawn by a hash of (``seed``, ``epoch``, CSR position).
    Runs on the current stream, no host sync; bitwise reproducible."""
    for name, t, dtype in (("indptr", graph.indptr, I32), ("indices", graph.indices, I32), ("rate", graph.rate, I32),
                           ("y_in", y_in, F32), ("y_out", y_out, F32)):
        _tensor(t, dtype, f"umap_epoch: {name}", 2 if name[0] == "y" else 1)
    n = graph.indptr.numel() - 1
    if not 3 <= n <= 8192:
        raise ValueError(f"umap_epoch: unsupported shape: {n} rows (3 <= n <= 8192)")
    cap = graph.indices.numel()
    if graph.rate.numel() != cap or cap > n * n:
        raise ValueError(f"umap_epoch: indices ({cap}) and rate ({graph.rate.numel()}) must have one length of at most n^2")
    for name, t in (("y_in", y_in), ("y_out", y_out)):
        if t.shape[0] != n or t.device != graph.indptr.device:
            raise ValueError(f"umap_epoch: {name} must be [{n}, 2] on {graph.indptr.device}, got {tuple(t.shape)}")
        if t.shape[1] != 2:
            raise ValueError(f"umap_epoch: {name} has {t.shape[1]} columns; only n_components = 2 is built")
    if y_in.data_ptr() == y_out.data_ptr():
        raise ValueError("umap_epoch: y_out must not be y_in")
    L.check(L.lib().pti_umap_epoch(_ptr(graph.indptr), _ptr(graph.indices), _ptr(graph.rate), cap, n, 2, _ptr(y_in), _ptr(y_out),
                                   float(a), float(b), float(alpha), int(epoch), int(seed) & 0xFFFFFFFF,
                                   int(negative_sample_rate), _stream()), "pti_umap_epoch")


# ---- UMAP transform: new rows into a fitted embedding (csrc/umap.hip; include/pti_vae.h "UMAP transform") ------------------
UmapTransformGraph = namedtuple("UmapTransformGraph", "indices weights rate sigma y0")
UmapTransformGraph.__doc__ = """What ``umap_transform_graph`` makes of m new rows' k nearest training rows, a regular device slab:
``indices`` int32 [m, k] (the ``knn_idx`` it was given), ``weights`` fp32 [m, k], ``rate`` int32 [m, k] (0 = dropped),
``sigma`` fp32 [m] and the start points ``y0`` fp32 [m, 2]."""


def _umap_cross_shape(who, m, n, k):
    if not (1 <= m <= 8192 and 3 <= n <= 8192 and 2 <= k <= 256 and k < n):
        raise ValueError(f"{who}: unsupported shape: {m} new rows, {n} training rows, k={k} "
                         f"(1 <= m <= 8192, 3 <= n <= 8192, 2 <= k <= 256, k < n)")


def _umap_embedding(who, name, t, rows, device):
    _tensor(t, F32, f"{who}: {name}", 2)
    if (rows is not None and t.shape[0] != rows) or t.device != device:
        raise ValueError(f"{who}: {name} must be [{'n' if rows is None else rows}, 2] on {device}, got {tuple(t.shape)}")
    if t.shape[1] != 2:
        raise ValueError(f"{who}: {name} has {t.shape[1]} columns; only n_components = 2 is built")


def umap_knn_cross(dist, k, *, out=None):
    """The ``k`` nearest TRAINING rows of every new row (``pti_umap_knn_cross``): ``dist`` fp32 [m, n] holds the distances
    from m new rows to n training rows -> ``(knn_idx int32 [m, k], knn_dist fp32 [m, k])``, ascending by (distance,
    column); equal distances go by the lower column.  Exact.  A view with a row stride is read in place.  ``out``: a pair
    of tensors to write into.  1 <= m <= 8192, 3 <= n <= 8192, 2 <= k <= 256, k < n.  Runs on the current stream, no host
    sync."""
    idx, kd = _outs("umap_knn_cross", out, ("knn_idx", "knn_dist"))
    dist = _dense_rows(dist, "umap_knn_cross: dist")
    (m, n), k = dist.shape, int(k)
    _umap_cross_shape("umap_knn_cross", m, n, k)
    idx = _out(idx, (m, k), I32, dist.device, "umap_knn_cross: knn_idx")
    kd = _out(kd, (m, k), F32, dist.device, "umap_knn_cross: knn_dist")
    L.check(L.lib().pti_umap_knn_cross(_ptr(dist), dist.stride(0), m, n, k, _ptr(idx), _ptr(kd), _stream()), "pti_umap_knn_cross")
    return idx, kd


def umap_transform_graph(knn_idx, knn_dist, y_train, n_epochs):
    """umap-learn's ``transform`` preamble from the neighbours of ``umap_knn_cross`` (``pti_umap_transform_graph``) ->
    ``UmapTransformGraph``.  ``rho = 0`` for every row; ``sigma`` from ``umap_graph``'s fp64 search, floored at 1e-3 times
    the mean of all distances; bipartite strengths ``d <= 0 ? 1 : exp(-d / sigma)``; slots below ``wmax / n_epochs`` get
    ``rate`` 0, the others ``floor(w 2^20 / wmax)``; ``y0`` = the strength-weighted mean of the neighbours' points in the
    fitted embedding ``y_train`` fp32 [n, 2], over all k slots.  1 <= n_epochs <= 2000.  Runs on the current stream, no
    host sync; bitwise reproducible."""
    who = "umap_transform_graph"
    for name, t, dtype in (("knn_idx", knn_idx, I32), ("knn_dist", knn_dist, F32)):
        _tensor(t, dtype, f"{who}: {name}", 2)
    m, k = knn_idx.shape
    dev = knn_idx.device
    if tuple(knn_dist.shape) != (m, k) or knn_dist.device != dev:
        raise ValueError(f"{who}: knn_dist must be [{m}, {k}] on {dev}, got {tuple(knn_dist.shape)}")
    _umap_embedding(who, "y_train", y_train, None, dev)
    n, n_epochs = y_train.shape[0], int(n_epochs)
    _umap_cross_shape(who, m, n, k)
    if not 1 <= n_epochs <= 2000:
        raise ValueError(f"{who}: unsupported n_epochs={n_epochs} (1 <= n_epochs <= 2000)")
    sigma, y0 = torch.empty(m, dtype=F32, device=dev), torch.empty(m, 2, dtype=F32, device=dev)
    weights, rate = torch.empty(m, k, dtype=F32, device=dev), torch.empty(m, k, dtype=I32, device=dev)
    stream = _stream()
    ws = _scratch("umap_tgraph", (m, k), L.lib().pti_umap_transform_graph_ws_floats(m, n, k), dev, stream)
    L.check(L.lib().pti_umap_transform_graph(_ptr(knn_idx), _ptr(knn_dist), m, k, _ptr(y_train), n, n_epochs, _ptr(sigma),
                                             _ptr(weights), _ptr(rate), _ptr(y0), _ptr(ws), stream), "pti_umap_transform_graph")
    return UmapTransformGraph(knn_idx, weights, rate, sigma, y0)


def umap_transform_layout(tg, y_train, y_in, y_out, *, a, b, n_epochs, seed, start=0, stop=None, initial_alpha=0.25,
                          negative_sample_rate=5):
    """Epochs ``start`` .. ``stop`` - 1 (all ``n_epochs`` by default) of the layout of NEW rows against the fitted embedding
    ``y_train`` fp32 [n, 2], in ONE launch (``pti_umap_transform_layout``): ``y_in`` -> ``y_out``, contiguous fp32 [m, 2];
    ``y_out`` may be ``y_in`` (a row reads only itself and ``y_train``) but must not overlap ``y_train``.  ``tg``: an
    ``UmapTransformGraph`` (only ``indices`` and ``rate`` are read).  ``alpha = initial_alpha (1 - e / n_epochs)``; a fired
    slot attracts its row to the neighbour's training point (once: that end does not move) and repels it from
    ``negative_sample_rate`` training points drawn by a hash of (``seed``, epoch, slot).  The point is rounded to fp32 after
    every epoch, so any split of the epochs into launches gives the same bits.
    Runs on the current stream, no host sync; bitwise reproducible."""
    who = "umap_transform_layout"
    for name, t in (("indices", tg.indices), ("rate", tg.rate)):
        _tensor(t, I32, f"{who}: {name}", 2)
    m, k = tg.indices.shape
    dev = tg.indices.device
    if tuple(tg.rate.shape) != (m, k) or tg.rate.device != dev:
        raise ValueError(f"{who}: rate must be [{m}, {k}] on {dev}, got {tuple(tg.rate.shape)}")
    _umap_embedding(who, "y_train", y_train, None, dev)
    _umap_embedding(who, "y_in", y_in, m, dev)
    _umap_embedding(who, "y_out", y_out, m, dev)
    n, n_epochs = y_train.shape[0], int(n_epochs)
    _umap_cross_shape(who, m, n, k)
    stop = n_epochs if stop is None else int(stop)
    if not 1 <= n_epochs <= 2000 or not 0 <= int(start) <= stop <= n_epochs:
        raise ValueError(f"{who}: unsupported n_epochs={n_epochs} with epochs [{start}, {stop}) "
                         f"(1 <= n_epochs <= 2000, 0 <= start <= stop <= n_epochs)")
    lo, hi = y_out.data_ptr(), y_out.data_ptr() + 8 * m
    if y_train.data_ptr() < hi and lo < y_train.data_ptr() + 8 * n:
        raise ValueError(f"{who}: y_out must not overlap y_train")
    if y_in.data_ptr() != lo and y_in.data_ptr() < hi and lo < y_in.data_ptr() + 8 * m:
        raise ValueError(f"{who}: y_out must be y_in itself or apart from it")
    L.check(L.lib().pti_umap_transform_layout(_ptr(tg.indices), _ptr(tg.rate), m, k, _ptr(y_train), n, _ptr(y_in), _ptr(y_out),
                                              float(a), float(b), float(initial_alpha), n_epochs, int(start), stop,
                                              int(seed) & 0xFFFFFFFF, int(negative_sample_rate), _stream()),
            "pti_umap_transform_layout")


# ---- mask geometry (csrc/mask_geometry.hip; include/pti_vae.h "mask geometry") -----------------------------------------
MASK_DTYPES = (torch.uint8, torch.uint16, F32)   # dtype of the mask buffer for `elem` 0, 1, 2 of pti_mask_geometry
MASK_ROW_CAP = 4096                                     # the kernel's bound on max_h


def mask_geometry(src, offsets, hw, *, elem, max_h, sample_rows, bottom_offsets, out=None):
    """Bounding box and row widths of a batch of binary masks of mixed size in one launch (``pti_mask_geometry``) ->
    ``(bbox [b, 4], bbox_widths [b, samples], bottom_widths [b, n_bottom])`` as int32 device tensors.

    ``src``: the masks concatenated in their stored type, a flat uint8 / uint16 / float32 device tensor whose dtype
    matches ``elem`` (0 / 1 / 2); ``offsets`` int64 [b]: element offset of every image (no alignment needed); ``hw``
    int32 [b, 2].  ``sample_rows`` int32 [max_h + 1, samples]: for every bounding-box height the rows, relative to the
    box's first row, whose widths are wanted (``data.mask_metrics.sample_row_table``); ``bottom_offsets`` int32
    [n_bottom]: rows counted up from the image's last row, clamped per image.  Either may have zero entries.
    ``bbox`` is ``{x0, y0, w, h}``, ``{-1, -1, 0, 0}`` for a mask without foreground and ``{-2, -2, 0, 0}`` for an image
    whose height exceeds ``max_h`` (it is not read).  ``out``: the three int32 tensors to write instead of new ones.
    Runs on the current stream, no host sync."""
    if elem not in (0, 1, 2):
        raise ValueError(f"mask_geometry: elem must be 0 (uint8), 1 (uint16) or 2 (float32), got {elem!r}")
    wanted = (("src", src, MASK_DTYPES[elem]), ("offsets", offsets, I64), ("hw", hw, torch.int32),
              ("sample_rows", sample_rows, torch.int32), ("bottom_offsets", bottom_offsets, torch.int32))
    for name, t, dtype in wanted:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError(f"mask_geometry: {name} must be a {dtype} tensor" + (f" for elem {elem}" if name == "src" else "")
                            + f", got {getattr(t, 'dtype', type(t))}")
    for name, t, _ in wanted:
        if not t.is_cuda or t.device != src.device:
            raise ValueError(f"mask_geometry: {name} must be a CUDA(HIP) tensor on the device of src")
        if not t.is_contiguous():
            raise ValueError(f"mask_geometry: {name} must be contiguous")
    b = offsets.numel()
    if src.dim() != 1 or offsets.dim() != 1 or b < 1 or tuple(hw.shape) != (b, 2):
        raise ValueError("mask_geometry: src must be flat, offsets [b] with b >= 1 and hw [b, 2]")
    max_h = int(max_h)
    if not 0 <= max_h <= MASK_ROW_CAP:
        raise ValueError(f"mask_geometry: max_h must be in [0, {MASK_ROW_CAP}], got {max_h}")
    if sample_rows.dim() != 2 or sample_rows.shape[0] != max_h + 1:
        raise ValueError(f"mask_geometry: sample_rows must be [max_h + 1, samples] = [{max_h + 1}, samples], "
                         f"got {tuple(sample_rows.shape)}")
    if bottom_offsets.dim() != 1:
        raise ValueError(f"mask_geometry: bottom_offsets must be a vector, got {tuple(bottom_offsets.shape)}")
    samples, n_bottom = sample_rows.shape[1], bottom_offsets.numel()
    shapes = ((b, 4), (b, samples), (b, n_bottom))
    names = ("bbox", "bbox_widths", "bottom_widths")   # caller-owned outputs (views of larger buffers included)
    bbox, bbox_widths, bottom_widths = (_out(t, sh, torch.int32, src.device, f"mask_geometry: out {name}", rank=False)
                                        for name, t, sh in zip(names, _outs("mask_geometry", out, names), shapes))
    # a table or an output without entries is passed as NULL
    L.check(L.lib().pti_mask_geometry(_ptr(src), _ptr(offsets), _ptr(hw), b, elem, max_h,
                                      _ptr(sample_rows) if samples else None, samples,
                                      _ptr(bottom_offsets) if n_bottom else None, n_bottom, _ptr(bbox),
                                      _ptr(bbox_widths) if samples else None, _ptr(bottom_widths) if n_bottom else None,
                                      _stream()), "pti_mask_geometry")
    return bbox, bbox_widths, bottom_widths


# ---- shape comparison of image pairs (csrc/mask_compare.hip; include/pti_vae.h "shape comparison") ------------------------
MASK_COMPARE_MAX_EDGE = 1024                            # PTI_MASK_COMPARE_MAX_EDGE: the kernel's bound on h and w
MASK_COMPARE_COLUMNS = L.MASK_COMPARE_COLUMNS              # the int32 columns, in order
MASK_COMPARE_SUMS = ("sq_err_sum", "max_gt", "max_pred")


def _image_pair(who, names, a, b, *, min_edge=1, max_edge=MASK_COMPARE_MAX_EDGE, max_n=65535, optional_b=False):
    """The common checks of a pair of image batches -> (a, b, n, h, w) as ``[n, h, w]`` views.  ``min_edge`` / ``max_edge``
    bound h and w; ``max_n=None``: the launcher has no cap on n; ``optional_b``: ``b`` may be ``None`` and stays ``None``."""
    pair = [(names[0], a)] if optional_b and b is None else list(zip(names, (a, b)))
    for name, t in pair:
        if not isinstance(t, torch.Tensor) or t.dtype != F32:
            raise TypeError(f"{who}: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    for name, t in pair:
        if not t.is_cuda or t.device != a.device:
            raise ValueError(f"{who}: {name} must be a CUDA(HIP) tensor on the device of {names[0]}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
    if a.dim() == 4 and a.shape[1] == 1:
        a = a[:, 0]
    if b is not None and b.dim() == 4 and b.shape[1] == 1:
        b = b[:, 0]
    if a.dim() != 3 or (b is not None and b.shape != a.shape):
        raise ValueError(f"{who}: expected [n, h, w] or [n, 1, h, w] images of one shape, got {tuple(a.shape)}"
                         + (f" / {tuple(b.shape)}" if b is not None else ""))
    n, h, w = a.shape
    if not (1 <= n <= (max_n or n) and min_edge <= h <= max_edge and min_edge <= w <= max_edge):
        raise ValueError(f"{who}: unsupported shape {tuple(a.shape)} ({f'1 <= n <= {max_n}' if max_n else 'n >= 1'}, "
                         f"{min_edge} <= h, w <= {max_edge})")
    return a, b, n, h, w


def mask_compare(gt, pred, *, threshold=0.2, out=None, cleaned=None, masks=None):
    """Foreground masks, largest component, hole fill and the shape numbers of a batch of image pairs in one launch
    (``pti_mask_compare``) -> ``(counts, sums)`` device tensors.

    ``masks``: ``None``, or ``True`` / a contiguous uint8 ``[n, h, w]`` device tensor: the same launch
    (``pti_mask_compare_outputs``) also writes the two regions the Dice is formed from, bit 0 = ``gt != 0``, bit 1 = the
    prediction's filled largest component (``cleaned != 0`` is not that: a filled hole can hold zeros) -- the input of
    ``surface_distance`` -- and it is appended to the return value; ``counts``, ``sums`` and ``cleaned`` are the same bits either way.

    ``cleaned``: ``None``, or ``True`` / a contiguous fp32 ``[n, h, w]`` device tensor (not ``gt`` or ``pred``): the same launch
    (``pti_mask_compare_cleaned``) also writes the prediction inside its cleaned mask and 0 elsewhere -- the image the MSE is
    formed from -- and ``(counts, sums, cleaned)`` is returned; ``counts`` and ``sums`` are the same bits either way.

    ``gt`` / ``pred``: contiguous fp32 device images ``[n, h, w]`` or ``[n, 1, h, w]`` of one shape, finite, ``1 <= h, w <=
    MASK_COMPARE_MAX_EDGE``.  Masks: ``gt != 0`` and ``|pred| > threshold``; the prediction's mask is cleaned to its largest
    8-connected component (pixel count; ties go to the smallest row-major index) with its holes filled.  ``counts``: int32
    ``[n, 24]`` in ``MASK_COMPARE_COLUMNS`` order; ``sums``: float64 ``[n, 3]`` in ``MASK_COMPARE_SUMS`` order (include/pti_vae.h
    has the definitions).  ``counts[:, 23]`` (``status``) is 0 unless the kernel's bounded label loops overran -- it travels
    with the results, ``utils.compare_metrics.pair_metrics`` raises on it.  ``out=(counts, sums)`` are written in place.
    Runs on the current stream, no host sync; bitwise reproducible; the scratch buffer is cached per (stream, shape)."""
    who = "mask_compare"
    gt, pred, n, h, w = _image_pair(who, ("gt", "pred"), gt, pred, max_n=None)
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError(f"{who}: threshold must be >= 0, got {threshold}")
    out = _outs(who, out, ("counts", "sums"))
    counts = _out(out[0], (n, len(MASK_COMPARE_COLUMNS)), torch.int32, gt.device, f"{who}: out[0] (counts)")
    sums = _out(out[1], (n, len(MASK_COMPARE_SUMS)), torch.float64, gt.device, f"{who}: out[1] (sums)")
    stream = _stream()
    ws, ws_bytes = _scratch_bytes(who, "mask_compare", (n, h, w), L.lib().pti_mask_compare_ws_bytes(n, h, w), tuple(gt.shape),
                                  gt.device, stream)
    no_cleaned = cleaned is None or cleaned is False
    if masks is not None and masks is not False:
        masks = _out(None if masks is True else masks, (n, h, w), torch.uint8, gt.device, f"{who}: masks")
        if not no_cleaned:
            cleaned = _out(None if cleaned is True else cleaned, (n, h, w), F32, gt.device, f"{who}: cleaned")
        taken = (gt.data_ptr(), pred.data_ptr()) + (() if no_cleaned else (cleaned.data_ptr(),))
        if masks.data_ptr() in taken or (not no_cleaned and cleaned.data_ptr() in taken[:2]):
            raise ValueError(f"{who}: cleaned and masks must not be gt, pred or each other")
        L.check(L.lib().pti_mask_compare_outputs(_ptr(gt), _ptr(pred), n, h, w, threshold, _ptr(counts), _ptr(sums),
                                                 None if no_cleaned else _ptr(cleaned), _ptr(masks), _ptr(ws), ws_bytes, stream),
                "pti_mask_compare_outputs")
        return (counts, sums, masks) if no_cleaned else (counts, sums, cleaned, masks)
    if no_cleaned:
        L.check(L.lib().pti_mask_compare(_ptr(gt), _ptr(pred), n, h, w, threshold, _ptr(counts), _ptr(sums), _ptr(ws),
                                         ws_bytes, stream), "pti_mask_compare")
        return counts, sums
    cleaned = _out(None if cleaned is True else cleaned, (n, h, w), F32, gt.device, f"{who}: cleaned")
    if cleaned.data_ptr() in (gt.data_ptr(), pred.data_ptr()):
        raise ValueError(f"{who}: cleaned must not be gt or pred")
    L.check(L.lib().pti_mask_compare_cleaned(_ptr(gt), _ptr(pred), n, h, w, threshold, _ptr(counts), _ptr(sums), _ptr(cleaned),
                                             _ptr(ws), ws_bytes, stream), "pti_mask_compare_cleaned")
    return counts, sums, cleaned


# ---- uniform-window SSIM of image pairs (csrc/ssim_uniform.hip; include/pti_vae.h "uniform-window SSIM") ------------------
SSIM_UNIFORM_MIN_EDGE = 7                               # the 7 x 7 window must fit
SSIM_UNIFORM_COLUMNS = ("ssim", "data_range")


def ssim_uniform(gt, pred, *, data_range=None, out=None):
    """skimage's uniform-window SSIM of a batch of image pairs (``pti_ssim_uniform``) -> fp64 ``[n, 2]`` device tensor in
    ``SSIM_UNIFORM_COLUMNS`` order.

    ``gt`` / ``pred``: contiguous fp32 device images ``[n, h, w]`` or ``[n, 1, h, w]`` of one shape, finite, ``7 <= h, w <=
    MASK_COMPARE_MAX_EDGE``; ``pred`` is usually ``mask_compare``'s ``cleaned``.  7 x 7 box window, sample covariance, the mean
    over the pixels whose window lies inside the image (a 3-pixel border is left out), ``K1, K2 = 0.01, 0.03``.
    ``data_range``: ``None`` takes ``max(gt) - min(gt)`` per image on the device, a number ``>= 0`` is used for every image.
    An image whose range is 0 reports ``{0, 0}`` (the SSIM is 0 / 0 there).  ``out`` is written in place.  At most three
    launches on the current stream, no host sync; bitwise reproducible; the scratch buffer is cached per (stream, shape)."""
    who = "ssim_uniform"
    if data_range is not None:
        data_range = float(data_range)
        if not data_range >= 0.0:
            raise ValueError(f"{who}: data_range must be >= 0 or None, got {data_range}")
    gt, pred, n, h, w = _image_pair(who, ("gt", "pred"), gt, pred, min_edge=SSIM_UNIFORM_MIN_EDGE)
    out = _out(out, (n, len(SSIM_UNIFORM_COLUMNS)), torch.float64, gt.device, f"{who}: out")
    stream = _stream()
    ws, ws_bytes = _scratch_bytes(who, "ssim_uniform", (n, h, w), L.lib().pti_ssim_uniform_ws_bytes(n, h, w), tuple(gt.shape),
                                  gt.device, stream)
    L.check(L.lib().pti_ssim_uniform(_ptr(gt), _ptr(pred), n, h, w, -1.0 if data_range is None else data_range, _ptr(out),
                                     _ptr(ws), ws_bytes, stream), "pti_ssim_uniform")
    return out


# ---- surface distance between two regions (csrc/surface_distance.hip; include/pti_vae.h "surface distance") --------------
SURFACE_COLUMNS = L.SURFACE_COLUMNS                       # the int32 columns per (image, side), in order
SURFACE_MAX_TOLERANCES = L.SURFACE_MAX_TOLERANCES


def surface_percentile_pm(who, percentile) -> int:
    """A percentile in per-mille; it must be a multiple of 0.1 in 0 .. 100."""
    pm = round(float(percentile) * 10.0)
    if not (0 <= pm <= 1000) or abs(float(percentile) * 10.0 - pm) > 1e-9:
        raise ValueError(f"{who}: percentile must be a multiple of 0.1 in 0 .. 100, got {percentile}")
    return int(pm)


def surface_tolerances_d2(who, tolerances) -> list:
    """Tolerances in pixels -> ``floor(t * t)`` each (capped at int32): for an integer ``d2``, ``d <= t`` is ``d2 <= floor(t^2)``."""
    tolerances = [float(t) for t in tolerances]
    if len(tolerances) > SURFACE_MAX_TOLERANCES or any(not t >= 0.0 for t in tolerances):
        raise ValueError(f"{who}: at most {SURFACE_MAX_TOLERANCES} tolerances, each >= 0, got {tolerances}")
    return [int(math.floor(min(t * t, 2.0 ** 31 - 1))) for t in tolerances]


def surface_distance(masks, other=None, *, percentile=95.0, tolerances=(), out=None):
    """Distances between the outlines of two binary regions per image (``pti_surface_distance``) -> ``(counts, sums)``: int32
    ``[n, 2, 11]`` in ``SURFACE_COLUMNS`` order and float64 ``[n, 2]``, per image and side (side 0 measures from the first
    region's edge to the second's, side 1 the other way).  ``utils.compare_metrics.surface_metrics`` turns them into Hausdorff,
    its percentile form, the average symmetric surface distance and surface Dice.

    ``masks`` alone: contiguous uint8 ``[n, h, w]`` as ``mask_compare(..., masks=True)`` writes it, bit 0 the first region and
    bit 1 the second.  With ``other``: two uint8 / bool ``[n, h, w]`` tensors, any non-zero byte is foreground.  ``1 <= h, w <=
    MASK_COMPARE_MAX_EDGE``.  An edge pixel is a foreground pixel with a 4-neighbour that is background or outside the image;
    ``d2`` of an edge pixel is its exact squared distance to the nearest edge pixel of the other region.  ``percentile``: a
    multiple of 0.1; ``d2_lo`` / ``d2_hi`` are the two order statistics it is interpolated between.  ``tolerances``: up to four
    distances in pixels, ``within_j`` counts the edge pixels within each.  If either region of an image has no edge pixel both
    its rows hold ``-1`` for the three ``d2`` columns and 0 elsewhere (``n_fg``, ``n_edge`` stay true).  ``out=(counts, sums)``
    are written in place.  Three launches on the current stream, no host sync; every integer is exact and the output is
    bitwise reproducible; the scratch buffer (12 bytes per pixel and image) is cached per (stream, shape)."""
    who = "surface_distance"
    pair = [("masks", masks)] + ([("other", other)] if other is not None else [])
    for name, t in pair:
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.bool):
            raise TypeError(f"{who}: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t))}")
        if not t.is_cuda or t.device != masks.device:
            raise ValueError(f"{who}: {name} must be a CUDA(HIP) tensor on the device of masks")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
    if masks.dim() != 3 or (other is not None and other.shape != masks.shape):
        raise ValueError(f"{who}: expected [n, h, w] masks of one shape, got {tuple(masks.shape)}"
                         + (f" / {tuple(other.shape)}" if other is not None else ""))
    n, h, w = masks.shape
    if not (1 <= n <= 32767 and 1 <= h <= MASK_COMPARE_MAX_EDGE and 1 <= w <= MASK_COMPARE_MAX_EDGE):
        raise ValueError(f"{who}: unsupported shape {tuple(masks.shape)} (1 <= n <= 32767, 1 <= h, w <= {MASK_COMPARE_MAX_EDGE})")
    pm = surface_percentile_pm(who, percentile)
    tol = surface_tolerances_d2(who, tolerances)
    out = _outs(who, out, ("counts", "sums"))
    counts = _out(out[0], (n, 2, len(SURFACE_COLUMNS)), torch.int32, masks.device, f"{who}: out[0] (counts)")
    sums = _out(out[1], (n, 2), torch.float64, masks.device, f"{who}: out[1] (sums)")
    stream = _stream()
    ws, ws_bytes = _scratch_bytes(who, "surface_distance", (n, h, w), L.lib().pti_surface_distance_ws_bytes(n, h, w),
                                  tuple(masks.shape), masks.device, stream)
    a, b, a_bits, b_bits = (masks, masks, 1, 2) if other is None else (masks, other, 255, 255)
    L.check(L.lib().pti_surface_distance(_ptr(a), a_bits, _ptr(b), b_bits, n, h, w, pm, (C.c_int32 * max(len(tol), 1))(*tol),
                                         len(tol), _ptr(counts), _ptr(sums), _ptr(ws), ws_bytes, stream), "pti_surface_distance")
    return counts, sums


# ---- pair registration: straighten, then align (csrc/mask_compare.hip; include/pti_vae.h "pair registration") -------------
MASK_MOMENTS_COLUMNS = L.MASK_MOMENTS_COLUMNS              # int64 columns per (image, side)
MASK_MOMENTS_COEFFS = ("beta", "cos_beta", "sin_beta")     # fp64 per (image, side)
ALIGN_BOTTOM_COLUMNS = L.ALIGN_BOTTOM_COLUMNS              # int32 columns per image
ALIGN_BOTTOM_MIN_HEIGHT = 5                                # below it there is no bottom fifth


def mask_moments(gt, pred, *, threshold=0.2, out=None):
    """Orientation of the object on both sides of a batch of image pairs in one launch (``pti_mask_moments``) ->
    ``(cleaned, moments, coeffs)`` device tensors.

    ``gt`` / ``pred`` as for ``mask_compare``.  ``cleaned``: fp32 like ``pred``, the prediction inside its cleaned mask and 0
    elsewhere.  ``moments``: int64 ``[n, 2, 10]`` in ``MASK_MOMENTS_COLUMNS`` order, side 0 the ground truth's filled largest
    component, side 1 the prediction's; ``coeffs``: float64 ``[n, 2, 3]`` = the rotation ``beta`` (radians) that makes the
    region's major axis vertical, its cosine and its sine (include/pti_vae.h has the rules).  A side without foreground has
    ``m00 == 0`` and ``beta == 0``.  ``out=(cleaned, moments, coeffs)`` are written in place.  Current stream, no host sync,
    bitwise reproducible; the scratch buffer (twice ``mask_compare``'s) is cached per (stream, shape)."""
    who = "mask_moments"
    gt, pred, n, h, w = _image_pair(who, ("gt", "pred"), gt, pred)
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError(f"{who}: threshold must be >= 0, got {threshold}")
    out = _outs(who, out, ("cleaned", "moments", "coeffs"))
    cleaned = _out(out[0], (n, h, w), F32, gt.device, f"{who}: out[0] (cleaned)")
    moments = _out(out[1], (n, 2, len(MASK_MOMENTS_COLUMNS)), torch.int64, gt.device, f"{who}: out[1] (moments)")
    coeffs = _out(out[2], (n, 2, 3), torch.float64, gt.device, f"{who}: out[2] (coeffs)")
    stream = _stream()
    ws, ws_bytes = _scratch_bytes(who, "mask_moments", (n, h, w), L.lib().pti_mask_moments_ws_bytes(n, h, w), tuple(gt.shape),
                                  gt.device, stream)
    L.check(L.lib().pti_mask_moments(_ptr(gt), _ptr(pred), n, h, w, threshold, _ptr(cleaned), _ptr(moments), _ptr(coeffs),
                                     _ptr(ws), ws_bytes, stream), "pti_mask_moments")
    return cleaned, moments, coeffs


def warp_cubic(gt, pred, coeffs, *, out=None):
    """Both sides of a batch rotated about ``(w // 2, h // 2)`` by their own coefficients in one launch (``pti_warp_cubic``)
    -> ``(rotated_gt, rotated_pred)``.

    ``coeffs``: float64 ``[n, 2, 3]`` as ``mask_moments`` returns them (``cos`` and ``sin`` are what is used).  4 x 4 cubic
    convolution (Keys, a = -0.75), replicate border, fp64 coordinates, fp32 weights and sums; coefficients ``(1, 0)`` give a
    copy.  ``out=(rotated_gt, rotated_pred)`` are written in place and must not be the inputs."""
    who = "warp_cubic"
    gt, pred, n, h, w = _image_pair(who, ("gt", "pred"), gt, pred)
    if not isinstance(coeffs, torch.Tensor) or coeffs.dtype != torch.float64:
        raise TypeError(f"{who}: coeffs must be a float64 tensor, got {getattr(coeffs, 'dtype', type(coeffs))}")
    if coeffs.device != gt.device or not coeffs.is_contiguous() or tuple(coeffs.shape) != (n, 2, 3):
        raise ValueError(f"{who}: coeffs must be contiguous [{n}, 2, 3] on {gt.device}, got {tuple(coeffs.shape)}")
    out = _outs(who, out, ("rotated_gt", "rotated_pred"))
    rot_gt = _out(out[0], (n, h, w), F32, gt.device, f"{who}: out[0] (rotated_gt)")
    rot_pred = _out(out[1], (n, h, w), F32, gt.device, f"{who}: out[1] (rotated_pred)")
    L.check(L.lib().pti_warp_cubic(_ptr(gt), _ptr(pred), _ptr(coeffs), n, h, w, _ptr(rot_gt), _ptr(rot_pred), _stream()),
            "pti_warp_cubic")
    return rot_gt, rot_pred


def align_bottom(rot_gt, rot_pred, *, out=None):
    """The prediction moved sideways so that the centres of the non-zero pixels in the last ``h // 5`` rows agree, in one
    launch (``pti_align_bottom``) -> ``(aligned_pred, info)``; ``info``: int32 ``[n, 6]`` in ``ALIGN_BOTTOM_COLUMNS`` order.
    ``status`` is 0, +1 when the ground truth has nothing in those rows, +2 when the prediction has nothing (the shift is
    then 0).  Needs ``h >= 5``.  ``out=(aligned_pred, info)`` are written in place; ``aligned_pred`` must not be an input."""
    who = "align_bottom"
    rot_gt, rot_pred, n, h, w = _image_pair(who, ("rot_gt", "rot_pred"), rot_gt, rot_pred)
    if h < ALIGN_BOTTOM_MIN_HEIGHT:
        raise ValueError(f"{who}: unsupported shape {tuple(rot_gt.shape)} (h >= {ALIGN_BOTTOM_MIN_HEIGHT}: there is no bottom fifth)")
    out = _outs(who, out, ("aligned_pred", "info"))
    aligned = _out(out[0], (n, h, w), F32, rot_gt.device, f"{who}: out[0] (aligned_pred)")
    info = _out(out[1], (n, len(ALIGN_BOTTOM_COLUMNS)), torch.int32, rot_gt.device, f"{who}: out[1] (info)")
    L.check(L.lib().pti_align_bottom(_ptr(rot_gt), _ptr(rot_pred), n, h, w, _ptr(aligned), _ptr(info), _stream()),
            "pti_align_bottom")
    return aligned, info


def register_pairs(gt, pred, *, threshold=0.2, out=None):
    """``mask_moments``, ``warp_cubic`` and ``align_bottom`` in order: what the reference does to a pair before it measures
    -> ``(rotated_gt, aligned_pred, info)``, ``info = {"moments", "coeffs", "align"}`` (the device tensors of the three ops).

    Three launches on the current stream, no host sync.  ``out=(rotated_gt, aligned_pred, moments, coeffs, align)`` are
    written in place; the cleaned and the rotated prediction live in scratch cached per (stream, shape)."""
    who = "register_pairs"
    gt, pred, n, h, w = _image_pair(who, ("gt", "pred"), gt, pred)
    if h < ALIGN_BOTTOM_MIN_HEIGHT:
        raise ValueError(f"{who}: unsupported shape {tuple(gt.shape)} (h >= {ALIGN_BOTTOM_MIN_HEIGHT}: there is no bottom fifth)")
    out = _outs(who, out, ("rotated_gt", "aligned_pred", "moments", "coeffs", "align"))
    tmp = _scratch("register_pairs", (n, h, w), 2 * n * h * w, gt.device, _stream()).view(2, n, h, w)
    _, moments, coeffs = mask_moments(gt, pred, threshold=threshold, out=(tmp[0], out[2], out[3]))
    rot_gt, _ = warp_cubic(gt, tmp[0], coeffs, out=(out[0], tmp[1]))
    aligned, align = align_bottom(rot_gt, tmp[1], out=(out[1], out[4]))
    return rot_gt, aligned, {"moments": moments, "coeffs": coeffs, "align": align}


# ---- display normalisation (csrc/display.hip; include/pti_vae.h "display normalisation") --------------------------------
DISPLAY_MAX_EDGE, DISPLAY_MAX_PLANES = 4096, 65535   # the bounds of pti_display_planes


def display_planes(a, b=None, *, nsrc=None, low=2, high=98, rot90=0, dtype=torch.uint8):
    """``normalize_batch_for_display`` of every plane, rotated and laid side by side, in one launch
    (``pti_display_planes``) -> ``(canvas, stats)``.

    ``a`` / ``b``: fp32 device images ``[n, h, w]`` or ``[n, 1, h, w]`` of one shape.  ``nsrc`` picks the sources per image:
    1 = ``a``; 2 = ``a, b``; 3 = ``a, b, |a - b|`` (default: 1 without ``b``, 2 with it).  Every plane is mapped on its own
    from the ``low`` .. ``high`` percentile of its non-zero pixels to 0 .. 1 (clipped, below 1e-3 -> 0, zeros stay 0), turned
    by ``rot90`` quarter turns like ``torch.rot90(k, dims=[-2, -1])`` and written into columns ``[s * wo, (s + 1) * wo)`` of
    ``canvas [n, ho, nsrc * wo]``: ``dtype`` float32 holds the mapped value, uint8 holds ``trunc(value * 255)``.
    ``stats``: float64 ``[n, nsrc, 3]`` = ``{non-zero count, p_low, p_high}`` on the device.  Inputs must be finite.  Runs
    on the current stream, no host sync, no scratch (one workgroup per plane keeps everything in LDS)."""
    who = "display_planes"
    if nsrc is None:
        nsrc = 1 if b is None else 2
    if nsrc not in (1, 2, 3):
        raise ValueError(f"{who}: nsrc must be 1, 2 or 3, got {nsrc!r}")
    if nsrc >= 2 and b is None:
        raise ValueError(f"{who}: nsrc = {nsrc} needs b")
    low, high = float(low), float(high)
    if not 0.0 <= low <= high <= 100.0:
        raise ValueError(f"{who}: percentiles must satisfy 0 <= low <= high <= 100, got {low}, {high}")
    rot90 = int(rot90)
    if not 0 <= rot90 <= 3:
        raise ValueError(f"{who}: rot90 must be 0, 1, 2 or 3, got {rot90}")
    if dtype not in (torch.uint8, F32):
        raise TypeError(f"{who}: dtype must be torch.uint8 or torch.float32, got {dtype}")
    a, b, n, h, w = _image_pair(who, ("a", "b"), a, b, max_edge=DISPLAY_MAX_EDGE, max_n=DISPLAY_MAX_PLANES // nsrc,
                                optional_b=True)
    if nsrc == 1:
        b = None
    ho, wo = (w, h) if rot90 & 1 else (h, w)
    canvas = torch.empty((n, ho, nsrc * wo), dtype=dtype, device=a.device)
    stats = torch.empty((n, nsrc, 3), dtype=torch.float64, device=a.device)
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_display_planes(_ptr(a), _ptr(b), n, h, w, nsrc, low, high, rot90,
                                       _ptr(canvas) if dtype == F32 else None, _ptr(canvas) if dtype == torch.uint8 else None,
                                       _ptr(stats), _stream()), "pti_display_planes")
    if rec is not None:   # four select passes over the plane's values (two inputs for |a - b|) and one map pass
        reads = 4.0 * a.numel() * (nsrc + (nsrc == 3))
        _prof_end(rec, 0.0, 5 * reads + canvas.numel() * canvas.element_size(), ("display", nsrc, h, w, rot90, n))
    return canvas, stats


# ---- attribute-ordering report (csrc/rank_agreement.hip; include/pti_vae.h "attribute-ordering report") ------------------
RANK_AGREEMENT_MAX_N, RANK_AGREEMENT_MAX_L, RANK_AGREEMENT_MAX_NA = 32768, 16, 16   # the bounds of pti_rank_agreement
RANK_CLASSES = ("concordant", "discordant", "z_tied", "a_tied", "both_tied")


def rank_agreement(z, attrs, channels, deltas, *, out=None):
    """Pair-ordering counts of every (attribute, latent channel) over ALL image pairs (``pti_rank_agreement``) ->
    ``(counts, loss_sum)`` device tensors.

    ``z``: floating-point device matrix ``[N, L]`` (one latent code per image) in any layout -- a transposed view of a
    channel-major ``[L, N]`` buffer, row stride included, is used in place, anything else is copied once; ``attrs``: ``[na, N]``
    attribute values with dense rows.  ``channels`` / ``deltas``: ``na`` host values (sequences or CPU tensors; a device
    tensor is read back, which synchronises): the latent channel attribute ``q`` regularises (negative: none) and its tanh
    slope.  ``counts``: int64 ``[na, L, 5]``, exact, in ``RANK_CLASSES`` order over the ``N (N - 1) / 2`` unordered pairs;
    ``loss_sum``: float64 ``[na]``, the AR summand of ``pti_ar_vae_loss`` added over the pairs whose attribute values differ.
    ``out=(counts, loss_sum)`` are written in place.  2 <= N <= 32768, L <= 16, na <= 16; inputs must be finite.  Runs on
    the current stream, no host sync; bitwise reproducible; the scratch buffer is cached per (stream, shape)."""
    who = "rank_agreement"
    out = _outs(who, out, ("counts", "loss_sum"))
    zt, attrs, n, l, na, ldz, lda = _latent_attrs(who, z, attrs)
    if not (2 <= n <= RANK_AGREEMENT_MAX_N and 1 <= l <= RANK_AGREEMENT_MAX_L and 1 <= na <= RANK_AGREEMENT_MAX_NA):
        raise ValueError(f"{who}: unsupported shape z {tuple(z.shape)} attrs {tuple(attrs.shape)} (2 <= N <= {RANK_AGREEMENT_MAX_N}, "
                         f"1 <= L <= {RANK_AGREEMENT_MAX_L}, 1 <= na <= {RANK_AGREEMENT_MAX_NA})")
    channels = [int(v) for v in (channels.tolist() if isinstance(channels, torch.Tensor) else channels)]
    deltas = [float(v) for v in (deltas.tolist() if isinstance(deltas, torch.Tensor) else deltas)]
    if len(channels) != na or len(deltas) != na:
        raise ValueError(f"{who}: channels / deltas must hold one value per attribute ({na}), got {len(channels)} / {len(deltas)}")
    if any(c >= l for c in channels):
        raise ValueError(f"{who}: channels {channels} must lie below the {l} latent channels")
    counts = _out(out[0], (na, l, 5), I64, z.device, f"{who}: out[0] (counts)")
    loss_sum = _out(out[1], (na,), torch.float64, z.device, f"{who}: out[1] (loss_sum)")
    stream = _stream()
    ws, ws_bytes = _scratch_bytes(who, "rank", (n, l, na), L.lib().pti_rank_agreement_ws_bytes(n, l, na),
                                  f"z {tuple(z.shape)} attrs {tuple(attrs.shape)}", z.device, stream)
    L.check(L.lib().pti_rank_agreement(_ptr(zt), ldz, _ptr(attrs), lda, n, l, na,
                                       (C.c_int32 * na)(*channels), (C.c_float * na)(*deltas), _ptr(counts), _ptr(loss_sum),
                                       _ptr(ws), ws_bytes, stream), "pti_rank_agreement")
    return counts, loss_sum


# ---- disentanglement report (csrc/disentanglement.hip; include/pti_vae.h "disentanglement report") ----------------------
DISENT_MAX_N, DISENT_MAX_COLS, DISENT_MAX_BINS = 32768, 32, 32   # the bounds of pti_tied_ranks / pti_joint_histogram


def tied_ranks(cols, *, out=None):
    """Twice the average rank of every value within its column (``pti_tied_ranks``) -> int32 ``[M, N]`` device tensor.

    ``cols``: floating-point device matrix ``[M, N]``, one column of ``N`` values per ROW; rows with a dense last dimension
    (a row-strided slice included) are used in place, anything else is copied once.  ``rank2[m, i] = 2 #{j: x_j < x_i} +
    #{j: x_j == x_i} + 1``, exactly ``2 * scipy.stats.rankdata(x, "average")``; ``-0.0`` ties with ``0.0``.  ``out`` is
    written in place.  2 <= N <= 32768, 1 <= M <= 32; inputs must be finite.  Current stream, no host sync, exact."""
    who = "tied_ranks"
    cols = _dense_rows(cols, f"{who}: cols", copy=True)
    m, n = cols.shape
    if not (2 <= n <= DISENT_MAX_N and 1 <= m <= DISENT_MAX_COLS):
        raise ValueError(f"{who}: unsupported shape cols {tuple(cols.shape)} (2 <= N <= {DISENT_MAX_N}, 1 <= M <= {DISENT_MAX_COLS})")
    rank2 = _out(out, (m, n), torch.int32, cols.device, f"{who}: out (rank2)")
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_tied_ranks(_ptr(cols), cols.stride(0) if m > 1 else n, n, m, _ptr(rank2), _stream()), "pti_tied_ranks")
    if rec is not None:   # two compares and two adds per (i, j); every column is read once per row tile
        _prof_end(rec, 0.0, 4.0 * m * n * (1 + (n + 255) // 256), ("tied_ranks", m, n))
    return rank2


def rank_moments(rank2, *, out=None):
    """Column sums and the Gram matrix of ``tied_ranks``' output (``pti_rank_moments``) -> ``(sums, gram)``: int64 ``[M]``
    and int64 ``[M, M]`` device tensors, ``gram[a, b] = sum_i rank2[a, i] * rank2[b, i]`` in 64-bit integers: exact.
    ``rank2``: contiguous int32 ``[M, N]``.  ``out=(sums, gram)`` are written in place.  Current stream, no host sync."""
    who = "rank_moments"
    out = _outs(who, out, ("sums", "gram"))
    _tensor(rank2, I32, f"{who}: rank2", 2)
    m, n = rank2.shape
    if not (2 <= n <= DISENT_MAX_N and 1 <= m <= DISENT_MAX_COLS):
        raise ValueError(f"{who}: unsupported shape rank2 {tuple(rank2.shape)} (2 <= N <= {DISENT_MAX_N}, 1 <= M <= {DISENT_MAX_COLS})")
    sums = _out(out[0], (m,), I64, rank2.device, f"{who}: out[0] (sums)")
    gram = _out(out[1], (m, m), I64, rank2.device, f"{who}: out[1] (gram)")
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_rank_moments(_ptr(rank2), n, m, _ptr(sums), _ptr(gram), _stream()), "pti_rank_moments")
    if rec is not None:   # the pairs a <= b, two columns read per pair
        _prof_end(rec, 0.0, 4.0 * n * m * (m + 1), ("rank_moments", m, n))
    return sums, gram


def _edges(t, rows, bins, device, name):
    """Left bin edges ``[rows, bins]`` (tensor, array or nested sequence, host or device) as a contiguous fp64 device tensor."""
    t = torch.as_tensor(t)
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != bins:
        raise ValueError(f"{name}: expected [{rows}, {bins}] left edges, got {tuple(t.shape)}")
    if not t.is_floating_point():
        raise TypeError(f"{name}: expected floating-point edges, got {t.dtype}")
    return t.to(device=device, dtype=torch.float64).contiguous()


def joint_histogram(z, attrs, edges_z, edges_a, *, out=None):
    """Joint histograms of every (attribute, latent channel) over fixed bins (``pti_joint_histogram``) ->
    ``(bins_z, bins_a, counts)`` device tensors.

    ``z``: floating-point device matrix ``[N, L]`` in any layout -- a transposed view of a channel-major ``[L, N]`` buffer,
    row stride included, is used in place, anything else is copied once; ``attrs``: ``[na, N]`` with dense rows.
    ``edges_z`` ``[L, B]`` / ``edges_a`` ``[na, B]``: the ascending LEFT edges of every column's bins (host or device; used as
    fp64).  ``bin(x) = #{k: edges[k] <= x} - 1``: the last bin takes everything from its edge upwards.  ``bins_z`` uint8
    ``[L, N]``, ``bins_a`` uint8 ``[na, N]``; ``counts`` int32 ``[na, L, B, B]`` indexed ``[q, c, bin_a, bin_z]``, exact; every
    table sums to ``N`` and its row / column sums are the marginals.  ``out=(bins_z, bins_a, counts)`` are written in place.
    A value below its column's first edge has no bin and is refused with a ValueError -- the one check that reads a
    device result back (one host synchronisation per call).  2 <= N <= 32768, L <= 16, na <= 16, 2 <= B <= 32.  Runs on
    the current stream; bitwise reproducible; the scratch buffer is cached per (stream, shape)."""
    who = "joint_histogram"
    out = _outs(who, out, ("bins_z", "bins_a", "counts"))
    zt, attrs, n, l, na, ldz, lda = _latent_attrs(who, z, attrs)
    edges_z = torch.as_tensor(edges_z)
    bins = int(edges_z.shape[1]) if edges_z.dim() == 2 else 0
    if not (2 <= n <= DISENT_MAX_N and 1 <= l <= 16 and 1 <= na <= 16 and 2 <= bins <= DISENT_MAX_BINS):
        raise ValueError(f"{who}: unsupported shape z {tuple(z.shape)} attrs {tuple(attrs.shape)} bins {bins} (2 <= N <= "
                         f"{DISENT_MAX_N}, 1 <= L <= 16, 1 <= na <= 16, 2 <= B <= {DISENT_MAX_BINS})")
    edges_z = _edges(edges_z, l, bins, z.device, f"{who}: edges_z")
    edges_a = _edges(edges_a, na, bins, z.device, f"{who}: edges_a")
    low = torch.cat([zt.amin(1).double() < edges_z[:, 0], attrs.amin(1).double() < edges_a[:, 0]])
    if bool(low.any()):                                      # the host synchronisation of this wrapper
        col = int(low.nonzero()[0])
        raise ValueError(f"{who}: {'channel ' + str(col) if col < l else 'attribute ' + str(col - l)} holds a value below its "
                         "first edge: it has no bin")
    bins_z = _out(out[0], (l, n), torch.uint8, z.device, f"{who}: out[0] (bins_z)")
    bins_a = _out(out[1], (na, n), torch.uint8, z.device, f"{who}: out[1] (bins_a)")
    counts = _out(out[2], (na, l, bins, bins), torch.int32, z.device, f"{who}: out[2] (counts)")
    stream = _stream()
    nbytes = L.lib().pti_joint_histogram_ws_bytes(n, l, na, bins)
    ws, ws_bytes = _scratch_bytes(who, "jhist", (n, l, na, bins), nbytes,
                                  f"z {tuple(z.shape)} attrs {tuple(attrs.shape)} bins {bins}", z.device, stream)
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_joint_histogram(_ptr(zt), ldz, _ptr(attrs), lda, n, l, na, bins, _ptr(edges_z), _ptr(edges_a),
                                        _ptr(bins_z), _ptr(bins_a), _ptr(counts), _ptr(ws), ws_bytes, stream),
            "pti_joint_histogram")
    if rec is not None:   # the values once, the bin indices once per partner column, the partial tables twice
        _prof_end(rec, 0.0, 5.0 * n * (l + na) + 2.0 * n * l * na + 2.0 * nbytes + 4.0 * counts.numel(),
                  ("joint_histogram", l, na, n, bins))
    return bins_z, bins_a, counts


# ---- k-nearest-neighbour mutual information (csrc/ksg.hip; include/pti_vae.h "k-nearest-neighbour mutual information") ----
KSG_MAX_K, KSG_MAX_N = 16, 32768   # the bounds of pti_ksg_counts (L and na: RANK_AGREEMENT_MAX_L / _NA)


def ksg_counts(z, attrs, k, *, out=None):
    """Neighbour radii and range counts of the KSG mutual-information estimator for every (attribute, latent channel)
    (``pti_ksg_counts``) -> ``(eps, nx, ny)`` device tensors.

    ``z``: floating-point device matrix ``[N, L]`` in any layout -- a transposed view of a channel-major ``[L, N]`` buffer,
    row stride included, is used in place, anything else is copied once; ``attrs``: ``[na, N]`` with dense rows; ``k``: the
    neighbour count.  With ``dx = |x_i - x_j|``, ``dy = |y_i - y_j|`` (one fp32 subtraction each) for the channel ``x`` and the
    attribute ``y`` of a pair: ``eps`` fp32 ``[na, L, N]`` is the ``k``-th smallest ``max(dx, dy)`` over the OTHER rows, ``nx`` /
    ``ny`` int32 ``[na, L, N]`` count the other rows with ``dx`` / ``dy`` at most the largest fp32 below ``eps`` (at most 0 when
    ``eps == 0``: exact duplicates) -- scikit-learn's ``_compute_mi_cc`` before its digammas; ``utils.disentanglement.
    ksg_mutual_information`` turns the counts into MI.  ``out=(eps, nx, ny)`` are written in place.  1 <= k <= 16,
    k + 1 <= N <= 32768, L <= 16, na <= 16.  A non-finite value is refused with a ValueError that names its column -- the
    one check that reads a device result back (one host synchronisation per call).  Runs on the current stream; exact,
    bitwise reproducible, no scratch buffer."""
    who = "ksg_counts"
    out = _outs(who, out, ("eps", "nx", "ny"))
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{who}: k: expected an int, got {type(k).__name__}")
    zt, attrs, n, l, na, ldz, lda = _latent_attrs(who, z, attrs)
    if not 1 <= k <= KSG_MAX_K:
        raise ValueError(f"{who}: k = {k} out of range (1 <= k <= {KSG_MAX_K})")
    if not (k + 1 <= n <= KSG_MAX_N and 1 <= l <= RANK_AGREEMENT_MAX_L and 1 <= na <= RANK_AGREEMENT_MAX_NA):
        raise ValueError(f"{who}: unsupported shape z {tuple(z.shape)} attrs {tuple(attrs.shape)} k {k} (k + 1 <= N <= {KSG_MAX_N}, "
                         f"1 <= L <= {RANK_AGREEMENT_MAX_L}, 1 <= na <= {RANK_AGREEMENT_MAX_NA})")
    bad = torch.cat([~torch.isfinite(zt).all(1), ~torch.isfinite(attrs).all(1)])
    if bool(bad.any()):                                      # the host synchronisation of this wrapper
        col = int(bad.nonzero()[0])
        raise ValueError(f"{who}: {'channel ' + str(col) if col < l else 'attribute ' + str(col - l)} holds a non-finite value")
    eps = _out(out[0], (na, l, n), F32, z.device, f"{who}: out[0] (eps)")
    nx = _out(out[1], (na, l, n), torch.int32, z.device, f"{who}: out[1] (nx)")
    ny = _out(out[2], (na, l, n), torch.int32, z.device, f"{who}: out[2] (ny)")
    prof = KERNEL_PROFILE
    rec = None if prof is None else _prof_begin(prof)
    L.check(L.lib().pti_ksg_counts(_ptr(zt), ldz, _ptr(attrs), lda, n, l, na, k, _ptr(eps), _ptr(nx), _ptr(ny), _stream()),
            "pti_ksg_counts")
    if rec is not None:   # both columns of a pair are read twice per row tile; three outputs
        _prof_end(rec, 0.0, 4.0 * l * na * n * (4 * ((n + 255) // 256) + 3), ("ksg_counts", l, na, n, k))
    return eps, nx, ny


# ---- projection quality (csrc/projection_quality.hip; include/pti_vae.h "projection quality") --------------------------
NEIGHBOR_RANKS_MAX_N, NEIGHBOR_RANKS_MAX_M, SEGMENT_ROW_SUMS_MAX_G = 8192, 256, 2048


PROJECTION_MAX_COLS = 8


def projection_distances(y, *, out=None):
    """Euclidean distances between the rows of a PROJECTION ``y`` [n, d], d <= 8 (``pti_projection_distances``) -> fp32
    ``[n, n]``: differences, squares, sum and root in fp64, rounded to fp32 once.  Two entries of a row are therefore ordered
    as the true distances are unless they round to the same fp32 (``latent_pairwise`` accumulates in fp32 and orders
    distances a few units in the last place apart by its rounding).  Symmetric bit for bit with a zero diagonal.  A
    row-strided ``y`` and an ``out`` view with a row stride are used in place.  1 <= n <= 8192.  Runs on the current stream,
    no host sync."""
    y = _dense_rows(y, "projection_distances: y", copy=True)
    n, d = y.shape
    if not (1 <= n <= NEIGHBOR_RANKS_MAX_N and 1 <= d <= PROJECTION_MAX_COLS):
        raise ValueError(f"projection_distances: unsupported shape {tuple(y.shape)} (1 <= n <= {NEIGHBOR_RANKS_MAX_N}, "
                         f"1 <= d <= {PROJECTION_MAX_COLS})")
    out = _rows_out(out, (n, n), F32, y.device, "projection_distances")
    L.check(L.lib().pti_projection_distances(_ptr(y), y.stride(0), n, d, _ptr(out), out.stride(0), _stream()),
            "pti_projection_distances")
    return out


def neighbor_ranks(dist, nbr_idx, *, out=None):
    """The rank, within row ``i`` of the fp32 distance matrix ``dist`` [n, n], of every listed neighbour ``nbr_idx[i, c]``
    (``pti_neighbor_ranks``) -> int32 ``[n, m]``: ``1 + #{l != i : key(i, l) < key(i, j)}`` under ``umap_knn``'s order
    (distance, then column; -0 is 0), so "rank <= k" is the set ``umap_knn`` returns once the diagonal is left out.  An
    entry equal to its own row gives 0, an index outside ``[0, n)`` gives -1.  ``dist`` is used in place (a row stride is
    allowed); ``nbr_idx`` int32 ``[n, m]`` contiguous.  3 <= n <= 8192, 1 <= m <= 256.  Integers only: exact; a row of the
    result depends on that row of ``dist`` and of ``nbr_idx`` alone.  Runs on the current stream, no host sync."""
    who = "neighbor_ranks"
    dist = _dense_rows(dist, f"{who}: dist", square=True)
    _tensor(nbr_idx, I32, f"{who}: nbr_idx", 2)
    n, m = dist.shape[0], nbr_idx.shape[1]
    if nbr_idx.shape[0] != n or nbr_idx.device != dist.device:
        raise ValueError(f"{who}: nbr_idx must be [{n}, m] on {dist.device}, got {tuple(nbr_idx.shape)} on {nbr_idx.device}")
    if not (3 <= n <= NEIGHBOR_RANKS_MAX_N and 1 <= m <= NEIGHBOR_RANKS_MAX_M):
        raise ValueError(f"{who}: unsupported shape dist {tuple(dist.shape)} nbr_idx {tuple(nbr_idx.shape)} "
                         f"(3 <= n <= {NEIGHBOR_RANKS_MAX_N}, 1 <= m <= {NEIGHBOR_RANKS_MAX_M})")
    out = _out(out, (n, m), I32, dist.device, f"{who}: out")
    L.check(L.lib().pti_neighbor_ranks(_ptr(dist), dist.stride(0), n, _ptr(nbr_idx), m, _ptr(out), _stream()),
            "pti_neighbor_ranks")
    return out


def segment_row_sums(dist, seg, *, out=None):
    """Per-segment sums of every row of the fp32 distance matrix ``dist`` [n, n] (``pti_segment_row_sums``) -> fp64
    ``[n, G]``: ``out[i, g] = sum_{j = seg[g]}^{seg[g+1]-1} (double)dist[i, j]``.  ``seg``: the ``G + 1`` ascending int32
    offsets with ``seg[0] = 0`` and ``seg[G] = n`` (``latent_group_stats``'s ``seg_a`` convention), as a host sequence / CPU
    tensor (checked on the host, copied to the device) or an int32 device vector (checked through one read-back, the only
    host synchronisation here).  The fp32 values are widened as they are loaded -- no fp64 copy of the matrix -- and added in
    one order that depends on the segment's length alone: the bits of an entry depend on its row and its segment, not on
    ``n``, ``G`` or the launch.  An empty segment gives 0.0.  3 <= n <= 8192, 1 <= G <= 2048.  Runs on the current stream."""
    who = "segment_row_sums"
    dist = _dense_rows(dist, f"{who}: dist", square=True)
    n = dist.shape[0]
    if not isinstance(seg, torch.Tensor):
        seg = torch.tensor([int(v) for v in seg], dtype=I32)
    _offsets(who, "seg", seg, dist.device, "G", host=True)
    host = seg.tolist()
    g = len(host) - 1
    if not (3 <= n <= NEIGHBOR_RANKS_MAX_N and 1 <= g <= SEGMENT_ROW_SUMS_MAX_G):
        raise ValueError(f"{who}: unsupported shape dist {tuple(dist.shape)} with {g} segments "
                         f"(3 <= n <= {NEIGHBOR_RANKS_MAX_N}, 1 <= G <= {SEGMENT_ROW_SUMS_MAX_G})")
    if host[0] != 0 or host[-1] != n or any(b < a for a, b in zip(host, host[1:])):
        raise ValueError(f"{who}: seg must ascend from 0 to n = {n}, got {host[0]} .. {host[-1]}")
    if not seg.is_cuda:
        seg = seg.to(dist.device)
    out = _out(out, (n, g), torch.float64, dist.device, f"{who}: out")
    L.check(L.lib().pti_segment_row_sums(_ptr(dist), dist.stride(0), n, _ptr(seg), g, _ptr(out), _stream()),
            "pti_segment_row_sums")
    return out


# ---- co-ranking curves and the Shepard figure (csrc/coranking.hip; include/pti_vae.h "co-ranking curves") --------------
CORANKING_MIN_N, CORANKING_MAX_N, SHEPARD_MIN_BINS, SHEPARD_MAX_BINS = 4, 8192, 2, 128


def _coranking_rows(t, dtype, name):
    """A device matrix [m, n] of ``dtype`` with dense rows and 4 <= n <= 8192, 1 <= m <= n, used in place."""
    m, n = _dense_rows(t, name, dtype).shape
    if not (CORANKING_MIN_N <= n <= CORANKING_MAX_N and 1 <= m <= n):
        raise ValueError(f"{name}: unsupported shape {tuple(t.shape)} ({CORANKING_MIN_N} <= n <= {CORANKING_MAX_N} columns, "
                         f"1 <= m <= n rows)")
    return t


def full_ranks(dist, row_offset=0, *, out=None):
    """The rank of EVERY column within every row of the fp32 distance rows ``dist`` [m, n] (``pti_full_ranks``) -> int16
    ``[m, n]``.  ``dist`` holds rows ``row_offset .. row_offset + m - 1`` of an ``n``-column matrix (the whole matrix when it
    is square and ``row_offset`` is 0): ``out[r, j] = 1 + #{l != i : key(i, l) < key(i, j)}`` with ``i = row_offset + r``
    under ``neighbor_ranks``' order (distance, then column; -0 is 0) and 0 at the row's own column, so a row is a
    permutation of ``0 .. n - 1`` and ``full_ranks(d).gather(1, idx)`` is ``neighbor_ranks(d, idx)``.  One workgroup sorts a
    row's 64-bit keys in LDS.  ``dist`` and an ``out`` view with a row stride are used in place.  4 <= n <= 8192.
    Comparisons only: exact.  Runs on the current stream, no host sync."""
    who = "full_ranks"
    dist = _coranking_rows(dist, F32, f"{who}: dist")
    m, n = dist.shape
    row_offset = int(row_offset)
    if not 0 <= row_offset <= n - m:
        raise ValueError(f"{who}: rows {row_offset} .. {row_offset + m - 1} are outside the matrix of {n} rows")
    out = _rows_out(out, (m, n), I16, dist.device, who)
    L.check(L.lib().pti_full_ranks(_ptr(dist), dist.stride(0), m, n, row_offset, _ptr(out), out.stride(0), _stream()),
            "pti_full_ranks")
    return out


def coranking_fold(rank_high, rank_low, hist=None):
    """The co-ranking histograms of two int16 rank tables ``[m, n]`` of the same rows (``pti_coranking_fold``) ->
    ``(hist, sqdiff)``.  ``hist`` uint32-valued int32 ``[3, n]``: for every entry with both ranks in ``[1, n - 1]``, bin
    ``max(rank_high, rank_low)`` of row 0 (equal ranks), 1 (``rank_low < rank_high``: an intrusion) or 2 (an extrusion)
    is raised; anything else -- the own column's 0, a foreign value -- is skipped.  A ``hist`` handed in is ADDED to, so
    calls over row blocks compose; without one a zeroed table is made.  ``sqdiff`` int64 ``[m]``: the row's sum of
    ``(rank_high - rank_low)^2``.  Integer atomics only: exact and independent of scheduling.  Current stream, no host sync."""
    who = "coranking_fold"
    rank_high = _coranking_rows(rank_high, I16, f"{who}: rank_high")
    rank_low = _coranking_rows(rank_low, I16, f"{who}: rank_low")
    m, n = rank_high.shape
    if tuple(rank_low.shape) != (m, n) or rank_low.device != rank_high.device:
        raise ValueError(f"{who}: rank_low must be [{m}, {n}] on {rank_high.device}, got {tuple(rank_low.shape)}")
    if hist is None:
        hist = torch.zeros((3, n), dtype=I32, device=rank_high.device)
    else:
        hist = _out(hist, (3, n), I32, rank_high.device, f"{who}: hist")
    sqdiff = torch.empty((m,), dtype=torch.int64, device=rank_high.device)
    L.check(L.lib().pti_coranking_fold(_ptr(rank_high), rank_high.stride(0), _ptr(rank_low), rank_low.stride(0), m, n,
                                       _ptr(hist), _ptr(sqdiff), _stream()), "pti_coranking_fold")
    return hist, sqdiff


def shepard_fold(dist_high, dist_low, bins=64, *, hist=None):
    """The Shepard figure's raw material from two fp32 distance matrices ``[n, n]`` (``pti_shepard_fold``) ->
    ``(sums, hist, scale)``.  ``sums`` fp64 ``[n, 3]``: per row the sums of ``d_high^2``, ``d_low^2`` and ``d_high d_low``
    over the other columns, the products exact in fp64, added in one fixed order (the bits depend on the row and ``n``).
    ``hist`` int32 ``[bins, bins]``: the count of ordered pairs in cell ``(min(bins - 1, int(d_high * scale[0])),
    min(bins - 1, int(d_low * scale[1])))``, products in fp32; ``+inf`` goes to the last bin; a ``hist`` handed in is ADDED
    to.  ``scale`` fp32 device pair: ``bins / (largest finite entry)`` of each matrix, 0 where that entry is 0 -- formed here
    by torch, since the library's own division is not correctly rounded; bin ``b`` covers ``[b / scale, (b + 1) / scale)``.
    4 <= n <= 8192, 2 <= bins <= 128.  Runs on the current stream, no host sync."""
    who = "shepard_fold"
    dist_high = _dense_rows(dist_high, f"{who}: dist_high", square=True)
    dist_low = _dense_rows(dist_low, f"{who}: dist_low", square=True)
    n, bins = dist_high.shape[0], int(bins)
    if tuple(dist_low.shape) != (n, n) or dist_low.device != dist_high.device:
        raise ValueError(f"{who}: dist_low must be [{n}, {n}] on {dist_high.device}, got {tuple(dist_low.shape)}")
    if not (CORANKING_MIN_N <= n <= CORANKING_MAX_N and SHEPARD_MIN_BINS <= bins <= SHEPARD_MAX_BINS):
        raise ValueError(f"{who}: unsupported shape n = {n}, bins = {bins} ({CORANKING_MIN_N} <= n <= {CORANKING_MAX_N}, "
                         f"{SHEPARD_MIN_BINS} <= bins <= {SHEPARD_MAX_BINS})")
    top = torch.stack([torch.where(torch.isfinite(d), d, torch.zeros((), dtype=F32, device=d.device)).max()
                       for d in (dist_high, dist_low)])
    # a tensor over a tensor: one correctly rounded division (a Python number over a tensor is reciprocal-then-multiply)
    scale = torch.where(top > 0, torch.full_like(top, float(bins)) / top, torch.zeros_like(top)).contiguous()
    if hist is None:
        hist = torch.zeros((bins, bins), dtype=I32, device=dist_high.device)
    else:
        hist = _out(hist, (bins, bins), I32, dist_high.device, f"{who}: hist")
    sums = torch.empty((n, 3), dtype=torch.float64, device=dist_high.device)
    L.check(L.lib().pti_shepard_fold(_ptr(dist_high), dist_high.stride(0), _ptr(dist_low), dist_low.stride(0), n, _ptr(scale),
                                     bins, _ptr(sums), _ptr(hist), _stream()), "pti_shepard_fold")
    return sums, hist, scale


# ---- PatchDiscriminator passes (csrc/discriminator.hip; include/pti_vae.h "PatchDiscriminator") -----------------------
def pd_out_hw(h, w, stride):
    return (h + 2 - 4) // stride + 1, (w + 2 - 4) // stride + 1


def pd_im2col_image(img, patches):
    """img fp32 [B,1,H,W] (or [B,H,W]) -> patches bf16 [B,H/2,W/2,32] of the 4x4 stride-2 pad-1 window (+16 zero columns)."""
    _chk(img, F32, "img")
    _chk(patches, BF16, "patches", 4)
    b, h, w = img.shape[0], img.shape[-2], img.shape[-1]
    if img.numel() != b * h * w or tuple(patches.shape) != (b, h // 2, w // 2, 32):
        raise ValueError(f"pd_im2col_image: img {tuple(img.shape)} / patches {tuple(patches.shape)}")
    L.check(L.lib().pti_pd_im2col_image(_ptr(img), _ptr(patches), b, h, w, _stream()), "pti_pd_im2col_image")
    return patches


def pd_im2col(src, norm, patches, *, stride, act=True, slope=0.2):
    _chk(src, BF16, "src", 4)
    _chk(patches, BF16, "patches", 4)
    n, h, w, c = src.shape
    ho, wo = pd_out_hw(h, w, stride)
    if tuple(patches.shape) != (n, ho, wo, 16 * c):
        raise ValueError(f"pd_im2col: patches {tuple(patches.shape)} != {(n, ho, wo, 16 * c)}")
    if norm is not None:
        _chk(norm, F32, "norm")
        if norm.numel() != n * c * 2:
            raise ValueError("pd_im2col: norm table size")
    L.check(L.lib().pti_pd_im2col(_ptr(src), _ptr(norm), _ptr(patches), n, h, w, c, stride, int(act), float(slope), _stream()),
            "pti_pd_im2col")
    return patches


def pd_in_stats(y, eps=1e-5, table=None):
    _chk(y, BF16, "y", 4)
    n, h, w, c = y.shape
    if table is None:
        table = torch.empty(n, c, 2, dtype=F32, device=y.device)
    L.check(L.lib().pti_pd_in_stats(_ptr(y), _ptr(table), n, h * w, c, float(eps), _stream()), "pti_pd_in_stats")
    return table


def _pd_norm_sums(norm, g, launch):
    """Shared tail of pd_col2im / pd_final_dgrad, whose kernels write ``g`` [n, h, w, c]: ``launch(part)`` with the block
    partials of the InstanceNorm-backward sums (None without ``norm``), then their fixed-order fold by
    pti_gn_sums_finalize -> sums [n, c, 2] | None."""
    n, h, w, c = g.shape
    if norm is None:
        launch(None)
        return None
    part = torch.empty(n, L.lib().pti_pd_col2im_blocks(n, h * w, c), c, 2, dtype=F32, device=g.device)
    launch(part)
    sums = torch.empty(n, c, 2, dtype=F32, device=g.device)
    L.check(L.lib().pti_gn_sums_finalize(_ptr(part), _ptr(sums), n, part.shape[1], 2 * c, _stream()), "pti_gn_sums_finalize")
    return sums


def pd_col2im(d_patches, y_prev, norm, g, *, stride, slope=0.2):
    """-> (g, sums [n,c,2] | None): g = LeakyReLU'(norm(y_prev)) * col2im(d_patches); with ``norm`` also the
    InstanceNorm-backward sums {sum g, sum g*xhat} (block partials folded in fixed order by pti_gn_sums_finalize)."""
    _chk(d_patches, BF16, "d_patches", 4)
    _chk(y_prev, BF16, "y_prev", 4)
    _chk(g, BF16, "g", 4)
    n, h, w, c = y_prev.shape
    ho, wo = pd_out_hw(h, w, stride)
    if tuple(d_patches.shape) != (n, ho, wo, 16 * c) or g.shape != y_prev.shape:
        raise ValueError(f"pd_col2im: d_patches {tuple(d_patches.shape)} for y_prev {tuple(y_prev.shape)} stride {stride}")
    if norm is not None:
        _chk(norm, F32, "norm")
    return g, _pd_norm_sums(norm, g, lambda part: L.check(
        L.lib().pti_pd_col2im(_ptr(d_patches), _ptr(y_prev), _ptr(norm), _ptr(g), _ptr(part), n, h, w, c, stride,
                              float(slope), _stream()), "pti_pd_col2im"))


def pd_col2im_image(d_patches, d_img, *, scale=1.0, accumulate=False):
    _chk(d_patches, BF16, "d_patches", 4)
    _chk(d_img, F32, "d_img")
    n, ho, wo, k = d_patches.shape
    if k != 32 or d_img.numel() != n * 4 * ho * wo:
        raise ValueError("pd_col2im_image: shapes")
    L.check(L.lib().pti_pd_col2im_image(_ptr(d_patches), _ptr(d_img), n, 2 * ho, 2 * wo, float(scale), int(accumulate),
                                        _stream()), "pti_pd_col2im_image")
    return d_img


def pd_in_bwd_apply(g, y, norm, sums, dy=None):
    _chk(g, BF16, "g", 4)
    _chk(y, BF16, "y", 4)
    n, h, w, c = y.shape
    dy = g if dy is None else dy
    L.check(L.lib().pti_pd_in_bwd_apply(_ptr(g), _ptr(y), _ptr(norm), _ptr(sums), _ptr(dy), n, h * w, c, _stream()),
            "pti_pd_in_bwd_apply")
    return dy


def pd_lsgan(logits_rows, *, target, slope=0.05, grad_scale=0.0, d_logits=None):
    """logits_rows: [M, stride], the logit in column 0 -- 16-bit padded rows, or fp32 (the direct final block: stride 1).
    Returns the one-element fp32 device tensor mean((LeakyReLU_slope(l) - target)^2); ``d_logits`` (same shape; bf16
    for 16-bit logits, fp32 for fp32 logits) gets grad_scale * (a - target) * LeakyReLU'(l) in column 0 (16-bit rows:
    zeros elsewhere)."""
    _chk(logits_rows, (BF16, F16, F32), "logits", 2)
    m, stride = logits_rows.shape
    fmt = 2 if logits_rows.dtype == F32 else int(logits_rows.dtype == F16)
    if d_logits is not None:
        _chk(d_logits, F32 if fmt == 2 else BF16, "d_logits", 2)
        if d_logits.shape != logits_rows.shape:
            raise ValueError("pd_lsgan: d_logits shape")
    buf = torch.empty(1 + L.lib().pti_pd_lsgan_blocks(m), dtype=F32, device=logits_rows.device)
    L.check(L.lib().pti_pd_lsgan(_ptr(logits_rows), fmt, stride, m, float(target), float(slope), float(grad_scale), _ptr(buf),
                                 _ptr(d_logits), _stream()), "pti_pd_lsgan")
    return buf[:1]


def pd_final_fwd(y_prev, norm, w16c, bias, logits, *, slope=0.2):
    """Final discriminator block without a patch matrix: logits fp32 [n, h-1, w-1] = conv4x4(LeakyReLU(norm(y_prev)), w) + b;
    w16c fp32 [16*c] (tap-major), bias fp32 [>=1]."""
    _chk(y_prev, BF16, "y_prev", 4)
    _chk(logits, F32, "logits", 3)
    n, h, w, c = y_prev.shape
    if tuple(logits.shape) != (n, h - 1, w - 1) or w16c.numel() != 16 * c:
        raise ValueError("pd_final_fwd: shapes")
    L.check(L.lib().pti_pd_final_fwd(_ptr(y_prev), _ptr(norm), _ptr(w16c), _ptr(bias), _ptr(logits), n, h, w, c, float(slope),
                                     _stream()), "pti_pd_final_fwd")
    return logits


def pd_final_dgrad(d_logits, y_prev, norm, w16c, g, *, slope=0.2):
    """-> (g, sums | None) like pd_col2im, for the direct final block (d_logits fp32 [n, h-1, w-1])."""
    _chk(d_logits, F32, "d_logits")
    _chk(y_prev, BF16, "y_prev", 4)
    _chk(g, BF16, "g", 4)
    n, h, w, c = y_prev.shape
    if d_logits.numel() != n * (h - 1) * (w - 1) or g.shape != y_prev.shape or w16c.numel() != 16 * c:
        raise ValueError("pd_final_dgrad: shapes")
    return g, _pd_norm_sums(norm, g, lambda part: L.check(
        L.lib().pti_pd_final_dgrad(_ptr(d_logits), _ptr(y_prev), _ptr(norm), _ptr(w16c), _ptr(g), _ptr(part), n, h, w, c,
                                   float(slope), _stream()), "pti_pd_final_dgrad"))


def pd_final_wgrad(d_logits, y_prev, norm, *, slope=0.2):
    """-> fp32 [16*c + 8]: {dw[16][c], dbias, 0...} of the direct final block (block partials summed in block order)."""
    _chk(d_logits, F32, "d_logits")
    _chk(y_prev, BF16, "y_prev", 4)
    n, h, w, c = y_prev.shape
    if d_logits.numel() != n * (h - 1) * (w - 1):
        raise ValueError("pd_final_wgrad: shapes")
    blocks = L.lib().pti_pd_final_wgrad_blocks(n, h, w)
    row = 16 * c + 8
    part = torch.empty(blocks, row, dtype=F32, device=y_prev.device)
    L.check(L.lib().pti_pd_final_wgrad(_ptr(d_logits), _ptr(y_prev), _ptr(norm), _ptr(part), n, h, w, c, float(slope), _stream()),
            "pti_pd_final_wgrad")
    out = torch.empty(row, dtype=F32, device=y_prev.device)
    L.check(L.lib().pti_gn_sums_finalize(_ptr(part), _ptr(out), 1, blocks, row, _stream()), "pti_gn_sums_finalize")
    return out


# ---- LPIPS comparison tail (perceptual term) -------------------------------------------------------------
def lpips_tap_fwd(a, b, w):
    """a, b: fp32 NCHW feature maps [n, c, h, w_] (contiguous), w: fp32 [c] -> (value [n], saved [n, 3, h*w_]):
    value_i = mean_p sum_c w_c (a_c/(|a_p|+1e-10) - b_c/(|b_p|+1e-10))^2 (lpips normalize_tensor + lin layer + spatial mean)."""
    _chk(a, F32, "a", 4)
    _chk(b, F32, "b", 4)
    _chk(w, F32, "w", 1)
    if a.shape != b.shape or w.numel() != a.shape[1]:
        raise ValueError("lpips_tap_fwd: shapes")
    n, c, h, ww = a.shape
    hw = h * ww
    blocks = L.lib().pti_lpips_tap_blocks(c, hw)
    if blocks <= 0:
        raise ValueError("lpips_tap_fwd: empty feature map")
    saved = torch.empty(n, 3, hw, dtype=F32, device=a.device)
    part = torch.empty(n, blocks, dtype=F32, device=a.device)
    L.check(L.lib().pti_lpips_tap_fwd(_ptr(a), _ptr(b), _ptr(w), _ptr(saved), _ptr(part), n, c, hw, _stream()), "pti_lpips_tap_fwd")
    return part.sum(1) / hw, saved


def lpips_tap_bwd(a, b, w, saved, gout):
    """-> d(sum_i gout_i * value_i) / d a, fp32 like a."""
    _chk(a, F32, "a", 4)
    _chk(b, F32, "b", 4)
    _chk(gout, F32, "gout", 1)
    n, c, h, ww = a.shape
    if a.shape != b.shape or tuple(saved.shape) != (n, 3, h * ww) or gout.numel() != n or w.numel() != c:
        raise ValueError("lpips_tap_bwd: shapes")
    ga = torch.empty_like(a)
    L.check(L.lib().pti_lpips_tap_bwd(_ptr(a), _ptr(b), _ptr(w), _ptr(saved), _ptr(gout), _ptr(ga), n, c, h * ww, _stream()),
            "pti_lpips_tap_bwd")
    return ga


# ---- trunk of the perceptual network (csrc/squeeze.hip) -----------------------------------------------------------------
def relu_f16_(x):
    _chk(x, F16, "x")
    L.check(L.lib().pti_relu_f16(_ptr(x), x.numel(), _stream()), "pti_relu_f16")
    return x


def relu_bwd_(g, y):
    """g (bf16) = y > 0 ? g : 0 in place; y: the fp16 ReLU output of the same shape."""
    _chk(g, BF16, "g")
    _chk(y, F16, "y")
    if g.shape != y.shape:
        raise ValueError("relu_bwd_: shapes")
    L.check(L.lib().pti_relu_bwd(_ptr(g), _ptr(y), g.numel(), _stream()), "pti_relu_bwd")
    return g


def relu_bwd_add_(g, g2, y):
    """g (bf16) = y > 0 ? g + g2 : 0 in place."""
    _chk(g, BF16, "g")
    _chk(g2, BF16, "g2")
    _chk(y, F16, "y")
    if g.shape != y.shape or g2.shape != y.shape:
        raise ValueError("relu_bwd_add_: shapes")
    L.check(L.lib().pti_relu_bwd_add(_ptr(g), _ptr(g2), _ptr(y), g.numel(), _stream()), "pti_relu_bwd_add")
    return g


def maxpool3s2_fwd(x):
    """MaxPool2d(3, 2, ceil_mode=True) on NHWC fp16."""
    _chk(x, F16, "x", 4)
    n, h, w, c = x.shape
    y = torch.empty(n, L.lib().pti_maxpool3s2_out(h), L.lib().pti_maxpool3s2_out(w), c, dtype=F16, device=x.device)
    L.check(L.lib().pti_maxpool3s2_fwd(_ptr(x), _ptr(y), n, h, w, c, _stream()), "pti_maxpool3s2_fwd")
    return y


def maxpool3s2_bwd(gy, x, y, gx=None):
    """-> gx (bf16, x's shape): gradient of maxpool3s2_fwd; accumulated into ``gx`` when given."""
    _chk(gy, BF16, "gy", 4)
    _chk(x, F16, "x", 4)
    _chk(y, F16, "y", 4)
    if gy.shape != y.shape:
        raise ValueError("maxpool3s2_bwd: shapes")
    n, h, w, c = x.shape
    acc = gx is not None
    if acc:
        _chk(gx, BF16, "gx", 4)
        if gx.shape != x.shape:
            raise ValueError("maxpool3s2_bwd: gx shape")
    else:
        gx = torch.empty(x.shape, dtype=BF16, device=x.device)
    L.check(L.lib().pti_maxpool3s2_bwd(_ptr(gy), _ptr(x), _ptr(y), _ptr(gx), n, h, w, c, int(acc), _stream()), "pti_maxpool3s2_bwd")
    return gx


def nchw_f32_to_nhwc_f16(x):
    """fp32 [n, c, h, w] -> fp16 [n, h, w, c] (c a multiple of 64)."""
    _chk(x, F32, "x", 4)
    n, c, h, w = x.shape
    y = torch.empty(n, h, w, c, dtype=F16, device=x.device)
    L.check(L.lib().pti_nchw_f32_to_nhwc_f16(_ptr(x), _ptr(y), n, c, h * w, _stream()), "pti_nchw_f32_to_nhwc_f16")
    return y


def nhwc_bf16_add_to_nchw_f32_(g, y):
    """y (fp32 [n, c, h, w]) += g (bf16 [n, h, w, c])."""
    _chk(g, BF16, "g", 4)
    _chk(y, F32, "y", 4)
    n, c, h, w = y.shape
    if tuple(g.shape) != (n, h, w, c):
        raise ValueError("nhwc_bf16_add_to_nchw_f32_: shapes")
    L.check(L.lib().pti_nhwc_bf16_add_to_nchw_f32(_ptr(g), _ptr(y), n, c, h * w, _stream()), "pti_nhwc_bf16_add_to_nchw_f32")
    return y


def pad_nchw_to_nhwc32(x, dtype_a, dtype_b=None):
    """fp32 [n, c, h, w] (1 <= c <= 8) -> 16-bit [n, h, w, 32] with channels >= c zero; a second copy in ``dtype_b`` (the
    weight gradient's bf16 operand next to the forward conv's fp16 one) comes out of the same pass."""
    _chk(x, F32, "x", 4)
    n, c, h, w = x.shape
    ya = torch.empty(n, h, w, 32, dtype=dtype_a, device=x.device)
    yb = torch.empty(n, h, w, 32, dtype=dtype_b, device=x.device) if dtype_b is not None else None
    L.check(L.lib().pti_pad_nchw_to_nhwc32(_ptr(x), _ptr(ya), _ptr(yb), n, c, h * w, int(dtype_a == F16),
                                           int(dtype_b == F16), _stream()), "pti_pad_nchw_to_nhwc32")
    return ya, yb


def slice_nhwc32_to_nchw(x, c, out=None):
    """The first ``c`` channels of a 16-bit [n, h, w, 32] tensor -> fp32 [n, c, h, w]."""
    _chk(x, ACT16, "x", 4)
    n, h, w, c32 = x.shape
    if c32 != 32:
        raise ValueError("slice_nhwc32_to_nchw: expected 32 channels")
    y = out if out is not None else torch.empty(n, c, h, w, dtype=F32, device=x.device)
    _chk(y, F32, "y", 4)
    L.check(L.lib().pti_slice_nhwc32_to_nchw(_ptr(x), _ptr(y), n, c, h * w, int(x.dtype == F16), _stream()),
            "pti_slice_nhwc32_to_nchw")
    return y


def lpips_tap_nhwc_supported(c):
    return L.lib().pti_lpips_tap_nhwc_blocks(int(c), 1) > 0


def lpips_tap_nhwc_fwd(a, b, w):
    """lpips_tap_fwd on NHWC fp16 maps [n, h, w_, c] -> (value [n], saved [n, 3, h*w_])."""
    _chk(a, F16, "a", 4)
    _chk(b, F16, "b", 4)
    _chk(w, F32, "w", 1)
    if a.shape != b.shape or w.numel() != a.shape[3]:
        raise ValueError("lpips_tap_nhwc_fwd: shapes")
    n, h, ww, c = a.shape
    hw = h * ww
    blocks = L.lib().pti_lpips_tap_nhwc_blocks(c, hw)
    if blocks <= 0:
        raise ValueError(f"lpips_tap_nhwc_fwd: unsupported channel count {c}")
    saved = torch.empty(n, 3, hw, dtype=F32, device=a.device)
    part = torch.empty(n, blocks, dtype=F32, device=a.device)
    L.check(L.lib().pti_lpips_tap_nhwc_fwd(_ptr(a), _ptr(b), _ptr(w), _ptr(saved), _ptr(part), n, c, hw, _stream()),
            "pti_lpips_tap_nhwc_fwd")
    return part.sum(1) / hw, saved


def lpips_tap_nhwc_bwd(a, b, w, saved, gout):
    """-> d(sum_i gout_i * value_i) / d a as NHWC bf16."""
    _chk(a, F16, "a", 4)
    _chk(b, F16, "b", 4)
    _chk(gout, F32, "gout", 1)
    n, h, ww, c = a.shape
    if a.shape != b.shape or tuple(saved.shape) != (n, 3, h * ww) or gout.numel() != n or w.numel() != c:
        raise ValueError("lpips_tap_nhwc_bwd: shapes")
    ga = torch.empty(a.shape, dtype=BF16, device=a.device)
    L.check(L.lib().pti_lpips_tap_nhwc_bwd(_ptr(a), _ptr(b), _ptr(w), _ptr(saved), _ptr(gout), _ptr(ga), n, c, h * ww, _stream()),
            "pti_lpips_tap_nhwc_bwd")
    return ga


def squeeze_conv1_fwd(x, w10):
    """x fp32 [n, 1, h, w] (or [n, h, w]) -> tap 0 of the perceptual network, fp16 [n, (h-3)//2+1, (w-3)//2+1, 64];
    w10: the folded first layer, fp32 [10, 64] (perceptual_engine.fold_first_layer)."""
    _chk(x, F32, "x")
    _chk(w10, F32, "w10")
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3 or w10.numel() != 640:
        raise ValueError("squeeze_conv1_fwd: expected a one-channel image batch and a [10, 64] table")
    n, h, w = x.shape
    y = torch.empty(n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, 64, dtype=F16, device=x.device)
    L.check(L.lib().pti_squeeze_conv1_fwd(_ptr(x), _ptr(w10), _ptr(y), n, h, w, _stream()), "pti_squeeze_conv1_fwd")
    return y


def squeeze_conv1_bwd(g, t0, w10, h, w):
    """g bf16 [n, ho, wo, 64] (gradient w.r.t. tap 0), t0 = the forward's output (None: g already carries the ReLU
    mask) -> dx fp32 [n, 1, h, w]."""
    _chk(g, BF16, "g", 4)
    _chk(w10, F32, "w10")
    n = g.shape[0]
    if t0 is not None:
        _chk(t0, F16, "t0", 4)
    if (t0 is not None and g.shape != t0.shape) or tuple(g.shape[1:]) != ((h - 3) // 2 + 1, (w - 3) // 2 + 1, 64):
        raise ValueError("squeeze_conv1_bwd: shapes")
    dx = torch.empty(n, 1, h, w, dtype=F32, device=g.device)
    L.check(L.lib().pti_squeeze_conv1_bwd(_ptr(g), _ptr(t0), _ptr(w10), _ptr(dx), n, h, w, _stream()), "pti_squeeze_conv1_bwd")
    return dx


# ---- regression head, evaluation side (csrc/regression_head.hip; include/pti_vae.h "regression head") -----------------
MLP_MAX_LAYERS, MLP_MAX_WIDTH, MLP_MAX_OUT = 8, 1024, 64    # PTI_MLP_MAX_* of include/pti_vae.h
MLP_ACTS = ("relu", "gelu", "leaky_relu", "elu")            # activation codes 0 .. 3 of pti_mlp_head_fwd
MLP_LOSSES = {"mse": 0, "mse_loss": 0, "smooth_l1": 1, "huber": 1}


def mlp_head_pack(regressor):
    """``LatentRegressor`` -> ``(params, dims, act)``: one flat fp32 tensor ``W0, b0, W1, b1, ...`` (``nn.Linear`` layout)
    on the head's device, the layer widths ``[in, hidden..., out]`` and the activation's code (0 when there is no hidden
    layer).  Dropout layers are skipped: the kernel is the eval-mode forward."""
    from torch import nn
    kinds = {nn.ReLU: 0, nn.GELU: 1, nn.LeakyReLU: 2, nn.ELU: 3}
    linears, acts = [], set()
    for m in regressor.mlp:
        if isinstance(m, nn.Linear):
            linears.append(m)
        elif type(m) in kinds:
            acts.add(kinds[type(m)])
        elif not isinstance(m, nn.Dropout):
            raise TypeError(f"mlp_head_pack: unsupported layer {type(m).__name__}")
    if not linears or len(acts) > 1:
        raise ValueError("mlp_head_pack: expected nn.Linear layers with one kind of activation between them")
    for m in regressor.mlp:
        if isinstance(m, nn.GELU) and getattr(m, "approximate", "none") != "none":
            raise ValueError("mlp_head_pack: only the exact (erf) GELU is built")
        if isinstance(m, nn.LeakyReLU) and m.negative_slope != 0.01 or isinstance(m, nn.ELU) and m.alpha != 1.0:
            raise ValueError("mlp_head_pack: only LeakyReLU(0.01) / ELU(1.0) are built")
    dims = [linears[0].in_features] + [m.out_features for m in linears]
    for a, b in zip(linears[:-1], linears[1:]):
        if b.in_features != a.out_features:
            raise ValueError("mlp_head_pack: layer widths do not chain")
    if any(m.bias is None for m in linears):
        raise ValueError("mlp_head_pack: every nn.Linear must have a bias")
    with torch.no_grad():
        params = torch.cat([t.detach().to(F32).reshape(-1) for m in linears for t in (m.weight, m.bias)]).contiguous()
    return params, dims, (acts.pop() if acts else 0)


def mlp_head_supported(dims) -> bool:
    """Whether ``pti_mlp_head_fwd`` is built for these layer widths ``[in, hidden..., out]``."""
    dims = [int(v) for v in dims]
    return (2 <= len(dims) <= MLP_MAX_LAYERS + 1 and all(v >= 1 for v in dims) and dims[-1] <= MLP_MAX_OUT
            and all(v <= MLP_MAX_WIDTH for v in dims[1:-1]))


def mlp_head_route(n, d, h1) -> str:
    """The route ``pti_mlp_head_fwd`` takes for ``n`` rows of ``d`` columns into a first layer of ``h1`` units (pure host
    arithmetic, the library's own rule): ``"split"`` -- at most 16 (16-row tile, 64-unit block) workgroups and more than
    one 512-column slab: the slabs are spread over workgroups and folded by the tail -- else ``"direct"``.  The route
    never changes a result bit."""
    slabs = -(-int(d) // 512)
    wgs = -(-int(n) // 16) * -(-int(h1) // 64)
    return "split" if slabs > 1 and wgs <= 16 and slabs * int(n) * int(h1) <= 1 << 26 else "direct"


def _dims_array(dims):
    return (C.c_int32 * len(dims))(*[int(v) for v in dims])


def mlp_head_fwd(x, params, dims, act, *, mean=None, std=None, targets=None, loss="mse", pred=None, rowloss=None):
    """Eval-mode forward of the regression head on ``x`` [n, d] (``torch.flatten(mu, 1)``; a row-strided view is used in
    place) with the packed ``params`` / ``dims`` / ``act`` of ``mlp_head_pack`` -> ``(pred [n, T], rowloss [n] or None)``.
    ``pred = out * std + mean`` when the normaliser's ``mean`` / ``std`` [T] are given; with ``targets`` [n, T]
    ``rowloss[i] = sum_t loss(out[i, t], (targets[i, t] - mean[t]) / std[t])`` (``loss``: "mse" or "smooth_l1"), the loss
    on the normalised scale.  Row ``i`` of both depends on row ``i`` only, bit for bit.  Runs on the current stream, no
    host sync; the scratch buffer is cached per (stream, shape).  An unsupported head (``mlp_head_supported``) raises."""
    x = _dense_rows(x, "mlp_head_fwd: x", copy=True)
    n, d = x.shape
    dims = [int(v) for v in dims]
    if len(dims) < 2 or dims[0] != d:
        raise ValueError(f"mlp_head_fwd: dims {dims} do not start with the {d} columns of x")
    if not mlp_head_supported(dims):
        raise ValueError(f"mlp_head_fwd: unsupported head {dims} (at most {MLP_MAX_LAYERS} layers, hidden widths <= "
                         f"{MLP_MAX_WIDTH}, outputs <= {MLP_MAX_OUT}); there is no silent fallback")
    if loss not in MLP_LOSSES:
        raise ValueError(f"mlp_head_fwd: loss must be one of {sorted(MLP_LOSSES)}, got {loss!r}")
    if not 0 <= int(act) < len(MLP_ACTS):
        raise ValueError(f"mlp_head_fwd: activation code {act!r}")
    t_out = dims[-1]
    _chk(params, F32, "mlp_head_fwd: params", 1)
    if params.numel() != sum(a * b + b for a, b in zip(dims[:-1], dims[1:])) or params.device != x.device:
        raise ValueError(f"mlp_head_fwd: params must hold the weights and biases of {dims} on {x.device}")
    if (mean is None) != (std is None):
        raise ValueError("mlp_head_fwd: mean and std go together")
    vecs = []
    for name, v in (("mean", mean), ("std", std)):
        if v is not None:
            if not isinstance(v, torch.Tensor) or v.numel() != t_out:
                raise ValueError(f"mlp_head_fwd: {name} must hold {t_out} values")
            v = v.to(device=x.device, dtype=F32).reshape(-1).contiguous()
        vecs.append(v)
    mean, std = vecs
    if targets is not None:
        _chk(targets, F32, "mlp_head_fwd: targets", 2)
        if tuple(targets.shape) != (n, t_out) or targets.device != x.device:
            raise ValueError(f"mlp_head_fwd: targets must be [{n}, {t_out}] on {x.device}")
    pred = _out(pred, (n, t_out), F32, x.device, "mlp_head_fwd: pred")
    rowloss = None if targets is None else _out(rowloss, (n,), F32, x.device, "mlp_head_fwd: rowloss")
    arr = _dims_array(dims)
    floats = L.lib().pti_mlp_head_ws_floats(n, d, arr, len(dims) - 1)
    if floats <= 0:
        raise ValueError(f"mlp_head_fwd: unsupported shape x {tuple(x.shape)} head {dims}")
    stream = _stream()
    ws = _scratch("mlp", (n, d, dims[1]), floats, x.device, stream)
    L.check(L.lib().pti_mlp_head_fwd(_ptr(x), x.stride(0), n, d, _ptr(params), arr, len(dims) - 1, int(act), _ptr(mean),
                                     _ptr(std), _ptr(targets), MLP_LOSSES[loss], _ptr(pred), _ptr(rowloss), _ptr(ws), stream),
            "pti_mlp_head_fwd")
    return pred, rowloss


def regression_metrics(pred, targets, rowloss, batch):
    """One fixed-order fp64 fold over a whole evaluation set (``pti_regression_metrics``): ``pred`` / ``targets`` fp32
    [n, T], ``rowloss`` fp32 [n] (``mlp_head_fwd``) -> fp64 device tensor ``[2T + 3]``: the mean over consecutive chunks of
    ``batch`` rows of ``sum(rowloss) / (rows * T)`` (``validate_one_epoch``'s mean of batch means), MAE per target, MSE per
    target, and the means of the two over the targets.  Runs on the current stream, no host sync."""
    _chk(pred, F32, "regression_metrics: pred", 2)
    _chk(targets, F32, "regression_metrics: targets", 2)
    _chk(rowloss, F32, "regression_metrics: rowloss", 1)
    n, t = pred.shape
    if n < 1 or not 1 <= t <= MLP_MAX_OUT or int(batch) < 1:
        raise ValueError(f"regression_metrics: need n >= 1, 1 <= T <= {MLP_MAX_OUT} and batch >= 1, got {n}, {t}, {batch}")
    if targets.shape != pred.shape or rowloss.numel() != n or targets.device != pred.device or rowloss.device != pred.device:
        raise ValueError("regression_metrics: pred / targets [n, T] and rowloss [n] must agree in shape and device")
    out = torch.empty(2 * t + 3, dtype=torch.float64, device=pred.device)
    L.check(L.lib().pti_regression_metrics(_ptr(pred), _ptr(targets), _ptr(rowloss), n, t, int(batch), _ptr(out), _stream()),
            "pti_regression_metrics")
    return out


# ---- train-time augmentation (csrc/augment.hip; include/pti_vae.h "train-time geometric augmentation") -----------------
ELASTIC_MAX_RADIUS = 30   # PTI_ELASTIC_MAX_RADIUS


def elastic_field(keys, alpha, sigma, h, w, out=None):
    """Smoothed random displacement field (``pti_elastic_field``): ``keys`` int64 / uint64 [B] (the 64 key bits of every
    sample), ``alpha`` fp32 [B], both on the device -> fp32 ``[B, 2, h, w]``, channel 0 the x and 1 the y displacement in
    pixels: ``alpha[b]`` times the hash noise of ``keys[b]`` under ``scipy.ndimage.gaussian_filter(sigma, mode="reflect")``.
    A sample's field depends on its key alone; ``alpha == 0`` gives zeros.  Runs on the current stream, no host sync."""
    if not isinstance(keys, torch.Tensor) or keys.dtype not in (I64, torch.uint64):
        raise TypeError(f"elastic_field: keys must be an int64 or uint64 tensor, got {getattr(keys, 'dtype', type(keys))}")
    _chk(keys, keys.dtype, "elastic_field: keys", 1)
    _chk(alpha, F32, "elastic_field: alpha", 1)
    b, h, w, sigma = keys.numel(), int(h), int(w), float(sigma)
    if b < 1 or alpha.numel() != b or alpha.device != keys.device:
        raise ValueError("elastic_field: keys and alpha must be [B] with B >= 1 on one device")
    if h < 1 or w < 1 or not sigma > 0.0:
        raise ValueError(f"elastic_field: need h, w >= 1 and sigma > 0, got {h}, {w}, {sigma}")
    radius = int(4.0 * sigma + 0.5)
    if radius > min(h, w) or radius > ELASTIC_MAX_RADIUS:
        raise ValueError(f"elastic_field: radius {radius} of sigma {sigma} must not exceed min(h, w) = {min(h, w)} "
                         f"nor {ELASTIC_MAX_RADIUS}")
    out = _out(out, (b, 2, h, w), F32, keys.device, "elastic_field: out")
    L.check(L.lib().pti_elastic_field(_ptr(keys), _ptr(alpha), sigma, b, h, w, _ptr(out), _stream()), "pti_elastic_field")
    return out


def augment_warp(src, mat, field=None, out=None):
    """One bilinear gather for a batch (``pti_augment_warp``): ``out[b, c, y, x]`` = ``src[b, c]`` sampled at
    ``mat[b] @ (x + field[b, 0, y, x], y + field[b, 1, y, x], 1)``, taps outside the image contributing zero.
    ``src`` fp32 [B, C, H, W]; ``mat`` fp32 [B, 6] (row-major 2x3 inverse map, pixel centres on integers); ``field`` fp32
    [B, 2, H, W] or None; ``out`` must not share memory with ``src``.  Runs on the current stream, no host sync."""
    _chk(src, F32, "augment_warp: src", 4)
    _chk(mat, F32, "augment_warp: mat", 2)
    b, c, h, w = src.shape
    if min(b, c, h, w) < 1 or tuple(mat.shape) != (b, 6) or mat.device != src.device:
        raise ValueError(f"augment_warp: src must be a non-empty [B, C, H, W] and mat [B, 6] on its device, got "
                         f"{tuple(src.shape)}, {tuple(mat.shape)}")
    if field is not None:
        _chk(field, F32, "augment_warp: field", 4)
        if tuple(field.shape) != (b, 2, h, w) or field.device != src.device:
            raise ValueError(f"augment_warp: field must be [{b}, 2, {h}, {w}] on {src.device}")
    out = _out(out, src.shape, F32, src.device, "augment_warp: out", msg="augment_warp: out must have the shape and device of src")
    L.check(L.lib().pti_augment_warp(_ptr(src), _ptr(mat), _ptr(field), b, c, h, w, _ptr(out), _stream()), "pti_augment_warp")
    return out


# ---- two-sample permutation tests (csrc/two_sample.hip; include/pti_vae.h "two-sample permutation tests") ------------------
TWO_SAMPLE_MIN_N, TWO_SAMPLE_MAX_N, TWO_SAMPLE_MAX_P, TWO_SAMPLE_MAX_BANDWIDTHS, TWO_SAMPLE_LEVELS = 4, 8192, 65536, 8, 65536


def _two_sample_square(who, name, t, dtype):
    """The limits of an [n, n] argument of the two-sample launchers, by name and before anything touches the device; the
    shared checks (_dense_rows) then see to device, dtype and layout."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name}: expected a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise TypeError(f"{who}: {name}: expected {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"{who}: {name}: expected a square [n, n] matrix, got {tuple(t.shape)}")
    if not TWO_SAMPLE_MIN_N <= t.shape[0] <= TWO_SAMPLE_MAX_N:
        raise ValueError(f"{who}: {name}: unsupported shape {tuple(t.shape)} ({TWO_SAMPLE_MIN_N} <= n <= {TWO_SAMPLE_MAX_N})")
    return _dense_rows(t, f"{who}: {name}", dtype, square=True)


def distance_median(dist, *, out=None):
    """The exact lower median of the ``M = n (n - 1) / 2`` entries above the diagonal of the fp32 distance matrix ``dist``
    [n, n] (``pti_distance_median``) -> 0-d fp32 DEVICE tensor: element ``(M - 1) // 2`` in ascending order, selected on the
    bit patterns by an MSB-first radix select with integer histograms.  No sort, no copy of the triangle.  4 <= n <= 8192.
    Runs on the current stream, no host sync."""
    who = "distance_median"
    dist = _two_sample_square(who, "dist", dist, F32)
    n = dist.shape[0]
    out = _out(out, (), F32, dist.device, f"{who}: out")
    stream = _stream()
    ws, nbytes = _scratch_bytes(who, "ts_median", (n,), L.lib().pti_distance_median_ws_bytes(n), tuple(dist.shape), dist.device,
                                stream)
    L.check(L.lib().pti_distance_median(_ptr(dist), dist.stride(0), n, _ptr(out), _ptr(ws), nbytes, stream), "pti_distance_median")
    return out


def two_sample_kernel(dist, kind, *, scale=None, bandwidths=(0.5, 1.0, 2.0), out=None, scale_out=None):
    """The 16-bit integer weight matrix of a two-sample test from the fp32 distance matrix ``dist`` [n, n]
    (``pti_two_sample_kernel``) -> int32 ``[n, n]`` with entries in [0, 65535] and a zero diagonal.
    ``kind="gaussian"``: ``rint(65535 mean_b exp(-d^2 / (2 (b scale)^2)))`` over ``bandwidths``, ``scale`` a one-element fp32
    device tensor (``distance_median``'s result).  ``kind="energy"``: ``rint(65535 d / scale)``, ``scale`` the matrix maximum
    (found on the device) unless one is given.  The expression is evaluated in fp64 and rounded once; a scale that is not
    positive gives an all-zero matrix.  ``scale_out``: a one-element fp32 device tensor that receives the scale used.
    4 <= n <= 8192, 1 .. 8 positive bandwidths.  Runs on the current stream, no host sync."""
    who = "two_sample_kernel"
    if kind not in ("gaussian", "energy"):
        raise ValueError(f"{who}: kind must be 'gaussian' or 'energy', got {kind!r}")
    bw = [float(b) for b in bandwidths]
    if not 1 <= len(bw) <= TWO_SAMPLE_MAX_BANDWIDTHS or not all(0.0 < b < math.inf for b in bw):
        raise ValueError(f"{who}: bandwidths must be 1 .. {TWO_SAMPLE_MAX_BANDWIDTHS} positive finite values, got {bandwidths!r}")
    if kind == "gaussian" and scale is None:
        raise ValueError(f"{who}: scale: the gaussian kind needs one (distance_median's result)")
    dist = _two_sample_square(who, "dist", dist, F32)
    n = dist.shape[0]
    if scale is not None:
        _tensor(scale, F32, f"{who}: scale")
        if scale.numel() != 1 or scale.device != dist.device:
            raise ValueError(f"{who}: scale must hold one float on {dist.device}")
    out = _out(out, (n, n), I32, dist.device, f"{who}: out")
    if scale_out is None:
        scale_out = torch.empty((), dtype=F32, device=dist.device)
    else:
        _tensor(scale_out, F32, f"{who}: scale_out")
        if scale_out.numel() != 1 or scale_out.device != dist.device:
            raise ValueError(f"{who}: scale_out must hold one float on {dist.device}")
    arr = (C.c_double * len(bw))(*bw)
    L.check(L.lib().pti_two_sample_kernel(_ptr(dist), dist.stride(0), n, int(kind == "energy"), _ptr(scale), arr, len(bw),
                                          _ptr(out), _ptr(scale_out), _stream()), "pti_two_sample_kernel")
    return out


def knn_indicator(knn_idx, n, *, out=None):
    """The 0/1 neighbour matrix of ``umap_knn``'s index table (``pti_knn_indicator``): ``knn_idx`` int32 [n, k] -> int32
    ``[n, n]`` with ``out[i, j] = 1`` where ``j`` is listed in row ``i`` and ``j != i``.  Asymmetric by nature.
    4 <= n <= 8192, 1 <= k <= n.  Runs on the current stream, no host sync."""
    who = "knn_indicator"
    if not isinstance(knn_idx, torch.Tensor):
        raise ValueError(f"{who}: knn_idx: expected a CUDA(HIP) tensor")
    if knn_idx.dtype != I32:
        raise TypeError(f"{who}: knn_idx: expected {I32}, got {knn_idx.dtype}")
    n = int(n)
    if not TWO_SAMPLE_MIN_N <= n <= TWO_SAMPLE_MAX_N:
        raise ValueError(f"{who}: n: unsupported value {n} ({TWO_SAMPLE_MIN_N} <= n <= {TWO_SAMPLE_MAX_N})")
    if knn_idx.dim() != 2 or knn_idx.shape[0] != n or not 1 <= knn_idx.shape[1] <= n:
        raise ValueError(f"{who}: knn_idx must be [{n}, k] with 1 <= k <= {n}, got {tuple(knn_idx.shape)}")
    _tensor(knn_idx, I32, f"{who}: knn_idx", 2)
    out = _out(out, (n, n), I32, knn_idx.device, f"{who}: out")
    L.check(L.lib().pti_knn_indicator(_ptr(knn_idx), n, knn_idx.shape[1], _ptr(out), _stream()), "pti_knn_indicator")
    return out


def permutation_forms(w, masks, *, out=None):
    """The three integer forms of every 0/1 labelling over one integer matrix (``pti_permutation_forms``): ``w`` int32 [n, n]
    with entries in [0, 65535] (the caller's contract; it need not be symmetric), ``masks`` uint8 [P, n] of 0/1, row 0 by
    convention the observed labelling -> int64 ``[P, 3]`` = ``(s^T W s, s . (W 1), s . (W^T 1))`` per row ``s``.  ``w`` is
    split into two int8 byte planes and ``S . plane`` runs on the int8 MFMA with i32 accumulators; everything is combined in
    64-bit integers: every output integer is exact, independent of tiling and launch order, bitwise reproducible.
    4 <= n <= 8192, 1 <= P <= 65536.  The scratch buffer is cached per (stream, shape).  Runs on the current stream, no
    host sync."""
    who = "permutation_forms"
    w = _two_sample_square(who, "w", w, I32)
    n = w.shape[0]
    if not isinstance(masks, torch.Tensor):
        raise ValueError(f"{who}: masks: expected a CUDA(HIP) tensor")
    if masks.dtype != torch.uint8:
        raise TypeError(f"{who}: masks: expected {torch.uint8}, got {masks.dtype}")
    if masks.dim() != 2 or masks.shape[1] != n:
        raise ValueError(f"{who}: masks must be [P, {n}] (one column per row of w), got {tuple(masks.shape)}")
    p = masks.shape[0]
    if not 1 <= p <= TWO_SAMPLE_MAX_P:
        raise ValueError(f"{who}: masks: unsupported number of labellings {p} (1 <= P <= {TWO_SAMPLE_MAX_P})")
    _tensor(masks, torch.uint8, f"{who}: masks", 2)
    if masks.device != w.device:
        raise ValueError(f"{who}: masks must be on {w.device}")
    out = _out(out, (p, 3), I64, w.device, f"{who}: out")
    stream = _stream()
    ws, nbytes = _scratch_bytes(who, "ts_forms", (n, p), L.lib().pti_permutation_forms_ws_bytes(n, p), (tuple(w.shape), p),
                                w.device, stream)
    L.check(L.lib().pti_permutation_forms(_ptr(w), w.stride(0), n, _ptr(masks), p, _ptr(out), _ptr(ws), nbytes, stream),
            "pti_permutation_forms")
    return out

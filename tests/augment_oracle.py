"""fp64 numpy / scipy restatement of the augmentation kernels (csrc/augment.hip; include/pti_vae.h), plus an fp32 variant
of the same arithmetic that is used ONLY to size tolerances: a comparison of a kernel with the fp64 oracle is bounded by
four times the error the fp32 restatement makes on the same inputs (floor 1e-6) -- see ``bound``.

  noise / field      the counter hash in uint32 / uint64 numpy arithmetic, scipy.ndimage.gaussian_filter(mode="reflect")
  warp               scipy.ndimage.map_coordinates(order=1, mode="grid-constant", cval=0) at M (x + fx, y + fy, 1)
  field_f32 / warp_f32   the same sums in np.float32, one rounding per operation, no fused multiply-add
"""
import numpy as np
from scipy import ndimage

U32 = np.uint32


def mix32(h):
    """lowbias32 on a uint32 array (wraps modulo 2^32)."""
    h = h.astype(U32)
    h ^= h >> U32(16)
    h *= U32(0x7FEB352D)
    h ^= h >> U32(15)
    h *= U32(0x846CA68B)
    h ^= h >> U32(16)
    return h


def noise(key, c, H, W):
    """n[y][x] in [-1, 1) of sample key ``key`` (any int below 2^64), channel ``c`` -> float64 [H, W] (exact values)."""
    key = int(key) & ((1 << 64) - 1)
    k0, k1 = U32(key & 0xFFFFFFFF), U32(key >> 32)
    i = np.arange(H * W, dtype=np.uint64).astype(U32)
    with np.errstate(over="ignore"):
        k1c = U32((int(k1) ^ (c * 0x9E3779B9)) & 0xFFFFFFFF)
        h = mix32(mix32(i + k0) ^ k1c)
    return ((h >> U32(8)).astype(np.int64) - (1 << 23)).astype(np.float64).reshape(H, W) / float(1 << 23)


def radius_of(sigma):
    return int(4.0 * float(sigma) + 0.5)


def taps_of(sigma):
    r = radius_of(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * k * k / (float(sigma) * float(sigma)))
    return g / g.sum()


def field(keys, alphas, sigma, H, W):
    """fp64 [B, 2, H, W]: alpha[b] * gaussian_filter(noise(key[b], c))."""
    out = np.zeros((len(keys), 2, H, W))
    for b, (key, alpha) in enumerate(zip(keys, alphas)):
        if float(alpha) == 0.0:
            continue
        for c in range(2):
            out[b, c] = float(alpha) * ndimage.gaussian_filter(noise(key, c, H, W), float(sigma), mode="reflect", truncate=4.0)
    return out


def field_f32(keys, alphas, sigma, H, W):
    """The same field with every product and sum rounded to fp32 (taps cast from fp64 once, x pass then y pass, taps in
    ascending order)."""
    t = taps_of(sigma).astype(np.float32)
    r = radius_of(sigma)
    out = np.zeros((len(keys), 2, H, W), np.float32)
    for b, (key, alpha) in enumerate(zip(keys, alphas)):
        if float(alpha) == 0.0:
            continue
        for c in range(2):
            n = np.pad(noise(key, c, H, W).astype(np.float32), r, mode="symmetric")
            rows = np.zeros((H + 2 * r, W), np.float32)
            for k in range(2 * r + 1):
                rows = rows + t[k] * n[:, k:k + W]
            acc = np.zeros((H, W), np.float32)
            for k in range(2 * r + 1):
                acc = acc + t[k] * rows[k:k + H]
            out[b, c] = np.float32(alpha) * acc
    return out


def _coords(mat, fld, H, W, dtype):
    m = np.asarray(mat, dtype).reshape(6)
    yy, xx = np.mgrid[0:H, 0:W]
    qx, qy = xx.astype(dtype), yy.astype(dtype)
    if fld is not None:
        qx, qy = qx + np.asarray(fld[0], dtype), qy + np.asarray(fld[1], dtype)
    return (m[0] * qx + m[1] * qy) + m[2], (m[3] * qx + m[4] * qy) + m[5]


def warp(src, mats, fld=None):
    """fp64 [B, C, H, W]: bilinear sample of src[b, c] at mats[b] (x + fx, y + fy, 1), outside taps zero."""
    src = np.asarray(src, np.float64)
    B, C, H, W = src.shape
    out = np.empty_like(src)
    for b in range(B):
        sx, sy = _coords(mats[b], None if fld is None else fld[b], H, W, np.float64)
        for c in range(C):
            out[b, c] = ndimage.map_coordinates(src[b, c], [sy, sx], order=1, mode="grid-constant", cval=0.0)
    return out


def warp_f32(src, mats, fld=None):
    """The same warp in fp32 arithmetic: fp32 coordinates, floor, tap weights and the four-term sum."""
    f = np.float32
    src = np.asarray(src, f)
    B, C, H, W = src.shape
    out = np.empty_like(src)
    for b in range(B):
        sx, sy = _coords(mats[b], None if fld is None else fld[b], H, W, f)
        fx, fy = np.floor(sx), np.floor(sy)
        wx, wy = sx - fx, sy - fy
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        pad = np.zeros((C, H + 2, W + 2), f)      # one zero ring: taps at -1 and at H / W
        pad[:, 1:-1, 1:-1] = src[b]
        far = (ix < -1) | (ix >= W) | (iy < -1) | (iy >= H)
        jx, jy = np.clip(ix, -1, W - 1) + 1, np.clip(iy, -1, H - 1) + 1
        one = f(1)
        for c in range(C):
            p = pad[c]
            v = (p[jy, jx] * ((one - wx) * (one - wy)) + p[jy, jx + 1] * (wx * (one - wy))
                 + p[jy + 1, jx] * ((one - wx) * wy) + p[jy + 1, jx + 1] * (wx * wy))
            out[b, c] = np.where(far, f(0), v)
    return out


def bound(ref64, ref32, floor=1e-6):
    """Largest deviation allowed from the fp64 oracle: four times the fp32 restatement's own, at least ``floor``."""
    return max(4.0 * float(np.abs(np.asarray(ref32, np.float64) - ref64).max()), floor)


def ellipse_images(rng, shapes):
    """Raw images in the style of tests/test_gpu_data.py: noisy foreground ellipse, exact-zero background."""
    out = []
    for h, w in shapes:
        a = rng.standard_normal((h, w)).astype(np.float32) * 300 + 900
        yy, xx = np.mgrid[0:h, 0:w]
        a[((xx - w / 2) / (0.4 * w)) ** 2 + ((yy - h / 2) / (0.32 * h)) ** 2 > 1.0] = 0.0
        out.append(a)
    return out

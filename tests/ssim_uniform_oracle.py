"""Oracles of the uniform-window SSIM (include/pti_vae.h "uniform-window SSIM"; skimage.metrics.structural_similarity with its
defaults and ``data_range = gt.max() - gt.min()``), all on the CPU:

``ssim_valid``   the definition restated in fp64 numpy over the windows that lie inside the image;
``ssim_scipy``   a literal transcription of skimage's function: ``scipy.ndimage.uniform_filter`` of the whole image with
                 ``mode='reflect'``, then the 3-pixel crop -- with knobs for the mutations the tests try;
``ssim_fp32``    the same formula with every per-pixel operation rounded to fp32 on its own, in the kernel's arrangement: the
                 moments of a window are taken about a pixel of the window (row 5, column 3 of the 10 x 7 patch that four
                 vertically adjacent valid pixels share), the window sums are 7 row sums, columns ascending, added rows
                 ascending, times 1/49, and the mean is fp64: its distance from ``ssim_valid`` is the yardstick of the GPU
                 test's gate.

Every function takes 2-D float32 arrays ``x`` (ground truth) and ``y`` (cleaned prediction) and returns ``(ssim, R)``; a zero data
range gives ``(0.0, 0.0)``."""
from __future__ import annotations

import numpy as np

WIN = 7
K1, K2 = 0.01, 0.03


def data_range_of(x) -> float:
    return float(np.float64(x.max()) - np.float64(x.min()))


def _box(a, win, dtype):
    """Sums over every ``win`` x ``win`` window inside ``a``: row sums with the columns ascending, then the rows ascending, each
    addition rounded to ``dtype``."""
    a = a.astype(dtype)
    h, w = a.shape
    rows = a[:, 0:w - win + 1].copy()
    for k in range(1, win):
        rows = rows + a[:, k:w - win + 1 + k]
    out = rows[0:h - win + 1].copy()
    for k in range(1, win):
        out = out + rows[k:h - win + 1 + k]
    return out


def ssim_valid(x, y, data_range=None, cn=None, win=WIN, k2=K2):
    """fp64, valid windows only.  ``cn``: the covariance normalisation, default ``win^2 / (win^2 - 1)``."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    R = data_range_of(x) if data_range is None else float(data_range)
    if R == 0:
        return 0.0, 0.0
    npx = win * win
    cn = npx / (npx - 1) if cn is None else cn
    ux, uy = _box(x64, win, np.float64) / npx, _box(y64, win, np.float64) / npx
    uxx, uyy, uxy = _box(x64 * x64, win, np.float64) / npx, _box(y64 * y64, win, np.float64) / npx, _box(x64 * y64, win, np.float64) / npx
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    c1, c2 = (K1 * R) ** 2, (k2 * R) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float(s.mean(dtype=np.float64)), R


def ssim_scipy(x, y, data_range=None, win=WIN, sample_covariance=True, crop=True, k2=K2):
    """skimage/metrics/_structural_similarity.py line by line (gaussian_weights=False, full=False), in fp64."""
    from scipy.ndimage import uniform_filter
    R = data_range_of(x) if data_range is None else float(data_range)
    if R == 0:
        return 0.0, 0.0
    im1, im2 = x.astype(np.float64), y.astype(np.float64)
    NP = win ** 2
    cov_norm = NP / (NP - 1) if sample_covariance else 1.0
    ux, uy = uniform_filter(im1, size=win), uniform_filter(im2, size=win)
    uxx, uyy, uxy = uniform_filter(im1 * im1, size=win), uniform_filter(im2 * im2, size=win), uniform_filter(im1 * im2, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (k2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (win - 1) // 2
    if crop:
        S = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    return float(S.mean(dtype=np.float64)), R


def ssim_fp32(x, y, data_range=None):
    """Every per-pixel operation in fp32, no fused multiply-add, moments about a pixel of the window; the mean in fp64."""
    f = np.float32
    x, y = x.astype(f), y.astype(f)
    R = data_range_of(x) if data_range is None else float(data_range)
    if R == 0:
        return 0.0, 0.0
    inv, cn = f(1.0) / f(49.0), f(49.0) / f(48.0)
    c1, c2 = f((K1 * R) ** 2), f((K2 * R) ** 2)
    h, w = x.shape
    hv, wv = h - WIN + 1, w - WIN + 1
    from numpy.lib.stride_tricks import sliding_window_view
    total, count = 0.0, 0
    for g0 in range(0, hv, 4):                       # valid rows g0 .. g0 + 3 share their origin, as the kernel's threads do
        rows = min(g0 + 4, hv) + WIN - 1 - g0        # patch rows g0 .. g0 + rows - 1
        a, b = x[g0 + 5, 3:3 + wv], y[g0 + 5, 3:3 + wv]          # the origin: row 5, column 3 of the patch, per valid column
        dx = sliding_window_view(x[g0:g0 + rows], WIN, axis=1) - a[None, :, None]     # [rows, wv, 7]
        dy = sliding_window_view(y[g0:g0 + rows], WIN, axis=1) - b[None, :, None]
        rs = []
        for q in (dx, dy, dx * dx, dy * dy, dx * dy):
            acc = q[:, :, 0].copy()
            for k in range(1, WIN):                  # columns ascending
                acc = acc + q[:, :, k]
            rs.append(acc)
        for o in range(min(g0 + 4, hv) - g0):
            e = []
            for acc in rs:
                t = acc[o].copy()
                for k in range(1, WIN):              # rows ascending
                    t = t + acc[o + k]
                e.append(t)
            mx, my = e[0] * inv, e[1] * inv
            ux, uy = a + mx, b + my
            vx, vy, vxy = cn * (e[2] * inv - mx * mx), cn * (e[3] * inv - my * my), cn * (e[4] * inv - mx * my)
            s = ((f(2) * ux * uy + c1) * (f(2) * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
            assert s.dtype == f
            total += float(s.sum(dtype=np.float64))
            count += s.size
    assert count == hv * wv
    return total / count, R


# ---- the cases: an ellipse of values on a zero background, the prediction the object plus Gaussian noise -------------------
def ellipse_mask(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    return ((yy - cy) / max(0.42 * h, 1.0)) ** 2 + ((xx - cx) / max(0.36 * w, 1.0)) ** 2 <= 1.0


def make_pair(h, w, seed, noise=0.05, offset=0.0, variant="noisy"):
    """-> (gt, cleaned prediction, mask) as float32 / bool.  ``variant``: ``noisy``; ``identical`` (the prediction is the ground
    truth); ``background`` (an all-zero prediction); ``flat_gt`` (a constant non-zero ground truth: data range 0)."""
    rs = np.random.RandomState(seed)
    m = ellipse_mask(h, w)
    values = (0.25 + 0.5 * rs.rand(h, w) + offset).astype(np.float32)   # a data range near 0.75, not 1: R = 1 is a mutation
    gt = np.where(m, values, np.float32(0)).astype(np.float32)
    pred = np.where(m, gt + np.float32(noise) * rs.randn(h, w).astype(np.float32), np.float32(0)).astype(np.float32)
    if variant == "identical":
        pred = gt.copy()
    elif variant == "background":
        pred = np.zeros_like(gt)
    elif variant == "flat_gt":
        gt = np.full_like(gt, 0.7)
    elif variant != "noisy":
        raise ValueError(variant)
    return gt, pred, m


SHAPES = ((7, 7), (7, 40), (40, 7), (8, 13), (38, 38), (39, 39), (45, 71), (64, 64), (1024, 7), (1024, 1024))
VARIANT_SHAPES = ((45, 71), (64, 64))


def case_list():
    """-> list of dicts ``{name, h, w, seed, noise, offset, variant}``: every shape at noise 0.05, then the value variants."""
    cases = []
    for i, (h, w) in enumerate(SHAPES):
        cases.append(dict(name=f"{h}x{w}", h=h, w=w, seed=100 + i, noise=0.05, offset=0.0, variant="noisy"))
    for j, (h, w) in enumerate(VARIANT_SHAPES):
        seed = 200 + 20 * j
        for noise in (0.01, 0.2):
            cases.append(dict(name=f"{h}x{w}_noise{noise}", h=h, w=w, seed=seed, noise=noise, offset=0.0, variant="noisy"))
            seed += 1
        for offset in (0.5, 100.0, -0.6):
            cases.append(dict(name=f"{h}x{w}_offset{offset:+g}", h=h, w=w, seed=seed, noise=0.05, offset=offset, variant="noisy"))
            seed += 1
        for variant in ("identical", "background", "flat_gt"):
            cases.append(dict(name=f"{h}x{w}_{variant}", h=h, w=w, seed=seed, noise=0.05, offset=0.0, variant=variant))
            seed += 1
    return cases


def case_pair(c):
    return make_pair(int(c["h"]), int(c["w"]), int(c["seed"]), float(c["noise"]), float(c["offset"]), str(c["variant"]))[:2]


def pack_cases(cases, expected):
    """-> dict of arrays for ``np.savez_compressed``: what rebuilds every image, and the expected ``{ssim, R}`` rows."""
    return {"names": np.array([c["name"] for c in cases]), "shapes": np.array([(c["h"], c["w"]) for c in cases], dtype=np.int32),
            "seeds": np.array([c["seed"] for c in cases], dtype=np.int64), "noise": np.array([c["noise"] for c in cases]),
            "offset": np.array([c["offset"] for c in cases]), "variants": np.array([c["variant"] for c in cases]),
            "expected": np.asarray(expected, dtype=np.float64).reshape(len(cases), 2)}


def unpack_cases(z):
    """The inverse of ``pack_cases`` on a loaded npz -> (list of case dicts, expected float64 ``[n, 2]``)."""
    cases = [dict(name=str(n), h=int(s[0]), w=int(s[1]), seed=int(sd), noise=float(no), offset=float(of), variant=str(v))
             for n, s, sd, no, of, v in zip(z["names"], z["shapes"], z["seeds"], z["noise"], z["offset"], z["variants"])]
    return cases, np.asarray(z["expected"], dtype=np.float64)


_DREF = {}


def d_ref(cases):
    """name -> ``|ssim_fp32 - ssim_valid|`` of every case (computed once per process)."""
    for c in cases:
        if c["name"] not in _DREF:
            x, y = case_pair(c)
            _DREF[c["name"]] = abs(ssim_fp32(x, y)[0] - ssim_valid(x, y)[0])
    return {c["name"]: _DREF[c["name"]] for c in cases}


FLOOR = 2.0 ** -24   # the unit roundoff of fp32 at the size of the result (an SSIM is at most 1 in magnitude)


def gate_of(d, twin=0.0):
    """The bound on ``|kernel - fp64 oracle|`` from the restatement's own distance ``d``: ``8 * max(d, twin, FLOOR)``."""
    return 8.0 * max(d, twin, FLOOR)


def gates(cases):
    """name -> the bound on ``|kernel - fp64 oracle|``: ``8 * max(D_ref(case), D_ref at offset 0, 2^-24)``.  The second term is
    the ``D_ref`` of the case's twin -- the case of the same shape at noise 0.05 whose object is not offset -- so that an offset
    image is not asked for more than the plain one.  The kernel differs from ``ssim_fp32`` only in where it rounds (fused
    multiply-adds), so it is allowed a few times the restatement's own distance from fp64.  The third term is fp32's unit
    roundoff: the mean of thousands of rounded pixels can land closer to fp64 than any single fp32 operation is (identical
    images: the restatement gives exactly 1), and a kernel that rounds elsewhere cannot be held to that luck."""
    d = d_ref(cases)
    twin = {(c["h"], c["w"]): d[c["name"]] for c in cases if c["offset"] == 0.0 and c["noise"] == 0.05 and c["variant"] == "noisy"}
    return {c["name"]: gate_of(d[c["name"]], twin[(c["h"], c["w"])] if c["offset"] != 0.0 else 0.0) for c in cases}

"""Host oracle of the pair registration (``ops.mask_moments`` / ``warp_cubic`` / ``align_bottom`` / ``register_pairs``,
appended to csrc/mask_compare.hip; include/pti_vae.h "pair registration"): the rules in numpy and fp64, on top of
``mask_compare_oracle`` for the masks, ``K`` and ``F``.

* moments: exact Python integers, twice over (sums over the pixel list; sums over row and column profiles);
* rotation: ``rotate(..., dtype=np.float64)`` is the oracle (fp64 coordinates, weights and sums), ``dtype=np.float32`` the
  restatement of the kernel (fp64 coordinates, fp32 weights and sums in the kernel's association, every operation rounded
  on its own; the kernel may fuse a multiply with the add that follows) -- the distance between the two is the yardstick
  of the GPU test's gate;
* alignment: integers.

``register`` takes switches that turn on one deliberate MISTAKE each (``MUTATIONS``).  ``golden_cases`` builds the masks of
``tests/golden/mask_register_golden.npz``; ``tools/make_mask_register_golden.py`` records them with the answers."""
import math

import numpy as np

import mask_compare_oracle as O

MOMENT_COLUMNS = ("m00", "m10", "m01", "m20", "m11", "m02", "A", "B", "C", "status")
ALIGN_COLUMNS = ("centre_gt", "centre_pred", "count_gt", "count_pred", "shift", "status")
THRESHOLD = O.THRESHOLD
MUTATIONS = ({"transpose": True}, {"a": -0.5}, {"border": "zero"}, {"centre": "half"}, {"region": "K"}, {"shift_sign": -1},
             {"centre_rounding": "round"}, {"rows": "ceil"})


# ---- regions and moments -----------------------------------------------------------------------------------------------------
def filled_largest(mask, impl="scipy", fill=True):
    """F(K(mask)) as a boolean array (``fill=False``: K alone); all False for an empty mask."""
    label = O.label_scipy if impl == "scipy" else O.label_numpy
    lab, n = label(mask, 8)
    k, _ = O.largest(lab, n)
    if not n or not fill:
        return k
    return (O.fill_scipy if impl == "scipy" else O.fill_numpy)(k, 4)


def raw_moments(region):
    """[m00, m10, m01, m20, m11, m02] as Python integers: sums over the list of set pixels."""
    ys, xs = np.nonzero(region)
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    return [len(xs), sum(xs), sum(ys), sum(x * x for x in xs), sum(x * y for x, y in zip(xs, ys)), sum(y * y for y in ys)]


def raw_moments_profiles(region):
    """The same six integers from the row and column profiles (a second restatement: no pixel list)."""
    cols = [int(v) for v in region.sum(axis=0)]
    rows = [int(v) for v in region.sum(axis=1)]
    rowx = [int(v) for v in (region * np.arange(region.shape[1], dtype=np.int64)[None, :]).sum(axis=1)]   # sum of x per row
    return [sum(cols), sum(x * c for x, c in enumerate(cols)), sum(y * r for y, r in enumerate(rows)),
            sum(x * x * c for x, c in enumerate(cols)), sum(y * s for y, s in enumerate(rowx)),
            sum(y * y * r for y, r in enumerate(rows))]


def central(m):
    """(A, B, C) from the six raw moments, exact."""
    m00, m10, m01, m20, m11, m02 = m
    return m00 * m20 - m10 * m10, m00 * m11 - m10 * m01, m00 * m02 - m01 * m01


def angle(m):
    """-> (beta, cos beta, sin beta).  The B == 0 branch is taken on the integers and its coefficients are exact."""
    a, b, c = central(m)
    assert max(abs(a), abs(b), abs(c), abs(a - c)) < 2 ** 61
    if m[0] == 0 or (b == 0 and c >= a):
        return 0.0, 1.0, 0.0
    if b == 0:
        return math.pi / 2, 0.0, 1.0
    theta = 0.5 * math.atan2(float(2 * b), float(a - c))
    beta = theta - math.pi / 2 if theta > 0 else theta + math.pi / 2
    return beta, math.cos(beta), math.sin(beta)


def moments_row(region):
    m = raw_moments(region)
    return m + list(central(m)) + [0]


# ---- rotation --------------------------------------------------------------------------------------------------------------------
def cubic_weights(t, a, dtype):
    """Keys' weights for the taps at -1, 0, +1, +2, every operation rounded to ``dtype`` in the kernel's order."""
    f = dtype
    t, a = t.astype(f), f(a)
    u, v = t + f(1), f(1) - t
    w0 = ((a * u - f(5) * a) * u + f(8) * a) * u - f(4) * a
    w1 = ((a + f(2)) * t - (a + f(3))) * (t * t) + f(1)
    w2 = ((a + f(2)) * v - (a + f(3))) * (v * v) + f(1)
    w3 = ((f(1) - w0) - w1) - w2
    return w0, w1, w2, w3


def source_points(h, w, cb, sb, transpose=False, centre="floor"):
    cx, cy = (w // 2, h // 2) if centre == "floor" else ((w - 1) / 2, (h - 1) / 2)
    dx = (np.arange(w, dtype=np.float64) - cx)[None, :]
    dy = (np.arange(h, dtype=np.float64) - cy)[:, None]
    cb, sb = np.float64(cb), np.float64(-sb if transpose else sb)
    return (cx + cb * dx) - sb * dy, (cy + sb * dx) + cb * dy


def rotate(img, cb, sb, dtype=np.float32, a=-0.75, border="replicate", transpose=False, centre="floor"):
    """The 4 x 4 cubic convolution at the rotated source points -> array of ``dtype``."""
    h, w = img.shape
    sx, sy = source_points(h, w, cb, sb, transpose, centre)
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = cubic_weights(sx - fx, a, dtype), cubic_weights(sy - fy, a, dtype)
    fx = np.clip(fx, -3, w + 2).astype(np.int64)
    fy = np.clip(fy, -3, h + 2).astype(np.int64)
    src = img.astype(dtype)

    def tap(yy, xx):
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        if border == "zero":
            v = np.where((yy < 0) | (yy > h - 1) | (xx < 0) | (xx > w - 1), dtype(0), v)
        return v

    rows = [((wx[0] * tap(fy - 1 + j, fx - 1) + wx[1] * tap(fy - 1 + j, fx)) + wx[2] * tap(fy - 1 + j, fx + 1))
            + wx[3] * tap(fy - 1 + j, fx + 2) for j in range(4)]
    out = ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3]
    assert out.dtype == dtype
    return out


# ---- alignment -----------------------------------------------------------------------------------------------------------------
def bottom_centre(img, rows="floor", rounding="trunc"):
    """-> (centre or -1, count) of the non-zero pixels in the bottom fifth."""
    h = img.shape[0]
    k = h // 5 if rows == "floor" else -(-h // 5)
    xs = np.nonzero(img[h - k:] != 0)[1]
    if len(xs) == 0:
        return -1, 0
    total, count = int(xs.sum()), len(xs)
    return (total // count if rounding == "trunc" else (2 * total + count) // (2 * count)), count


def shifted(img, shift):
    out = np.zeros_like(img)
    w = img.shape[1]
    if shift >= 0:
        out[:, shift:] = img[:, :w - shift]
    else:
        out[:, :w + shift] = img[:, -shift:]
    return out


def align(rot_gt, rot_pred, shift_sign=1, centre_rounding="trunc", rows="floor"):
    """-> (aligned prediction, the six ``ALIGN_COLUMNS``)."""
    cg, ng = bottom_centre(rot_gt, rows, centre_rounding)
    cp, npred = bottom_centre(rot_pred, rows, centre_rounding)
    status = (0 if ng else 1) | (0 if npred else 2)
    shift = 0 if status else shift_sign * (cg - cp)
    return shifted(rot_pred, shift), [cg, cp, ng, npred, shift, status]


# ---- the whole -----------------------------------------------------------------------------------------------------------------
def moments_stage(gt, pred, threshold=THRESHOLD, impl="scipy", region="F"):
    """One pair -> (cleaned prediction, [2][10] integer rows, [2][3] coefficients)."""
    g, r = O.masks(gt, pred, threshold)
    fg, p = filled_largest(g, impl, region == "F"), filled_largest(r, impl, region == "F")
    cleaned = np.where(filled_largest(r, impl), pred, np.float32(0)).astype(np.float32)
    rows = [moments_row(fg), moments_row(p)]
    return cleaned, rows, [list(angle(rows[0][:6])), list(angle(rows[1][:6]))]


def register(gt, pred, threshold=THRESHOLD, dtype=np.float32, transpose=False, a=-0.75, border="replicate", centre="floor",
             region="F", shift_sign=1, centre_rounding="trunc", rows="floor"):
    """One pair through all stages with ``dtype`` rotation -> dict."""
    cleaned, mom, co = moments_stage(gt, pred, threshold, region=region)
    kw = dict(dtype=dtype, a=a, border=border, transpose=transpose, centre=centre)
    rot_gt, rot_pred = rotate(gt, co[0][1], co[0][2], **kw), rotate(cleaned, co[1][1], co[1][2], **kw)
    aligned, info = align(rot_gt, rot_pred, shift_sign, centre_rounding, rows)
    return {"cleaned": cleaned, "moments": mom, "coeffs": co, "rot_gt": rot_gt, "rot_pred": rot_pred, "aligned": aligned, "align": info}


def digest(res):
    """The recorded answers of one ``register`` result: integers, angles, and order-independent sums of the images."""
    nz = [int((res[k] != 0).sum()) for k in ("rot_gt", "rot_pred", "aligned")]
    sums = [math.fsum(float(v) for v in res[k].reshape(-1)) for k in ("rot_gt", "rot_pred", "aligned")]
    return {"moments": np.array([r[:9] for r in res["moments"]], dtype=np.int64), "beta": np.array([c[0] for c in res["coeffs"]]),
            "align": np.array(res["align"], dtype=np.int32), "nonzero": np.array(nz, dtype=np.int64), "sums": np.array(sums)}


# ---- golden masks ------------------------------------------------------------------------------------------------------------
GOLDEN_SHAPE = (96, 80)
ELLIPSE_TILTS = (12.0, -27.0, 55.0, -80.0)


def ellipse(h, w, tilt_deg, ry, rx, cy=None, cx=None):
    """An ellipse whose major half-axis ``ry`` is turned by ``tilt_deg`` from the vertical (positive: top to the right)."""
    cy, cx = (h / 2 if cy is None else cy), (w / 2 if cx is None else cx)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = math.radians(tilt_deg)
    u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)        # across the major axis
    v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)       # along it
    return (u / rx) ** 2 + (v / ry) ** 2 <= 1.0


def golden_masks():
    """name -> (G, R, flavour): the ground-truth mask, the prediction's mask and how the values inside are drawn."""
    h, w = GOLDEN_SHAPE
    out = {}
    for i, tilt in enumerate(ELLIPSE_TILTS):
        g = ellipse(h, w, tilt, 34, 14, cy=52)
        r = np.roll(ellipse(h, w, tilt + 4.0, 32, 15, cy=52), 3, axis=1)
        r[2:4, 2:5] = True                                       # a speck the cleaning removes
        out[f"ellipse_{tilt:+.0f}"] = (g, r, ("flat", "textured", "signed", "textured")[i])
    up = ellipse(h, w, 0.0, 36, 14, cy=52, cx=40)                # symmetric about column 40 and row 52: B == 0, C > A
    out["upright"] = (up, np.roll(up, -2, axis=1), "flat")
    disc = ellipse(h, w, 0.0, 20, 20, cy=66, cx=40)              # B == 0 and C == A
    out["disc"] = (disc, disc.copy(), "textured")
    bar = np.zeros((h, w), dtype=bool)
    bar[40:52, 10:70] = True                                     # B == 0, C < A: a quarter turn
    out["bar"] = (bar, np.roll(bar, 5, axis=0), "flat")
    hole = ellipse(h, w, 20.0, 34, 20)
    hole &= ~ellipse(h, w, 20.0, 12, 8, cy=36, cx=44)            # a hole off the centre: F(K) and K differ in every moment
    hole |= ellipse(h, w, 0.0, 3, 3, cy=36, cx=44)               # an island in it
    out["hole_island"] = (hole, np.roll(hole, 2, axis=1), "signed")
    edge = ellipse(h, w, -15.0, 40, 16, cy=60, cx=12)            # cut by the left and bottom border
    out["on_border"] = (edge, ellipse(h, w, -10.0, 38, 15, cy=60, cx=14), "textured")
    ell = np.zeros((h, w), dtype=bool)
    ell[10:90, 20:32] = True
    ell[78:90, 20:70] = True                                     # the foot of the L: the bottom fifth is off-centre
    out["l_shape"] = (ell, np.roll(ell, -4, axis=1), "flat")
    odd = ellipse(65, 67, 33.0, 24, 9)
    out["odd_65x67"] = (odd, np.roll(ellipse(65, 67, 30.0, 23, 10), -3, axis=1), "signed")
    return out


def images(g, r, flavour, seed, threshold=THRESHOLD):
    """fp32 images whose masks are exactly ``g`` / ``r``; ``flavour``: "flat" (1.0 inside), "textured" (0.3 .. 1) or
    "signed" (textured, a fifth of the pixels negative).  The prediction's background is inside +-threshold."""
    rs = np.random.RandomState(seed)
    t = float(threshold)

    def inside(m):
        if flavour == "flat":
            return np.ones(m.shape)
        v = rs.uniform(0.3, 1.0, m.shape)
        return v * rs.choice([-1.0, 1.0], m.shape, p=[0.2, 0.8]) if flavour == "signed" else v

    gt = np.where(g, inside(g), 0.0).astype(np.float32)
    bg = rs.choice([0.0, 0.0, 0.5 * t, -0.75 * t], r.shape)
    v = inside(r)
    pred = np.where(r, v * (1.0 - t) + np.sign(v) * t * 1.01, bg).astype(np.float32)
    got_g, got_r = O.masks(gt, pred, threshold)
    assert np.array_equal(got_g, g) and np.array_equal(got_r, r)
    return gt, pred


def golden_cases():
    """-> list of (name, G, R, flavour, seed)."""
    return [(name, g, r, fl, 40 + i) for i, (name, (g, r, fl)) in enumerate(golden_masks().items())]


def pack_cases(cases):
    """-> dict of arrays for ``np.savez_compressed``: the masks as bits and the digest of ``register`` on their images."""
    out = {"names": np.array([c[0] for c in cases]), "shapes": np.array([c[1].shape for c in cases], dtype=np.int32),
           "flavours": np.array([c[3] for c in cases]), "seeds": np.array([c[4] for c in cases], dtype=np.int32),
           "bits_gt": np.concatenate([np.packbits(c[1].reshape(-1)) for c in cases]),
           "bits_pred": np.concatenate([np.packbits(c[2].reshape(-1)) for c in cases])}
    digests = [digest(register(*images(c[1], c[2], c[3], c[4]))) for c in cases]
    for key in digests[0]:
        out["expected_" + key] = np.stack([d[key] for d in digests])
    return out


def unpack_cases(z):
    """The inverse of ``pack_cases`` on a loaded npz -> list of (name, G, R, flavour, seed, expected digest)."""
    out, og, orr = [], 0, 0
    for i, (name, (h, w)) in enumerate(zip(z["names"], z["shapes"])):
        nb = (int(h) * int(w) + 7) // 8
        g = np.unpackbits(z["bits_gt"][og:og + nb])[:h * w].reshape(h, w).astype(bool)
        r = np.unpackbits(z["bits_pred"][orr:orr + nb])[:h * w].reshape(h, w).astype(bool)
        og, orr = og + nb, orr + nb
        exp = {k[len("expected_"):]: z[k][i] for k in z.files if k.startswith("expected_")}
        out.append((str(name), g, r, str(z["flavours"][i]), int(z["seeds"][i]), exp))
    return out

"""Host oracle of ``ops.surface_distance`` (csrc/surface_distance.hip; include/pti_vae.h "surface distance"), twice over:

* ``impl="scipy"``: ``scipy.ndimage.distance_transform_edt(~edges, return_indices=True)``; the squared distance is formed in
  integers from the returned indices, so no floating-point distance is ever rounded;
* ``impl="numpy"``: the separable transform written out -- per column the vertical distance to the nearest edge pixel, per row
  the minimum of ``dx^2 + g^2`` over all columns -- no scipy, so the oracle does not rest on one library.

``brute`` is the definition itself (all pairs of edge pixels) for small masks.  ``table`` gives the eleven integer columns per
side and the fp64 sum (``math.fsum`` over correctly rounded roots); ``percentile_of`` is the interpolation the host report does.
The cases of ``tests/golden/surface_distance_golden.npz`` are built here (``golden_cases``);
``tools/make_surface_distance_golden.py`` records them with the oracle's answers."""
import math

import numpy as np

import mask_compare_oracle as MC

COLUMNS = ("n_fg", "n_edge", "max_d2", "rank_lo", "d2_lo", "d2_hi", "within_0", "within_1", "within_2", "within_3", "status")
MAX_TOLERANCES = 4
GOLDEN_PM = 950
GOLDEN_TOLERANCES = (1.0, 2.0)
SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 9), (31, 33), (67, 129), (130, 300))


def edges(m):
    """Foreground pixels with a 4-neighbour that is background; outside the image is background."""
    m = np.asarray(m, dtype=bool)
    p = np.pad(m, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def tol_d2(tolerances):
    return [int(min(math.floor(float(t) * float(t)), 2 ** 31 - 1)) for t in tolerances]


# ---- squared distances ---------------------------------------------------------------------------------------------------------
def d2_scipy(e_from, e_to):
    """int64 ``d2`` of every edge pixel of ``e_from`` (row-major order) to the nearest pixel of ``e_to`` (which is not empty)."""
    from scipy import ndimage
    idx = ndimage.distance_transform_edt(~e_to, return_distances=False, return_indices=True)
    ys, xs = np.nonzero(e_from)
    qy, qx = idx[0][ys, xs].astype(np.int64), idx[1][ys, xs].astype(np.int64)
    return (qy - ys) ** 2 + (qx - xs) ** 2


def d2_numpy(e_from, e_to):
    h, w = e_to.shape
    big = 4 * (h + w) ** 2
    g = np.full((h, w), big, dtype=np.int64)                       # vertical distance to the nearest edge pixel of the column
    rows = np.arange(h, dtype=np.int64)
    for x in range(w):
        at = np.flatnonzero(e_to[:, x])
        if len(at):
            g[:, x] = np.abs(rows[:, None] - at[None, :]).min(axis=1)
    g2 = np.where(g >= big, big, g * g)
    cols = np.arange(w, dtype=np.int64)
    dx2 = (cols[:, None] - cols[None, :]) ** 2                     # [x, column]
    ys, xs = np.nonzero(e_from)
    return np.array([int((dx2[x] + g2[y]).min()) for y, x in zip(ys, xs)], dtype=np.int64)


def brute(e_from, e_to):
    fy, fx = np.nonzero(e_from)
    ty, tx = np.nonzero(e_to)
    d = (fy[:, None].astype(np.int64) - ty[None, :]) ** 2 + (fx[:, None].astype(np.int64) - tx[None, :]) ** 2
    return d.min(axis=1)


def distances(a, b, impl="scipy"):
    """-> (edge map of a, edge map of b, d2 of a's edge pixels, d2 of b's), the last two ``None`` when a side has no edge."""
    ea, eb = edges(a), edges(b)
    if not ea.any() or not eb.any():
        return ea, eb, None, None
    f = {"scipy": d2_scipy, "numpy": d2_numpy, "brute": brute}[impl]
    return ea, eb, f(ea, eb), f(eb, ea)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def ranks(m, pm):
    r = (m - 1) * pm
    return r // 1000, r % 1000


def side_row(mask, edge, d2, pm, tols):
    """The eleven columns and the fp64 sum of one side; ``d2`` None: the empty-side row."""
    n_fg, m = int(np.asarray(mask, dtype=bool).sum()), int(edge.sum())
    if d2 is None:
        return [n_fg, m, -1, 0, -1, -1, 0, 0, 0, 0, 0], 0.0
    s = np.sort(d2)
    lo, rem = ranks(m, pm)
    within = [int((d2 <= t).sum()) for t in tols] + [0] * (MAX_TOLERANCES - len(tols))
    row = [n_fg, m, int(s[-1]), lo, int(s[lo]), int(s[lo + 1] if rem else s[lo])] + within + [0]
    return row, math.fsum(np.sqrt(d2.astype(np.float64)).tolist())


def table(a, b, pm=GOLDEN_PM, tolerances=GOLDEN_TOLERANCES, impl="scipy"):
    """One pair of boolean masks -> (int ``[2][11]``, float ``[2]``)."""
    ea, eb, da, db = distances(a, b, impl)
    tols = tol_d2(tolerances)
    r0, s0 = side_row(a, ea, da, pm, tols)
    r1, s1 = side_row(b, eb, db, pm, tols)
    return [r0, r1], [s0, s1]


def batch(pairs, pm=GOLDEN_PM, tolerances=GOLDEN_TOLERANCES, impl="scipy"):
    """List of (a, b) -> (int32 ``[n, 2, 11]``, float64 ``[n, 2]``)."""
    got = [table(a, b, pm, tolerances, impl) for a, b in pairs]
    return (np.array([g[0] for g in got], dtype=np.int32).reshape(-1, 2, len(COLUMNS)),
            np.array([g[1] for g in got], dtype=np.float64).reshape(-1, 2))


def percentile_of(d2_lo, d2_hi, m, pm):
    """The host report's interpolation between the two order statistics."""
    lo, hi = math.sqrt(d2_lo), math.sqrt(d2_hi)
    return lo + (ranks(m, pm)[1] / 1000.0) * (hi - lo)


def sum_bound(n_edge):
    """Relative gate on the device's fp64 sum against ``math.fsum``: sequential-summation bound plus a 2-ulp root."""
    return (n_edge + 4) * 2.0 ** -52


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _fit(m, h, w):
    """``m`` cut or zero-padded to ``h x w`` (top left aligned)."""
    out = np.zeros((h, w), dtype=bool)
    hh, ww = min(h, m.shape[0]), min(w, m.shape[1])
    out[:hh, :ww] = m[:hh, :ww]
    return out


def checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx) % 2 == 0


def corner(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[h - 1, w - 1] = True
    return m


def shape_cases(h, w):
    """-> list of (name, A, B) of one shape: blobs, the hand-built masks fitted to it and the special pairs."""
    blob_a, blob_b = MC.blob_speckle(h, w, 7000 + h * 3 + w, speckle=0.02), MC.blob_speckle(h, w, 8000 + h + w * 3, speckle=0.05, voids=0.1)
    sp, cb = _fit(MC.spiral(min(max(h, w), 31)), h, w), MC.comb(h, w)
    rg = MC.ring(h, w, h // 5, w // 5, h - 1 - h // 5, w - 1 - w // 5) if min(h, w) >= 5 else np.ones((h, w), dtype=bool)
    full, empty = np.ones((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    tag = f"{h}x{w}"
    return [(f"{tag}/blobs", blob_a, blob_b), (f"{tag}/spiral_vs_comb", sp, cb), (f"{tag}/ring_vs_blob", rg, blob_a),
            (f"{tag}/full_vs_blob", full, blob_b), (f"{tag}/corner_vs_checker", corner(h, w), checker(h, w)),
            (f"{tag}/identical", blob_b, blob_b.copy()), (f"{tag}/empty_vs_blob", empty, blob_a), (f"{tag}/blob_vs_empty", blob_a, empty),
            (f"{tag}/both_empty", empty, empty.copy()), (f"{tag}/full_vs_full", full, full.copy())]


def hand_cases():
    """Every hand-built mask of the comparison oracle against its own half turn."""
    return [(f"hand/{name}", m, m[::-1, ::-1].copy()) for name, m in MC.hand_masks().items()]


def golden_cases():
    cases = hand_cases()
    for h, w in SHAPES:
        cases += shape_cases(h, w)
    return cases


def sparse_blobs(h, w, seed, count=6):
    """A few discs on a large canvas: few edge pixels, so the oracle stays fast at the kernel's cap."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=bool)
    for _ in range(count):
        cy, cx, r = rs.randint(0, h), rs.randint(0, w), rs.randint(3, 40)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m


# ---- the golden file -----------------------------------------------------------------------------------------------------------
def pack_cases(cases):
    counts, sums = batch([(c[1], c[2]) for c in cases])
    return {"names": np.array([c[0] for c in cases]), "shapes": np.array([c[1].shape for c in cases], dtype=np.int32),
            "bits_a": np.concatenate([np.packbits(c[1].reshape(-1)) for c in cases]),
            "bits_b": np.concatenate([np.packbits(c[2].reshape(-1)) for c in cases]),
            "counts": counts, "sums": sums, "pm": np.int32(GOLDEN_PM), "tolerances": np.array(GOLDEN_TOLERANCES, dtype=np.float64)}


def unpack_cases(z):
    """-> list of (name, A, B, counts ``[2, 11]``, sums ``[2]``)."""
    out, oa, ob = [], 0, 0
    for name, (h, w), c, s in zip(z["names"], z["shapes"], z["counts"], z["sums"]):
        nb = (int(h) * int(w) + 7) // 8
        a = np.unpackbits(z["bits_a"][oa:oa + nb])[:h * w].reshape(h, w).astype(bool)
        b = np.unpackbits(z["bits_b"][ob:ob + nb])[:h * w].reshape(h, w).astype(bool)
        oa, ob = oa + nb, ob + nb
        out.append((str(name), a, b, c, s))
    return out

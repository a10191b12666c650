"""Host oracle of ``ops.mask_compare`` (csrc/mask_compare.hip; include/pti_vae.h "shape comparison"), twice over:

* ``impl="scipy"``: ``scipy.ndimage.label`` with a 3 x 3 structure of ones, ``binary_fill_holes`` with its default structure,
  ``bincount`` / ``argmax`` over labels renumbered by first row-major occurrence for the tie rule;
* ``impl="numpy"``: minimum-index propagation over the eight neighbours until nothing changes, and a flood of the
  background from the border over the four neighbours -- no scipy, so the oracle does not rest on one library.

``table`` takes switches that turn on one deliberate MISTAKE each (``MUTATIONS``); the CPU tests use them to show that the
golden cases can tell the mistake from the rule.  The hand-built masks and the seeded random ones of
``tests/golden/mask_compare_golden.npz`` are built here (``golden_cases``); ``tools/make_mask_compare_golden.py`` records
them with the oracle's answers."""
import numpy as np

COLUMNS = ("n_gt", "n_pred", "components_gt", "components_pred", "kept_gt", "kept_pred", "filled_pred", "intersection", "union",
           "gt_x", "gt_y", "gt_w", "gt_h", "pred_x", "pred_y", "pred_w", "pred_h", "gt_width_upper", "gt_width_middle",
           "gt_width_lower", "pred_width_upper", "pred_width_middle", "pred_width_lower", "status")
THRESHOLD = np.float32(0.2)
MUTATIONS = ({"conn": 4}, {"fill_conn": 8}, {"widths": "extent"}, {"tie": "last"}, {"box": "all"})


# ---- masks -----------------------------------------------------------------------------------------------------------------
def masks(gt, pred, threshold=THRESHOLD):
    t = np.float32(threshold)
    return gt != 0, (pred > t) | (pred < -t)


# ---- components ------------------------------------------------------------------------------------------------------------
def _shift(a, dy, dx, fill):
    """``out[y, x] = a[y + dy, x + dx]``, ``fill`` where that leaves the array."""
    out = np.full_like(a, fill)
    h, w = a.shape
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def _neighbours(conn):
    four = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    return four if conn == 4 else four + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def label_numpy(m, conn=8):
    """-> int64 labels, 0 = background, components numbered 1.. by their first row-major pixel."""
    h, w = m.shape
    big = h * w
    lab = np.where(m, np.arange(big, dtype=np.int64).reshape(h, w), big)
    while True:
        new = lab.copy()
        for dy, dx in _neighbours(conn):
            new = np.minimum(new, _shift(lab, dy, dx, big))
        new = np.where(m, new, big)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[m])                       # ascending smallest index = order of first occurrence
    out = np.zeros((h, w), dtype=np.int64)
    out[m] = np.searchsorted(roots, lab[m]) + 1
    return out, len(roots)


def label_scipy(m, conn=8):
    from scipy import ndimage
    structure = np.ones((3, 3), dtype=bool) if conn == 8 else None
    lab, n = ndimage.label(m, structure=structure)
    lab = lab.astype(np.int64)
    if n:                                           # renumber by first row-major occurrence, whatever scipy's order is
        flat = lab.reshape(-1)
        labs, first = np.unique(flat[flat > 0], return_index=True)
        renum = np.zeros(n + 1, dtype=np.int64)
        renum[labs[np.argsort(first)]] = np.arange(1, n + 1)
        lab = renum[lab]
    return lab, n


def largest(lab, n, tie="first"):
    """-> (boolean K, its size); no component: (all False, 0)."""
    if n == 0:
        return np.zeros(lab.shape, dtype=bool), 0
    sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
    pick = int(np.argmax(sizes)) if tie == "first" else n - 1 - int(np.argmax(sizes[::-1]))
    return lab == pick + 1, int(sizes[pick])


def fill_numpy(k, conn=4):
    """K plus what the outside cannot reach over ``conn``-connected steps through the pixels outside K."""
    free = ~np.pad(k, 1)                            # the virtual ring of background
    reach = np.zeros_like(free)
    reach[0, :] = reach[-1, :] = reach[:, 0] = reach[:, -1] = True
    while True:
        new = reach.copy()
        for dy, dx in _neighbours(conn):
            new |= _shift(reach, dy, dx, False)
        new &= free
        if np.array_equal(new, reach):
            break
        reach = new
    return ~reach[1:-1, 1:-1]


def fill_scipy(k, conn=4):
    from scipy import ndimage
    return ndimage.binary_fill_holes(k, structure=None if conn == 4 else np.ones((3, 3), dtype=bool))


def box_of(m):
    if not m.any():
        return [-1, -1, 0, 0]
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def widths_of(m, box, mode="count"):
    x, y, w, h = box
    if h == 0:
        return [0, 0, 0]
    out = []
    for r in (y + h // 4, y + h // 2, y + 3 * h // 4):
        row = m[r, x:x + w]
        if mode == "count":
            out.append(int(row.sum()))
        else:
            cols = np.flatnonzero(row)
            out.append(int(cols[-1] - cols[0] + 1) if len(cols) else 0)
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------
def regions(g, r, impl="scipy", conn=8, fill_conn=4, tie="first"):
    """-> dict with K(G), K(R), P = F(R) and the component counts / sizes."""
    label = label_scipy if impl == "scipy" else label_numpy
    fill = fill_scipy if impl == "scipy" else fill_numpy
    lab_g, n_g = label(g, conn)
    lab_r, n_r = label(r, conn)
    kg, size_g = largest(lab_g, n_g, tie)
    kr, size_r = largest(lab_r, n_r, tie)
    p = fill(kr, fill_conn) if n_r else np.zeros_like(r)
    return {"kg": kg, "kr": kr, "p": p, "n_g": n_g, "n_r": n_r, "size_g": size_g, "size_r": size_r}


def table_masks(g, r, impl="scipy", conn=8, fill_conn=4, widths="count", tie="first", box="K"):
    """The 24 integer columns for one pair of boolean masks."""
    q = regions(g, r, impl, conn, fill_conn, tie)
    p = q["p"]
    box_g = box_of(q["kg"] if box == "K" else g)
    box_r = box_of(q["kr"] if box == "K" else r)
    row = [int(g.sum()), int(r.sum()), q["n_g"], q["n_r"], q["size_g"], q["size_r"], int(p.sum()), int((p & g).sum()),
           int((p | g).sum())] + box_g + box_r + widths_of(g, box_g, widths) + widths_of(p, box_r, widths) + [0]
    assert len(row) == len(COLUMNS)
    return row


def sums_of(gt, pred, p):
    """The three fp64 values for one image: sum((gt - pred P)^2), max(gt), max(pred P)."""
    pp = np.where(p, pred, np.float32(0))
    d = gt.astype(np.float64) - pp.astype(np.float64)
    return [float((d * d).sum()), float(gt.max()), float(pp.max())]


def sq_err_sum_fp32(gt, pred, p):
    """The same squared-error sum with fp32 differences, squares and a sequential fp32 accumulator: its distance from the
    fp64 sum is the yardstick of the GPU test's gate."""
    pp = np.where(p, pred, np.float32(0)).astype(np.float32)
    d = (gt.astype(np.float32) - pp).astype(np.float32)
    return float(np.cumsum((d * d).astype(np.float32).reshape(-1), dtype=np.float32)[-1])


def compare(gt, pred, threshold=THRESHOLD, impl="scipy"):
    """Batch oracle: fp32 ``[n, h, w]`` -> (int32 ``[n, 24]``, float64 ``[n, 3]``, list of boolean P)."""
    counts, sums, ps = [], [], []
    for a, b in zip(gt, pred):
        g, r = masks(a, b, threshold)
        counts.append(table_masks(g, r, impl))
        p = regions(g, r, impl)["p"]
        sums.append(sums_of(a, b, p))
        ps.append(p)
    return np.array(counts, dtype=np.int32).reshape(-1, len(COLUMNS)), np.array(sums, dtype=np.float64).reshape(-1, 3), ps


# ---- images from masks -------------------------------------------------------------------------------------------------------
def images_from_masks(g, r, seed, threshold=THRESHOLD):
    """fp32 images whose masks are exactly ``g`` / ``r``: ground truth non-zero of either sign on ``g``; prediction beyond
    +-threshold on ``r`` and inside it elsewhere, the values exactly AT +threshold and -threshold among the background."""
    rs = np.random.RandomState(seed)
    t = np.float32(threshold)
    gt = np.where(g, (rs.uniform(0.05, 1.0, g.shape) * rs.choice([-1.0, 1.0], g.shape, p=[0.1, 0.9])), 0.0).astype(np.float32)
    fg = (t + rs.uniform(0.01, 0.8, r.shape)) * rs.choice([-1.0, 1.0], r.shape, p=[0.2, 0.8])
    bg = rs.choice([0.0, float(t), -float(t), 0.1, -0.15], r.shape) if t > 0 else np.zeros(r.shape)
    pred = np.where(r, fg, bg).astype(np.float32)
    pred[(~r) & (np.abs(pred) > t)] = t             # rounding to fp32 must not push a background value over the edge
    got_g, got_r = masks(gt, pred, t)
    assert np.array_equal(got_g, g) and np.array_equal(got_r, r)
    return gt, pred


# ---- hand-built masks ----------------------------------------------------------------------------------------------------------
def from_text(rows):
    return np.array([[c == "#" for c in row] for row in rows], dtype=bool)


def spiral(n):
    """An inward spiral one pixel wide on an n x n grid, one pixel of background between its turns: a single component
    whose pixels form one long chain."""
    m = np.zeros((n, n), dtype=bool)
    inside = lambda y, x: 0 <= y < n and 0 <= x < n   # noqa: E731
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(fy, fx) and m[fy, fx]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy                        # turn right
        else:
            return m


def comb(h, w, step=2):
    m = np.zeros((h, w), dtype=bool)
    m[:, ::step] = True
    m[-1, :] = True
    return m


def ring(h, w, y0, x0, y1, x1):
    m = np.zeros((h, w), dtype=bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    m[y0 + 1:y1, x0 + 1:x1] = False
    return m


CHECKER = from_text(["#.#.#", ".#.#.", "#.#.#", ".#.#.", "#.#.#"])
U_SHAPE = from_text(["#.....#", "#.....#", "#.....#", "#.....#", "#######"])


def hand_masks():
    """name -> boolean mask."""
    out = {"spiral_31": spiral(31), "u_shape": U_SHAPE, "comb_9x17": comb(9, 17), "checker_5": CHECKER}
    isl = ring(9, 11, 1, 1, 7, 9)
    isl[4, 5] = isl[4, 6] = True
    out["ring_island"] = isl
    gap = ring(9, 9, 1, 1, 7, 7)
    gap[1, 7] = False                               # the corner pixel: its two neighbours still touch diagonally
    out["ring_diagonal_gap"] = gap
    out["ring_on_border"] = ring(8, 10, 0, 0, 5, 6)  # two sides lie on the image border: still an enclosed hole
    open_c = ring(8, 10, 2, 0, 6, 5)
    open_c[3:6, 0] = False                          # open towards the border: no hole
    out["c_open_to_border"] = open_c
    tie = np.zeros((7, 9), dtype=bool)
    tie[1:3, 5:8] = True                            # six pixels, first in raster order
    tie[4:6, 1:4] = True                            # six pixels
    tie[6, 8] = True
    out["two_equal"] = tie
    late = np.zeros((9, 9), dtype=bool)
    late[0, 0:3] = True
    late[4:8, 3:8] = True
    late[5:7, 4:7] = False                          # the larger one is a ring and comes later; the small one is outside it
    late[1, 8] = True
    out["larger_later"] = late
    out["empty_6x5"] = np.zeros((6, 5), dtype=bool)
    out["full_6x5"] = np.ones((6, 5), dtype=bool)
    out["single_1x1"] = np.ones((1, 1), dtype=bool)
    return out


def blob_speckle(h, w, seed, speckle=0.02, voids=0.03):
    """An ellipse with small voids inside and speckle around it: what a decoded image's mask looks like."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = (h - 1) / 2 + rs.uniform(-0.1, 0.1) * h, (w - 1) / 2 + rs.uniform(-0.1, 0.1) * w
    ry, rx = max(h * rs.uniform(0.2, 0.4), 0.6), max(w * rs.uniform(0.2, 0.4), 0.6)
    blob = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return (blob & (rs.rand(h, w) >= voids)) | (~blob & (rs.rand(h, w) < speckle))


RANDOM_SHAPES = ((1, 1), (1, 7), (7, 1), (5, 5), (31, 33), (64, 64), (67, 129), (256, 256), (1024, 3), (3, 1024))


def golden_cases():
    """-> list of (name, G, R): every hand-built mask as the prediction against a box, and against its own half turn as the
    ground truth; empty and full on either side; seeded random pairs of every tested shape."""
    cases = []
    hand = hand_masks()
    for name, m in hand.items():
        h, w = m.shape
        boxm = np.zeros((h, w), dtype=bool)
        boxm[h // 4:h - h // 4, w // 4:w - w // 4] = True
        cases.append((f"{name}/pred_vs_box", boxm, m))
        cases.append((f"{name}/gt_vs_turned", m, m[::-1, ::-1].copy()))
    e, f = hand["empty_6x5"], hand["full_6x5"]
    cases += [("empty_vs_full", e, f), ("full_vs_empty", f, e)]
    for i, (h, w) in enumerate(RANDOM_SHAPES):
        dense = (h, w) in ((5, 5), (31, 33))
        g = blob_speckle(h, w, 1000 + i, speckle=0.0, voids=0.0)
        g |= np.random.RandomState(1100 + i).rand(h, w) < 0.01
        r = blob_speckle(h, w, 1200 + i, speckle=0.3 if dense else 0.03)
        cases.append((f"random_{h}x{w}", g, r))
    return cases


# ---- the golden file -----------------------------------------------------------------------------------------------------------
def pack_cases(cases):
    """-> dict of arrays for ``np.savez_compressed``: names, shapes, the masks packed as bits, the expected tables."""
    names = np.array([c[0] for c in cases])
    shapes = np.array([c[1].shape for c in cases], dtype=np.int32)
    bits_g = np.concatenate([np.packbits(c[1].reshape(-1)) for c in cases])
    bits_r = np.concatenate([np.packbits(c[2].reshape(-1)) for c in cases])
    expected = np.array([table_masks(c[1], c[2]) for c in cases], dtype=np.int32)
    return {"names": names, "shapes": shapes, "bits_gt": bits_g, "bits_pred": bits_r, "expected": expected}


def unpack_cases(z):
    """The inverse of ``pack_cases`` on a loaded npz -> list of (name, G, R, expected row)."""
    out, og, orr = [], 0, 0
    for name, (h, w), exp in zip(z["names"], z["shapes"], z["expected"]):
        nb = (int(h) * int(w) + 7) // 8
        g = np.unpackbits(z["bits_gt"][og:og + nb])[:h * w].reshape(h, w).astype(bool)
        r = np.unpackbits(z["bits_pred"][orr:orr + nb])[:h * w].reshape(h, w).astype(bool)
        og, orr = og + nb, orr + nb
        out.append((str(name), g, r, exp.tolist()))
    return out

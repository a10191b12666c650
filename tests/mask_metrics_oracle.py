"""Plain-numpy restatement of the reference's mask metrics (``vae_scripts/compute_mask_metrics.py``) and the deterministic
masks the tests run it on.  Nothing here touches the device or the package under test.

The five rules:
  1. a mask is binarised as ``pixel > 0``;
  2. the bounding box ``(x0, y0, w, h)`` covers ALL foreground pixels; a mask without any raises ``ValueError(EMPTY)``;
  3. edente widths: rows ``np.linspace(0, h, S + 2, dtype=int)[1:-1][::-1] + y0`` (lowest first), width of a row =
     last foreground column - first + 1 (gaps count), 0 for an empty row, none for ``S <= 0``;
  4. dente widths: offsets ``int(round(mm / pixel_size_mm))`` (Python round, half to even), row
     ``clamp(H - 1 - offset, 0, H - 1)``, the same width rule over the whole row;
  5. both dicts are ``{"height_0": edente bbox height, "width_0": ...}``.
"""
import numpy as np

EMPTY = "Mask does not contain any foreground pixels"


# ---- the rules ---------------------------------------------------------------------------------------------------------
def binarise(mask):
    return np.asarray(mask) > 0


def row_width(row):
    cols = np.flatnonzero(row)
    return int(cols[-1] - cols[0] + 1) if cols.size else 0


def bbox(fg):
    ys, xs = np.nonzero(fg)
    if ys.size == 0:
        raise ValueError(EMPTY)
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def sample_rows(h, samples):
    """Rows relative to the box's first row, lowest first."""
    if samples <= 0:
        return []
    return [int(r) for r in np.linspace(0, h, samples + 2, dtype=int)[1:-1][::-1]]


def pixel_offsets(heights_mm, pixel_size_mm):
    return [int(round(mm / pixel_size_mm)) for mm in heights_mm]


def bottom_rows(height, offsets):
    return [max(0, min(height - 1, height - 1 - int(o))) for o in offsets]


def pair_attributes(edente, dente, samples, offsets):
    """-> (attrs_edente, attrs_dente); ValueError(EMPTY) for an edente mask without foreground."""
    ed, de = binarise(edente), binarise(dente)
    _, y0, _, h = bbox(ed)
    attrs_e, attrs_d = {"height_0": h}, {"height_0": h}
    for k, r in enumerate(sample_rows(h, samples)):
        attrs_e[f"width_{k}"] = row_width(ed[y0 + r])
    for k, r in enumerate(bottom_rows(de.shape[0], offsets)):
        attrs_d[f"width_{k}"] = row_width(de[r])
    return attrs_e, attrs_d


def geometry(mask, samples, offsets):
    """What ``pti_mask_geometry`` writes for one image: (bbox4, bbox_widths, bottom_widths) as int lists."""
    fg = binarise(mask)
    bottoms = [row_width(fg[r]) for r in bottom_rows(fg.shape[0], offsets)]
    try:
        x0, y0, w, h = bbox(fg)
    except ValueError:
        return [-1, -1, 0, 0], [0] * max(samples, 0), bottoms
    return [x0, y0, w, h], [row_width(fg[y0 + r]) for r in sample_rows(h, samples)], bottoms


# ---- deterministic masks -----------------------------------------------------------------------------------------------
def make_mask(p):
    """Parameters -> mask.  ``p``: {"h", "w", "dtype", "value", "shapes": [["rect", y0, x0, h, w] |
    ["ellipse", cy, cx, ry, rx]], optional "seed" with "speckle" (probability of extra foreground anywhere) and "holes"
    (probability of knocking foreground out inside the shapes, first and last shape rows excepted)}."""
    h, w = p["h"], p["w"]
    fg = np.zeros((h, w), dtype=bool)
    yy, xx = np.mgrid[0:h, 0:w]
    keep = np.zeros((h, w), dtype=bool)
    for kind, a, b, c, d in p["shapes"]:
        if kind == "rect":
            fg[a:a + c, b:b + d] = True
            keep[a, b:b + d] = keep[a + c - 1, b:b + d] = True
        elif kind == "ellipse":
            fg |= ((yy - a) * (yy - a) * d * d + (xx - b) * (xx - b) * c * c) <= c * c * d * d
        else:
            raise ValueError(kind)
    if "seed" in p:
        rs = np.random.RandomState(p["seed"])
        holes, speckle = rs.rand(h, w), rs.rand(h, w)
        fg &= ~((holes < p.get("holes", 0.0)) & ~keep)
        fg |= speckle < p.get("speckle", 0.0)
    return fg.astype(p["dtype"]) * np.dtype(p["dtype"]).type(p["value"])


def ramp_mask(h):
    """Row r has foreground columns 0..r: its width is r + 1, so the widths of a sampled ramp reveal the sampled rows."""
    return (np.arange(h)[None, :] <= np.arange(h)[:, None]).astype(np.uint8)


_DEFAULT_MM = [5.0, 10.0, 14.0, 18.0, 22.0]


def _case(name, edente, dente, samples=5, heights_mm=None, pixel_size_mm=0.15):
    return {"name": name, "edente": edente, "dente": dente, "samples": samples,
            "heights_mm": list(_DEFAULT_MM if heights_mm is None else heights_mm), "pixel_size_mm": pixel_size_mm}


def _m(h, w, shapes, dtype="uint8", value=255, **extra):
    return dict({"h": h, "w": w, "dtype": dtype, "value": value, "shapes": shapes}, **extra)


_DENTE = _m(220, 180, [["ellipse", 120, 90, 95, 70]], seed=11, holes=0.2, speckle=0.001)

# The pairs recorded in tests/golden/mask_metrics_golden.json (tools/make_mask_metrics_golden.py).
CASES = [
    _case("defaults", _m(200, 160, [["ellipse", 110, 80, 60, 50]], seed=3, holes=0.1), _DENTE),
    _case("linspace_s13_h122", _m(140, 90, [["rect", 7, 11, 122, 60]], seed=5, holes=0.3), _DENTE, samples=13),
    _case("linspace_s21_h30", _m(40, 50, [["rect", 4, 3, 30, 41]], seed=6, holes=0.3), _DENTE, samples=21),
    _case("linspace_s25_h30", _m(37, 50, [["rect", 2, 3, 30, 41]], seed=7, holes=0.3), _DENTE, samples=25),
    _case("linspace_s27_h68", _m(80, 33, [["rect", 9, 1, 68, 30]], seed=8, holes=0.3), _DENTE, samples=27),
    _case("no_samples", _m(64, 64, [["ellipse", 30, 30, 20, 25]]), _DENTE, samples=0),
    _case("short_dente_clamps_and_half_even", _m(30, 37, [["rect", 5, 5, 20, 20]], dtype="uint16", value=256),
          _m(20, 45, [["ellipse", 10, 22, 9, 20], ["rect", 0, 10, 1, 7]], dtype="uint16", value=0x8000),
          heights_mm=[0.5, 1.5, 2.5, 19.0, 20.0, 400.0], pixel_size_mm=1.0),
    _case("gap_and_empty_sampled_row", _m(70, 131, [["rect", 3, 70, 12, 8], ["rect", 3, 100, 12, 20], ["rect", 60, 2, 4, 128]],
                                          dtype="float32", value=0.5),
          _m(50, 131, [["rect", 10, 64, 40, 3], ["rect", 10, 128, 40, 3]], dtype="float32", value=2.0),
          heights_mm=[0.0, 1.5, 4.5], pixel_size_mm=0.15),
    _case("single_pixel", _m(9, 70, [["rect", 8, 69, 1, 1]]), _m(1, 70, [["rect", 0, 66, 1, 2]])),
    _case("empty_edente", _m(16, 16, []), _DENTE),
]

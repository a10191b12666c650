"""GPU tests of the mask-metrics path: ``ops.mask_geometry`` (csrc/mask_geometry.hip) against the numpy oracle of
``tests/mask_metrics_oracle.py`` -- every comparison is exact integer equality -- and ``compute_mask_metrics`` end to end
on folders of TIF files.

Every launch here goes through ``_run``: images sit at odd element offsets with foreground-valued poison in the gaps and
behind the last image (a read past a row or an image changes a result), and every output tensor is followed by 64 canary
elements that must survive the launch."""
import json
import os

import numpy as np
import pytest
import torch

import mask_metrics_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 70), (70, 1), (3, 5), (30, 37), (64, 64), (130, 67), (257, 131)]
DTYPES = {"uint8": (np.uint8, 0, [128, 255]), "uint16": (np.uint16, 1, [256, 0x8000]), "float32": (np.float32, 2, [0.5, np.inf])}
POISON = {"uint8": 255, "uint16": 0xFFFF, "float32": 1.0}
MAX_H = 300
CANARY = 0x5A5A5A5A
BOTTOMS = [0, 1, 3, 29, 1000]


def _paint(fg, dtype_name, seed=0):
    """Boolean foreground -> mask of the dtype, foreground pixels drawing from the dtype's foreground values."""
    np_dtype, _, values = DTYPES[dtype_name]
    pick = np.random.RandomState(seed).randint(0, len(values), size=fg.shape)
    return np.where(fg, np.array(values, dtype=np_dtype)[pick], np_dtype(0)).astype(np_dtype)


def _speckle(h, w, seed, density=0.3):
    fg = np.random.RandomState(seed).rand(h, w) < density
    if h * w == 1:
        fg[:] = True
    return fg


def _pack_poisoned(masks, dtype_name):
    """-> (buffer, offsets): every image after the first at an ODD element offset, poison in the gaps and 64 behind."""
    np_dtype = DTYPES[dtype_name][0]
    offsets, cur = [], 0
    for m in masks:
        if offsets:
            cur += 1 if cur % 2 == 0 else 2
        offsets.append(cur)
        cur += m.size
    buf = np.full(cur + 64, POISON[dtype_name], dtype=np_dtype)
    for m, o in zip(masks, offsets):
        assert m.dtype == np_dtype and (o % 2 == 1 or o == 0)
        buf[o:o + m.size] = m.reshape(-1)
    return buf, np.array(offsets, dtype=np.int64)


def _run(dev, masks, dtype_name, samples, bottoms, max_h=MAX_H, hw=None):
    """One launch -> (bbox, bbox_widths, bottom_widths) as nested int lists; checks the canaries behind every output."""
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd.data.mask_metrics import sample_row_table
    buf, offsets = _pack_poisoned(masks, dtype_name)
    b = len(masks)
    hw = np.array([m.shape for m in masks] if hw is None else hw, dtype=np.int32)
    flats, outs = [], []
    for shape in ((b, 4), (b, samples), (b, len(bottoms))):
        n = shape[0] * shape[1]
        flat = torch.full((n + 64,), CANARY, dtype=torch.int32, device=dev)
        flats.append((flat, n))
        outs.append(flat[:n].view(shape))
    got = ops.mask_geometry(torch.from_numpy(buf).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(hw).to(dev),
                            elem=DTYPES[dtype_name][1], max_h=max_h,
                            sample_rows=torch.from_numpy(np.array(sample_row_table(max_h, samples))).to(dev),
                            bottom_offsets=torch.tensor(bottoms, dtype=torch.int32, device=dev), out=tuple(outs))
    torch.cuda.synchronize()
    for flat, n in flats:
        assert bool((flat[n:] == CANARY).all()), "canary behind an output was overwritten"
    return tuple(t.cpu().numpy().tolist() for t in got)


def _expect(fgs, samples, bottoms):
    per = [O.geometry(fg, samples, bottoms) for fg in fgs]
    return tuple([p[k] for p in per] for k in range(3))


def _check(dev, fgs, dtype_name, samples=5, bottoms=BOTTOMS, seed=0):
    masks = [_paint(fg, dtype_name, seed + i) for i, fg in enumerate(fgs)]
    for fg, m in zip(fgs, masks):
        assert np.array_equal(O.binarise(m), fg)
    got, want = _run(dev, masks, dtype_name, samples, bottoms), _expect(fgs, samples, bottoms)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    return got


# ---- shapes, mixed batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_all_shapes_in_one_mixed_batch(dev, dtype_name):
    _check(dev, [_speckle(h, w, 100 + i) for i, (h, w) in enumerate(SHAPES)], dtype_name)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_every_shape_alone(dev, dtype_name):
    for i, (h, w) in enumerate(SHAPES):
        _check(dev, [_speckle(h, w, 200 + i)], dtype_name)


# ---- content ---------------------------------------------------------------------------------------------------------
def _content_cases():
    h, w = 12, 200
    z = lambda: np.zeros((h, w), dtype=bool)   # noqa: E731
    cases = {"empty": z(), "full": ~z()}
    for name, (y, x) in {"top_left": (0, 0), "top_right": (0, w - 1), "bottom_left": (h - 1, 0), "bottom_right": (h - 1, w - 1)}.items():
        cases[name] = z()
        cases[name][y, x] = True
    cases["columns_from_64"] = z()
    cases["columns_from_64"][2:9, 64:70] = True
    cases["columns_from_128"] = z()
    cases["columns_from_128"][1:11, 128:131] = True
    cases["columns_from_128"][5, 199] = True
    gap = z()                                   # bbox rows 0..11: the five sampled rows are 10, 8, 6, 4, 2
    gap[0, 5] = gap[11, 150] = True
    gap[6, 10:20] = gap[6, 90:101] = True       # two blobs: the width spans the gap (10..100 -> 91)
    gap[2, 77] = True                           # rows 4, 8, 10 stay empty: width 0
    cases["gap_and_empty_sampled_rows"] = gap
    return cases


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_content_cases(dev, dtype_name):
    cases = _content_cases()
    got = _check(dev, list(cases.values()), dtype_name)
    by_name = dict(zip(cases, zip(*got)))
    assert by_name["empty"] == ([-1, -1, 0, 0], [0] * 5, [0] * len(BOTTOMS))
    assert by_name["full"][0] == [0, 0, 200, 12]
    assert by_name["gap_and_empty_sampled_rows"][1] == [0, 0, 91, 0, 1]


# ---- values ----------------------------------------------------------------------------------------------------------
def test_integer_foreground_values(dev):
    for dtype_name, np_dtype, values in (("uint8", np.uint8, [128, 255, 1]), ("uint16", np.uint16, [256, 0x8000, 0xFF00, 1])):
        fgs, masks = [], []
        for v in values:
            fg = _speckle(9, 70, int(v))
            fgs.append(fg)
            masks.append((fg * np_dtype(v)).astype(np_dtype))
        assert _run(dev, masks, dtype_name, 5, BOTTOMS) == _expect(fgs, 5, BOTTOMS)


def test_float32_foreground_is_the_bit_pattern_of_x_gt_0(dev):
    bits = lambda u: np.array([u], dtype=np.uint32).view(np.float32)[0]   # noqa: E731
    backgrounds = [np.float32(np.nan), np.float32(-0.0), np.float32(-1.0), bits(0x80000001), bits(0xFFC00000), np.float32(-np.inf),
                   np.float32(0.0)]
    h, w = 9, 140
    mask = np.empty((h, w), dtype=np.float32)
    for r in range(h):
        mask[r] = backgrounds[r % len(backgrounds)]     # every background value fills whole rows
    fg = np.zeros((h, w), dtype=bool)
    fg[1, 3] = fg[4, 133] = True                         # the smallest subnormal, alone in its row
    mask[1, 3] = mask[4, 133] = bits(0x00000001)
    fg[6, 64:70] = fg[7, 0] = fg[7, 139] = True
    mask[6, 64:70] = np.inf
    mask[7, 0], mask[7, 139] = bits(0x7F7FFFFF), np.float32(1e-30)
    assert np.array_equal(mask > 0, fg)                 # IEEE x > 0 on the host (no flush to zero there)
    got, want = _run(dev, [mask], "float32", 5, [0, 1, 2, 4, 7]), _expect([fg], 5, [0, 1, 2, 4, 7])
    assert got == want
    assert got[0] == [[0, 1, 140, 7]] and got[2] == [[0, 140, 6, 1, 1]]


# ---- the rows numpy's linspace samples --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linspace_s13_h122", "linspace_s21_h30"])
def test_linspace_cases_follow_numpy_not_integer_arithmetic(dev, name):
    with open(os.path.join(ROOT, "tests", "golden", "mask_metrics_golden.json"), encoding="utf-8") as fh:
        case = {c["name"]: c for c in json.load(fh)["cases"]}[name]
    mask, exp = O.make_mask(case["edente"]), case["expected"]
    bbox, widths, _ = _run(dev, [mask], case["edente"]["dtype"], case["samples"], [])
    assert bbox == [exp["bbox"]] and widths == [exp["edente_widths"]]
    ramp = O.ramp_mask(exp["bbox"][3])          # widths of the ramp = sampled rows + 1
    _, widths, _ = _run(dev, [ramp], "uint8", case["samples"], [])
    assert [v - 1 for v in widths[0]] == exp["reference_rows"]


# ---- counts and clamps -----------------------------------------------------------------------------------------------
def test_zero_counts_and_bottom_clamps(dev):
    fgs = [_speckle(30, 37, 7), _speckle(3, 5, 8, density=0.9)]
    masks = [_paint(fg, "uint8") for fg in fgs]
    for samples, bottoms in ((0, BOTTOMS), (5, []), (0, [])):
        got = _run(dev, masks, "uint8", samples, bottoms)
        assert got == _expect(fgs, samples, bottoms)
        assert np.array(got[1]).reshape(2, -1).shape[1] == samples and np.array(got[2]).reshape(2, -1).shape[1] == len(bottoms)
    bottoms = [0, 2, 3, 29, 30, 31, 2 ** 31 - 1, -1, -(2 ** 31)]      # 0: last row; >= H: row 0; negative: last row
    got = _run(dev, masks, "uint8", 0, bottoms)
    assert got == _expect(fgs, 0, bottoms)
    last, first = O.row_width(fgs[1][2]), O.row_width(fgs[1][0])
    assert got[2][1] == [last, first, first, first, first, first, first, last, last]


# ---- independence ----------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_batch_or_position(dev):
    fgs = [_speckle(*SHAPES[i % len(SHAPES)], 300 + i, density=0.05 + 0.02 * (i % 9)) for i in range(37)]
    masks = [_paint(fg, "uint16", i) for i, fg in enumerate(fgs)]
    batch = _run(dev, masks, "uint16", 5, BOTTOMS)
    assert batch == _expect(fgs, 5, BOTTOMS)
    assert _run(dev, masks, "uint16", 5, BOTTOMS) == batch                       # two runs are identical
    perm = np.random.RandomState(1).permutation(37)
    permuted = _run(dev, [masks[i] for i in perm], "uint16", 5, BOTTOMS)
    for pos, i in enumerate(perm):
        assert tuple(out[pos] for out in permuted) == tuple(out[i] for out in batch)
    for i in range(37):
        alone = _run(dev, [masks[i]], "uint16", 5, BOTTOMS)
        assert tuple(out[0] for out in alone) == tuple(out[i] for out in batch)


# ---- bad descriptors -------------------------------------------------------------------------------------------------
def test_bad_descriptor_is_reported_and_neighbours_are_unaffected(dev):
    fgs = [_speckle(30, 37, 1), _speckle(64, 64, 2), _speckle(3, 5, 3), _speckle(9, 9, 4), _speckle(5, 7, 5)]
    masks = [_paint(fg, "uint8") for fg in fgs]
    want = _expect(fgs, 5, BOTTOMS)
    hw = [m.shape for m in masks]
    hw[3], hw[2] = (0, 9), (3, 0)                       # H < 1, W < 1
    got = _run(dev, masks, "uint8", 5, BOTTOMS, max_h=40, hw=hw)     # image 1: H = 64 > max_h = 40
    for i in (1, 2, 3):
        assert got[0][i] == [-2, -2, 0, 0] and got[1][i] == [0] * 5 and got[2][i] == [0] * len(BOTTOMS)
    for i in (0, 4):
        assert tuple(out[i] for out in got) == tuple(out[i] for out in want)


def test_ops_rejects_bad_shapes_on_the_device(dev):
    from pti_ldm_vae_amd import ops
    src = torch.zeros(16, dtype=torch.uint8, device=dev)
    off, hw = torch.zeros(1, dtype=torch.int64, device=dev), torch.tensor([[4, 4]], dtype=torch.int32, device=dev)
    rows, bot = torch.zeros(5, 2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ok = dict(elem=0, max_h=4, sample_rows=rows, bottom_offsets=bot)
    assert ops.mask_geometry(src, off, hw, **ok)[0].cpu().tolist() == [[-1, -1, 0, 0]]
    for bad in (dict(ok, max_h=5), dict(ok, sample_rows=rows.t()), dict(ok, sample_rows=rows.reshape(-1)),
                dict(ok, bottom_offsets=bot.reshape(1, 1)), dict(ok, bottom_offsets=bot.cpu()),
                dict(ok, max_h=ops.MASK_ROW_CAP + 1, sample_rows=torch.zeros(ops.MASK_ROW_CAP + 2, 2, dtype=torch.int32, device=dev)),
                dict(ok, out=(torch.zeros(1, 4, dtype=torch.int32, device=dev),) * 2)):
        with pytest.raises(ValueError):
            ops.mask_geometry(src, off, hw, **bad)
    with pytest.raises(ValueError):
        ops.mask_geometry(src, off, hw.reshape(2, 1), **ok)


# ---- the Python layer and the command ------------------------------------------------------------------------------------
def test_mask_attributes_on_the_recorded_cases(dev):
    from pti_ldm_vae_amd.data.mask_metrics import mask_attributes, pixel_offsets_mm
    with open(os.path.join(ROOT, "tests", "golden", "mask_metrics_golden.json"), encoding="utf-8") as fh:
        cases = json.load(fh)["cases"]
    for case in cases:
        exp = case["expected"]
        offsets = pixel_offsets_mm(case["heights_mm"], case["pixel_size_mm"])
        assert offsets == exp["offsets"]
        (got,) = mask_attributes([O.make_mask(case["edente"])], [O.make_mask(case["dente"])], samples=case["samples"],
                                 bottom_offsets=offsets, device=dev)
        if "error" in exp:
            assert got == exp["error"]
            continue
        attrs_e, attrs_d = got
        assert list(attrs_e.items()) == [("height_0", exp["height"])] + [(f"width_{k}", v) for k, v in enumerate(exp["edente_widths"])]
        assert list(attrs_d.items()) == [("height_0", exp["height"])] + [(f"width_{k}", v) for k, v in enumerate(exp["dente_widths"])]
    # one mixed-dtype batch of all pairs that share the default parameters
    same = [c for c in cases if c["samples"] == 5 and c["heights_mm"] == [5.0, 10.0, 14.0, 18.0, 22.0] and c["pixel_size_mm"] == 0.15]
    got = mask_attributes([O.make_mask(c["edente"]) for c in same], [O.make_mask(c["dente"]) for c in same], device=dev)
    for c, g in zip(same, got):
        exp = c["expected"]
        if "error" in exp:
            assert g == exp["error"]
        else:
            assert list(g[0].values()) == [exp["height"]] + exp["edente_widths"]
            assert list(g[1].values()) == [exp["height"]] + exp["dente_widths"]


def test_compute_mask_metrics_end_to_end(dev, tmp_path, capsys):
    from pti_ldm_vae_amd import compute_mask_metrics as cli
    from pti_ldm_vae_amd.data import write_tiff
    from pti_ldm_vae_amd.data.attributes import attributes_for_paths
    ed_dir, de_dir = tmp_path / "edente", tmp_path / "dente"
    ed_dir.mkdir()
    de_dir.mkdir()
    ell = lambda h, w, **kw: O._m(h, w, [["ellipse", h // 2, w // 2, h // 3, w // 3]], **kw)   # noqa: E731
    # stem -> (edente mask, edente file, dente mask, dente file, deflate); with --batch-size 2 the sorted stems form the
    # batches (a, b): uint8 throughout, (c, d): float32 throughout, (e, f): mixed types -> binarised on the host
    pairs = {
        "a_u8": (ell(200, 160, seed=1, holes=0.2), "a_u8.tif", ell(210, 150, seed=2, speckle=0.001), "a_u8.tif", False),
        "b_deflate": (ell(190, 170, seed=3, holes=0.1), "b_deflate.tif", ell(230, 180, seed=4), "b_deflate.tif", True),
        "c_f32": (ell(200, 160, dtype="float32", value=0.25, seed=5, holes=0.2), "c_f32.tif",
                  ell(200, 160, dtype="float32", value=3.0, seed=6), "c_f32.tif", False),
        "d_sizes": (ell(131, 257, dtype="float32", value=1.0, seed=7, holes=0.3), "d_sizes.TIFF",
                    ell(257, 67, dtype="float32", value=1.0, seed=8), "d_sizes.tif", False),
        "e_empty": (O._m(50, 60, []), "e_empty.tif", ell(200, 160), "e_empty.tif", False),
        "f_u16": (ell(180, 140, dtype="uint16", value=256, seed=9), "f_u16.tif", ell(222, 140, seed=10), "f_u16.tif", False),
    }
    want_e, want_d = {}, {}
    for stem, (ed, ed_name, de, de_name, deflate) in pairs.items():
        ed, de = O.make_mask(ed), O.make_mask(de)
        write_tiff(str(ed_dir / ed_name), ed, deflate=deflate, rows_per_strip=64 if deflate else None)
        write_tiff(str(de_dir / de_name), de, deflate=deflate)
        if stem != "e_empty":
            want_e[ed_name], want_d[de_name] = O.pair_attributes(ed, de, 5, O.pixel_offsets([5, 10, 14, 18, 22], 0.15))
    write_tiff(str(ed_dir / "g_only_edente.tif"), O.make_mask(ell(40, 40)))
    write_tiff(str(de_dir / "h_only_dente.tif"), O.make_mask(ell(40, 40)))
    (de_dir / "notes.txt").write_text("not a mask")
    out_e, out_d = tmp_path / "metrics" / "deep" / "attributes_edente.json", tmp_path / "metrics" / "attributes_dente.json"
    cli.main(["--edente-dir", str(ed_dir), "--dente-dir", str(de_dir), "--output-edente", str(out_e), "--output-dente", str(out_d),
              "--batch-size", "2"])
    printed = capsys.readouterr().out
    assert f"Skipping e_empty: {O.EMPTY}" in printed
    assert "g_only_edente" not in printed.split("{", 1)[0] and "h_only_dente" not in printed
    got_e, got_d = json.loads(out_e.read_text()), json.loads(out_d.read_text())
    assert got_e == want_e and list(got_e) == list(want_e) and [list(v) for v in got_e.values()] == [list(v) for v in want_e.values()]
    assert got_d == want_d and list(got_d) == list(want_d)
    assert out_e.read_text() == json.dumps(want_e, indent=4) and out_d.read_text() == json.dumps(want_d, indent=4)
    assert all(type(v) is int for attrs in list(got_e.values()) + list(got_d.values()) for v in attrs.values())
    assert "e_empty.tif" not in got_e and "e_empty.tif" not in got_d
    for (ed_name, attrs_e), attrs_d in zip(got_e.items(), got_d.values()):
        assert attrs_d["height_0"] == attrs_e["height_0"]           # the dente file carries the EDENTE bbox height
    summary = json.loads(printed[printed.index("\n{\n") + 1:])
    assert list(summary) == ["config", "generated", "edente_entries", "dente_entries"]
    assert summary["edente_entries"] == summary["dente_entries"] == 5
    assert summary["generated"] == [str(out_e), str(out_d)]
    assert summary["config"]["pixel_size_mm"] == 0.15 and summary["config"]["dente_heights_mm"] == [5.0, 10.0, 14.0, 18.0, 22.0]
    assert summary["config"]["edente_width_samples"] == 5
    # the edente file is what the AR-VAE config's attribute_file names
    with open(os.path.join(ROOT, "config", "ar_vae_dente_kl1e3.json"), encoding="utf-8") as fh:
        reg = dict(json.load(fh)["regularized_attributes"], attribute_file=str(out_e))
    paths = [str(ed_dir / name) for name in want_e]
    attrs = attributes_for_paths(paths, reg, "edente")
    assert len(attrs) == len(paths) == 5
    assert [a["height_0"] for a in attrs] == [float(v["height_0"]) for v in want_e.values()]
    assert all(set(a) == {"height_0", "width_0", "width_1", "width_2", "width_3", "width_4"} for a in attrs)
    # no stems in common: FileNotFoundError, as the reference
    lonely = tmp_path / "lonely"
    lonely.mkdir()
    with pytest.raises(FileNotFoundError):
        cli.main(["--edente-dir", str(ed_dir), "--dente-dir", str(lonely), "--output-edente", str(out_e), "--output-dente", str(out_d)])

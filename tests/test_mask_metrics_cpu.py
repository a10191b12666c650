"""CPU tests of the mask-metrics path: the numpy oracle against the reference's recorded results
(``tests/golden/mask_metrics_golden.json``), the host helpers of ``data.mask_metrics``, the CLI's defaults, and the
argument checks of ``ops.mask_geometry`` / ``pti_mask_geometry`` that return before any launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import mask_metrics_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mask_metrics_golden.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN, encoding="utf-8") as fh:
        return {c["name"]: c for c in json.load(fh)["cases"]}


# ---- oracle against the reference's recorded results ------------------------------------------------------------------
def test_fixture_describes_the_generator_cases(gold):
    assert [{k: v for k, v in c.items() if k != "expected"} for c in gold.values()] == O.CASES


@pytest.mark.parametrize("name", [c["name"] for c in O.CASES])
def test_oracle_equals_the_reference(gold, name):
    case = gold[name]
    exp = case["expected"]
    ed, de = O.make_mask(case["edente"]), O.make_mask(case["dente"])
    offsets = O.pixel_offsets(case["heights_mm"], case["pixel_size_mm"])
    assert offsets == exp["offsets"]
    if "error" in exp:
        with pytest.raises(ValueError) as e:
            O.pair_attributes(ed, de, case["samples"], offsets)
        assert str(e.value) == exp["error"] == O.EMPTY
        return
    assert list(O.bbox(O.binarise(ed))) == exp["bbox"]
    assert O.sample_rows(exp["bbox"][3], case["samples"]) == exp["reference_rows"]
    attrs_e, attrs_d = O.pair_attributes(ed, de, case["samples"], offsets)
    keys = ["height_0"] + [f"width_{k}" for k in range(len(exp["edente_widths"]))]
    assert list(attrs_e) == keys and list(attrs_e.values()) == [exp["height"]] + exp["edente_widths"]
    keys = ["height_0"] + [f"width_{k}" for k in range(len(exp["dente_widths"]))]
    assert list(attrs_d) == keys and list(attrs_d.values()) == [exp["height"]] + exp["dente_widths"]
    g = O.geometry(ed, case["samples"], [])
    assert g[0] == exp["bbox"] and g[1] == exp["edente_widths"]
    assert O.geometry(de, 0, offsets)[2] == exp["dente_widths"]


@pytest.mark.parametrize("name,samples,height", [("linspace_s13_h122", 13, 122), ("linspace_s21_h30", 21, 30)])
def test_linspace_cases_bite(gold, name, samples, height):
    """The rows the reference samples there are not the integer-arithmetic rows: a kernel computing them itself fails."""
    case = gold[name]
    assert case["samples"] == samples and case["expected"]["bbox"][3] == height
    integer_rows = [(i * height) // (samples + 1) for i in range(1, samples + 1)][::-1]
    assert case["expected"]["reference_rows"] != integer_rows
    if name == "linspace_s13_h122":
        assert 60 in case["expected"]["reference_rows"] and 61 in integer_rows


# ---- host helpers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [0, 1, 5, 13, 21])
def test_sample_row_table_is_the_numpy_expression(samples):
    from pti_ldm_vae_amd.data.mask_metrics import sample_row_table
    table = sample_row_table(300, samples)
    assert table.dtype == np.int32 and table.shape == (301, samples)
    for h in range(301):
        want = np.linspace(0, h, samples + 2, dtype=int)[1:-1][::-1] if samples > 0 else []
        assert table[h].tolist() == list(want), (samples, h)
    assert sample_row_table(7, -3).shape == (8, 0)


def test_pixel_offsets_mm():
    from pti_ldm_vae_amd.data.mask_metrics import pixel_offsets_mm
    assert pixel_offsets_mm((5, 10, 14, 18, 22), 0.15) == [33, 67, 93, 120, 147]
    assert pixel_offsets_mm([0.5, 1.5, 2.5], 1.0) == [0, 2, 2]          # half to even
    assert all(isinstance(v, int) for v in pixel_offsets_mm([5.0], 0.15))


def test_pack_masks_pass_through_and_fallback():
    from pti_ldm_vae_amd.data.mask_metrics import pack_masks
    rs = np.random.RandomState(0)
    for dtype, elem in ((np.uint8, 0), (np.uint16, 1), (np.float32, 2)):
        masks = [(rs.rand(3, 5) * 300).astype(dtype), (rs.rand(7, 1) * 300).astype(dtype), (rs.rand(1, 9) * 300).astype(dtype)]
        buf, offsets, hw, got = pack_masks(masks)
        assert got == elem and buf.dtype == dtype and buf.ndim == 1
        assert offsets.dtype == np.int64 and offsets.tolist() == [0, 15, 22]       # odd element offsets: no alignment
        assert hw.dtype == np.int32 and hw.tolist() == [[3, 5], [7, 1], [1, 9]]
        for m, o in zip(masks, offsets):
            assert np.array_equal(buf[o:o + m.size].reshape(m.shape), m)           # untouched values
    # other dtypes and mixed batches: binarised on the host, in the array's own dtype
    f64 = np.array([[1e-300, 0.0, -1.0, np.nan, 5e-324]])
    for masks in ([f64], [f64, np.ones((2, 2), np.uint8)], [np.array([[-3, 0, 7]], dtype=np.int16)],
                  [np.array([[True, False]])], [np.ones((2, 2), np.uint8), np.ones((2, 2), np.float32)]):
        buf, offsets, hw, elem = pack_masks(masks)
        assert elem == 0 and buf.dtype == np.uint8
        want = np.concatenate([(np.asarray(m) > 0).reshape(-1) for m in masks]).astype(np.uint8)
        assert np.array_equal(buf, want)
    assert pack_masks([f64])[0].tolist() == [1, 0, 0, 0, 1]                          # no underflow through float32
    big = np.arange(6, dtype=">u2").reshape(2, 3)                                     # byte order is not a dtype of its own
    buf, _, _, elem = pack_masks([big])
    assert elem == 1 and buf.tolist() == list(range(6))
    with pytest.raises(ValueError):
        pack_masks([np.zeros(5, np.uint8)])


def test_cli_defaults_are_the_reference_values():
    from pathlib import Path
    from pti_ldm_vae_amd import compute_mask_metrics as cli
    a = cli.parse_args([])
    assert a.edente_dir == Path("./data/edente") and a.dente_dir == Path("./data/dente")
    assert a.output_edente == Path("./data/metrics/attributes_edente.json")
    assert a.output_dente == Path("./data/metrics/attributes_dente.json")
    assert a.pixel_size_mm == 0.15 and tuple(a.dente_heights_mm) == (5.0, 10.0, 14.0, 18.0, 22.0)
    assert a.edente_width_samples == 5 and a.batch_size == 64
    a = cli.parse_args(["--dente-heights-mm", "1", "2.5", "--edente-width-samples", "13", "--batch-size", "3"])
    assert a.dente_heights_mm == [1.0, 2.5] and a.edente_width_samples == 13 and a.batch_size == 3


def test_cli_lists_tif_files_case_insensitively(tmp_path):
    from pti_ldm_vae_amd import compute_mask_metrics as cli
    for name in ("b.TIF", "a.tiff", "c.Tif", "d.png", "e.tif.txt"):
        (tmp_path / name).write_bytes(b"")
    assert list(cli.list_tif_files(tmp_path)) == ["a", "b", "c"]


# ---- argument checks that return before any launch -----------------------------------------------------------------
def test_ops_mask_geometry_rejects_cpu_tensors_and_wrong_dtypes():
    from pti_ldm_vae_amd import ops
    src, off, hw = torch.zeros(16, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.tensor([[4, 4]], dtype=torch.int32)
    rows, bot = torch.zeros(5, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    ok = dict(elem=0, max_h=4, sample_rows=rows, bottom_offsets=bot)
    with pytest.raises(ValueError, match="CUDA"):
        ops.mask_geometry(src, off, hw, **ok)                                     # right dtypes, host tensors
    with pytest.raises(ValueError, match="elem"):
        ops.mask_geometry(src, off, hw, **dict(ok, elem=3))
    for bad in (dict(ok, elem=2), dict(ok, elem=1), dict(ok, sample_rows=rows.long()), dict(ok, bottom_offsets=bot.long()),
                dict(ok, sample_rows=rows.numpy())):
        with pytest.raises(TypeError):
            ops.mask_geometry(src, off, hw, **bad)
    with pytest.raises(TypeError):
        ops.mask_geometry(src.float(), off, hw, **ok)
    with pytest.raises(TypeError):
        ops.mask_geometry(src, off.int(), hw, **ok)
    with pytest.raises(TypeError):
        ops.mask_geometry(src, off, hw.long(), **ok)


def test_pti_mask_geometry_validates_before_launch():
    from pti_ldm_vae_amd import _lib, ops
    h = _lib.lib()
    p = C.c_void_p(64)      # never dereferenced: every call below returns before a launch

    def call(src=p, offsets=p, hw=p, b=1, elem=0, max_h=64, rows=p, samples=5, bottom=p, n_bottom=5, bbox=p, bw=p, tw=p):
        return h.pti_mask_geometry(src, offsets, hw, b, elem, max_h, rows, samples, bottom, n_bottom, bbox, bw, tw, None)

    for kw in ({"src": None}, {"offsets": None}, {"hw": None}, {"bbox": None}, {"rows": None}, {"bw": None}, {"bottom": None},
               {"tw": None}):
        assert call(**kw) == -1, kw
        assert b"null pointer" in h.pti_last_error_string()
    assert call(elem=3) == -2 and b"elem" in h.pti_last_error_string()
    assert call(elem=-1) == -2
    assert call(max_h=ops.MASK_ROW_CAP + 1) == -2 and b"row cap" in h.pti_last_error_string()
    assert ops.MASK_ROW_CAP >= 4096
    for kw in ({"b": 0}, {"samples": -1}, {"n_bottom": -1}, {"max_h": -1}):
        assert call(**kw) == -2, kw
        assert b"bad counts" in h.pti_last_error_string()
    with pytest.raises(_lib.PtiError, match="row cap"):
        _lib.check(call(max_h=ops.MASK_ROW_CAP + 1), "pti_mask_geometry")

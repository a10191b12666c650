"""CPU tests of the pair registration (``compare_images --straighten``): the oracle of ``tests/mask_register_oracle.py``
against hand-worked answers and against its own second restatements, the recorded answers of
``tests/golden/mask_register_golden.npz``, the golden cases' power to tell each of eight plausible mistakes from the rule,
and every refusal of the ops, the entry points and the command that returns before a launch."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import mask_compare_oracle as O
import mask_register_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mask_register_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return R.unpack_cases(z)


@pytest.fixture(scope="module")
def registered(gold):
    """name -> (gt, pred, register(gt, pred)) of every golden case: computed once, never changed."""
    out = {}
    for name, g, r, flavour, seed, _ in gold:
        gt, pred = R.images(g, r, flavour, seed)
        out[name] = (gt, pred, R.register(gt, pred))
    return out


# ---- consistency -------------------------------------------------------------------------------------------------------------
def test_golden_file_holds_the_cases_and_the_oracles_answers(gold, registered):
    built = R.golden_cases()
    assert [c[0] for c in gold] == [c[0] for c in built]
    assert {"ellipse_+12", "ellipse_-27", "ellipse_+55", "ellipse_-80", "upright", "disc", "bar", "hole_island", "on_border", "l_shape"} <= set(registered)
    assert {c[3] for c in gold} == {"flat", "textured", "signed"}
    for (name, g, r, _, _, exp), (_, g2, r2, _, _) in zip(gold, built):
        assert np.array_equal(g, g2) and np.array_equal(r, r2), name
        got = R.digest(registered[name][2])
        for key in ("moments", "align", "nonzero"):
            assert got[key].tolist() == exp[key].tolist(), (name, key)
        assert got["beta"].tobytes() == exp["beta"].tobytes() and got["sums"].tobytes() == exp["sums"].tobytes(), name
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_two_restatements_of_the_moments_agree(gold):
    for name, g, r, _, _, exp in gold:
        for side, mask in enumerate((g, r)):
            a, b = R.filled_largest(mask, "scipy"), R.filled_largest(mask, "numpy")
            assert np.array_equal(a, b), name
            m = R.raw_moments(a)
            assert m == R.raw_moments_profiles(b) and m + list(R.central(m)) == exp["moments"][side].tolist(), (name, side)
    # at the largest image the integers stay inside int64 with room to spare
    full = [1024 * 1024, 1024 * 1024 * 1023 // 2, 1024 * 1024 * 1023 // 2, 0, 0, 0]
    full[3] = full[5] = 1024 * sum(x * x for x in range(1024))
    full[4] = (1023 * 1024 // 2) ** 2
    assert max(abs(v) for v in R.central(full)) < 2 ** 61 and full == R.raw_moments_profiles(np.ones((1024, 1024), dtype=bool))


def test_angle_branches_are_taken_on_the_integers(registered):
    co = {name: v[2]["coeffs"] for name, v in registered.items()}
    mo = {name: v[2]["moments"] for name, v in registered.items()}
    for name in ("upright", "disc"):
        assert co[name] == [[0.0, 1.0, 0.0]] * 2 and mo[name][0][7] == 0 and mo[name][1][7] == 0
    assert mo["disc"][0][6] == mo["disc"][0][8] and mo["upright"][0][8] > mo["upright"][0][6]
    assert co["bar"] == [[math.pi / 2, 0.0, 1.0]] * 2 and mo["bar"][0][7] == 0 and mo["bar"][0][8] < mo["bar"][0][6]
    for tilt in R.ELLIPSE_TILTS:                     # beta undoes the tilt: within a degree of it on a pixel ellipse
        beta = math.degrees(co[f"ellipse_{tilt:+.0f}"][0][0])
        assert abs(beta - tilt) < 1.0, (tilt, beta)
    assert all(abs(c[0]) <= math.pi / 2 for v in co.values() for c in v)
    hole = mo["hole_island"][0]
    assert hole[:6] != R.raw_moments(R.filled_largest(R.golden_masks()["hole_island"][0], fill=False))
    assert R.angle([0] * 6) == (0.0, 1.0, 0.0)       # an empty region asks for no rotation


def test_rotated_ellipses_stand_upright(registered):
    """The angle rule applied once more to the rotated images.  MEASURED with this oracle (degrees, |residual|):
    ground truth (mask != 0, which includes the cubic's ringing halo) 0.568 / 0.544 / 0.253 / 0.471, prediction (|v| > 0.2)
    0.114 / 0.049 / 0.142 / 0.085 for the tilts 12 / -27 / 55 / -80.  Gates: twice the largest of each side."""
    worst = [0.0, 0.0]
    for tilt in R.ELLIPSE_TILTS:
        res = registered[f"ellipse_{tilt:+.0f}"][2]
        again = [R.angle(R.raw_moments(R.filled_largest(res["rot_gt"] != 0)))[0],
                 R.angle(R.raw_moments(R.filled_largest(np.abs(res["rot_pred"]) > R.THRESHOLD)))[0]]
        print(f"tilt {tilt:+.0f}: residual beta gt {math.degrees(again[0]):+.4f} deg, pred {math.degrees(again[1]):+.4f} deg")
        worst = [max(w, abs(math.degrees(b))) for w, b in zip(worst, again)]
    assert worst[0] <= 2 * 0.568 and worst[1] <= 2 * 0.142, worst


def test_the_halo_of_the_cubic_is_kept(registered):
    """Known and kept: after the rotation ``!= 0`` is the object plus a ringing halo."""
    res = registered["ellipse_+12"][2]
    g = R.golden_masks()["ellipse_+12"][0]
    assert int(g.sum()) == 1495 and int((res["rot_gt"] != 0).sum()) == 1799
    assert res["rot_gt"].min() < 0.0 and res["rot_gt"].max() > 1.0       # overshoot on a flat object of ones


def test_bottom_fifth_is_h_over_5():
    for h in range(1, 1025):
        assert h // 5 == int(h * 0.2), h


# ---- hand-worked answers --------------------------------------------------------------------------------------------------------
def test_weights_at_the_lattice_points_are_exact():
    for dtype in (np.float32, np.float64):
        w = [float(v[0]) for v in R.cubic_weights(np.array([0.0]), -0.75, dtype)]
        assert w == [0.0, 1.0, 0.0, 0.0]
        w = [float(v[0]) for v in R.cubic_weights(np.array([1.0]), -0.75, dtype)]
        assert w == [0.0, 0.0, 1.0, 0.0]
        w = [float(v[0]) for v in R.cubic_weights(np.array([0.5]), -0.75, dtype)]
        assert w == [-0.09375, 0.59375, 0.59375, -0.09375]                # OpenCV's INTER_CUBIC row at one half


def test_identity_and_quarter_turns_move_pixels_exactly():
    rs = np.random.RandomState(3)
    for h, w in ((5, 1), (5, 5), (7, 9), (12, 8)):
        img = rs.uniform(-1, 1, (h, w)).astype(np.float32)
        for dtype in (np.float32, np.float64):
            assert np.array_equal(R.rotate(img, 1.0, 0.0, dtype), img.astype(dtype))
        # a quarter turn: out(x, y) = in(cx - (y - cy), cy + (x - cx)), clamped to the image
        out = R.rotate(img, 0.0, 1.0)
        cx, cy = w // 2, h // 2
        for y in range(h):
            for x in range(w):
                sx, sy = min(max(cx - (y - cy), 0), w - 1), min(max(cy + (x - cx), 0), h - 1)
                assert out[y, x] == img[sy, sx]
    sq = rs.uniform(-1, 1, (9, 9)).astype(np.float32)       # odd and square: the centre is a pixel, nothing is clamped
    assert np.array_equal(R.rotate(sq, 0.0, 1.0), np.rot90(sq, 1)) and np.array_equal(R.rotate(sq, 0.0, -1.0), np.rot90(sq, -1))


def test_alignment_by_hand():
    gt = np.zeros((10, 9), dtype=np.float32)
    pred = np.zeros((10, 9), dtype=np.float32)
    gt[8, 4:7] = 1.0                                 # columns 4, 5, 6 -> 15 // 3 = 5
    gt[0, 0] = 9.0                                   # above the bottom two rows: not counted
    pred[9, 1] = pred[9, 2] = -0.001                 # any non-zero value counts; 3 // 2 = 1 (truncated, not rounded to 2)
    pred[3, 8] = 0.5
    aligned, info = R.align(gt, pred)
    assert info == [5, 1, 3, 2, 4, 0]
    assert aligned[9, 5] == aligned[9, 6] == np.float32(-0.001) and aligned[3].tolist() == [0] * 9 and aligned.sum() == pred[9].sum()
    back, info = R.align(pred, gt)
    assert info == [1, 5, 2, 3, -4, 0] and back[8, 0:3].tolist() == [1, 1, 1] and back[0].tolist() == [0] * 9
    assert R.align(gt, np.zeros_like(gt))[1] == [5, -1, 3, 0, 0, 2] and R.align(np.zeros_like(gt), gt)[1] == [-1, 5, 0, 3, 0, 1]
    assert R.align(np.zeros_like(gt), np.zeros_like(gt))[1] == [-1, -1, 0, 0, 0, 3]
    assert np.array_equal(R.align(gt, np.zeros_like(gt) + pred * 0)[0], pred * 0)


# ---- deliberate mistakes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", R.MUTATIONS, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
def test_each_mistake_changes_a_golden_answer(gold, registered, mutation):
    changed = []
    for name, _, _, _, _, exp in gold:
        gt, pred, _ = registered[name]
        got = R.digest(R.register(gt, pred, **mutation))
        if any(not np.array_equal(got[k], exp[k]) for k in exp):
            changed.append(name)
    print(f"{mutation}: changes {changed}")
    assert changed
    if mutation == {"centre": "half"}:               # on an odd size (w - 1) / 2 IS w // 2: only the even-sized cases can tell
        assert "odd_65x67" not in changed and "ellipse_+12" in changed


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
def test_ops_refuse_before_a_launch():
    from pti_ldm_vae_amd import ops
    assert ops.MASK_MOMENTS_COLUMNS == R.MOMENT_COLUMNS and ops.ALIGN_BOTTOM_COLUMNS == R.ALIGN_COLUMNS
    a = torch.zeros(2, 6, 4)
    co = torch.zeros(2, 2, 3, dtype=torch.float64)
    for call in (lambda x, y: ops.mask_moments(x, y), lambda x, y: ops.warp_cubic(x, y, co), lambda x, y: ops.align_bottom(x, y),
                 lambda x, y: ops.register_pairs(x, y)):
        with pytest.raises(ValueError, match="CUDA"):
            call(a, a)                                                    # right dtype, host tensors
        for gt, pred in ((a.double(), a), (a, a.half()), (a.numpy(), a), (a, None)):
            with pytest.raises(TypeError, match="float32"):
                call(gt, pred)


def test_entry_points_validate_before_launch():
    from pti_ldm_vae_amd import _lib, ops
    h = _lib.lib()
    p = C.c_void_p(64)      # never dereferenced: every call below returns before a launch
    q = C.c_void_p(128)
    ws = h.pti_mask_moments_ws_bytes

    def moments(gt=p, pred=p, n=2, hh=8, w=8, thr=0.2, cleaned=p, mo=p, co=p, wsp=p, ws_bytes=None):
        return h.pti_mask_moments(gt, pred, n, hh, w, thr, cleaned, mo, co, wsp, ws(n, hh, w) if ws_bytes is None else ws_bytes, None)

    def warp(gt=p, pred=p, co=p, n=2, hh=8, w=8, og=q, op=C.c_void_p(192)):
        return h.pti_warp_cubic(gt, pred, co, n, hh, w, og, op, None)

    def align(rg=p, rp=p, n=2, hh=8, w=8, out=q, info=p):
        return h.pti_align_bottom(rg, rp, n, hh, w, out, info, None)

    for kw in ({"gt": None}, {"pred": None}, {"cleaned": None}, {"mo": None}, {"co": None}, {"wsp": None}):
        assert moments(**kw) == -1 and b"null pointer" in h.pti_last_error_string(), kw
    for kw in ({"gt": None}, {"pred": None}, {"co": None}, {"og": None}, {"op": None}):
        assert warp(**kw) == -1 and b"null pointer" in h.pti_last_error_string(), kw
    for kw in ({"rg": None}, {"rp": None}, {"out": None}, {"info": None}):
        assert align(**kw) == -1 and b"null pointer" in h.pti_last_error_string(), kw
    for call in (lambda **kw: moments(ws_bytes=1 << 40, **kw), warp, align):
        for kw in ({"n": 0}, {"hh": 0}, {"w": 0}, {"n": -1}):
            assert call(**kw) == -1 and b"bad shape" in h.pti_last_error_string(), kw
        for kw in ({"hh": 1025}, {"w": 1025}, {"n": 65536}):
            assert call(**kw) == -2 and b"unsupported" in h.pti_last_error_string(), kw
    for hh in (1, 4):                                # the moments and the rotation take any height, the alignment needs a fifth
        assert align(hh=hh) == -2 and b"bottom fifth" in h.pti_last_error_string()
        assert moments(hh=hh, ws_bytes=8) == -1 and b"workspace of" in h.pti_last_error_string()
    for thr in (-0.1, float("nan")):
        assert moments(thr=thr) == -1 and b"threshold" in h.pti_last_error_string()
    odd4, odd8 = C.c_void_p(66), C.c_void_p(68)
    for kw in ({"gt": odd4}, {"pred": odd4}, {"cleaned": odd4}, {"mo": odd8}, {"co": odd8}):
        assert moments(**kw) == -1 and b"misaligned" in h.pti_last_error_string(), kw
    assert moments(wsp=odd4) == -1 and b"4-byte aligned" in h.pti_last_error_string()
    assert moments(ws_bytes=ws(2, 8, 8) - 1) == -1 and b"workspace of" in h.pti_last_error_string()
    for kw in ({"gt": odd4}, {"pred": odd4}, {"co": odd8}, {"og": odd4}, {"op": odd4}):
        assert warp(**kw) == -1 and b"misaligned" in h.pti_last_error_string(), kw
    for kw in ({"og": p}, {"op": p}, {"op": q}):
        assert warp(**kw) == -1 and b"alias" in h.pti_last_error_string(), kw
    for kw in ({"rg": odd4}, {"rp": odd4}, {"out": odd4}, {"info": odd4}):
        assert align(**kw) == -1 and b"misaligned" in h.pti_last_error_string(), kw
    assert align(out=p) == -1 and b"alias" in h.pti_last_error_string()
    # the size query: pure host arithmetic, twice the comparison's workspace
    for n, hh, w in ((1, 1, 1), (2, 8, 8), (3, 65, 67), (64, 1024, 1024)):
        assert ws(n, hh, w) == 2 * h.pti_mask_compare_ws_bytes(n, hh, w) > 0
    assert ws(0, 8, 8) == ws(1, 0, 8) == ws(1, 8, 0) == ws(1, 1025, 8) == ws(1, 8, 1025) == 0
    text = open(os.path.join(ROOT, "include", "pti_vae.h")).read()
    assert f"#define PTI_MASK_MOMENTS_COLUMNS {len(ops.MASK_MOMENTS_COLUMNS)}" in text
    assert f"#define PTI_ALIGN_BOTTOM_COLUMNS {len(ops.ALIGN_BOTTOM_COLUMNS)}" in text
    assert ops.ALIGN_BOTTOM_MIN_HEIGHT == 5


def test_command_arguments_and_report_rows(capsys):
    from pti_ldm_vae_amd import compare_images as cli
    from pti_ldm_vae_amd.utils import compare_metrics as M
    a = cli.parse_args(["--results-dir", "r"])
    assert a.straighten is False and a.write_registered is None
    a = cli.parse_args(["--results-dir", "r", "--straighten", "--write-registered", "out"])
    assert a.straighten is True and str(a.write_registered) == "out"
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--results-dir", "r", "--write-registered", "out"])
    assert e.value.code == 2 and "--write-registered needs --straighten" in capsys.readouterr().err
    mo = np.zeros((2, 10), dtype=np.int64)
    mo[0, :6] = [4, 6, 10, 10, 15, 30]
    mo[1, :6] = [2, 3, 5, 5, 8, 13]
    co = np.array([[math.radians(12.5), 0.0, 0.0], [-math.pi / 2, 0.0, -1.0]])
    block = cli.registration_block(mo, co, np.array([5, 1, 3, 2, 4, 0], dtype=np.int32))
    assert block == {"angle_gt_deg": pytest.approx(12.5, abs=1e-12), "moments_gt": dict(m00=4, m10=6, m01=10, m20=10, m11=15, m02=30),
                     "angle_pred_deg": -90.0, "moments_pred": dict(m00=2, m10=3, m01=5, m20=5, m11=8, m02=13),
                     "centre_gt": 5, "centre_pred": 1, "shift": 4}
    ok = np.array([5, 1, 3, 2, 4, 0], dtype=np.int32)
    assert cli.registration_skip(mo, ok) is None
    for status, who in ((1, "ground truth"), (2, "prediction"), (3, "ground truth and the prediction")):
        assert cli.registration_skip(mo, np.array([0, 0, 0, 0, 0, status])) == "no foreground in the bottom 20 % of the " + who
    empty = mo.copy()
    empty[1, 0] = 0
    assert cli.registration_skip(empty, ok) == M.NO_PRED
    empty[0, 0] = 0
    assert cli.registration_skip(empty, ok) == M.NO_GT
    bad = mo.copy()
    bad[1, 9] = 1
    with pytest.raises(RuntimeError, match="overrun"):
        cli.registration_skip(bad, ok)

"""GPU tests of the pair registration: ``ops.mask_moments`` / ``warp_cubic`` / ``align_bottom`` / ``register_pairs`` (appended to
csrc/mask_compare.hip) against ``tests/mask_register_oracle.py`` and ``tests/golden/mask_register_golden.npz``, STAGE BY
STAGE so that no integer depends on a float computed elsewhere: the moments are compared with the oracle's integers, the
rotation with the fp64 oracle under a gate worked out per case from the fp32 restatement, and the alignment with the oracle
applied to the very arrays the device rotated.

Launches go through helpers that put the images inside larger buffers with foreground-valued poison round them, follow every
output and the workspace with 64 canary words, and fill the workspace with random words first."""
import math
import os

import numpy as np
import pytest
import torch

import mask_compare_oracle as O
import mask_register_oracle as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mask_register_golden.npz")
CANARY_I, CANARY_F, POISON = 0x5A5A5A5A, -12345.678, 7.5
SIZES = ((5, 1), (5, 5), (7, 9), (65, 67), (96, 80), (256, 256), (1024, 5), (5, 1024))


def _poisoned(dev, a, lead):
    buf = torch.full((lead + a.size + 64,), POISON, dtype=torch.float32, device=dev)
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return view


def _canaried(dev, shape, dtype):
    """-> (flat buffer, view of ``shape`` at its front): 64 canaries behind the view."""
    count = int(np.prod(shape))
    flat = torch.full((count + 64,), CANARY_F if dtype.is_floating_point else CANARY_I, dtype=dtype, device=dev)
    return flat, flat[:count].view(shape)


def _intact(flat, count):
    want = CANARY_F if flat.dtype.is_floating_point else CANARY_I
    return bool((flat[count:] == torch.tensor(want, dtype=flat.dtype, device=flat.device)).all())


def _moments(dev, gt, pred, threshold=R.THRESHOLD, stale=0):
    """One ``ops.mask_moments`` launch -> (cleaned, moments, coeffs) as numpy; all canaries checked."""
    from pti_ldm_vae_amd import _lib, ops
    n, h, w = gt.shape
    d_gt, d_pred = _poisoned(dev, gt, 17), _poisoned(dev, pred, 5)
    f_c, cleaned = _canaried(dev, (n, h, w), torch.float32)
    f_m, moments = _canaried(dev, (n, 2, 10), torch.int64)
    f_k, coeffs = _canaried(dev, (n, 2, 3), torch.float64)
    words = (_lib.lib().pti_mask_moments_ws_bytes(n, h, w) + 3) // 4
    key = ("mask_moments", dev.index, ops._stream(), n, h, w)
    flat_w = ops._SCRATCH.get(("canaried",) + key)
    if flat_w is None:                              # the scratch ops.mask_moments will find: a view with canaries behind it
        flat_w = ops._SCRATCH[("canaried",) + key] = torch.empty(words + 64, dtype=torch.int32, device=dev)
        ops._SCRATCH[key] = flat_w[:words].view(torch.float32)
    gen = torch.Generator(device=dev).manual_seed(stale)
    flat_w[:words] = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    flat_w[words:] = CANARY_I
    ops.mask_moments(d_gt, d_pred, threshold=float(threshold), out=(cleaned, moments, coeffs))
    torch.cuda.synchronize()
    assert _intact(f_c, n * h * w) and _intact(f_m, n * 20) and _intact(f_k, n * 6), "a canary behind an output was overwritten"
    assert bool((flat_w[words:] == CANARY_I).all()), "canary behind the workspace was overwritten"
    return cleaned.cpu().numpy(), moments.cpu().numpy(), coeffs.cpu().numpy()


def _warp(dev, gt, pred, coeffs):
    """One ``ops.warp_cubic`` launch with hand-set coefficients -> (rotated gt, rotated pred) as numpy; canaries checked."""
    from pti_ldm_vae_amd import ops
    n, h, w = gt.shape
    f_g, out_g = _canaried(dev, (n, h, w), torch.float32)
    f_p, out_p = _canaried(dev, (n, h, w), torch.float32)
    co = torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float64)).to(dev)
    ops.warp_cubic(_poisoned(dev, gt, 9), _poisoned(dev, pred, 33), co, out=(out_g, out_p))
    torch.cuda.synchronize()
    assert _intact(f_g, n * h * w) and _intact(f_p, n * h * w), "a canary behind a rotated image was overwritten"
    return out_g.cpu().numpy(), out_p.cpu().numpy()


def _align(dev, rot_gt, rot_pred):
    from pti_ldm_vae_amd import ops
    n, h, w = rot_gt.shape
    f_a, aligned = _canaried(dev, (n, h, w), torch.float32)
    f_i, info = _canaried(dev, (n, 6), torch.int32)
    ops.align_bottom(_poisoned(dev, rot_gt, 3), _poisoned(dev, rot_pred, 21), out=(aligned, info))
    torch.cuda.synchronize()
    assert _intact(f_a, n * h * w) and _intact(f_i, n * 6), "a canary behind an alignment output was overwritten"
    return aligned.cpu().numpy(), info.cpu().numpy()


def _check_moments(got, gt, pred, threshold=R.THRESHOLD):
    """Device (cleaned, moments, coeffs) against the oracle on every image of the batch."""
    cleaned, moments, coeffs = got
    for i in range(len(gt)):
        want_c, want_m, want_k = R.moments_stage(gt[i], pred[i], threshold)
        assert moments[i].tolist() == want_m, f"image {i} {gt[i].shape}"
        assert cleaned[i].tobytes() == want_c.tobytes(), f"cleaned prediction of image {i}"
        for side in range(2):
            beta, cb, sb = (float(v) for v in coeffs[i, side])
            assert abs(beta - want_k[side][0]) <= 1e-12 and abs(cb - want_k[side][1]) <= 1e-12 and abs(sb - want_k[side][2]) <= 1e-12
            if want_m[side][7] == 0:                # B == 0: decided on the integers, exact coefficients
                assert (beta, cb, sb) in ((0.0, 1.0, 0.0), (math.pi / 2, 0.0, 1.0)) and [beta, cb, sb] == want_k[side]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return R.unpack_cases(z)


@pytest.fixture(scope="module")
def golden_batch(gold):
    """The 96 x 80 golden cases as one batch: (names, gt, pred, expected digests).  Never changed."""
    cases = [c for c in gold if c[1].shape == R.GOLDEN_SHAPE]
    pairs = [R.images(g, r, flavour, seed) for _, g, r, flavour, seed, _ in cases]
    return [c[0] for c in cases], np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), [c[5] for c in cases]


@pytest.fixture(scope="module")
def sized():
    """(h, w) -> (gt, pred) batches of two seeded blob-plus-speckle pairs per tested size (one at 256 x 256)."""
    out = {}
    for k, (h, w) in enumerate(SIZES):
        pairs = [O.images_from_masks(O.blob_speckle(h, w, 700 + 10 * k + i, speckle=0.02), O.blob_speckle(h, w, 800 + 10 * k + i, speckle=0.05),
                                     seed=k + i) for i in range(1 if h * w > 10000 else 2)]
        out[(h, w)] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    return out


@pytest.fixture(scope="module")
def staged(dev, golden_batch):
    """The golden batch through the device's moments and rotation, once: dict of numpy arrays."""
    _, gt, pred, _ = golden_batch
    cleaned, moments, coeffs = _moments(dev, gt, pred)
    rot_gt, rot_pred = _warp(dev, gt, cleaned, coeffs)
    return {"cleaned": cleaned, "moments": moments, "coeffs": coeffs, "rot_gt": rot_gt, "rot_pred": rot_pred}


# ---- moments ---------------------------------------------------------------------------------------------------------------------
def test_moments_of_every_golden_case(dev, gold, golden_batch, staged):
    names, gt, pred, exp = golden_batch
    for i, name in enumerate(names):
        assert staged["moments"][i, :, :9].tolist() == exp[i]["moments"].tolist(), name
        assert staged["moments"][i, :, 9].tolist() == [0, 0]
        assert np.abs(staged["coeffs"][i, :, 0] - exp[i]["beta"]).max() <= 1e-12, name
    _check_moments((staged["cleaned"], staged["moments"], staged["coeffs"]), gt, pred)
    by = dict(zip(names, staged["coeffs"].tolist()))
    assert by["upright"] == by["disc"] == [[0.0, 1.0, 0.0]] * 2 and by["bar"] == [[math.pi / 2, 0.0, 1.0]] * 2
    for name, g, r, flavour, seed, e in gold:       # the odd-sized case
        if g.shape != R.GOLDEN_SHAPE:
            a, b = R.images(g, r, flavour, seed)
            got = _moments(dev, a[None], b[None])
            assert got[1][0, :, :9].tolist() == e["moments"].tolist(), name
            _check_moments(got, a[None], b[None])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_at_every_size(dev, sized, size):
    gt, pred = sized[size]
    _check_moments(_moments(dev, gt, pred, stale=size[0]), gt, pred)


def test_moments_of_empty_sides_and_another_threshold(dev):
    gt = np.zeros((3, 6, 7), dtype=np.float32)
    pred = np.zeros((3, 6, 7), dtype=np.float32)
    gt[0, 1:5, 2:4] = 1.0                            # image 0: no prediction; image 1: no ground truth; image 2: neither
    pred[1, 2:4, 1:6] = 0.7
    pred[1, 0, 0] = 0.2                              # exactly at the threshold: background, and removed from c
    cleaned, moments, coeffs = got = _moments(dev, gt, pred)
    _check_moments(got, gt, pred)
    assert moments[0, 1].tolist() == moments[1, 0].tolist() == moments[2, 0].tolist() == [0] * 10
    assert coeffs[2].tolist() == [[0.0, 1.0, 0.0]] * 2 and coeffs[0, 0].tolist() == [0.0, 1.0, 0.0]
    assert coeffs[1, 1].tolist() == [math.pi / 2, 0.0, 1.0] and cleaned[1, 0, 0] == 0.0 and not cleaned[0].any()
    g, r = R.golden_masks()["hole_island"][:2]
    for thr in (0.0, 0.5):
        a, b = R.images(g, r, "signed", 5, threshold=thr)
        _check_moments(_moments(dev, a[None], b[None], threshold=thr), a[None], b[None], thr)


def test_moment_rows_do_not_depend_on_batch_position_and_calls_repeat(dev, golden_batch, staged):
    _, gt, pred, _ = golden_batch
    probe = 7                                        # hole_island
    order = [3, probe, 0, 0, probe, 9]
    got = _moments(dev, gt[order], pred[order], stale=5)
    again = _moments(dev, gt[order], pred[order], stale=6)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    for pos in (1, 4):
        for a, ref in zip(got, (staged["cleaned"], staged["moments"], staged["coeffs"])):
            assert a[pos].tobytes() == ref[probe].tobytes()
    alone = _moments(dev, gt[probe:probe + 1], pred[probe:probe + 1], stale=7)
    assert alone[1][0].tobytes() == staged["moments"][probe].tobytes() and alone[2][0].tobytes() == staged["coeffs"][probe].tobytes()


# ---- rotation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_coefficients_give_a_bitwise_copy(dev, sized, size):
    gt, pred = sized[size]
    ident = np.tile(np.array([0.0, 1.0, 0.0]), (len(gt), 2, 1))
    out_g, out_p = _warp(dev, gt, pred, ident)
    assert out_g.tobytes() == gt.tobytes() and out_p.tobytes() == pred.tobytes()


def _rotation_case(name, dev_out, src, cb, sb):
    """Device output against the fp64 oracle; the gate is twice what the fp32 restatement deviates from it."""
    want = R.rotate(src, cb, sb, np.float64)
    mirror = R.rotate(src, cb, sb, np.float32)
    gate = 2.0 * float(np.abs(mirror.astype(np.float64) - want).max())
    got = float(np.abs(dev_out.astype(np.float64) - want).max())
    print(f"rotation {name}: deviation from the fp64 oracle {got:.3e}, fp32 restatement {gate / 2:.3e}, gate {gate:.3e}, "
          f"bitwise equal to the restatement: {dev_out.tobytes() == mirror.tobytes()}")
    assert got <= gate, name
    return got


def test_rotation_by_the_golden_angles(dev, golden_batch, staged):
    names, gt, _, _ = golden_batch
    worst = 0.0
    for i, name in enumerate(names):
        for side, (out, src) in enumerate(((staged["rot_gt"], gt), (staged["rot_pred"], staged["cleaned"]))):
            _, cb, sb = staged["coeffs"][i, side]
            worst = max(worst, _rotation_case(f"{name}/{'gt' if side == 0 else 'pred'}", out[i], src[i], cb, sb))
    print(f"largest deviation of a rotated golden image from the fp64 oracle: {worst:.3e}")


@pytest.mark.parametrize("size", ((65, 67), (96, 80), (7, 9)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_rotation_by_hand_set_angles(dev, sized, size):
    """Quarter turns (exact coefficients: the gate is 0, pixels only move) and two odd angles, with canaries at 65 x 67."""
    gt, pred = sized[size]
    n = len(gt)
    for beta, cb, sb in ((math.pi / 2, 0.0, 1.0), (-math.pi / 2, 0.0, -1.0), (0.3, math.cos(0.3), math.sin(0.3)),
                         (-1.1, math.cos(-1.1), math.sin(-1.1))):
        co = np.tile(np.array([[beta, cb, sb], [-beta, cb, -sb]]), (n, 1, 1))
        out_g, out_p = _warp(dev, gt, pred, co)
        for i in range(n):
            _rotation_case(f"{size} beta {beta:+.3f} gt", out_g[i], gt[i], cb, sb)
            _rotation_case(f"{size} beta {-beta:+.3f} pred", out_p[i], pred[i], cb, -sb)


def test_rotation_reads_inside_the_image_for_any_coefficients(dev, sized):
    gt, pred = sized[(7, 9)]
    for co in ([0.0, 1e300, -1e300], [0.0, float("nan"), 1.0], [0.0, 3.0, 250.0]):
        out_g, out_p = _warp(dev, gt, pred, np.tile(np.array(co), (len(gt), 2, 1)))     # poison round the inputs: 7.5
        ok = np.isnan(out_g) | (np.abs(out_g) <= np.abs(gt).max() * 4)
        assert ok.all()


# ---- alignment -------------------------------------------------------------------------------------------------------------------
def _check_align(dev, rot_gt, rot_pred):
    aligned, info = _align(dev, rot_gt, rot_pred)
    for i in range(len(rot_gt)):
        want_a, want_i = R.align(rot_gt[i], rot_pred[i])
        assert info[i].tolist() == want_i, i
        assert aligned[i].tobytes() == want_a.tobytes(), i
    return info


def test_alignment_of_the_device_rotated_golden_images(dev, golden_batch, staged):
    info = _check_align(dev, staged["rot_gt"], staged["rot_pred"])
    assert (info[:, 5] == 0).all() and (info[:, 4] != 0).any()
    print("golden shifts:", dict(zip(golden_batch[0], info[:, 4].tolist())))


@pytest.mark.parametrize("size", ((5, 1), (5, 5), (7, 9), (65, 67), (1024, 5), (5, 1024)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_alignment_by_hand(dev, size):
    h, w = size
    k = h // 5
    gt = np.zeros((6, h, w), dtype=np.float32)
    pred = np.zeros((6, h, w), dtype=np.float32)
    rs = np.random.RandomState(h + w)
    body = rs.uniform(0.1, 1.0, (h, w)).astype(np.float32)
    gt[0], pred[0] = body, body                      # 0: shift 0
    gt[1, h - 1, w - 1] = 1.0                        # 1: shift +(w - 1)
    pred[1, h - 1, 0] = -2.0
    pred[1, 0, :] = 3.0
    gt[2, h - k, 0] = 1.0                            # 2: shift -(w - 1)
    pred[2, h - 1, w - 1] = 0.5
    pred[2, :, w - 1] = 0.5
    gt[3, :h - k] = 1.0                              # 3: nothing in the ground truth's bottom fifth
    pred[3] = body
    gt[4] = body                                     # 4: nothing in the prediction's
    pred[4, :h - k] = body[:h - k]
    gt[5, :h - k, :] = 1.0                           # 5: neither
    info = _check_align(dev, gt, pred)
    assert info[:, 5].tolist() == [0, 0, 0, 1, 2, 3]
    assert info[:3, 4].tolist() == [0, w - 1, -(w - 1)] and info[3:, 4].tolist() == [0, 0, 0]


# ---- the whole -------------------------------------------------------------------------------------------------------------------
def test_register_pairs_is_the_three_ops_and_feeds_mask_compare(dev, golden_batch, staged):
    from pti_ldm_vae_amd import ops
    _, gt, pred, _ = golden_batch
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    rot_gt, aligned, info = ops.register_pairs(d_gt[:, None], d_pred[:, None])              # [n, 1, h, w], fresh outputs
    cleaned, moments, coeffs = ops.mask_moments(d_gt, d_pred)
    r_gt, r_pred = ops.warp_cubic(d_gt, cleaned, coeffs)
    a_pred, a_info = ops.align_bottom(r_gt, r_pred)
    torch.cuda.synchronize()
    for a, b in ((rot_gt, r_gt), (aligned, a_pred), (info["moments"], moments), (info["coeffs"], coeffs), (info["align"], a_info)):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert rot_gt.cpu().numpy().tobytes() == staged["rot_gt"].tobytes() and moments.cpu().numpy().tobytes() == staged["moments"].tobytes()
    # the measurement of the registered pair: the comparison kernel against ITS oracle on the same device arrays
    counts, sums = ops.mask_compare(rot_gt, aligned)
    want_c, want_s, _ = O.compare(rot_gt.cpu().numpy(), aligned.cpu().numpy())
    assert counts.cpu().numpy().tolist() == want_c.tolist()
    got_s = sums.cpu().numpy()
    assert got_s[:, 1:].tolist() == want_s[:, 1:].tolist() and np.allclose(got_s[:, 0], want_s[:, 0], rtol=1e-12, atol=0)
    # caller-owned outputs, and the refusals that need a device
    out = (torch.empty_like(d_gt), torch.empty_like(d_gt), torch.empty_like(moments), torch.empty_like(coeffs), torch.empty_like(a_info))
    got = ops.register_pairs(d_gt, d_pred, out=out)
    assert got[0] is out[0] and got[1] is out[1] and got[2]["align"] is out[4]
    torch.cuda.synchronize()
    assert out[1].cpu().numpy().tobytes() == a_pred.cpu().numpy().tobytes()
    low = torch.zeros(1, 4, 8, device=dev)
    for call in (lambda: ops.register_pairs(low, low), lambda: ops.align_bottom(low, low), lambda: ops.warp_cubic(d_gt, d_pred, coeffs[:1]),
                 lambda: ops.warp_cubic(d_gt, d_pred, coeffs.float()), lambda: ops.mask_moments(d_gt, d_pred, threshold=-1.0),
                 lambda: ops.mask_moments(d_gt, d_pred[:, :4]), lambda: ops.register_pairs(d_gt, d_pred, out=out[:3]),
                 lambda: ops.warp_cubic(d_gt, d_pred, coeffs, out=(d_gt, out[1]))):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            call()
    assert ops.mask_moments(low, low)[1].cpu().numpy().tolist() == [[[0] * 10] * 2]          # the moments take any height

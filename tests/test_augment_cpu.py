"""CPU tests of the train-time augmentation: the parameter draws of ``data/augment.py``, the policy's config
forms, the oracle's noise statistics, and the argument validation of the two C entry points that returns before any
launch.  The kernels themselves are compared with the oracle in tests/test_gpu_augment.py."""
import ctypes as C
import itertools
import json
import math

import numpy as np
import pytest

import augment_oracle as O
from pti_ldm_vae_amd.data.augment import AugmentPolicy, draw_params, draw_raw, inverse_map

ALWAYS = dict(hflip_p=1.0, vflip_p=1.0, rot90_p=1.0, ssr_p=1.0, elastic_p=1.0)
NEVER = dict(hflip_p=0.0, vflip_p=0.0, rot90_p=0.0, ssr_p=0.0, elastic_p=0.0)


def test_draw_depends_on_seed_epoch_index_only():
    pol = AugmentPolicy()
    a = draw_params(pol, 42, 3, 17, 64, 64)
    b = draw_params(pol, 42, 3, 17, 64, 64)
    assert a[0].dtype == np.float32 and a[0].shape == (6,) and a[1].dtype == np.uint64 and a[2].dtype == np.float32
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    # drawing other samples in between (another batch composition) changes nothing: there is no hidden state
    for i in range(5):
        draw_params(pol, 42, 3, i, 64, 64)
    c = draw_params(pol, 42, 3, 17, 64, 64)
    assert np.array_equal(a[0], c[0]) and a[1] == c[1] and a[2] == c[2]
    keys = {int(draw_params(pol, s, e, i, 64, 64)[1]) for s, e, i in ((42, 3, 17), (43, 3, 17), (42, 4, 17), (42, 3, 18))}
    assert len(keys) == 4


def test_all_probabilities_zero_is_identity():
    pol = AugmentPolicy(**NEVER)
    for i in range(50):
        mat, _, alpha = draw_params(pol, 1, 0, i, 48, 80)
        assert np.array_equal(mat, np.array([1, 0, 0, 0, 1, 0], np.float32)) and alpha == 0.0


def test_limits_over_2000_draws():
    pol = AugmentPolicy(**{**ALWAYS, "hflip_p": 0.0, "vflip_p": 0.0, "rot90_p": 0.0})
    H, W = 64, 96
    seen = {k: [] for k in ("dx", "dy", "scale", "angle")}
    for i in range(2000):
        raw = draw_raw(pol, 7, 1, i, H, W)
        for k in seen:
            seen[k].append(raw[k])
        assert raw["alpha"] == 50.0 and 0 <= raw["key"] < 1 << 64
        # the same limits read back from the matrix: linear part = Rot(-angle) / scale
        m = inverse_map(raw, H, W)
        scale = 1.0 / math.sqrt(m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
        angle = math.degrees(math.atan2(m[0, 1], m[0, 0]))
        assert scale == pytest.approx(raw["scale"], rel=1e-12) and angle == pytest.approx(raw["angle"], abs=1e-9)
        # the centre maps to centre - shift / ... : forward image of the source centre is centre + t
        ctr = np.array([(W - 1) / 2, (H - 1) / 2, 1.0])
        back = m @ np.array([ctr[0] + raw["dx"], ctr[1] + raw["dy"], 1.0])
        assert np.allclose(back, ctr, atol=1e-9)
    for k, lim in (("dx", 0.1 * W), ("dy", 0.1 * H), ("angle", 15.0)):
        v = np.array(seen[k])
        assert np.abs(v).max() <= lim and np.abs(v).max() > 0.9 * lim and v.min() < 0 < v.max(), k
    s = np.array(seen["scale"])
    assert 0.9 <= s.min() < 0.91 and 1.09 < s.max() <= 1.1


def test_hflip_frequency():
    pol = AugmentPolicy()
    n = sum(draw_raw(pol, 42, 0, i, 64, 64)["hflip"] for i in range(4000))
    print(f"hflip frequency over 4000 draws: {n / 4000:.4f}")
    assert abs(n / 4000 - 0.5) <= 0.04          # five binomial sigma
    ks = [draw_raw(AugmentPolicy(rot90_p=1.0), 42, 0, i, 64, 64)["k"] for i in range(600)]
    assert set(ks) == {1, 2, 3}
    assert {draw_raw(AugmentPolicy(rot90_p=1.0), 42, 0, i, 24, 40)["k"] for i in range(100)} == {2}


@pytest.mark.parametrize("shape", [(64, 64), (24, 40)])
def test_flips_and_quarter_turns_are_exact_lattice_maps(shape):
    """Every combination of flips and k: the drawn fp32 matrix has entries 0 / +-1 and integer offsets, and the oracle
    warp with it equals np.flip / np.rot90 of the input exactly."""
    H, W = shape
    rng = np.random.default_rng(3)
    img = rng.standard_normal((1, 2, H, W))
    pol = AugmentPolicy(ssr_p=0.0, elastic_p=0.0)
    want_combos = set(itertools.product((False, True), (False, True), (0, 1, 2, 3) if H == W else (0, 2)))
    seen = set()
    for i in range(400):
        raw = draw_raw(pol, 11, 0, i, H, W)
        combo = (raw["hflip"], raw["vflip"], raw["k"])
        if combo in seen:
            continue
        seen.add(combo)
        mat, _, alpha = draw_params(pol, 11, 0, i, H, W)
        assert alpha == 0.0 and set(np.abs(mat[[0, 1, 3, 4]]).tolist()) <= {0.0, 1.0} and np.all(mat == np.round(mat))
        want = img
        if raw["hflip"]:
            want = np.flip(want, axis=-1)
        if raw["vflip"]:
            want = np.flip(want, axis=-2)
        want = np.rot90(want, raw["k"], axes=(-2, -1))
        assert np.array_equal(O.warp(img, mat[None]), want), combo
        assert np.array_equal(O.warp_f32(img, mat[None]), want.astype(np.float32)), combo
    assert seen == want_combos


def test_policy_forms_and_ar_safe_defaults(capsys):
    assert AugmentPolicy.from_config(False) is None and AugmentPolicy.from_config(None) is None
    assert AugmentPolicy.from_config(True) == AugmentPolicy()
    d = AugmentPolicy().to_dict()
    assert (d["hflip_p"], d["vflip_p"], d["rot90_p"], d["ssr_p"], d["shift_limit"], d["scale_limit"], d["rotate_limit"],
            d["elastic_p"], d["elastic_alpha"], d["elastic_sigma"]) == (0.5, 0.5, 0.5, 0.5, 0.1, 0.1, 15.0, 0.3, 50.0, 5.0)
    p = AugmentPolicy.from_config({"rotate_limit": 5, "elastic_p": 0.0})
    assert p.rotate_limit == 5 and p.elastic_p == 0.0 and p.hflip_p == 0.5
    capsys.readouterr()
    ar = AugmentPolicy.from_config(True, ar_vae_enabled=True)
    said = capsys.readouterr().out
    assert ar.scale_limit == 0.0 and ar.elastic_p == 0.0 and ar.hflip_p == 0.5 and ar.shift_limit == 0.1
    assert said.count("\n") == 1 and "scale_limit" in said and "elastic_p" in said
    kept = AugmentPolicy.from_config({"scale_limit": 0.05, "elastic_p": 0.2}, ar_vae_enabled=True)
    assert kept.scale_limit == 0.05 and kept.elastic_p == 0.2 and capsys.readouterr().out == ""
    half = AugmentPolicy.from_config({"elastic_p": 0.2}, ar_vae_enabled=True)
    assert half.scale_limit == 0.0 and half.elastic_p == 0.2
    # an AR-safe policy never scales and never warps elastically
    for i in range(200):
        raw = draw_raw(ar, 5, 0, i, 64, 64)
        assert raw["scale"] == 1.0 and raw["alpha"] == 0.0


def test_unknown_key_and_bad_values_raise():
    with pytest.raises(ValueError, match="unknown key"):
        AugmentPolicy.from_config({"hflip": 0.5})
    with pytest.raises(ValueError):
        AugmentPolicy.from_config({"hflip_p": 1.5})
    with pytest.raises(ValueError):
        AugmentPolicy.from_config("yes")


def test_oracle_noise_statistics():
    a = np.stack([O.noise(0x1234567890ABCDEF, c, 64, 64) for c in range(2)])
    b = np.stack([O.noise(0x1234567890ABCDF0, c, 64, 64) for c in range(2)])
    assert a.min() >= -1.0 and a.max() < 1.0
    corr = np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]
    chan = np.corrcoef(a[0].reshape(-1), a[1].reshape(-1))[0, 1]
    print(f"noise over 2x64x64: mean {a.mean():+.4f}, var {a.var():.4f}, corr between keys {corr:+.4f}, between channels {chan:+.4f}")
    assert abs(a.mean()) < 0.03 and abs(a.var() - 1 / 3) < 0.03 and abs(corr) < 0.05 and abs(chan) < 0.05
    # exact in fp32: the kernel's float conversion loses nothing
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)


def test_field_restatement_is_close_to_scipy():
    """The fp32 restatement that sizes the GPU tolerances follows scipy's filter (reflection, radius, weights)."""
    keys, alphas = [3, 2 ** 63 + 5], [50.0, 0.0]
    ref = O.field(keys, alphas, 1.5, 20, 33)
    f32 = O.field_f32(keys, alphas, 1.5, 20, 33)
    assert not ref[1].any() and not f32[1].any() and np.abs(ref[0]).max() > 1.0
    assert np.abs(f32 - ref).max() < 1e-4


def test_validation_returns_before_any_launch():
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(4096)
    assert h.pti_elastic_field(p, p, 5.0, 1, 8, 64, p, None) == -1 and b"radius" in h.pti_last_error_string()
    assert h.pti_elastic_field(p, p, 0.0, 1, 64, 64, p, None) == -1 and b"sigma" in h.pti_last_error_string()
    assert h.pti_elastic_field(None, p, 5.0, 1, 64, 64, p, None) == -1 and b"null" in h.pti_last_error_string()
    assert h.pti_elastic_field(p, p, 5.0, 1, 0, 64, p, None) == -1
    assert h.pti_elastic_field(p, p, 9.0, 1, 64, 64, p, None) == -2          # radius 36 above the built limit
    assert h.pti_augment_warp(p, p, None, 1, 1, 8, 8, p, None) == -1 and b"alias" in h.pti_last_error_string()
    q = C.c_void_p(4096 + 4 * 8 * 8 - 4)                                        # overlaps the last element of src
    assert h.pti_augment_warp(p, p, None, 1, 1, 8, 8, q, None) == -1
    assert h.pti_augment_warp(p, None, None, 1, 1, 8, 8, q, None) == -1 and b"null" in h.pti_last_error_string()
    assert h.pti_augment_warp(p, p, None, 1, 0, 8, 8, q, None) == -1


def test_config_forms_load(tmp_path):
    from pti_ldm_vae_amd.utils.config import read_config
    for value, want in ((False, None), (True, AugmentPolicy()),
                        ({"elastic_p": 0.0, "shift_limit": 0.05}, AugmentPolicy(elastic_p=0.0, shift_limit=0.05))):
        f = tmp_path / "cfg.json"
        f.write_text(json.dumps({"augment": value, "autoencoder_train": {"batch_size": 4}}))
        assert AugmentPolicy.from_config(read_config(str(f))["augment"]) == want
    import glob
    import os
    shipped = glob.glob(os.path.join(os.path.dirname(os.path.dirname(__file__)), "config", "*.json"))
    assert shipped
    for path in shipped:        # the shipped configs carry the key (false) or leave it out
        assert AugmentPolicy.from_config(read_config(path).get("augment")) is None

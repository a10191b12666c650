"""CPU tests around the display normalisation: the fp64 oracle of ``pti_display_planes`` (tests/display_oracle.py) against
the host function it restates, the schedule of ``ValidationSampleWriter``, and the refusals of ``ops.display_planes`` and
of the C entry point that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import display_oracle as O

SEEDS = range(100, 112)
SHAPES = [(64, 64), (24, 40), (51, 1), (1, 51), (96, 80), (256, 256)]


@pytest.fixture(scope="module")
def planes():
    """The generator's planes: image, reconstruction and |difference| of every seed, with the oracle's and the host's map."""
    from pti_ldm_vae_amd.utils.visualization import normalize_batch_for_display
    out = []
    for seed in SEEDS:
        img, rec = O.case(seed, *SHAPES[seed % len(SHAPES)])
        for plane in (img, rec, np.abs(img - rec)):
            host = normalize_batch_for_display(torch.from_numpy(plane)[None, None])[0, 0].numpy()
            out.append((plane, O.normalize_plane(plane), host))
    return out


def test_oracle_matches_host_function(planes):
    """The host rounds three times in fp32 on values <= 1 (about 2e-7): 1e-6 holds it.  A pixel within 1e-6 of the 1e-3
    floor may fall on either side of it; at most 4 per plane may be left out for that."""
    worst, left_out = 0.0, 0
    for _, oracle, host in planes:
        assert oracle.dtype == np.float32 and host.dtype == np.float32
        err, near = O.compare(oracle, host)
        worst, left_out = max(worst, err), max(left_out, near)
    print(f"oracle vs host: worst |d| {worst:.3e}, most pixels left out of one plane {left_out}")
    assert worst <= 1e-6
    assert left_out <= O.MAX_LEFT_OUT


def test_uint8_oracle_within_one_level_of_host(planes):
    differ = total = 0
    for _, oracle, host in planes:
        d = np.abs(O.to_uint8(oracle).astype(np.int32) - (host * 255).astype(np.uint8).astype(np.int32))
        assert d.max() <= 1
        differ, total = differ + int((d != 0).sum()), total + d.size
    print(f"8-bit oracle vs host: {differ} of {total} pixels differ")
    assert differ <= 1e-3 * total


def test_oracle_percentile_is_numpys():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 51, 1000):
        v = np.sort(rng.normal(size=n).astype(np.float32))
        for q in (0, 2, 50, 98, 100):
            assert O.percentile(v, q) == pytest.approx(float(np.percentile(v.astype(np.float64), q)), rel=1e-14, abs=1e-300)


def test_oracle_canvas_layout():
    a, b = O.case(3, 6, 10)
    canvas, stats = O.display_planes(a[None], b[None], nsrc=3, rot90=3)
    assert canvas.shape == (1, 10, 18) and stats.shape == (1, 3, 3)
    assert np.array_equal(canvas[0, :, 6:12], np.rot90(O.normalize_plane(b), k=3))
    assert np.array_equal(canvas[0, :, 12:], np.rot90(O.normalize_plane(np.abs(a - b)), k=3))
    zero = np.zeros((1, 4, 4), np.float32)
    zero[0, 1, 1] = -0.0
    canvas, stats = O.display_planes(zero)
    assert not canvas.any() and not stats.any()


def test_writer_schedule():
    from pti_ldm_vae_amd.utils.validation_samples import ValidationSampleWriter
    w = ValidationSampleWriter("unused")
    assert [e for e in range(60) if w.wants_tifs(e)] == [10, 15, 20, 25, 30, 35, 40, 45, 50, 55]
    assert [e for e in range(60) if w.wants_triplet(e)] == [0, 20, 40]
    off = ValidationSampleWriter("unused", every=0, triplet_every=0)
    assert not any(off.wants_tifs(e) or off.wants_triplet(e) or off.begin(e) for e in range(60))
    early = ValidationSampleWriter("unused", start=0, every=1, triplet_every=1)
    assert all(early.wants_tifs(e) and early.wants_triplet(e) for e in range(5))
    only_tifs = ValidationSampleWriter("unused", start=3, every=2, triplet_every=0)
    assert [e for e in range(9) if only_tifs.begin(e)] == [4, 6, 8]


def test_train_vae_flags():
    from pti_ldm_vae_amd import inference_vae, train_vae
    a = train_vae.parse_args([])
    assert (a.val_samples_start, a.val_samples_every, a.val_triplet_every) == (10, 5, 20)
    a = train_vae.parse_args(["--val-samples-start", "0", "--val-samples-every", "1", "--val-triplet-every", "0"])
    assert (a.val_samples_start, a.val_samples_every, a.val_triplet_every) == (0, 1, 0)
    base = ["-c", "c", "--checkpoint", "k", "--input-dir", "i"]
    assert inference_vae.parse_args(base).display == "host"
    assert inference_vae.parse_args(base + ["--display", "hip"]).display == "hip"
    with pytest.raises(SystemExit):
        inference_vae.parse_args(base + ["--display", "numpy"])


def test_display_planes_refuses_before_touching_the_library(monkeypatch):
    from pti_ldm_vae_amd import ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(ops.L, "lib", no_library)
    a = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="low"):
        ops.display_planes(a, low=60, high=40)
    with pytest.raises(ValueError, match="needs b"):
        ops.display_planes(a, nsrc=2)
    with pytest.raises(ValueError, match="needs b"):
        ops.display_planes(a, nsrc=3)
    with pytest.raises(TypeError, match="float32"):
        ops.display_planes(a.double())
    with pytest.raises(TypeError, match="float32"):
        ops.display_planes(a, a.to(torch.bfloat16), nsrc=2)
    with pytest.raises(ValueError):
        ops.display_planes(a, rot90=4)
    with pytest.raises(ValueError):
        ops.display_planes(a, a[:, :4], nsrc=2)
    with pytest.raises(ValueError):            # host tensors: no CPU path
        ops.display_planes(a)


def test_entry_point_refuses_before_any_launch():
    """Argument checks of ``pti_display_planes`` return before a launch: callable without a GPU."""
    from pti_ldm_vae_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(4096)     # never dereferenced on these paths

    def call(a=p, b=p, n=1, hh=8, ww=8, nsrc=1, low=2.0, high=98.0, rot=0, f32=p, u8=None, stats=p):
        return h.pti_display_planes(a, b, n, hh, ww, nsrc, low, high, rot, f32, u8, stats, None)
    assert call(a=None) == -1 and b"null" in h.pti_last_error_string()
    assert call(stats=None) == -1
    assert call(f32=None, u8=None) == -1
    assert call(nsrc=0) == -1 and call(nsrc=4) == -1
    assert call(nsrc=2, b=None) == -1 and b"needs b" in h.pti_last_error_string()
    assert call(low=60.0, high=40.0) == -1 and call(low=-1.0) == -1 and call(high=101.0) == -1
    assert call(low=float("nan")) == -1
    assert call(rot=4) == -1 and call(rot=-1) == -1
    assert call(hh=0) == -1 and call(n=0) == -1
    assert call(stats=C.c_void_p(4100)) == -1 and b"misaligned" in h.pti_last_error_string()
    assert call(hh=4097) == -2 and call(ww=4097) == -2
    assert call(n=21846, nsrc=3) == -2 and call(n=65536) == -2

"""GPU tests of the display normalisation kernel (csrc/display.hip, ``ops.display_planes``) against the fp64 oracle of
tests/display_oracle.py, and of its two users: the validation pictures of ``train_vae`` and ``inference_vae --display hip``.

Bounds.  Counts are integers: exact.  The percentiles are two exact order statistics and one fp64 interpolation:
``1e-12 * max(1, |p|)`` is far below the 6e-8 spacing of fp32 data near 1 (a rank off by one fails) and far above fp64
rounding (a fused multiply-add in the interpolation passes).  The fp32 canvas is one fp64 map rounded once: 1e-6, with
the pixels whose wanted value lies within 1e-6 of the 1e-3 floor left out (they may fall on either side of it), at most 4
per plane.  Everything else -- the 8-bit canvas against the fp32 one, rotations, columns, repeated calls, a graph
replay -- is compared bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import display_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 8, 8), (2, 24, 40), (3, 51, 1), (1, 1, 51), (2, 64, 64), (1, 256, 256)]


def _batch(shape, seed):
    n, h, w = shape
    pairs = [O.case(seed + i, h, w) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _both(a, b, nsrc, rot90=0, low=2.0, high=98.0):
    """Both canvases and the stats of ONE ``pti_display_planes`` call."""
    import ctypes as C
    from pti_ldm_vae_amd import _lib as L
    n, h, w = a.shape
    ho, wo = (w, h) if rot90 & 1 else (h, w)
    f32 = torch.full((n, ho, nsrc * wo), -1.0, device=a.device)
    u8 = torch.full((n, ho, nsrc * wo), 77, dtype=torch.uint8, device=a.device)
    stats = torch.full((n, nsrc, 3), -1.0, dtype=torch.float64, device=a.device)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L.check(L.lib().pti_display_planes(ptr(a), ptr(b), n, h, w, nsrc, low, high, rot90, ptr(f32), ptr(u8), ptr(stats),
                                       torch.cuda.current_stream().cuda_stream), "pti_display_planes")
    return f32, u8, stats


def _check_against_oracle(a, b, nsrc, rot90, dev, low=2.0, high=98.0):
    want, want_stats = O.display_planes(a, b, nsrc=nsrc, low=low, high=high, rot90=rot90)
    ta = torch.from_numpy(a).to(dev)
    tb = None if b is None else torch.from_numpy(b).to(dev)
    f32, u8, stats = _both(ta, tb, nsrc, rot90, low, high)
    torch.cuda.synchronize()
    f32, u8, stats = f32.cpu().numpy(), u8.cpu().numpy(), stats.cpu().numpy()
    assert f32.shape == want.shape
    assert np.array_equal(stats[..., 0], want_stats[..., 0]), (stats[..., 0], want_stats[..., 0])
    tol = 1e-12 * np.maximum(1.0, np.abs(want_stats[..., 1:]))
    dp = np.abs(stats[..., 1:] - want_stats[..., 1:])
    print(f"percentiles: worst |d| {dp.max():.3e}")
    assert (dp <= tol).all(), (stats, want_stats)
    wo = want.shape[2] // nsrc
    worst = 0.0
    for i in range(want.shape[0]):
        for s in range(nsrc):
            err, near = O.compare(f32[i, :, s * wo:(s + 1) * wo], want[i, :, s * wo:(s + 1) * wo])
            worst = max(worst, err)
            assert near <= O.MAX_LEFT_OUT, (i, s, near)
    print(f"canvas: worst |d| {worst:.3e}")
    assert worst <= 1e-6
    assert np.array_equal(u8, O.to_uint8(f32))      # the 8-bit canvas is trunc(fp32 canvas * 255) of the same call
    return f32, u8, stats


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_oracle(dev, shape):
    a, b = _batch(shape, seed=200)
    _check_against_oracle(a, b, 3, 3, dev)
    _check_against_oracle(a, b, 2, 0, dev, low=0.0, high=100.0)


def _special_planes(h=24, w=40):
    rng = np.random.default_rng(5)
    zero = np.zeros((h, w), np.float32)
    one = zero.copy()
    one[h // 3, w // 2] = 3.25                                       # n = 1: p_low = p_high
    negative = np.full((h, w), -2.5, np.float32)                     # a constant negative plane
    ties = (np.round(rng.normal(size=(h, w)) * 8) / 8).astype(np.float32)     # quantised to 1/8: heavy ties (and zeros)
    signed_zero = rng.normal(size=(h, w)).astype(np.float32)
    signed_zero[2, 3] = -0.0
    signed_zero[5, :7] = -0.0
    n51 = zero.copy()                                                # n = 51: (n - 1) * 2 / 100 = 1 exactly, gamma = 0
    n51.reshape(-1)[rng.choice(h * w, 51, replace=False)] = rng.normal(size=51).astype(np.float32)
    return np.stack([zero, one, negative, ties, signed_zero, n51])


def test_special_planes(dev):
    a = _special_planes()
    f32, _, stats = _check_against_oracle(a, None, 1, 0, dev)
    assert stats[:, 0, 0].tolist() == [0, 1, 24 * 40, float((a[3] != 0).sum()), 24 * 40 - 8, 51]
    assert not stats[0].any() and not f32[0].any()                   # all zero: plane 0, stats {0, 0, 0}
    assert stats[1, 0, 1] == stats[1, 0, 2] == 3.25 and stats[2, 0, 1] == stats[2, 0, 2] == -2.5
    assert f32[4, 2, 3] == 0 and not f32[4, 5, :7].any()             # -0.0 is background
    s51 = np.sort(a[5][a[5] != 0])
    assert stats[5, 0, 1] == pytest.approx(float(s51[1]), abs=1e-12) and stats[5, 0, 2] == pytest.approx(float(s51[49]), abs=1e-12)
    # against a shifted copy: the third source of (x, x) is an all-zero plane
    b = np.roll(a, 1, axis=0)
    _check_against_oracle(a, b, 3, 1, dev)
    f32, _, stats = _check_against_oracle(a, a.copy(), 3, 2, dev)
    assert not stats[:, 2].any() and not f32[:, :, 80:].any()


def test_rotations_columns_and_repeatability(dev):
    from pti_ldm_vae_amd import ops
    a, b = (torch.from_numpy(t).to(dev) for t in _batch((2, 24, 40), seed=300))
    base, base_stats = ops.display_planes(a, b, nsrc=3, dtype=torch.float32)
    assert base.shape == (2, 24, 120) and base_stats.shape == (2, 3, 3) and base_stats.dtype == torch.float64
    parts = [base[:, :, s * 40:(s + 1) * 40] for s in range(3)]
    for k in range(4):
        for dtype in (torch.float32, torch.uint8):
            got, stats = ops.display_planes(a, b, nsrc=3, rot90=k, dtype=dtype)
            want = torch.cat([torch.rot90(p, k, dims=[1, 2]) for p in parts], dim=2)
            if dtype == torch.uint8:
                want = (want * 255.0).to(torch.uint8)
            assert got.dtype == dtype and got.shape == want.shape == ((2, 40, 72) if k & 1 else (2, 24, 120))
            assert torch.equal(got, want), (k, dtype)
            assert torch.equal(stats, base_stats)
            again, stats2 = ops.display_planes(a, b, nsrc=3, rot90=k, dtype=dtype)      # two calls: identical bytes
            assert torch.equal(got, again) and torch.equal(stats, stats2)
    # nsrc 1, 2, 3 place the sources in the right columns; the third source equals a separate call on |a - b|
    only_a, st_a = ops.display_planes(a, dtype=torch.float32)
    only_b, st_b = ops.display_planes(b, dtype=torch.float32)
    only_d, st_d = ops.display_planes(torch.abs(a - b), dtype=torch.float32)
    two, st_two = ops.display_planes(a, b, dtype=torch.float32)                         # nsrc defaults to 2 with b
    assert torch.equal(only_a, parts[0]) and torch.equal(only_b, parts[1]) and torch.equal(only_d, parts[2])
    assert torch.equal(two, base[:, :, :80])
    assert torch.equal(torch.cat([st_a, st_b, st_d], dim=1), base_stats) and torch.equal(st_two, base_stats[:, :2])
    # [n, 1, h, w] is accepted like [n, h, w]
    four, _ = ops.display_planes(a[:, None], b[:, None], nsrc=3, dtype=torch.float32)
    assert torch.equal(four, base)
    for bad in (lambda: ops.display_planes(a.cpu()), lambda: ops.display_planes(a[:, :, ::2]),
                lambda: ops.display_planes(a, dtype=torch.float16)):
        with pytest.raises((ValueError, TypeError)):
            bad()


def test_graph_capture_and_replay_equals_eager(dev):
    """One stream, one launch, a fresh capture, one replay."""
    from pti_ldm_vae_amd import ops
    a, b = (torch.from_numpy(t).to(dev) for t in _batch((2, 64, 64), seed=400))
    eager, eager_stats = ops.display_planes(a, b, nsrc=3, rot90=3)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.display_planes(a, b, nsrc=3, rot90=3)                                       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        canvas, stats = ops.display_planes(a, b, nsrc=3, rot90=3)
    canvas.zero_()
    stats.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(canvas, eager) and torch.equal(stats, eager_stats)


def _within_one_level(got, want):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{int((d != 0).sum())} of {d.size} pixels differ, worst {d.max()}")
    assert d.max() <= 1 and (d != 0).sum() <= 1e-3 * d.size


def _train_config(tmp_path, name):
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_no_adv.json")))
    cfg["run_dir"] = str(tmp_path / name)
    cfg["autoencoder_def"]["channels"] = [32, 64]
    cfg["autoencoder_def"]["attention_levels"] = [False, False]
    cfg["autoencoder_def"]["num_res_blocks"] = 1
    cfg["autoencoder_train"].update(batch_size=2, patch_size=[64, 64], max_epochs=2, perceptual_weight=0.0)
    cf = tmp_path / f"{name}.json"
    cf.write_text(json.dumps(cfg))
    return cfg, str(cf)


def test_train_vae_writes_validation_samples(dev, tmp_path):
    from PIL import Image
    from pti_ldm_vae_amd import train_vae
    from pti_ldm_vae_amd.data import read_tiff
    from pti_ldm_vae_amd.utils.visualization import normalize_batch_for_display
    cfg, cf = _train_config(tmp_path, "run")
    h, w = cfg["autoencoder_train"]["patch_size"]
    train_vae.main(["-c", cf, "--synthetic", "8", "--val-samples-start", "0", "--val-samples-every", "1",
                    "--val-triplet-every", "1"])
    run = tmp_path / "run"
    shards = train_vae.SyntheticShards(8, 1, (h, w), 2, 0, 1, 42, dev, cfg["train_split"])
    val = list(shards.batches(0, train=False))
    for epoch in (0, 1):
        folders = [run / "validation_samples" / f"epoch_{epoch}" / d for d in ("originale", "reconstruction", "diff")]
        for d in folders:
            assert sorted(p.name for p in d.iterdir()) == [f"step{s:03}.tif" for s in range(len(val))]
        for s in range(len(val)):
            orig, rec, diff = (read_tiff(str(d / f"step{s:03}.tif")) for d in folders)
            assert orig.dtype == rec.dtype == diff.dtype == np.float32 and orig.shape == rec.shape == diff.shape == (w, h)
            assert np.array_equal(diff, np.abs(orig - rec))
            assert np.array_equal(orig, torch.rot90(val[s][0, 0], k=3, dims=[0, 1]).cpu().numpy())
        png = np.asarray(Image.open(run / "triplets" / f"val_epoch{epoch:03}_step000.png"))
        assert png.dtype == np.uint8 and png.shape == (w, 3 * h)
        planes = [read_tiff(str(d / "step000.tif")) for d in folders]          # already rotated: the map commutes with it
        host = normalize_batch_for_display(torch.from_numpy(np.stack(planes))[None])[0].numpy()
        _within_one_level(png, (np.concatenate(list(host), axis=1) * 255).astype(np.uint8))
    assert sorted(p.name for p in (run / "triplets").iterdir()) == ["val_epoch000_step000.png", "val_epoch001_step000.png"]
    lines = [json.loads(l) for l in open(run / "metrics.jsonl")]
    assert sum("val/recon_loss" in l for l in lines) == 2
    # the defaults: TIFs from epoch 10 on, so a 2-epoch run writes none
    _, cf2 = _train_config(tmp_path, "run_defaults")
    train_vae.main(["-c", cf2, "--synthetic", "8"])
    assert not (tmp_path / "run_defaults" / "validation_samples").exists()
    assert (tmp_path / "run_defaults" / "trained_weights" / "autoencoder_last.pt").exists()


def test_inference_display_hip_matches_host(dev, tmp_path):
    from PIL import Image
    from oracle.autoencoderkl import CONFIG_A, build_oracle
    from pti_ldm_vae_amd import inference_vae
    from pti_ldm_vae_amd.data import read_tiff, write_tiff
    rng = np.random.default_rng(21)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for i in range(4):
        h, w = 96 + 8 * i, 120 - 4 * i
        a = rng.standard_normal((h, w)).astype(np.float32) * 300 + 900
        yy, xx = np.mgrid[0:h, 0:w]
        a[((xx - w / 2) / (0.4 * w)) ** 2 + ((yy - h / 2) / (0.32 * h)) ** 2 > 1.0] = 0.0
        write_tiff(str(imgs / f"img_{i:03d}.tif"), a)
    cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_recon_kl.json")))
    cfg["autoencoder_train"].update(patch_size=[64, 64], perceptual_weight=0.0)
    cf = tmp_path / "cfg.json"
    cf.write_text(json.dumps(cfg))
    ck = tmp_path / "autoencoder_epoch3.pth"
    torch.save(build_oracle(CONFIG_A, seed=42).state_dict(), ck)
    outs = {}
    for mode in ("host", "hip"):
        outs[mode] = tmp_path / f"out_{mode}"
        inference_vae.main(["-c", str(cf), "--checkpoint", str(ck), "--input-dir", str(imgs), "--output-dir", str(outs[mode]),
                            "--batch-size", "3", "--display", mode])
    for i in range(4):
        tifs = [read_tiff(str(outs[m] / "results_tif" / f"image{i:04d}.tif")) for m in ("host", "hip")]
        assert tifs[0].shape == (64, 128) and np.array_equal(tifs[0], tifs[1])
        pngs = [np.asarray(Image.open(outs[m] / "results_png" / f"image{i:04d}.png")) for m in ("host", "hip")]
        assert pngs[0].shape == pngs[1].shape == (64, 128)
        _within_one_level(pngs[1], pngs[0])

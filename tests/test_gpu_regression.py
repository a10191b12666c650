"""GPU tests of BASELINE config 5 (regression on frozen VAE latents): the encoder-only hot path at the
config's real resolution against the oracle, the head's gradients against plain torch, and the reference-shaped loop
(train_one_epoch / validate_one_epoch / head checkpoints / target normaliser) end to end on a TIFF directory."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encoder_only_mu_vs_oracle_at_256_and_head_gradients(dev):
    """no_grad encode_deterministic at 256x256, batch 2 (config A = the VAE config 5 points to): z_mu rel L2 <= 2e-2
    (measured ~2e-3 with fp16 forward operands); the MLP head on those latents: output and gradients equal
    to the same head fed the oracle's latents within that latent error, VAE parameters untouched."""
    from oracle.autoencoderkl import CONFIG_A, build_oracle, synthetic_images
    from pti_ldm_vae_amd.models import LatentRegressor, VAELatentRegressor, VAEModel
    torch.set_num_threads(16)
    oracle = build_oracle(CONFIG_A, 42)
    vae = VAEModel.from_config(CONFIG_A)
    vae.load_state_dict(oracle.state_dict())
    vae = vae.to(dev).eval()
    x = synthetic_images(2, 1, 256, seed=5)
    with torch.no_grad():
        mu_o, _ = oracle.encode(x)
    flat = VAELatentRegressor.infer_flat_dim_from_patch(vae, (256, 256), dev)
    assert flat == 4 * 32 * 32
    torch.manual_seed(3)
    head = LatentRegressor(flat, [256, 32], 6, dropout=0.0)
    head_ref = LatentRegressor(flat, [256, 32], 6, dropout=0.0)
    head_ref.load_state_dict(head.state_dict())
    model = VAELatentRegressor(vae, head.to(dev), latent_dim=flat)
    y = torch.randn(2, 6)
    out = model(x.to(dev))
    loss = torch.nn.functional.mse_loss(out, y.to(dev))
    loss.backward()
    with torch.no_grad():
        mu_h = vae.encode_deterministic(x.to(dev)).cpu()
    rel = ((mu_h - mu_o).norm() / mu_o.norm()).item()
    out_ref = head_ref(mu_o.flatten(1))
    torch.nn.functional.mse_loss(out_ref, y).backward()
    g = torch.cat([p.grad.detach().cpu().flatten() for p in head.parameters()])
    g_ref = torch.cat([p.grad.flatten() for p in head_ref.parameters()])
    grel = ((g - g_ref).norm() / g_ref.norm()).item()
    print(f"[config 5] encoder mu relL2 {rel:.2e}; head out max|diff| {(out.detach().cpu() - out_ref).abs().max():.2e}; "
          f"head grad relL2 {grel:.2e}")
    assert rel <= 2e-2
    assert grel <= 2e-2 and torch.allclose(out.detach().cpu(), out_ref.detach(), atol=2e-2)
    assert all(p.grad is None and not p.requires_grad for p in vae.parameters())


def test_regression_script_end_to_end_on_tiff_directory(dev, tmp_path):
    from pti_ldm_vae_amd import train_regression
    from pti_ldm_vae_amd.data import write_tiff
    rng = np.random.default_rng(9)
    d = tmp_path / "data" / "dente"
    d.mkdir(parents=True)
    table = {}
    for i in range(16):
        img = np.zeros((80, 72), np.float32)
        hh, ww = 20 + 3 * i, 10 + 2 * i                       # a bright block whose size the targets describe
        img[10:10 + hh // 2, 8:8 + ww] = 1.0 + rng.random((hh // 2, ww), dtype=np.float32)
        write_tiff(str(d / f"img_{i:03d}.tif"), img)
        table[f"img_{i:03d}.tif"] = {"height_0": float(hh), "width_0": float(ww), "other": 0.0}
    af = tmp_path / "attrs.json"
    af.write_text(json.dumps(table))
    vae_cfg = json.load(open(os.path.join(ROOT, "config", "vae_dente_no_adv.json")))
    vae_cfg["autoencoder_def"].update(channels=[32, 64], attention_levels=[False, False], num_res_blocks=1)
    vf = tmp_path / "vae.json"
    vf.write_text(json.dumps(vae_cfg))
    cfg = json.load(open(os.path.join(ROOT, "config", "reg_edente_from_dente.json")))
    cfg.update(run_dir=str(tmp_path / "run"), targets=["height_0", "width_0"])
    cfg["data"].update(data_base_dir=str(tmp_path / "data"), attributes_path=str(af), patch_size=[64, 64], num_workers=2)
    cfg["vae"].update(config_file=str(vf), checkpoint=str(tmp_path / "nope.pth"))
    cfg["regressor_def"].update(hidden_dims=[32], dropout=0.0)
    cfg["regression_train"].update(batch_size=4, lr=3e-3, max_epochs=6, target_norm="standard")
    cf = tmp_path / "reg.json"
    cf.write_text(json.dumps(cfg))
    with pytest.raises(FileNotFoundError):                     # the configured checkpoint does not exist: no silent fallback
        train_regression.main(["-c", str(cf)])
    train_regression.main(["-c", str(cf), "--random-init-vae"])
    wd = tmp_path / "run" / "trained_weights"
    assert {"head_last.pth", "head_best.pth", "target_norm_stats.json"} <= set(os.listdir(wd))
    stats = json.load(open(wd / "target_norm_stats.json"))
    assert stats["target_names"] == ["height_0", "width_0"] and len(stats["mean"]) == 2
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert len(lines) == 6 and all(np.isfinite(l["train/loss_mse"]) for l in lines)
    assert lines[-1]["train/loss_mse"] < lines[0]["train/loss_mse"]           # the head learns on frozen latents
    assert "val/mae_height_0" in lines[-1] and "val/best_loss_mse" in lines[-1]
    ck = torch.load(wd / "head_last.pth", weights_only=True)
    assert ck["epoch"] == 6 and ck["targets"] == ["height_0", "width_0"] and ck["latent_dim"] == 4 * 32 * 32


def test_inference_encode_graph_replay_equals_eager(dev):
    """``encode_deterministic`` under no_grad replays a HIP graph per input shape (engine._forward_graphed): same bits as
    the eager launches, across repeated calls, a second shape, and a weight update (the graphs are dropped and
    re-captured when the packed operands change)."""
    from pti_ldm_vae_amd.models import VAEModel
    cfg = dict(spatial_dims=2, in_channels=1, out_channels=1, latent_channels=4, channels=[32, 64], num_res_blocks=1,
               norm_num_groups=16, norm_eps=1e-6, attention_levels=[False, True], with_encoder_nonlocal_attn=True,
               with_decoder_nonlocal_attn=True)
    torch.manual_seed(0)
    m = VAEModel.from_config(cfg).to(dev).eval()
    eng = m.autoencoder.engine()
    xs = [torch.randn(3, 1, 64, 64, device=dev), torch.randn(3, 1, 64, 64, device=dev), torch.randn(2, 1, 32, 96, device=dev)]
    with torch.no_grad():
        eng.encode_graphs = False
        eager = [m.encode_deterministic(x).clone() for x in xs]
        eng.encode_graphs = True
        for _ in range(2):
            for x, e in zip(xs, eager):
                assert torch.equal(m.encode_deterministic(x), e)
        assert len(eng._enc_graphs) == 2
        # weights change -> re-pack -> the captured graphs are stale and must not be replayed
        for p in m.parameters():
            p.mul_(1.01)
        eng.encode_graphs = False
        eager2 = m.encode_deterministic(xs[0]).clone()
        eng.encode_graphs = True
        got = m.encode_deterministic(xs[0])
        assert torch.equal(got, eager2) and not torch.equal(got, eager[0])
        # the decoder side: reconstruct_deterministic = graph-replayed encode + graph-replayed decode
        eng.encode_graphs = False
        rec_e = m.reconstruct_deterministic(xs[2]).clone()
        eng.encode_graphs = True
        for _ in range(2):
            assert torch.equal(m.reconstruct_deterministic(xs[2]), rec_e)
        assert len(eng._dec_graphs) == 1
    # with autograd on a parameter-requiring-grad model the autograd path is taken (no graph)
    out = m.autoencoder.encode(xs[0])[0]
    assert out.requires_grad

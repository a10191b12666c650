#!/usr/bin/env python3
"""The disentanglement numbers the AR-VAE literature reports, for a trained AR-VAE and a directory of images with an
attribute file: Spearman's rank correlation, the Mutual Information Gap (MIG), modularity, the Separated Attribute
Predictability (SAP) score and interpretability.  ``evaluate_ar_vae`` asks whether the mapped channel ORDERS the images like
its attribute (pair counts, Kendall's tau-b); this command gives the figures to compare with published results.  The
reference has no counterpart.

The per-image code is the one of ``evaluate_ar_vae`` (``channel_means``: ``z_mu`` averaged over the map), or -- with
``--from-npz`` -- the ``channel_means.npz`` that command wrote, without loading a model; the attribute-to-channel mapping
always comes from the config.  On the device: ONE call each of ``ops.tied_ranks`` (average ranks of the ``L + na`` columns),
``ops.rank_moments`` (their sums and Gram matrix) and ``ops.joint_histogram`` (``--bins`` equal-width bins per column between
its minimum and maximum, numpy's ``histogram`` edges), all integer-exact; the tables come to the host in one packed copy and
``utils/disentanglement.py`` does the arithmetic.

``--mi-estimator ksg`` puts the Kraskov-Stoegbauer-Grassberger k-nearest-neighbour estimate (estimator 1, the one under
scikit-learn's ``mutual_info_regression``; ``--ksg-neighbors`` K, default 3) in the place of the histogram MI: MIG, modularity
and interpretability are then formed from it, with the histogram entropies as MIG's denominators.  One more device call,
``ops.ksg_counts``, on the columns scaled to unit deviation on the host (``utils.disentanglement.ksg_scale``); its integer
counts come back whole and ``ksg_mutual_information`` applies the digammas.  Unlike ``mutual_info_regression`` no noise is
added to break ties -- the result is deterministic -- and the scaling is done in fp64 and rounded to fp32 before upload.

Outputs in ``--output-dir`` (default ``<run_dir>/ar_eval``):

* ``disentanglement.json``: ``scores`` (``mig, modularity, sap, interpretability``), ``attributes`` (by name:
  ``latent_channel, spearman_rho, best_channel_spearman`` = argmax |rho| over the channels, ``mapped_channel_is_best, mig,
  sap``), the ``[na][L]`` matrices ``spearman_rho``, ``mutual_information`` (nats) and ``pearson_r``, ``entropy`` [na], ``bins``,
  ``n_images``, ``excluded`` (per score, the entries left out of its mean because they are undefined), ``args``, ``files``.  An
  undefined value is ``null``.  With ``--mi-estimator ksg`` also ``mi_estimator``, ``ksg_neighbors`` and
  ``mutual_information_binned`` (the histogram MI that ``mutual_information`` then no longer holds).
* ``disentanglement.png``: the |rho| and MI heat maps with the mapped cells outlined; the MI panel names its estimator.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from . import ops
from .evaluate_ar_vae import channel_means, check_table, load_model
from .trainer import ARSettings
from .utils import ar_metrics
from .utils import disentanglement as D
from .utils.cli_common import init_device_and_seed, resolve_run_dir
from .utils.vae_loader import load_vae_config

WHO = "evaluate_disentanglement"


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Spearman, MIG, modularity, SAP and interpretability of an AR-VAE (HIP rank and "
                                            "histogram kernels).")
    p.add_argument("-c", "--config-file", required=True, help="AR-VAE config JSON.")
    p.add_argument("--checkpoint", default=None, help="VAE checkpoint (bare state dict or training checkpoint).")
    p.add_argument("--input-dir", default=None, help="Directory containing the images.")
    p.add_argument("--attributes-path", default=None,
                   help="Attributes JSON (default: regularized_attributes.attribute_file of the config).")
    p.add_argument("--output-dir", default=None, help="Where to write the report (default: <run_dir>/ar_eval).")
    p.add_argument("--batch-size", type=int, default=8, help="Encoder batch size (default: 8).")
    p.add_argument("--num-samples", type=int, default=None, help="Use only the first N images.")
    p.add_argument("--num-workers", type=int, default=4, help="TIFF decoding threads (default: 4).")
    p.add_argument("--seed", type=int, default=42, help="Seed for determinism.")
    p.add_argument("--random-init-vae", action="store_true",
                   help="seeded random VAE weights instead of --checkpoint (throughput / smoke runs)")
    p.add_argument("--bins", type=int, default=20, help="Equal-width bins per column of the MI histograms (default: 20).")
    p.add_argument("--from-npz", default=None, metavar="PATH",
                   help="channel_means.npz of an evaluate_ar_vae run: use its z / attrs / names, load no model")
    p.add_argument("--mi-estimator", choices=("binned", "ksg"), default="binned",
                   help="MI under MIG / modularity / interpretability: the --bins histograms (default) or the KSG "
                        "k-nearest-neighbour estimate")
    p.add_argument("--ksg-neighbors", type=int, default=3, metavar="K",
                   help=f"Neighbour count of --mi-estimator ksg (default: 3; 1 .. {ops.KSG_MAX_K}).")
    args = p.parse_args(argv)
    if not 1 <= args.ksg_neighbors <= ops.KSG_MAX_K:
        p.error(f"--ksg-neighbors must lie in 1 .. {ops.KSG_MAX_K}")
    if args.from_npz is None and (args.checkpoint is None or args.input_dir is None):
        p.error("--checkpoint and --input-dir are required without --from-npz")
    if not 2 <= args.bins <= ops.DISENT_MAX_BINS:
        p.error(f"--bins must lie in 2 .. {ops.DISENT_MAX_BINS}")
    return args


def load_npz(path, names):
    """``z`` [N, L] fp32, ``attrs`` [na, N] fp32 and the file names of a ``channel_means.npz``; its attribute names must be
    the config's, in order."""
    with np.load(path) as f:
        missing = [k for k in ("z", "attrs", "names") if k not in f.files]
        if missing:
            raise SystemExit(f"{WHO}: {path} lacks {missing}: not a channel_means.npz of evaluate_ar_vae")
        z, attrs, got = f["z"].astype(np.float32), f["attrs"].astype(np.float32), [str(v) for v in f["names"]]
        files = [str(v) for v in f["files"]] if "files" in f.files else []
    if got != list(names):
        raise SystemExit(f"{WHO}: {path} holds attributes {got}, the config maps {list(names)}")
    if z.ndim != 2 or attrs.ndim != 2 or attrs.shape != (len(got), z.shape[0]):
        raise SystemExit(f"{WHO}: {path}: z {z.shape} and attrs {attrs.shape} do not fit {len(got)} attributes")
    return z, attrs, files


def device_tables(z: torch.Tensor, attrs: torch.Tensor, bins: int):
    """The device work of a run: ``z`` [N, L] and ``attrs`` [na, N] fp32 device tensors -> host ``(sums, gram, counts, z)``:
    int64 [M], int64 [M, M] (``M = L + na``, channels first), int64 [na, L, bins, bins] and the fp32 codes."""
    n, l = z.shape
    na = attrs.shape[0]
    m = l + na
    cols = torch.cat([z.t(), attrs])                                  # [M, N] column-major table, channels first
    lo, hi = torch.aminmax(cols, dim=1)
    ext = torch.stack([lo, hi]).cpu().numpy()                         # the extremes: one small copy for the edges
    edges = torch.from_numpy(D.edge_tables(ext[0], ext[1], bins)).to(z.device)
    sums, gram = ops.rank_moments(ops.tied_ranks(cols))
    _, _, counts = ops.joint_histogram(cols[:l].t(), cols[l:], edges[:l], edges[l:])
    packed = torch.cat([sums, gram.reshape(-1), counts.reshape(-1).to(torch.int64),
                        z.contiguous().view(torch.int32).reshape(-1).to(torch.int64)]).cpu()   # one copy to the host
    a, b, c = m, m + m * m, m + m * m + counts.numel()
    z_h = packed[c:].to(torch.int32).view(torch.float32).reshape(n, l).numpy()
    return packed[:a].numpy(), packed[a:b].reshape(m, m).numpy(), packed[b:c].reshape(counts.shape).numpy(), z_h


def device_ksg(cols: np.ndarray, l: int, k: int, device):
    """The device work of ``--mi-estimator ksg``: host columns ``cols`` [L + na, N] fp32 (channels first, already scaled) ->
    host ``(nx, ny)``: int32 [na, L, N] each, in one copy."""
    t = torch.from_numpy(np.ascontiguousarray(cols, dtype=np.float32)).to(device)
    _, nx, ny = ops.ksg_counts(t[:l].t(), t[l:], k)
    both = torch.stack([nx, ny]).cpu().numpy()
    return both[0], both[1]


def main(argv=None) -> None:
    args = parse_args(argv)
    config = load_vae_config(args.config_file)
    ra = getattr(config, "regularized_attributes", None) or {}
    latent_channels = int(config.autoencoder_def["latent_channels"])
    settings = ARSettings.from_config(ra, gamma=0.0, latent_channels=latent_channels)
    if latent_channels > ops.RANK_AGREEMENT_MAX_L or len(settings.names) > ops.RANK_AGREEMENT_MAX_NA:
        raise SystemExit(f"{WHO}: {len(settings.names)} attributes x {latent_channels} channels; the kernels take at most "
                         f"{ops.RANK_AGREEMENT_MAX_NA} x {ops.RANK_AGREEMENT_MAX_L}")
    device = init_device_and_seed(args.seed)
    resolved = vars(args).copy()
    ksg = args.mi_estimator == "ksg"
    if not ksg:                                    # the default report is the one this command has always written
        del resolved["mi_estimator"], resolved["ksg_neighbors"]
    if args.from_npz is not None:
        z_np, attrs_h, files = load_npz(args.from_npz, settings.names)
        if z_np.shape[1] != latent_channels:
            raise SystemExit(f"{WHO}: {args.from_npz} holds {z_np.shape[1]} channels, the config has {latent_channels}")
        check_table(torch.from_numpy(attrs_h.T.copy()), settings.names)
        z, attrs = torch.from_numpy(z_np).to(device), torch.from_numpy(attrs_h).to(device)
    else:
        from .data import create_regression_eval_dataloader
        attributes_path = args.attributes_path if args.attributes_path is not None else ra.get("attribute_file")
        if attributes_path is None:
            raise SystemExit(f"{WHO}: no --attributes-path and no regularized_attributes.attribute_file in the config")
        resolved["resolved_attributes_path"] = attributes_path
        model = load_model(config, args.checkpoint, device, args.random_init_vae)
        loader, paths = create_regression_eval_dataloader(
            input_dir=args.input_dir, attributes_path=attributes_path, targets=settings.names,
            patch_size=tuple(config.autoencoder_train["patch_size"]), batch_size=args.batch_size, num_workers=args.num_workers,
            num_samples=args.num_samples, data_source=getattr(config, "data_source", "edente"),
            normalize_attributes=ra.get("normalize_attributes"), device=device)
        table = loader.stacked_targets()                                   # host [N, na]
        check_table(table, settings.names)
        attrs_h = table.t().contiguous().numpy()
        attrs = table.t().contiguous().to(device)                          # [na, N]
        z = channel_means(model, loader, table.shape[0], latent_channels, device)
        files = [Path(p).name for p in paths]
    n = attrs_h.shape[1]
    if ksg and not args.ksg_neighbors + 1 <= n <= ops.KSG_MAX_N:
        raise SystemExit(f"{WHO}: {n} images; --mi-estimator ksg with {args.ksg_neighbors} neighbours takes "
                         f"{args.ksg_neighbors + 1} .. {ops.KSG_MAX_N}")
    sums, gram, counts, z_h = device_tables(z, attrs, args.bins)
    mi = None
    if ksg:
        nx, ny = device_ksg(D.ksg_scale(np.concatenate([z_h.T, attrs_h])), latent_channels, args.ksg_neighbors, device)
        mi = D.ksg_mutual_information(nx, ny, n, args.ksg_neighbors)
    report = D.disentanglement_report(settings.names, settings.channels, n, sums, gram, counts,
                                      ar_metrics.pearson_matrix(z_h, attrs_h), mi=mi)
    report.update(bins=args.bins, n_images=n, args=resolved, files=files)
    if ksg:
        report.update(mi_estimator="ksg", ksg_neighbors=args.ksg_neighbors)
    out_dir = Path(args.output_dir) if args.output_dir is not None else resolve_run_dir(vars(config), args.config_file) / "ar_eval"
    out_dir.mkdir(parents=True, exist_ok=True)
    with (out_dir / "disentanglement.json").open("w", encoding="utf-8") as handle:
        json.dump(report, handle, indent=2, allow_nan=False)
    title = {"mi_title": f"mutual information (nats), KSG k = {args.ksg_neighbors}"} if ksg else {}
    D.save_heatmaps(out_dir / "disentanglement.png", report["spearman_rho"], report["mutual_information"], settings.names,
                    settings.channels, **title)
    for name, entry in report["attributes"].items():
        rho = entry["spearman_rho"]
        print(f"   {name}: channel {entry['latent_channel']} rho {'n/a' if rho is None else format(rho, '+.4f')} "
              f"best channel {entry['best_channel_spearman']}")
    print("   " + "  ".join(f"{k} {'n/a' if v is None else format(v, '.4f')}" for k, v in report["scores"].items()))
    print("Evaluation complete")
    print(f"   Report written to {out_dir / 'disentanglement.json'}")


if __name__ == "__main__":
    main()

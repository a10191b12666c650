"""``ops.KERNEL_PROFILE``: the records the MFMA conv / weight-gradient / GroupNorm-backward launchers append (kernel name,
algorithmic flops and bytes, two events, shape tuple -- what ``bench.py --full`` turns into its per-kernel roofline table),
and that recording changes no result bit.  The flop / byte formulas are written out here, independent of ``ops``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B16 = torch.bfloat16


def _rand(dev, seed, *shape):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, device=dev, generator=g).bfloat16()


def _profiled(ops, launch):
    """-> (outputs with profiling off, outputs with profiling on, the records of the profiled run)."""
    assert ops.KERNEL_PROFILE is None
    try:
        plain = launch()
        torch.cuda.synchronize()
        ops.KERNEL_PROFILE = records = []
        prof = launch()
        torch.cuda.synchronize()
    finally:
        ops.KERNEL_PROFILE = None
    return plain, prof, records


def _same(plain, prof):
    assert len(plain) == len(prof)
    for a, b in zip(plain, prof):
        assert torch.equal(a, b), "profiling changed a result"


def _check_record(rec, flops, nbytes, shape):
    name, fl, nb, e0, e1, sh = rec
    assert isinstance(name, str) and name
    assert fl == flops and nb == nbytes and sh == shape
    assert e0.elapsed_time(e1) >= 0.0


def test_batched_wgrad_one_record_per_kernel_mode(dev, monkeypatch):
    """Four jobs, one per kernel mode of pti_conv_wgrad_mfma_batched: the profiled call issues the modes as separate calls
    in the library's own order (3, 2, 1, 0) and each record carries its job's work under its kernel's name."""
    from pti_ldm_vae_amd import ops
    monkeypatch.delenv("PTI_WGRAD_V6", raising=False)
    n, h, w = 2, 32, 32
    chans = [(32, 32), (32, 64), (64, 128), (64, 64)]          # modes 0, 1, 2, 3
    xs = [_rand(dev, 10 + i, n, h, w, cin) for i, (cin, _) in enumerate(chans)]
    dys = [_rand(dev, 20 + i, n, h, w, cout) for i, (_, cout) in enumerate(chans)]

    def launch():
        jobs = [(x, dy, torch.zeros(cout * cin * 9, device=dev), torch.zeros(cout, device=dev))
                for x, dy, (cin, cout) in zip(xs, dys, chans)]
        ops.conv_wgrad_mfma_batched(jobs, accumulate=True)
        return [t for job in jobs for t in job[2:]]

    plain, prof, records = _profiled(ops, launch)
    assert len(records) == 4
    for rec, job, kernel in zip(records, (3, 2, 1, 0), ("wgrad_mfma6_kernel",) * 2 + ("wgrad_mfma4_kernel",) * 2):
        cin, cout = chans[job]
        assert kernel in rec[0], rec[0]
        _check_record(rec, 2 * n * h * w * cout * cin * 9, 2 * (xs[job].numel() + dys[job].numel()),
                      ("conv wgrad (batched)", 0, 0, 0, 0, 3, "s1", 1))
    _same(plain, prof)


N, H, W, CH, GROUPS = 1, 16, 16, 32, 16      # the one layer of the single-launch cases: 3x3 stride 1, 32 -> 32


@pytest.fixture(scope="module")
def layer(dev):
    from pti_ldm_vae_amd import ops
    x, dy = _rand(dev, 1, N, H, W, CH), _rand(dev, 2, N, H, W, CH)
    wt = torch.randn(CH, CH, 3, 3, generator=torch.Generator().manual_seed(3)).to(dev) / (CH * 9) ** 0.5
    gamma = (1 + 0.2 * torch.randn(CH, generator=torch.Generator().manual_seed(4))).to(dev)
    beta = (0.1 * torch.randn(CH, generator=torch.Generator().manual_seed(5))).to(dev)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, stats=ops.gn_stats(x, GROUPS),
                wp=ops.pack_conv_weight(wt, 3, ops.PTI_CONV_S1), wpt=ops.pack_conv_weight(wt, 3, ops.PTI_CONV_S1, flip=True),
                bias=torch.linspace(-1, 1, CH, device=dev))


CONV_FLOPS = 2.0 * N * H * W * CH * CH * 3 * 3
ACT = N * H * W * CH                      # elements of one activation of the layer


def test_conv_mfma_record(dev, layer):
    from pti_ldm_vae_amd import ops

    def launch():
        y = torch.empty(N, H, W, CH, dtype=B16, device=dev)
        ops.conv_mfma(layer["x"], layer["wp"], layer["bias"], y, cout=CH, prologue=ops.PTI_PRO_GN_SILU,
                      in_stats=layer["stats"], gamma=layer["gamma"], beta=layer["beta"], groups=GROUPS)
        return [y]

    plain, prof, records = _profiled(ops, launch)
    assert len(records) == 1
    _check_record(records[0], CONV_FLOPS, 2.0 * (ACT + ACT), ("conv fwd", CH, CH, H, W, 3, "s1", N))   # x read, y written
    _same(plain, prof)


def test_conv_wgrad_mfma_record(dev, layer):
    from pti_ldm_vae_amd import ops

    def launch():
        dw, db = torch.zeros(CH, CH, 3, 3, device=dev), torch.zeros(CH, device=dev)
        ops.conv_wgrad_mfma(layer["x"], layer["dy"], dw, db, prologue=ops.PTI_PRO_GN_SILU, in_stats=layer["stats"],
                            gamma=layer["gamma"], beta=layer["beta"], groups=GROUPS)
        return [dw, db]

    plain, prof, records = _profiled(ops, launch)
    assert len(records) == 1
    _check_record(records[0], CONV_FLOPS, 2.0 * (ACT + ACT), ("conv wgrad", CH, CH, H, W, 3, "s1", N))   # x and dy read
    _same(plain, prof)


def _gnbwd(ops, dev, layer):
    g = torch.empty(N, H, W, CH, dtype=B16, device=dev)
    sums = torch.empty(N, CH, 2, device=dev)
    ops.conv_mfma_gnbwd(layer["dy"], layer["wpt"], layer["x"], layer["stats"], layer["gamma"], layer["beta"], g, sums,
                        cout=CH, groups=GROUPS)
    return [g, sums]


def test_conv_mfma_gnbwd_record(dev, layer):
    from pti_ldm_vae_amd import ops
    plain, prof, records = _profiled(ops, lambda: _gnbwd(ops, dev, layer))
    assert len(records) == 1
    # dy_in read; the GroupNorm input read and dy_out written
    _check_record(records[0], CONV_FLOPS, 2.0 * (ACT + 2 * ACT), ("conv dgrad+GN bwd", CH, CH, H, W, 3, "s1", N))
    _same(plain, prof)


def test_gn_bwd_apply_record(dev, layer):
    from pti_ldm_vae_amd import ops
    g, sums = _gnbwd(ops, dev, layer)

    def launch():
        dx = torch.empty(N, H, W, CH, dtype=B16, device=dev)
        dg, db = torch.zeros(CH, device=dev), torch.zeros(CH, device=dev)
        ops.gn_bwd_apply(layer["x"], g, dx, layer["stats"], layer["gamma"], layer["beta"], sums, dg, db, groups=GROUPS)
        return [dx, dg, db]

    plain, prof, records = _profiled(ops, launch)
    assert len(records) == 1
    # 8 flops per element; x and dy read, dx written (no residual gradient)
    _check_record(records[0], 8.0 * ACT, 2.0 * ACT * 3, ("GroupNorm bwd apply", CH, CH, H, W, 0, "-", N))
    _same(plain, prof)

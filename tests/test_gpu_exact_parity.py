"""Exact parity of the conv, weight-gradient, pooling and statistics kernels against float64 references on INTEGER data
(tests/exact_util.py: small integers are exact in bf16 / fp16, every product is exact, every fp32 sum stays below 2^24 and
every 16-bit store within |v| <= 256, so nothing rounds and kernel == reference, element for element).  A mismatch is an
indexing, masking or staging bug; ``assert_exact`` names its tile position and channel block.  The conditions are asserted
when a case is built, and tests/test_exact_util_cpu.py builds every case of this file on the CPU.

Covered: ``ops.conv_mfma`` forward and data gradient (v2 kernel, stride-2 kernel, kernel name asserted, fused
statistics, residual, pooled store, fp16 storage and operands), ``ops.conv_direct`` without prologue, ``ops.pool2x2_sum``, ``ops.gn_stats``, ``ops.conv_wgrad_mfma`` on every default route (route asserted, second
launch with accumulate=True), ``ops.conv_wgrad_mfma_batched``, ``ops.wgrad_direct``.  Outputs are pre-filled with NaN.

The kernels that consume GroupNorm statistics -- the GroupNorm prologue launches of the convs and weight gradients,
``gn_bwd`` / ``gn_bwd_apply``, the fused GroupNorm-backward epilogue of the data-gradient conv and the chained launch -- are
compared exactly in tests/test_gpu_exact_groupnorm.py (a hand-written statistics table makes mean an integer and rstd a
power of two).  What genuinely remains under tolerance only: SiLU at a non-zero argument (exp, division), the attention
softmax, the losses and Adam (tests/test_gpu_ops.py, test_gpu_ops2.py, test_gpu_fused_gnbwd.py, test_gpu_gnbwd_chain.py,
test_gpu_attention.py, ... stay as they are).  The only knob touched is one that existing tests toggle per launch:
PTI_WGRAD_V6.
"""
import pytest
import torch

import exact_util as E

pytestmark = pytest.mark.gpu

NAN = float("nan")
B16, H16, F32 = torch.bfloat16, torch.float16, torch.float32
_CASES = {}


def _cached(key, build):
    """References are built once per case and never written again."""
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _nhwc(t, dev, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


def _mode(ops, mode):
    return {"s1": ops.PTI_CONV_S1, "s2": ops.PTI_CONV_S2PAD, "up": ops.PTI_CONV_UP2, "zins": ops.PTI_CONV_ZINS}[mode]


# ---- forward and data-gradient convs -----------------------------------------------------------------------------------
def _conv(ops, dev, row, c, wp, xd, sdt, *, bias, residual, stats, pool=False):
    m = _mode(ops, row["mode"])
    ho, wo = ops.conv_out_hw(row["h"], row["w"], m)
    shape = (row["n"], ho // 2, wo // 2, row["cout"]) if pool else (row["n"], ho, wo, row["cout"])
    y = torch.full(shape, NAN, dtype=sdt, device=dev)
    ost = torch.zeros(row["n"], E.STATS_GROUPS, 2, dtype=torch.int64, device=dev) if stats else None
    ops.conv_mfma(xd, wp, c.bias.to(dev, F32) if bias else None, y, cout=row["cout"], ksize=row["ks"], mode=m,
                  residual=_nhwc(c.res, dev, sdt) if residual else None, out_stats=ost, out_groups=E.STATS_GROUPS if stats else 0,
                  pool2=pool)
    torch.cuda.synchronize()
    return y, ost, ops.last_kernel_name()


def _variants(row):
    """(bias, residual, fused statistics) of each launch of a case: always the bare conv; then bias plus what the mode's
    launches carry in the product (and in the tolerance tests): statistics on the 3x3 forward modes, the residual where the
    case table asks for it.  The ``nostats`` rows also run with bias and residual alone."""
    if row["pooled"]:
        return [(False, False, False)]
    stats = row["ks"] == 3 and row["mode"] in ("s1", "s2", "up")
    out = [(False, False, False), (True, row["residual"], stats)]
    if row["nostats"]:
        out.append((True, row["residual"], False))
    return out


@pytest.mark.parametrize("row", E.FWD_CASES, ids=[r["id"] for r in E.FWD_CASES])
def test_conv_mfma_exact(dev, row):
    from pti_ldm_vae_amd import ops
    c = _cached(("fwd", row["id"]), lambda: E.make_fwd_case(row))
    sdt = H16 if row["f16"] else B16
    m = _mode(ops, row["mode"])
    wp = ops.pack_conv_weight(c.w.to(dev, F32), row["ks"], m, flip=row["mode"] == "zins", f16=row["f16"])
    xd = _nhwc(c.x, dev, sdt)
    want = "conv_mfma_kernel<" if row["mode"] == "s2" else "conv_mfma2_kernel<"
    for bias, residual, stats in _variants(row):
        tag = f"conv_mfma[{row['id']}] bias={bias} res={residual} stats={stats}"
        y, ost, name = _conv(ops, dev, row, c, wp, xd, sdt, bias=bias, residual=residual, stats=stats, pool=row["pooled"])
        assert name.startswith(want), f"{tag}: went down {name}"
        ref = c.pool if row["pooled"] else c.ref_full if residual else c.ref_bias if bias else c.conv
        E.assert_exact(tag, y, ref, layout="nhwc", tile=(4, 8) if row["pooled"] else E.TILE)
        if stats:      # Q47.16 sums of integers: the int64 sums of the reference, shifted
            E.assert_exact(tag + " fused statistics", ost, (c.stats_full if residual else c.stats_bias) * E.STAT_SCALE,
                           layout="flat")


# ---- the degenerate-channel conv ---------------------------------------------------------------------------------------
_DIRECT = E.direct_rows()


@pytest.mark.parametrize("rid,n,cin,cout,h,w,il,ol", _DIRECT, ids=[r[0] for r in _DIRECT])
def test_conv_direct_exact(dev, rid, n, cin, cout, h, w, il, ol):
    from pti_ldm_vae_amd import ops
    c = _cached(("direct", cin, cout, h, w), lambda: E.make_direct_case(n, cin, cout, h, w, ol.endswith("bf16")))
    w_tck = c.w.permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous().to(dev, F32)
    if il == "nchw_f32":
        xd, xl = c.x.to(dev, F32), "nchw"
    elif il == "nhwc_f32":
        xd, xl = _nhwc(c.x, dev, F32), "nhwc"
    else:
        xd, xl = _nhwc(c.x, dev, B16), "nhwc"
    if ol == "nhwc_bf16":
        y, yl = torch.full((n, h, w, cout), NAN, dtype=B16, device=dev), "nhwc"
    elif ol == "nchw_f32":
        y, yl = torch.full((n, cout, h, w), NAN, device=dev), "nchw"
    else:
        y, yl = torch.full((n, h, w, cout), NAN, device=dev), "nhwc"
    ops.conv_direct(xd, w_tck, c.bias.to(dev, F32), y, n=n, h=h, w=w, cin=cin, cout=cout, x_layout=xl, y_layout=yl, prologue=0)
    torch.cuda.synchronize()
    E.assert_exact(f"conv_direct[{rid}]", y, c.ref, layout=yl)


# ---- pooling and statistics --------------------------------------------------------------------------------------------
def test_pool2x2_sum_exact(dev):
    from pti_ldm_vae_amd import ops
    c = _cached("pool", E.make_pool_case)
    n, ch, h, w = E.POOL_CASE
    y = torch.full((n, h // 2, w // 2, ch), NAN, dtype=B16, device=dev)
    ops.pool2x2_sum(_nhwc(c.x, dev, B16), y)
    torch.cuda.synchronize()
    E.assert_exact("pool2x2_sum", y, c.ref, layout="nhwc", tile=(4, 8))


@pytest.mark.parametrize("sdt", [B16, H16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", range(len(E.STATS_CASES)), ids=["x".join(map(str, s)) for s in E.STATS_CASES])
def test_gn_stats_exact(dev, k, sdt):
    from pti_ldm_vae_amd import ops
    c = _cached(("stats", k), lambda: E.make_stats_case(*E.STATS_CASES[k], seed=k))
    st = ops.gn_stats(_nhwc(c.x, dev, sdt), E.STATS_GROUPS)
    torch.cuda.synchronize()
    E.assert_exact(f"gn_stats[{E.STATS_CASES[k]}]", st, c.ref * E.STAT_SCALE, layout="flat")


# ---- weight gradients --------------------------------------------------------------------------------------------------
def _wgrad(ops, dev, tag, c, x_dtype, route, v6, monkeypatch):
    """First launch into NaN-filled dW / dbias through a NaN-filled workspace (its written extent gives the splits taken)
    with the route recorded; second launch with accumulate=True: exactly twice the reference."""
    m = _mode(ops, c.mode)
    if v6 is None:
        monkeypatch.delenv("PTI_WGRAD_V6", raising=False)
    else:
        monkeypatch.setenv("PTI_WGRAD_V6", v6)
    xd, dyd = _nhwc(c.x, dev, x_dtype), _nhwc(c.dy, dev, B16)
    slab = c.ks * c.ks * c.cout * c.cin + c.cout
    assert slab * 4 == ops.L.lib().pti_conv_wgrad_workspace_bytes(c.cout, c.cin, c.ks, 1)
    ho, wo = c.dy.shape[2:]
    most = c.n * ((ho + 3) // 4) * ((wo + 15) // 16)            # no route takes more splits than 4 x 16 pixel tiles
    ws = torch.full((most * slab,), NAN, device=dev)
    dw = torch.full((c.cout, c.cin, c.ks, c.ks), NAN, device=dev)
    db = torch.full((c.cout,), NAN, device=dev)
    prof = []
    ops.KERNEL_PROFILE = prof          # the two-call form (partials, then reduce) records the partial kernel's name
    try:
        ops.conv_wgrad_mfma(xd, dyd, dw, db, ksize=c.ks, mode=m, workspace=ws)
        torch.cuda.synchronize()
    finally:
        ops.KERNEL_PROFILE = None
    got_route = prof[0][0].replace(" ", "")
    wrote = int(torch.nonzero(~torch.isnan(ws))[-1]) + 1
    tiles = c.n * ((ho + 7) // 8) * ((wo + 15) // 16)
    print(f"[exact wgrad] {tag}: route {got_route}; {tiles} pixel tiles of 8 x 16, {wrote / slab:g} splits")
    assert route in got_route, f"{tag} went down {got_route}"
    assert wrote % slab == 0 and wrote // slab <= most
    E.assert_exact(f"{tag} dW", dw, c.dw, layout="dw")
    E.assert_exact(f"{tag} dbias", db, c.db, layout="flat")
    ops.conv_wgrad_mfma(xd, dyd, dw, db, ksize=c.ks, mode=m, accumulate=True)
    torch.cuda.synchronize()
    E.assert_exact(f"{tag} dW after accumulate=True", dw, 2 * c.dw, layout="dw")
    E.assert_exact(f"{tag} dbias after accumulate=True", db, 2 * c.db, layout="flat")
    monkeypatch.delenv("PTI_WGRAD_V6", raising=False)
    return wrote // slab


@pytest.mark.parametrize("name", list(E.WGRAD_CASES))
def test_conv_wgrad_mfma_exact(dev, monkeypatch, name):
    from pti_ldm_vae_amd import ops
    c = _cached(("wgrad", name), lambda: E.make_wgrad_case(name))
    route, v6 = E.WGRAD_CASES[name][7:]
    _wgrad(ops, dev, name, c, B16, route, v6, monkeypatch)


@pytest.mark.parametrize("name", list(E.WGRAD_F16_X))
def test_conv_wgrad_mfma_fp16_x_exact(dev, monkeypatch, name):
    from pti_ldm_vae_amd import ops
    c = _cached(("wgrad", name), lambda: E.make_wgrad_case(name))
    _wgrad(ops, dev, name + " fp16 x", c, H16, E.WGRAD_F16_X[name], None, monkeypatch)


def test_conv_wgrad_mfma_batched_exact(dev, monkeypatch):
    """One call with a job for every kernel mode (pairs, two-block, v6 shapes A and B); then the same call again with
    accumulate=True."""
    from pti_ldm_vae_amd import ops
    monkeypatch.delenv("PTI_WGRAD_V6", raising=False)
    cases = [_cached(("batched", i), lambda i=i: E.make_batched_case(i)) for i in range(len(E.BATCHED_JOBS))]
    modes = [ops.L.lib().pti_conv_wgrad_batched_mode(c.n, c.h, c.w_, c.cin, c.cout) for c in cases]
    print(f"[exact wgrad] batched: kernel modes {modes}")
    assert sorted(set(modes)) == [0, 1, 2, 3], modes
    jobs = [(_nhwc(c.x, dev, B16), _nhwc(c.dy, dev, B16), torch.full((c.cout * c.cin * 9,), NAN, device=dev),
             torch.full((c.cout,), NAN, device=dev)) for c in cases]
    for times, acc in ((1, False), (2, True)):
        ops.conv_wgrad_mfma_batched(jobs, accumulate=acc)
        torch.cuda.synchronize()
        for c, (_, _, dw, db) in zip(cases, jobs):
            tag = f"batched[{c.cin}->{c.cout}@{c.h}] x{times}"
            E.assert_exact(tag + " dW", dw.view(c.cout, c.cin, 3, 3), times * c.dw, layout="dw")
            E.assert_exact(tag + " dbias", db, times * c.db, layout="flat")


@pytest.mark.parametrize("kind,n,cw,cn,h,w", E.WGRAD_DIRECT_CASES)
def test_wgrad_direct_exact(dev, kind, n, cw, cn, h, w):
    from pti_ldm_vae_amd import ops
    c = _cached(("wgrad_direct", kind, cw, cn), lambda: E.make_wgrad_direct_case(kind, n, cw, cn, h, w))
    dims = dict(n=n, h=h, w=w, cw=cw, cn=cn, ksize=3, narrow_layout="nchw")
    if kind == "fewcout":       # y[cn] = conv(x[cw]): wide = x (bf16 NHWC), narrow = dY (fp32 NCHW)
        wide, narrow = _nhwc(c.x, dev, B16), c.dy.to(dev, F32)
        dw, db = torch.zeros(cn, cw, 3, 3, device=dev), torch.zeros(cn, device=dev)          # the call adds to them
        ops.wgrad_direct(wide, narrow, dw, sgn=1, dw_strides=(1, 9, cw * 9), dbias_narrow=db, prologue=0, **dims)
    else:                       # y[cw] = conv(x[cn]): wide = dY (bf16 NHWC), narrow = x (fp32 NCHW)
        wide, narrow = _nhwc(c.dy, dev, B16), c.x.to(dev, F32)
        dw, db = torch.zeros(cw, cn, 3, 3, device=dev), torch.zeros(cw, device=dev)
        ops.wgrad_direct(wide, narrow, dw, sgn=-1, dw_strides=(1, cn * 9, 9), dbias_wide=db, **dims)
    torch.cuda.synchronize()
    E.assert_exact(f"wgrad_direct[{kind},{cw}x{cn}] dW", dw, c.dw, layout="dw")
    E.assert_exact(f"wgrad_direct[{kind},{cw}x{cn}] dbias", db, c.db, layout="flat")

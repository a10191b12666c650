"""Exact parity of every kernel that CONSUMES GroupNorm statistics -- the GroupNorm prologue of the convs and weight
gradients, ``gn_bwd`` / ``gn_bwd_apply``, the fused GroupNorm-backward epilogue of the data-gradient conv and the chained
launch -- against float64 references (tests/exact_gn_util.py).  The Q47.16 statistics table is written by hand so that
mean is an integer and rstd a power of two; with integer data and power-of-two gamma every fp32 intermediate is exact in any
order, and the one rounding left is the 16-bit store (round to nearest even, which torch reproduces).  Kernel == reference,
element for element; there is no tolerance in this file.  Outputs are pre-filled with NaN and ``assert_exact`` names the
tile position and channel block of a mismatch.  Every case and its conditions are also built on the CPU by
tests/test_exact_gn_util_cpu.py.

The probe (``test_probe_*``).  All of this rests on the reciprocal square root being EXACT on powers of four, which each
kernel family computes in its own way (``rsqrtf`` in groupnorm.hip, the stride-2 conv kernel, the chained loader and the
weight gradients; ``__builtin_amdgcn_rsqf`` in ``gn_params``: the v2 conv kernel and the fused
epilogue; conv_direct.hip its own).  One tiny launch per family with x = 1, mean = 0, gamma = 1, beta = 0 and an identity
tap returns rstd itself, for var + eps in {1/4, 1, 4, 16}.  Measured on an MI355X (gfx950):

    family (kernel)                                              var+eps = 1/4    1     4     16
    gn_bwd (gn_bwd_reduce + gn_bwd_apply, rsqrtf)                            2      1    1/2   1/4
    gn_bwd_apply (rsqrtf)                                                    2      1    1/2   1/4
    conv_mfma_v2 (conv_mfma2_kernel, gn_params: v_rsq_f32)                   2      1    1/2   1/4
    conv_mfma_s2 (conv_mfma_kernel, stride 2, rsqrtf)                        2      1    1/2   1/4
    conv_direct prologue                                                     2      1    1/2   1/4
    wgrad_direct prologue                                                    2      1    1/2   1/4
    conv_wgrad_mfma prologue, 3x3 (wgrad_mfma3_kernel)                       2      1    1/2   1/4
    conv_wgrad_mfma prologue, 1x1 (wgrad_mfma_kernel)                        2      1    1/2   1/4
    conv_mfma_gnbwd epilogue (gn_params)                                     2      1    1/2   1/4
    chained launch (PRO_GNB loader, rsqrtf)                                  2      1    1/2   1/4

every value exact in every family, so no family is left to its tolerance tests for want of an exact rstd.

``exact_gn_util.EXACT_RSTD`` holds that table, the probe asserts it on every run, and the cases of a family draw only from
its entry (some cases narrow it further so that their sums stay within 24 bits; exact_gn_util says where and why).
``dsilu(0)`` is probed the same way (gamma = beta = 0, dy = 1): exactly 1/2 in ``gn_bwd`` (S1 / HW) and in the fused
epilogue (dy_out and S1 / HW), which the SiLU plumbing cases need.

What stays under tolerance tests only: SiLU at non-zero arguments (and the packed SiLU path of the 128-wide tiles).
"""
import pytest
import torch

import exact_gn_util as X
import exact_util as E

pytestmark = pytest.mark.gpu

NAN = float("nan")
B16, H16, F32 = torch.bfloat16, torch.float16, torch.float32
PROBE_VE = (0.25, 1.0, 4.0, 16.0)            # var + eps; the exact rstd would be 2, 1, 1/2, 1/4
_CASES = {}


def _cached(key, build):
    """References are built once per case and never written again."""
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _nhwc(t, dev, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


def _mode(ops, mode):
    return {"s1": ops.PTI_CONV_S1, "s2": ops.PTI_CONV_S2PAD, "up": ops.PTI_CONV_UP2}[mode]


def _nan(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _f32(t, dev):
    return t.to(dev, F32).contiguous()


# ---- the probe -------------------------------------------------------------------------------------------------------
def _identity(cout, cin, ks, dev):
    w = torch.zeros(cout, cin, ks, ks, device=dev)
    for i in range(min(cout, cin)):
        w[i, i, ks // 2, ks // 2] = 1.0
    return w


def _single(name, t):
    """The one value a probe output must hold everywhere."""
    v = t.detach().double().flatten()
    assert bool((v == v[0]).all()), f"{name}: the probe output is not constant: {v.unique().tolist()[:8]}"
    return v[0].item()


def _probe_conv(ops, dev, eps, *, c, mode, ks=3, f16=False):
    n, h, w = 1, 8, 16
    sdt = H16 if f16 else B16
    m = _mode(ops, mode)
    x = torch.ones(n, h, w, c, dtype=sdt, device=dev)
    wp = ops.pack_conv_weight(_identity(c, c, ks, dev), ks, m, f16=f16)
    ho, wo = ops.conv_out_hw(h, w, m)
    y = _nan((n, ho, wo, c), sdt, dev)
    ops.conv_mfma(x, wp, None, y, cout=c, ksize=ks, mode=m, prologue=ops.PTI_PRO_GN,
                  in_stats=torch.zeros(n, 16, 2, dtype=torch.int64, device=dev), gamma=torch.ones(c, device=dev),
                  beta=torch.zeros(c, device=dev), groups=16, eps=eps)
    torch.cuda.synchronize()
    return _single("conv_mfma", y), ops.last_kernel_name()


def _probe_family(ops, dev, family, eps):
    """-> the rstd the family computes for var + eps = ``eps`` (an all-zero table: mean 0, var 0)."""
    z = lambda n, g=16: torch.zeros(n, g, 2, dtype=torch.int64, device=dev)
    ones = lambda c: torch.ones(c, device=dev)
    zeros = lambda c: torch.zeros(c, device=dev)
    if family in ("gn_bwd", "gn_bwd_apply"):
        n, h, w, c = 1, 8, 8, 32
        x = torch.ones(n, h, w, c, dtype=B16, device=dev)
        dy = torch.ones(n, h * w, c, device=dev)
        dy[:, 1::2] = -1.0                                  # sums cancel: c1 = c2 = 0 and dx = rstd * dy
        dy = dy.view(n, h, w, c).to(B16)
        dx, sums = _nan(x.shape, B16, dev), torch.zeros(n, c, 2, device=dev)
        if family == "gn_bwd":
            ops.gn_bwd(x, dy, dx, z(n), ones(c), zeros(c), sums, zeros(c), zeros(c), groups=16, eps=eps, silu=False)
        else:
            ops.gn_bwd_apply(x, dy, dx, z(n), ones(c), zeros(c), sums, zeros(c), zeros(c), groups=16, eps=eps)
        torch.cuda.synchronize()
        return _single(family, dx.float() * dy.float())
    if family == "conv_mfma_v2":
        v, name = _probe_conv(ops, dev, eps, c=32, mode="s1")
        assert name.startswith("conv_mfma2_kernel<"), name
        return v
    if family == "conv_mfma_s2":
        v, name = _probe_conv(ops, dev, eps, c=32, mode="s2")
        assert name.startswith("conv_mfma_kernel<"), name
        return v
    if family == "conv_direct":
        n, h, w, cin, cout = 1, 8, 8, 32, 1
        w_tck = torch.zeros(9, cin, cout, device=dev)
        w_tck[4, 0, 0] = 1.0
        y = _nan((n, cout, h, w), F32, dev)
        ops.conv_direct(torch.ones(n, h, w, cin, dtype=B16, device=dev), w_tck, zeros(cout), y, n=n, h=h, w=w, cin=cin,
                        cout=cout, x_layout="nhwc", y_layout="nchw", prologue=ops.PTI_PRO_GN, in_stats=z(n), gamma=ones(cin),
                        beta=zeros(cin), groups=16, eps=eps)
        torch.cuda.synchronize()
        return _single(family, y)
    if family == "wgrad_direct":
        n, h, w, cw, cn = 2, 8, 8, 32, 1
        wide = torch.ones(n, h, w, cw, dtype=B16, device=dev)
        dw = torch.zeros(cn, cw, 3, 3, device=dev)
        ops.wgrad_direct(wide, torch.ones(n, cn, h, w, device=dev), dw, n=n, h=h, w=w, cw=cw, cn=cn, ksize=3, sgn=1,
                         narrow_layout="nchw", dw_strides=(1, 9, cw * 9), dbias_narrow=zeros(cn), prologue=ops.PTI_PRO_GN,
                         in_stats=z(n), gamma=ones(cw), beta=zeros(cw), groups=16, eps=eps)
        torch.cuda.synchronize()
        return _single(family, dw[:, :, 1, 1]) / (n * h * w)          # the centre tap sees every pixel: rstd * 128
    if family in ("conv_wgrad_mfma", "conv_wgrad_mfma_1x1"):
        n, h, w, c, ks = 2, 8, 8, 32, 3 if family == "conv_wgrad_mfma" else 1
        dw, db = _nan((c, c, ks, ks), F32, dev), _nan((c,), F32, dev)
        ops.conv_wgrad_mfma(torch.ones(n, h, w, c, dtype=B16, device=dev), torch.ones(n, h, w, c, dtype=B16, device=dev), dw, db,
                            ksize=ks, prologue=ops.PTI_PRO_GN, in_stats=z(n), gamma=ones(c), beta=zeros(c), groups=16, eps=eps)
        torch.cuda.synchronize()
        return _single(family, dw[:, :, ks // 2, ks // 2]) / (n * h * w)
    if family == "conv_mfma_gnbwd":
        n, h, w, c = 1, 8, 16, 32
        dy_out, gsums = _nan((n, h, w, c), B16, dev), _nan((n, c, 2), F32, dev)
        ops.conv_mfma_gnbwd(torch.ones(n, h, w, c, dtype=B16, device=dev),
                            ops.pack_conv_weight(_identity(c, c, 3, dev), 3, ops.PTI_CONV_S1, flip=True),
                            torch.ones(n, h, w, c, dtype=B16, device=dev), z(n), ones(c), zeros(c), dy_out, gsums, cout=c, groups=16,
                            eps=eps, silu=False)
        torch.cuda.synchronize()
        assert _single(family + " dy_out", dy_out) == 1.0 and _single(family + " S1", gsums[..., 0]) == h * w
        return _single(family, gsums[..., 1]) / (h * w)                # S2 = sum dy * xhat = rstd * 128
    if family == "chain":
        n, h, w, c = 1, 8, 16, 128
        one = lambda dt: torch.ones(n, h, w, c, dtype=dt, device=dev)
        dx_in, dy_out, gsums = _nan((n, h, w, c), B16, dev), _nan((n, h, w, c), B16, dev), _nan((n, c, 2), F32, dev)
        assert ops.gnbwd_chain_supported(c, c, 3, H16)
        ops.conv_mfma_gnbwd_chain(one(B16), one(H16), z(n), ones(c), torch.zeros(n, c, 2, device=dev), dx_in,
                                  ops.pack_conv_weight(_identity(c, c, 3, dev), 3, ops.PTI_CONV_S1, flip=True), one(H16), z(n),
                                  ones(c), zeros(c), dy_out, gsums, cout=c, groups=16, eps=eps, silu=False)
        torch.cuda.synchronize()
        v = _single(family, dx_in)                                      # in_sums = 0: dx_in = rstd * gamma * g = rstd
        assert _single(family + " dy_out", dy_out) == v                # the identity conv of it
        return v
    raise ValueError(family)


PROBE_FAMILIES = {"gn_bwd": "gn_bwd", "gn_bwd_apply": "gn_bwd_apply", "conv_mfma_v2": "conv_mfma_v2",
                  "conv_mfma_s2": "conv_mfma_s2", "conv_direct": "conv_direct",
                  "wgrad_direct": "wgrad_direct", "conv_wgrad_mfma": "conv_wgrad_mfma", "conv_wgrad_mfma_1x1": "conv_wgrad_mfma",
                  "conv_mfma_gnbwd": "conv_mfma_gnbwd", "chain": "chain"}


@pytest.mark.parametrize("family", list(PROBE_FAMILIES))
def test_probe_rstd_is_exact_on_powers_of_four(dev, family):
    from pti_ldm_vae_amd import ops
    got = {ve: _probe_family(ops, dev, family, ve) for ve in PROBE_VE}
    exact = tuple(ve ** -0.5 for ve in PROBE_VE if got[ve] == ve ** -0.5)
    print(f"[probe] {family}: " + ", ".join(f"var+eps={ve:g} -> {got[ve]!r}" for ve in PROBE_VE) + f"; exact: {exact}")
    assert 1.0 in exact, f"{family}: rstd(1) = {got[1.0]!r}: this family has to stay under its tolerance tests"
    claimed = X.EXACT_RSTD[PROBE_FAMILIES[family]]
    assert all(r in exact for r in claimed), f"{family}: EXACT_RSTD claims {claimed}, measured exact {exact}"


def test_probe_dsilu_of_zero_is_one_half(dev):
    """gamma = beta = 0: every pre-activation is 0; with dy = 1, S1 = sum dy * act'(0) = HW / 2 and dy_out = 1/2."""
    from pti_ldm_vae_amd import ops
    n, h, w, c = 1, 8, 16, 32
    z, zero = torch.zeros(n, 16, 2, dtype=torch.int64, device=dev), torch.zeros(c, device=dev)
    one = torch.ones(n, h, w, c, dtype=B16, device=dev)
    dx, sums = _nan(one.shape, B16, dev), _nan((n, c, 2), F32, dev)
    ops.gn_bwd(one, one, dx, z, zero, zero, sums, zero.clone(), zero.clone(), groups=16, eps=1.0, silu=True)
    dy_out, gsums = _nan(one.shape, B16, dev), _nan((n, c, 2), F32, dev)
    ops.conv_mfma_gnbwd(one, ops.pack_conv_weight(_identity(c, c, 3, dev), 3, ops.PTI_CONV_S1, flip=True), one, z, zero, zero,
                        dy_out, gsums, cout=c, groups=16, eps=1.0, silu=True)
    torch.cuda.synchronize()
    got = (_single("gn_bwd S1", sums[..., 0]) / (h * w), _single("gnbwd dy_out", dy_out), _single("gnbwd S1", gsums[..., 0]) / (h * w))
    print(f"[probe] dsilu(0): gn_bwd {got[0]!r}, conv_mfma_gnbwd dy_out {got[1]!r}, its S1 / HW {got[2]!r}")
    assert got == (0.5, 0.5, 0.5)


# ---- forward prologue: conv_mfma -------------------------------------------------------------------------------------
PRO = X.prologue_rows()


def _prologue_args(ops, s, dev):
    return dict(prologue=ops.PTI_PRO_GN, in_stats=s.stats.to(dev), gamma=_f32(s.gamma, dev), beta=_f32(s.beta, dev),
                groups=s.groups, eps=s.eps)


@pytest.mark.parametrize("row", PRO, ids=[r["id"] for r in PRO])
def test_conv_mfma_prologue_exact(dev, row):
    from pti_ldm_vae_amd import ops
    c = _cached(("pro", row["id"]), lambda: X.make_prologue_case(row))
    s, n, cin, cout, ks = c.s, row["n"], row["cin"], row["cout"], row["ks"]
    sdt = H16 if row["f16"] else B16
    m = _mode(ops, row["mode"])
    wp = ops.pack_conv_weight(_f32(c.w, dev), ks, m, f16=row["f16"])
    xd, resd = _nhwc(c.x, dev, sdt), _nhwc(c.res, dev, sdt)
    ho, wo = ops.conv_out_hw(row["h"], row["w"], m)
    want = "conv_mfma_kernel<" if row["mode"] == "s2" else "conv_mfma2_kernel<"
    # (reference, bias, residual, fused statistics, act_out)
    variants = [("plain", False, False, False, False), ("full", True, True, row["stats"], False)]
    if ks == 3 and row["mode"] == "s1" and (not row["f16"] or cout <= 64):
        variants.append(("bias", True, False, False, True))
    for name, bias, res, stats, act in variants:
        tag = f"conv_mfma GN prologue [{row['id']}] {name} stats={stats} act_out={act}"
        y = _nan((n, ho, wo, cout), sdt, dev)
        ost = torch.zeros(n, E.STATS_GROUPS, 2, dtype=torch.int64, device=dev) if stats else None
        actd = _nan(xd.shape, B16, dev) if act else None
        ops.conv_mfma(xd, wp, _f32(c.bias, dev) if bias else None, y, cout=cout, ksize=ks, mode=m, residual=resd if res else None,
                      out_stats=ost, out_groups=E.STATS_GROUPS if stats else 0, act_out=actd, **_prologue_args(ops, s, dev))
        torch.cuda.synchronize()
        got = ops.last_kernel_name()
        assert got.startswith(want), f"{tag}: went down {got}"
        E.assert_exact(tag, y, c.ref[name, sdt], layout="nhwc")
        if stats:
            E.assert_exact(tag + " fused statistics", ost, c.ref[name + "_stats", sdt], layout="flat")
        if act:
            E.assert_exact(tag + " act_out", actd, c.a, layout="nhwc")
    if row["f16"]:
        # fp16 storage with bf16-packed weights: the loader converts the staged operand to bf16 (the run-time-format kernel)
        tag = f"conv_mfma GN prologue [{row['id']}] full, bf16-packed weights"
        y = _nan((n, ho, wo, cout), sdt, dev)
        ost = torch.zeros(n, E.STATS_GROUPS, 2, dtype=torch.int64, device=dev) if row["stats"] else None
        ops.conv_mfma(xd, ops.pack_conv_weight(_f32(c.w, dev), ks, m), _f32(c.bias, dev), y, cout=cout, ksize=ks, mode=m,
                      residual=resd, out_stats=ost, out_groups=E.STATS_GROUPS if row["stats"] else 0, **_prologue_args(ops, s, dev))
        torch.cuda.synchronize()
        assert ops.last_kernel_name().startswith(want), f"{tag}: went down {ops.last_kernel_name()}"
        E.assert_exact(tag, y, c.ref["full", sdt], layout="nhwc")
        if row["stats"]:
            E.assert_exact(tag + " fused statistics", ost, c.ref["full_stats", sdt], layout="flat")


# ---- forward prologue: the degenerate-channel conv and its weight gradient ----------------------------------------------
@pytest.mark.parametrize("k", range(len(X.DIRECT_PROLOGUE)), ids=[f"{r[1]}to{r[2]}@{r[3]}x{r[4]}" for r in X.DIRECT_PROLOGUE])
def test_conv_direct_prologue_exact(dev, k):
    from pti_ldm_vae_amd import ops
    n, cin, cout, h, w, g, ol = X.DIRECT_PROLOGUE[k]
    c = _cached(("direct", k), lambda: X.make_prologue_case(X.direct_row(n, cin, cout, h, w, g, k=k)))
    ref = c.conv + c.bias.view(1, -1, 1, 1)
    X.check_f32("conv_direct reference", ref)
    w_tck = c.w.permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous().to(dev, F32)
    y, yl = (_nan((n, cout, h, w), F32, dev), "nchw") if ol == "nchw_f32" else (_nan((n, h, w, cout), F32, dev), "nhwc")
    ops.conv_direct(_nhwc(c.x, dev, B16), w_tck, _f32(c.bias, dev), y, n=n, h=h, w=w, cin=cin, cout=cout, x_layout="nhwc",
                    y_layout=yl, **_prologue_args(ops, c.s, dev))
    torch.cuda.synchronize()
    E.assert_exact(f"conv_direct GN prologue [{cin}->{cout}@{h}x{w}]", y, ref, layout=yl)


@pytest.mark.parametrize("k", range(len(X.WGRAD_DIRECT_PROLOGUE)), ids=[f"{r[1]}x{r[2]}@{r[3]}x{r[4]}" for r in X.WGRAD_DIRECT_PROLOGUE])
def test_wgrad_direct_prologue_exact(dev, k):
    """fewcout: y[cn] = conv(GN(x[cw])): wide = x (bf16 NHWC), narrow = dY (fp32 NCHW); the call adds to dW / dbias."""
    from pti_ldm_vae_amd import ops
    n, cw, cn, h, w = X.WGRAD_DIRECT_PROLOGUE[k]
    c = _cached(("wgrad_direct", k), lambda: X.make_wgrad_prologue_case(X.direct_row(n, cw, cn, h, w, 16, k=10 + k)))
    dw, db = torch.zeros(cn, cw, 3, 3, device=dev), torch.zeros(cn, device=dev)
    for times in (1, 2):
        ops.wgrad_direct(_nhwc(c.x, dev, B16), _f32(c.dy, dev), dw, n=n, h=h, w=w, cw=cw, cn=cn, ksize=3, sgn=1,
                         narrow_layout="nchw", dw_strides=(1, 9, cw * 9), dbias_narrow=db, **_prologue_args(ops, c.s, dev))
        torch.cuda.synchronize()
        E.assert_exact(f"wgrad_direct GN prologue [{cw}x{cn}] dW x{times}", dw, times * c.dw, layout="dw")
        E.assert_exact(f"wgrad_direct GN prologue [{cw}x{cn}] dbias x{times}", db, times * c.db, layout="flat")


# ---- forward prologue: conv_wgrad_mfma -------------------------------------------------------------------------------
WG = X.wgrad_rows()


def _wgrad_route(row):
    if row["mode"] == "s2":
        return "wgrad_mfma_kernel<3,2,"
    if row["ks"] == 1:
        return "wgrad_mfma_kernel<1,1,"
    return "wgrad_mfma3_kernel<2,false>" if row["mode"] == "s1" and row["cout"] % 64 == 0 else "wgrad_mfma3_kernel<1,false>"


@pytest.mark.parametrize("row", WG, ids=[r["id"] for r in WG])
def test_conv_wgrad_mfma_prologue_exact(dev, row):
    from pti_ldm_vae_amd import ops
    c = _cached(("wgrad", row["id"]), lambda: X.make_wgrad_prologue_case(row))
    cin, cout, ks, m = row["cin"], row["cout"], row["ks"], _mode(ops, row["mode"])
    xd, dyd = _nhwc(c.x, dev, B16), _nhwc(c.dy, dev, B16)
    dw, db = _nan((cout, cin, ks, ks), F32, dev), _nan((cout,), F32, dev)
    prof = []
    ops.KERNEL_PROFILE = prof          # the two-call form (partials, then reduce) records the partial kernel's name
    try:
        ops.conv_wgrad_mfma(xd, dyd, dw, db, ksize=ks, mode=m, **_prologue_args(ops, c.s, dev))
        torch.cuda.synchronize()
    finally:
        ops.KERNEL_PROFILE = None
    route = prof[0][0].replace(" ", "")
    assert _wgrad_route(row) in route, f"{row['id']} went down {route}"
    E.assert_exact(f"{row['id']} dW", dw, c.dw, layout="dw")
    E.assert_exact(f"{row['id']} dbias", db, c.db, layout="flat")
    ops.conv_wgrad_mfma(xd, dyd, dw, db, ksize=ks, mode=m, accumulate=True, **_prologue_args(ops, c.s, dev))
    torch.cuda.synchronize()
    E.assert_exact(f"{row['id']} dW after accumulate=True", dw, 2 * c.dw, layout="dw")
    E.assert_exact(f"{row['id']} dbias after accumulate=True", db, 2 * c.db, layout="flat")


# ---- backward: gn_bwd and gn_bwd_apply -------------------------------------------------------------------------------
BWD = X.bwd_rows()


@pytest.mark.parametrize("x16", [B16, H16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("row", BWD, ids=[r["id"] for r in BWD])
def test_gn_bwd_and_apply_exact(dev, row, x16):
    from pti_ldm_vae_amd import ops
    c = _cached(("bwd", row["id"]), lambda: X.make_bwd_case(row))
    s, n, ch = c.s, row["n"], row["c"]
    xd, dyd, dresd = _nhwc(c.x, dev, x16), _nhwc(c.dy, dev, B16), _nhwc(c.dres, dev, B16)
    st, gm, bt = s.stats.to(dev), _f32(s.gamma, dev), _f32(s.beta, dev)
    blocks = ops.L.lib().pti_gn_bwd_blocks(n, row["h"] * row["w"], ch)
    for ref, dres in ((c.ref, None), (c.ref_res, dresd)):
        tag = f"[{row['id']}{' +dres' if dres is not None else ''}, {blocks} workgroups per sample]"
        dg, db = torch.zeros(ch, device=dev), torch.zeros(ch, device=dev)
        dx, sums = _nan(xd.shape, B16, dev), _nan((n, ch, 2), F32, dev)
        ops.gn_bwd(xd, dyd, dx, st, gm, bt, sums, dg, db, groups=s.groups, eps=s.eps, silu=False, dres=dres)
        torch.cuda.synchronize()
        E.assert_exact("gn_bwd sums " + tag, sums, ref.sums, layout="flat")
        E.assert_exact("gn_bwd dx " + tag, dx, ref.dx16, layout="nhwc")
        E.assert_exact("gn_bwd dgamma " + tag, dg, ref.dgamma, layout="flat")
        E.assert_exact("gn_bwd dbeta " + tag, db, ref.dbeta, layout="flat")
        # the second half alone on the reference's sums; the affine gradients receive exactly one more share
        dx2 = _nan(xd.shape, B16, dev)
        ops.gn_bwd_apply(xd, dyd, dx2, st, gm, bt, _f32(ref.sums, dev), dg, db, groups=s.groups, eps=s.eps, dres=dres)
        torch.cuda.synchronize()
        E.assert_exact("gn_bwd_apply dx " + tag, dx2, ref.dx16, layout="nhwc")
        E.assert_exact("gn_bwd_apply dgamma, second call " + tag, dg, 2 * ref.dgamma, layout="flat")
        E.assert_exact("gn_bwd_apply dbeta, second call " + tag, db, 2 * ref.dbeta, layout="flat")


@pytest.mark.parametrize("row", BWD[:1] + BWD[5:6] + BWD[8:9], ids=[r["id"] for r in BWD[:1] + BWD[5:6] + BWD[8:9]])
def test_gn_bwd_silu_plumbing_exact(dev, row):
    """gamma = beta = 0: act' is exactly 1/2 everywhere while xhat is not zero."""
    from pti_ldm_vae_amd import ops
    c = _cached(("bwd silu", row["id"]), lambda: X.make_silu_bwd_case(row))
    s, n, ch = c.s, row["n"], row["c"]
    xd, dresd = _nhwc(c.x, dev, H16), _nhwc(c.dres, dev, B16)
    dg, db = torch.zeros(ch, device=dev), torch.zeros(ch, device=dev)
    dx, sums = _nan(xd.shape, B16, dev), _nan((n, ch, 2), F32, dev)
    ops.gn_bwd(xd, _nhwc(c.dy, dev, B16), dx, s.stats.to(dev), _f32(s.gamma, dev), _f32(s.beta, dev), sums, dg, db, groups=s.groups,
               eps=s.eps, silu=True, dres=dresd)
    torch.cuda.synchronize()
    E.assert_exact(f"gn_bwd silu sums [{row['id']}]", sums, c.ref.sums, layout="flat")
    E.assert_exact(f"gn_bwd silu dgamma [{row['id']}]", dg, c.ref.dgamma, layout="flat")
    E.assert_exact(f"gn_bwd silu dbeta [{row['id']}]", db, c.ref.dbeta, layout="flat")
    E.assert_exact(f"gn_bwd silu dx = dres [{row['id']}]", dx, c.dres, layout="nhwc")


# ---- the fused epilogue of the data-gradient conv ----------------------------------------------------------------------
FUSED = X.fused_rows()


def _fused_launch(ops, dev, c, row, x16, silu):
    s = c.s
    wpt = ops.pack_conv_weight(_f32(c.wf, dev), row["ks"], ops.PTI_CONV_S1, flip=True)
    dy_out, gsums = _nan((row["n"], row["h"], row["w"], row["cin"]), B16, dev), _nan((row["n"], row["cin"], 2), F32, dev)
    prof = []
    ops.KERNEL_PROFILE = prof          # records the conv kernel's name (the finalize launch follows it)
    try:
        ops.conv_mfma_gnbwd(_nhwc(c.dy_in, dev, B16), wpt, _nhwc(c.gx, dev, x16), s.stats.to(dev), _f32(s.gamma, dev),
                            _f32(s.beta, dev), dy_out, gsums, cout=row["cin"], ksize=row["ks"], groups=s.groups, eps=s.eps, silu=silu)
        torch.cuda.synchronize()
    finally:
        ops.KERNEL_PROFILE = None
    return dy_out, gsums, prof[0][0]


@pytest.mark.parametrize("x16", [B16, H16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("row", FUSED, ids=[r["id"] for r in FUSED])
def test_conv_mfma_gnbwd_exact(dev, row, x16):
    from pti_ldm_vae_amd import ops
    c = _cached(("fused", row["id"]), lambda: X.make_fused_case(row))
    s, ch = c.s, row["cin"]
    tag = f"conv_mfma_gnbwd [{row['id']}]"
    dy_out, gsums, name = _fused_launch(ops, dev, c, row, x16, False)
    assert name.startswith("conv_mfma2_kernel<"), f"{tag}: went down {name}"
    E.assert_exact(tag + " dy_out", dy_out, c.g, layout="nhwc")
    E.assert_exact(tag + " gsums", gsums, c.ref.sums, layout="flat")
    xd = _nhwc(c.gx, dev, x16)
    dx, dg, db = _nan(xd.shape, B16, dev), torch.zeros(ch, device=dev), torch.zeros(ch, device=dev)
    ops.gn_bwd_apply(xd, dy_out, dx, s.stats.to(dev), _f32(s.gamma, dev), _f32(s.beta, dev), gsums, dg, db, groups=s.groups,
                     eps=s.eps, dres=_nhwc(c.dres, dev, B16))
    torch.cuda.synchronize()
    E.assert_exact(tag + " -> gn_bwd_apply dx", dx, c.ref_res.dx16, layout="nhwc")
    E.assert_exact(tag + " -> gn_bwd_apply dgamma", dg, c.ref.dgamma, layout="flat")
    E.assert_exact(tag + " -> gn_bwd_apply dbeta", db, c.ref.dbeta, layout="flat")


@pytest.mark.parametrize("row", FUSED[:1] + FUSED[2:4], ids=[r["id"] for r in FUSED[:1] + FUSED[2:4]])
def test_conv_mfma_gnbwd_silu_plumbing_exact(dev, row):
    from pti_ldm_vae_amd import ops
    c = _cached(("fused silu", row["id"]), lambda: X.make_fused_case(row, silu_plumbing=True))
    dy_out, gsums, _ = _fused_launch(ops, dev, c, row, H16, True)
    E.assert_exact(f"conv_mfma_gnbwd silu [{row['id']}] dy_out", dy_out, c.ref.dy_act, layout="nhwc")
    E.assert_exact(f"conv_mfma_gnbwd silu [{row['id']}] gsums", gsums, c.ref.sums, layout="flat")
    dg, db = torch.zeros(row["cin"], device=dev), torch.zeros(row["cin"], device=dev)
    ops.gn_affine_grads(gsums, dg, db, row["n"], row["cin"])
    torch.cuda.synchronize()
    E.assert_exact(f"conv_mfma_gnbwd silu [{row['id']}] dgamma", dg, c.ref.dgamma, layout="flat")
    E.assert_exact(f"conv_mfma_gnbwd silu [{row['id']}] dbeta", db, c.ref.dbeta, layout="flat")


# ---- the chained launch ------------------------------------------------------------------------------------------------
CHAIN = X.chain_rows()


@pytest.mark.parametrize("row", CHAIN, ids=[r["id"] for r in CHAIN])
def test_conv_mfma_gnbwd_chain_exact(dev, row):
    from pti_ldm_vae_amd import ops
    c = _cached(("chain", row["id"]), lambda: X.make_chain_case(row))
    up, lo, n, ch = c.up, c.lo, row["n"], row["c"]
    assert ops.gnbwd_chain_supported(ch, ch, 3, H16)
    wpt = ops.pack_conv_weight(_f32(c.wf, dev), 3, ops.PTI_CONV_S1, flip=True)
    in_sums = _f32(c.up_ref.sums, dev)
    args = (_nhwc(c.g_in, dev, B16), _nhwc(c.x_in, dev, H16), up.stats.to(dev), _f32(up.gamma, dev), in_sums)
    lower = (wpt, _nhwc(c.gx, dev, H16), lo.stats.to(dev), _f32(lo.gamma, dev), _f32(lo.beta, dev))
    for ride in (False, True):
        tag = f"chain [{row['id']}]{' affine gradients on the finalize launch' if ride else ''}"
        dx_in, dy_out = _nan((n, row["h"], row["w"], ch), B16, dev), _nan((n, row["h"], row["w"], ch), B16, dev)
        gsums = _nan((n, ch, 2), F32, dev)
        dg, db = torch.zeros(ch, device=dev), torch.zeros(ch, device=dev)
        kw = dict(in_dgamma=dg, in_dbeta=db) if ride else {}
        ops.conv_mfma_gnbwd_chain(*args, dx_in, *lower, dy_out, gsums, cout=ch, groups=up.groups, eps=up.eps, silu=False, **kw)
        if not ride:
            ops.gn_affine_grads(in_sums, dg, db, n, ch)
        torch.cuda.synchronize()
        E.assert_exact(tag + " dx_in", dx_in, c.dx_in, layout="nhwc")
        E.assert_exact(tag + " dy_out", dy_out, c.dy_out, layout="nhwc")
        E.assert_exact(tag + " gsums", gsums, c.gsums, layout="flat")
        E.assert_exact(tag + " dgamma", dg, c.up_ref.dgamma, layout="flat")
        E.assert_exact(tag + " dbeta", db, c.up_ref.dbeta, layout="flat")


# ---- tie-in: the table gn_stats produces is the table the consumers read ----------------------------------------------
def test_produced_statistics_feed_the_consumers_exactly(dev):
    """x in {m - 1, m + 1} balanced per group and eps = 3: var + eps = 4.  Statistics from ops.gn_stats, not by hand."""
    from pti_ldm_vae_amd import ops
    c = _cached("tie-in", X.make_tie_in_case)
    s = c.s
    n, ch, h, w = c.x.shape
    xd = _nhwc(c.x, dev, B16)
    st = ops.gn_stats(xd, s.groups)
    torch.cuda.synchronize()
    E.assert_exact("gn_stats", st, s.stats, layout="flat")
    y = _nan((n, h, w, ch), B16, dev)
    ops.conv_mfma(xd, ops.pack_conv_weight(_identity(ch, ch, 1, dev), 1, ops.PTI_CONV_S1), None, y, cout=ch, ksize=1,
                  prologue=ops.PTI_PRO_GN, in_stats=st, gamma=_f32(s.gamma, dev), beta=_f32(s.beta, dev), groups=s.groups, eps=s.eps)
    dx, sums = _nan(xd.shape, B16, dev), _nan((n, ch, 2), F32, dev)
    dg, db = torch.zeros(ch, device=dev), torch.zeros(ch, device=dev)
    ops.gn_bwd(xd, _nhwc(c.dy, dev, B16), dx, st, _f32(s.gamma, dev), _f32(s.beta, dev), sums, dg, db, groups=s.groups, eps=s.eps,
               silu=False)
    torch.cuda.synchronize()
    E.assert_exact("identity 1x1 conv of GN(x)", y, c.a, layout="nhwc")
    E.assert_exact("gn_bwd dx on produced statistics", dx, c.ref.dx16, layout="nhwc")
    E.assert_exact("gn_bwd dgamma on produced statistics", dg, c.ref.dgamma, layout="flat")

"""Reads and writes of the training step's kernels stay inside the tensors they are given (csrc/conv_mfma.hip,
csrc/conv_direct.hip, csrc/groupnorm.hip, csrc/attention.hip).

The op-level parity tests hand these kernels exact-size tensors from the caching allocator and compare values only: a read
or a write outside a tensor lands in a neighbouring pooled block and nothing notices.  Here every case runs three ways
(``_confined``): on plain tensors; with every input inside a NaN-poisoned buffer and every output between canary words
(tests/bounds_util.py); and the same with +/-2^14 as the poison, because max-style instructions drop a NaN operand.  The
kernels use no floating-point atomics (``out_stats`` is accumulated with integer atomics), so the three runs must agree
bitwise and every canary must survive: a result that changes with what lies next to a tensor is a bug.

The shapes are the small ragged ones a 72 x 104 image produces (maps of 18 x 26 and 9 x 13, and 13 x 19): no multiple of
the 8 x 16 pixel tile on either axis, with an image boundary inside the batch.  The plain run is also compared with a
float64 CPU reference at the tolerances the existing test of that kernel states (tests/test_gpu_ops.py, test_gpu_ops2.py,
test_gpu_fp16_storage.py, test_gpu_fused_gnbwd.py, test_gpu_gnbwd_chain.py, test_gpu_attention.py).
"""
import pytest
import torch
import torch.nn.functional as F

import bounds_util as B
from test_gpu_ops import _gn_ref, _nhwc, _r, _report, _stats_ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16, F16, F32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int64


def _confined(dev, ins, outs, launch):
    """``ins``: name -> device tensor or None; ``outs``: name -> (shape, dtype, fill); ``launch(ins, outs)`` issues the
    kernel(s).  Runs plain, then inside NaN poison, then inside finite poison; -> the plain run's outputs."""
    plain = {k: torch.full(tuple(s), f, dtype=d, device=dev) for k, (s, d, f) in outs.items()}
    launch(ins, plain)
    torch.cuda.synchronize()
    for k, t in plain.items():
        if t.dtype.is_floating_point:
            assert not bool(torch.isnan(t).any()), f"{k}: the kernel left part of its output unwritten (or wrote NaN)"
    for poison in B.POISONS:
        gi = {k: None if t is None else B.guarded(dev, t, poison) for k, t in ins.items()}
        hs = {k: B.with_canary(dev, s, d, f) for k, (s, d, f) in outs.items()}
        launch(gi, {k: h.view for k, h in hs.items()})
        torch.cuda.synchronize()
        for k, h in hs.items():
            assert B.intact(h), f"{k}: a canary round the output was overwritten (inputs inside poison {poison})"
            assert torch.equal(h.view, plain[k]), f"{k}: differs from the run on plain tensors with poison {poison} round the inputs"
    return plain


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


# ---- conv_mfma --------------------------------------------------------------------------------------------------------
CONV = {
    # n, cin, cout, h, w, ksize, mode, prologue, residual, out_stats, pool2, activation storage
    "s1_3x3_pro2_res_stats_act": (2, 32, 64, 13, 19, 3, "s1", 2, True, True, False, BF16),
    "s1_3x3_plain":              (1, 64, 32, 9, 13, 3, "s1", 0, False, False, False, BF16),
    "s1_1x1_pro1":               (2, 32, 96, 9, 13, 1, "s1", 1, False, False, False, BF16),
    "s2_stats":                  (2, 32, 32, 18, 26, 3, "s2", 0, False, True, False, BF16),
    "up":                        (2, 64, 32, 9, 13, 3, "up", 0, False, False, False, BF16),
    "zins_flip":                 (2, 32, 64, 9, 13, 3, "zins", 0, False, False, False, BF16),
    "pooled":                    (1, 128, 64, 10, 6, 3, "s1", 0, False, False, True, BF16),
    "s1_3x3_fp16_storage":       (1, 64, 32, 13, 19, 3, "s1", 2, False, True, False, F16),
}


@pytest.mark.parametrize("name", list(CONV))
def test_conv_mfma_confined(dev, name):
    from pti_ldm_vae_amd import ops
    n, cin, cout, h, w, ks, mode, pro, res, ostats, pool, store = CONV[name]
    torch.manual_seed(1)
    groups, og, eps = 16, 16, 1e-6
    x = _r(torch.randn(n, cin, h, w) * 1.3 + 0.2)
    wt = _r(torch.randn(cout, cin, ks, ks) / (cin * ks * ks) ** 0.5)
    bias = None if pool else torch.randn(cout) * 0.1
    gamma = 1 + 0.2 * torch.randn(cin)
    beta = 0.1 * torch.randn(cin)
    a = _r(_gn_ref(x, groups, gamma, beta, eps, pro == 2)) if pro else x
    a64, w64 = a.double(), wt.double()
    b64 = None if bias is None else bias.double()
    wsrc, flip = wt, False
    if mode == "s1":
        ref, m = F.conv2d(a64, w64, b64, padding=ks // 2), ops.PTI_CONV_S1
    elif mode == "s2":
        ref, m = F.conv2d(F.pad(a64, (0, 1, 0, 1)), w64, b64, stride=2), ops.PTI_CONV_S2PAD
    elif mode == "up":
        ref, m = F.conv2d(F.interpolate(a64, scale_factor=2.0, mode="nearest"), w64, b64, padding=1), ops.PTI_CONV_UP2
    else:   # zins: data gradient of the stride-2 asymmetric-pad conv [n,cout,2h,2w] -> [n,cin,h,w] with weight wf[cin,cout,3,3]
        wf = _r(torch.randn(cin, cout, 3, 3) / (cout * 9) ** 0.5)
        xin = torch.zeros(n, cout, 2 * h, 2 * w, dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(xin, (0, 1, 0, 1)), wf.double(), None, stride=2).backward(a64)
        ref, m = xin.grad + b64.view(1, -1, 1, 1), ops.PTI_CONV_ZINS
        wsrc, flip = wf, True
    if pool:    # the unfused path rounds the full-resolution map to bf16 first
        ref = 4.0 * F.avg_pool2d(_r(ref.float()).double(), 2)
    rs = _r(torch.randn(ref.shape)) if res else None
    if res:
        ref = ref + rs.double()
    xd = _nhwc(x).to(dev, store)
    with_act = bool(pro) and mode == "s1" and ks == 3
    ins = dict(x=xd, w=ops.pack_conv_weight(wsrc.to(dev), ks, m, flip=flip), bias=None if bias is None else bias.to(dev),
               stats=ops.gn_stats(xd, groups) if pro else None, gamma=gamma.to(dev) if pro else None,
               beta=beta.to(dev) if pro else None, res=_nhwc(rs).to(dev, store) if res else None)
    ho, wo = ops.conv_out_hw(h, w, m)
    outs = dict(y=((n, ho // 2, wo // 2, cout) if pool else (n, ho, wo, cout), store, NAN))
    if ostats:
        outs["out_stats"] = ((n, og, 2), I64, 0)          # Q47.16 fixed-point sums, accumulated
    if with_act:
        outs["act_out"] = ((n, h, w, cin), BF16, NAN)

    def launch(i, o):
        ops.conv_mfma(i["x"], i["w"], i["bias"], o["y"], cout=cout, ksize=ks, mode=m, prologue=pro, in_stats=i["stats"],
                      gamma=i["gamma"], beta=i["beta"], groups=groups, eps=eps, residual=i["res"], out_stats=o.get("out_stats"),
                      out_groups=og, act_out=o.get("act_out"), pool2=pool)

    got = _confined(dev, ins, outs, launch)
    y = _nchw(got["y"])
    f16 = store == F16
    _report(f"conv_mfma {name}", y, ref, max_frac=1e-2, l2=3e-3 if f16 else 2e-3)
    if with_act:   # bf16 of an fp32 GN+SiLU: one rounding step of slack against the CPU reference
        _report("conv_mfma act_out", _nchw(got["act_out"]), a, max_frac=1e-2, l2=3e-3)
    if ostats:     # statistics are those of the values as stored
        _report("conv_mfma fused stats", ops.stats_to_float(got["out_stats"]), _stats_ref(y if f16 else _r(y), og), max_frac=1e-3, l2=1e-4)


# ---- data gradient with the GroupNorm backward in its epilogue, and its chained form ---------------------------------------
def test_conv_mfma_gnbwd_confined(dev):
    """pti_conv2d_mfma_gnbwd, then pti_gn_bwd_apply on what it wrote, n=2 at 13 x 19, against float64 autograd of
    conv(silu(GroupNorm(x))) (tolerances of tests/test_gpu_fused_gnbwd.py)."""
    from pti_ldm_vae_amd import ops
    n, cin, cout, h, w, ks = 2, 32, 64, 13, 19, 3
    torch.manual_seed(11)
    groups, eps = 16, 1e-6
    x = _r(torch.randn(n, cin, h, w) * 1.4 + 0.3)
    gamma, beta = 1 + 0.2 * torch.randn(cin), 0.1 * torch.randn(cin)
    wt = _r(torch.randn(cout, cin, ks, ks) / (cin * ks * ks) ** 0.5)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.conv2d(F.silu(F.group_norm(x64, groups, g64, b64, eps)), wt.double(), None, padding=1)
    dy = _r(torch.randn(y.shape))
    y.backward(dy.double())
    dres = _r(torch.randn(n, cin, h, w))
    xd = _nhwc(x).to(dev, BF16)
    ins = dict(dy=_nhwc(dy).to(dev, BF16), w=ops.pack_conv_weight(wt.to(dev), ks, ops.PTI_CONV_S1, flip=True), x=xd,
               stats=ops.gn_stats(xd, groups), gamma=gamma.to(dev), beta=beta.to(dev), dres=_nhwc(dres).to(dev, BF16))
    outs = dict(dy_out=((n, h, w, cin), BF16, NAN), sums=((n, cin, 2), F32, 0.0), dx=((n, h, w, cin), BF16, NAN),
                dgamma=((cin,), F32, 0.0), dbeta=((cin,), F32, 0.0))

    def launch(i, o):
        ops.conv_mfma_gnbwd(i["dy"], i["w"], i["x"], i["stats"], i["gamma"], i["beta"], o["dy_out"], o["sums"], cout=cin,
                            ksize=ks, groups=groups, eps=eps, silu=True)
        ops.gn_bwd_apply(i["x"], o["dy_out"], o["dx"], i["stats"], i["gamma"], i["beta"], o["sums"], o["dgamma"], o["dbeta"],
                         groups=groups, eps=eps, dres=i["dres"])

    got = _confined(dev, ins, outs, launch)
    _report("fused gnbwd dx", _nchw(got["dx"]), x64.grad + dres.double(), max_frac=1.5e-2, l2=6e-3)
    _report("fused gnbwd dgamma", got["dgamma"], g64.grad, max_frac=1e-2, l2=5e-3)
    _report("fused gnbwd dbeta", got["dbeta"], b64.grad, max_frac=1e-2, l2=5e-3)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def test_conv_mfma_gnbwd_chain_confined(dev):
    """pti_conv2d_mfma_gnbwd_chain, n=2 at 13 x 19, built as tests/test_gpu_gnbwd_chain.py builds it; values against the
    unchained composition it replaces, at that test's bounds."""
    from pti_ldm_vae_amd import ops
    n, h, w, c, G = 2, 13, 19, 128, 16
    g = torch.Generator(device=dev).manual_seed(113)
    dy = (torch.randn(n, h, w, c, device=dev, generator=g) * 0.3).bfloat16()
    h1 = (torch.randn(n, h, w, c, device=dev, generator=g) * 1.2 + 0.1).half()
    x = (torch.randn(n, h, w, c, device=dev, generator=g) * 0.9).half()
    w1 = torch.randn(c, c, 3, 3, device=dev, generator=g) * 0.03
    w2 = torch.randn(c, c, 3, 3, device=dev, generator=g) * 0.03
    gm1, bt1 = 1 + 0.2 * torch.randn(c, device=dev, generator=g), 0.1 * torch.randn(c, device=dev, generator=g)
    gm2, bt2 = 1 + 0.2 * torch.randn(c, device=dev, generator=g), 0.1 * torch.randn(c, device=dev, generator=g)
    wpt1 = ops.pack_conv_weight(w1, 3, ops.PTI_CONV_S1, flip=True)
    wpt2 = ops.pack_conv_weight(w2, 3, ops.PTI_CONV_S1, flip=True)
    st1, st2 = ops.gn_stats(x, G), ops.gn_stats(h1, G)
    assert ops.gnbwd_chain_supported(c, c, 3, x.dtype)
    g2 = torch.empty(n, h, w, c, dtype=BF16, device=dev)
    sums2 = torch.zeros(n * c * 2, device=dev)
    ops.conv_mfma_gnbwd(dy, wpt2, h1, st2, gm2, bt2, g2, sums2, cout=c, groups=G, silu=True)
    dh1 = torch.empty_like(g2)
    dg2, db2 = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    ops.gn_bwd_apply(h1, g2, dh1, st2, gm2, bt2, sums2, dg2, db2, groups=G)
    g1 = torch.empty(n, h, w, c, dtype=BF16, device=dev)
    sums1 = torch.zeros(n * c * 2, device=dev)
    ops.conv_mfma_gnbwd(dh1, wpt1, x, st1, gm1, bt1, g1, sums1, cout=c, groups=G, silu=True)
    ins = dict(g_in=g2, x_in=h1, in_stats=st2, in_gamma=gm2, in_sums=sums2, w=wpt1, gx=x, gstats=st1, ggamma=gm1, gbeta=bt1)
    outs = dict(dx_in=((n, h, w, c), BF16, NAN), dy_out=((n, h, w, c), BF16, NAN), gsums=((n * c * 2,), F32, 0.0),
                in_dgamma=((c,), F32, 0.0), in_dbeta=((c,), F32, 0.0))

    def launch(i, o):
        ops.conv_mfma_gnbwd_chain(i["g_in"], i["x_in"], i["in_stats"], i["in_gamma"], i["in_sums"], o["dx_in"], i["w"], i["gx"],
                                  i["gstats"], i["ggamma"], i["gbeta"], o["dy_out"], o["gsums"], cout=c, groups=G, silu=True,
                                  in_dgamma=o["in_dgamma"], in_dbeta=o["in_dbeta"])

    got = _confined(dev, ins, outs, launch)
    assert _rel(got["dx_in"], dh1) <= 4e-3
    assert _rel(got["dy_out"], g1) <= 6e-3
    assert _rel(got["gsums"], sums1) <= 6e-3
    assert torch.equal(got["in_dgamma"], dg2) and torch.equal(got["in_dbeta"], db2)


# ---- conv_direct ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,h,w,pro,il,ol", [(2, 3, 64, 9, 11, 0, "nchw_f32", "nhwc_bf16"),
                                                     (2, 64, 3, 12, 10, 1, "nhwc_bf16", "nchw_f32")])
def test_conv_direct_confined(dev, n, cin, cout, h, w, pro, il, ol):
    from pti_ldm_vae_amd import ops
    torch.manual_seed(2)
    groups, eps = (16 if cin % 16 == 0 else 1), 1e-6
    x = torch.randn(n, cin, h, w) * 1.2 + 0.1
    if il.endswith("bf16"):
        x = _r(x)
    wt = torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5
    bias = torch.randn(cout) * 0.1
    gamma = 1 + 0.2 * torch.randn(cin)
    beta = 0.1 * torch.randn(cin)
    a = _gn_ref(x, groups, gamma, beta, eps, pro == 2) if pro else x
    ref = F.conv2d(a.double(), wt.double(), bias.double(), padding=1)
    if il == "nchw_f32":
        xd, xl = x.to(dev), "nchw"
    else:
        xd, xl = _nhwc(x).to(dev, BF16), "nhwc"
    ins = dict(x=xd, w=wt.permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous().to(dev), bias=bias.to(dev),
               stats=ops.gn_stats(xd, groups) if pro else None, gamma=gamma.to(dev) if pro else None,
               beta=beta.to(dev) if pro else None)
    if ol == "nhwc_bf16":
        outs, yl = dict(y=((n, h, w, cout), BF16, NAN)), "nhwc"
    else:
        outs, yl = dict(y=((n, cout, h, w), F32, NAN)), "nchw"

    def launch(i, o):
        ops.conv_direct(i["x"], i["w"], i["bias"], o["y"], n=n, h=h, w=w, cin=cin, cout=cout, x_layout=xl, y_layout=yl,
                        prologue=pro, in_stats=i["stats"], gamma=i["gamma"], beta=i["beta"], groups=groups, eps=eps)

    got = _confined(dev, ins, outs, launch)["y"].float().cpu()
    if yl == "nhwc":
        got = got.permute(0, 3, 1, 2)
    tol = dict(max_frac=1e-2, l2=3e-3) if ol.endswith("bf16") else dict(max_frac=1e-4, l2=2e-5)
    _report(f"conv_direct[{cin}->{cout},pro{pro}]", got, ref, **tol)


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------
GN_SHAPES = [(3, 64, 9, 7, 16), (2, 32, 13, 19, 16)]


@pytest.mark.parametrize("n,c,h,w,g", GN_SHAPES)
def test_gn_stats_confined(dev, n, c, h, w, g):
    from pti_ldm_vae_amd import ops
    torch.manual_seed(0)
    x = _r(torch.randn(n, c, h, w) * 1.5 + 0.3)
    got = _confined(dev, dict(x=_nhwc(x).to(dev, BF16)), dict(stats=((n, g, 2), I64, 0)),
                    lambda i, o: ops.gn_stats(i["x"], g, stats=o["stats"]))
    _report("gn_stats", ops.stats_to_float(got["stats"]), _stats_ref(x, g), max_frac=1e-4, l2=1e-5)


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("n,c,h,w,g", GN_SHAPES)
def test_gn_bwd_confined(dev, n, c, h, w, g, res):
    from pti_ldm_vae_amd import ops
    torch.manual_seed(5)
    eps = 1e-6
    x = _r(torch.randn(n, c, h, w) * 1.5 + 0.3)
    gamma, beta = 1 + 0.2 * torch.randn(c), 0.1 * torch.randn(c)
    da = _r(torch.randn(n, c, h, w))
    dres = _r(torch.randn(n, c, h, w)) if res else None
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    _gn_ref(x64, g, g64, b64, eps, True).backward(da.double())
    ref_dx = x64.grad + (dres.double() if res else 0)
    xd = _nhwc(x).to(dev, BF16)
    ins = dict(x=xd, da=_nhwc(da).to(dev, BF16), stats=ops.gn_stats(xd, g), gamma=gamma.to(dev), beta=beta.to(dev),
               dres=_nhwc(dres).to(dev, BF16) if res else None)
    outs = dict(dx=((n, h, w, c), BF16, NAN), sums=((n, c, 2), F32, 0.0), dgamma=((c,), F32, 0.0), dbeta=((c,), F32, 0.0))

    def launch(i, o):
        ops.gn_bwd(i["x"], i["da"], o["dx"], i["stats"], i["gamma"], i["beta"], o["sums"], o["dgamma"], o["dbeta"], groups=g,
                   eps=eps, silu=True, dres=i["dres"])

    got = _confined(dev, ins, outs, launch)
    _report("gn_bwd dx", _nchw(got["dx"]), ref_dx, max_frac=1e-2, l2=3e-3)
    _report("gn_bwd dgamma", got["dgamma"], g64.grad, max_frac=1e-4, l2=2e-5)
    _report("gn_bwd dbeta", got["dbeta"], b64.grad, max_frac=1e-4, l2=2e-5)


# ---- attention ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,l,c,spike", [(2, 7, 64, False), (1, 40, 256, False), (2, 117, 128, True)])
def test_attention_confined(dev, b, l, c, spike):
    from pti_ldm_vae_amd import ops
    torch.manual_seed(10)
    qkv = _r(torch.randn(b, l, 3 * c))
    if spike:  # a key far along the stream that dominates some queries
        qkv[:, l - 3, c:2 * c] *= 6.0
        qkv[:, 5, 0:c] *= 4.0
        qkv = _r(qkv)
    q64 = qkv.double().requires_grad_(True)
    q, k, v = q64[..., :c], q64[..., c:2 * c], q64[..., 2 * c:]
    logits = torch.einsum("blc,bmc->blm", q, k) * c ** -0.5
    o_ref = torch.einsum("blm,bmc->blc", torch.softmax(logits, dim=-1), v)
    dout = _r(torch.randn(b, l, c))
    o_ref.backward(dout.double())
    qd = qkv.to(dev, BF16)
    fwd = _confined(dev, dict(qkv=qd), dict(o=((b, l, c), BF16, NAN), lse2=((b, l), F32, NAN)),
                    lambda i, o: ops.attention_fwd(i["qkv"], o["o"], o["lse2"]))
    _report(f"attn fwd[{l},{c}]", fwd["o"], o_ref.detach(), max_frac=2e-2, l2=1e-2)
    _report("attn lse2", fwd["lse2"], torch.logsumexp(logits.detach(), dim=-1) * 1.4426950408889634, max_frac=1e-3, l2=1e-4)
    # the backward consumes the bf16 forward output, as the engine does
    bwd = _confined(dev, dict(qkv=qd, o=fwd["o"], dout=dout.to(dev, BF16), lse2=fwd["lse2"]),
                    dict(delta=((b, l), F32, NAN), dqkv=((b, l, 3 * c), BF16, NAN)),
                    lambda i, o: ops.attention_bwd(i["qkv"], i["o"], i["dout"], i["lse2"], o["delta"], o["dqkv"]))
    dq, gr = bwd["dqkv"], q64.grad
    _report("attn dq", dq[..., :c], gr[..., :c], max_frac=2e-2, l2=1.5e-2)
    _report("attn dk", dq[..., c:2 * c], gr[..., c:2 * c], max_frac=2e-2, l2=1.5e-2)
    _report("attn dv", dq[..., 2 * c:], gr[..., 2 * c:], max_frac=2e-2, l2=1.5e-2)

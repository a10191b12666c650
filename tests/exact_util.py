"""Exact-integer parity cases for the conv, weight-gradient, pooling and statistics kernels (tests/test_gpu_exact_parity.py;
the conditions and the comparator are checked on the CPU by tests/test_exact_util_cpu.py).

Method.  Activations, gradients, weights, bias and residual are small INTEGERS, which bf16 and fp16 hold exactly.  Every
product is then exact, every fp32 partial sum stays below 2^24 in magnitude and is exact in any order (MFMA k-order, cin
chunks, split-K slabs, the Q47.16 statistics), and every value a kernel stores in 16 bits is an integer of magnitude
<= 256, which both formats hold.  So nothing rounds, and the kernel must EQUAL a float64 reference; a difference is an
indexing, masking or staging bug, and its position names the tile, tap or channel block.

``make_case`` asserts the conditions that make this true, on the reference alone:
  * every 16-bit output has |ref| <= 256 (``LIMIT16``);
  * every dW, dbias and statistics sum has sum |terms| < 2^24 (``LIMIT32``);
  * at least 1/16 of the weights of every (tap, 32-channel cin block, 32-channel cout block) are non-zero, so no block of a
    weight pack can go missing unnoticed;
  * at most 10 % of the reference outputs are zero, so a kernel that leaves zeros behind fails.

Plain torch on the CPU, float64 throughout.  Tensors are NCHW here; the GPU tests permute.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TILE = (8, 16)                # pixel tile of the MFMA kernels: 8 rows x 16 columns
LIMIT16 = 256.0               # integers up to 2^8 are exact in bf16 (8 significant bits) and in fp16 (11)
LIMIT32 = float(1 << 24)      # integers below 2^24 are exact in fp32
MIN_DENSITY = 1.0 / 16
MAX_ZERO = 0.10
STAT_SCALE = 65536            # Q47.16
F64 = torch.float64


# ---- the case tables shared by the CPU and the GPU file --------------------------------------------------------------
def _fwd(n, cin, cout, h, w, ks, mode, seed=0, **kw):
    d = dict(n=n, cin=cin, cout=cout, h=h, w=w, ks=ks, mode=mode, seed=seed, residual=False, pooled=False, nostats=False,
             f16=False, wdens=0.25, xmax=2)
    d.update(kw)
    d["id"] = (f"{mode}-k{ks}-{n}x{cin}to{cout}@{h}x{w}" + ("-pool" if d["pooled"] else "") + ("-f16" if d["f16"] else ""))
    return d


# ``residual``: the case also runs with bias + residual (+ fused statistics where the mode has them); ``nostats``: the
# case runs with bias + residual a second time, without the fused statistics; ``wdens``: P(weight != 0) (1/4 = P(+-1) =
# 1/8 each unless a row says why not); ``xmax``: activations are uniform integers in [-xmax, xmax].
FWD_CASES = [
    _fwd(2, 32, 32, 13, 19, 3, "s1", residual=True),
    _fwd(1, 64, 32, 9, 13, 3, "s1", residual=True),
    _fwd(2, 128, 64, 13, 19, 3, "s1", residual=True),
    _fwd(2, 128, 128, 13, 19, 3, "s1", residual=True, nostats=True),
    _fwd(1, 256, 256, 13, 19, 3, "s1", residual=True),            # two cin chunks, two cout tiles
    _fwd(3, 128, 128, 24, 40, 3, "s1", residual=True, nostats=True),  # 27 tiles: the tile walk
    # 1x1 on 32 channels: 32 terms of variance 1/2 leave 10 % zeros at P(+-1) = 1/8; 1/4 each brings that to 7 %
    _fwd(2, 32, 64, 13, 19, 1, "s1", wdens=0.5),
    _fwd(2, 128, 384, 9, 13, 1, "s1"),
    _fwd(2, 64, 192, 13, 19, 1, "s1", residual=True),
    _fwd(2, 32, 32, 18, 26, 3, "s2"),
    _fwd(1, 64, 64, 17, 33, 3, "s2"),                             # both odd: the pad row / column is never read; one tile
    _fwd(2, 128, 128, 18, 26, 3, "s2"),
    _fwd(1, 256, 256, 10, 34, 3, "s2"),
    _fwd(2, 64, 64, 9, 13, 3, "up"),
    _fwd(2, 128, 128, 9, 13, 3, "up", nostats=True),
    _fwd(1, 256, 256, 5, 9, 3, "up"),
    _fwd(2, 32, 64, 9, 13, 3, "zins"),
    _fwd(2, 128, 128, 9, 13, 3, "zins"),
    _fwd(1, 256, 256, 5, 9, 3, "zins"),
    # pooled store: four outputs are summed, so the activations are narrower ([-1, 1]) to keep the sum <= 256
    _fwd(1, 128, 64, 10, 6, 3, "s1", pooled=True, xmax=1),
    _fwd(2, 64, 64, 12, 20, 3, "s1", pooled=True, xmax=1),
    # fp16 storage and fp16 MFMA operands
    _fwd(2, 64, 64, 13, 19, 3, "s1", residual=True, f16=True),
    _fwd(2, 128, 128, 9, 13, 3, "up", f16=True),
]

# name: n, cin, cout, h, w, ksize, mode, the partial kernel the default rules pick (spelled as
# tests/test_gpu_wgrad_workspace.py::SINGLE spells it), PTI_WGRAD_V6 for the launch (None: unset)
WGRAD_CASES = {
    "v4_pairs":       (3, 32, 32, 24, 40, 3, "s1", "wgrad_mfma4_kernel<false>", None),
    "v4_two_block":   (2, 32, 64, 13, 19, 3, "s1", "wgrad_mfma4_kernel<true>", None),
    "v6_shape_a":     (2, 128, 128, 16, 32, 3, "s1", "wgrad_mfma6_kernel<W6Cfg<4,2,1>>", None),
    "v6_shape_a_256": (1, 256, 256, 13, 19, 3, "s1", "wgrad_mfma6_kernel<W6Cfg<4,2,1>>", None),
    "v6_shape_b":     (2, 64, 64, 30, 20, 3, "s1", "wgrad_mfma6_kernel<W6Cfg<2,2,2>>", "2"),
    "v3_up":          (2, 32, 32, 12, 20, 3, "up", "wgrad_mfma3_kernel<1,true>", None),
    "v3_up_128":      (2, 128, 128, 9, 13, 3, "up", "wgrad_mfma3_kernel<1,true>", None),
    "v3_up_256":      (1, 256, 256, 5, 9, 3, "up", "wgrad_mfma3_kernel<1,true>", None),
    "v1_s2":          (3, 32, 32, 47, 39, 3, "s2", "wgrad_mfma_kernel<3,2,", None),
    "v1_s2_64":       (2, 64, 64, 18, 26, 3, "s2", "wgrad_mfma_kernel<3,2,", None),
    "v1_s2_128":      (1, 128, 128, 17, 33, 3, "s2", "wgrad_mfma_kernel<3,2,", None),
    "v1_1x1":         (3, 32, 64, 24, 40, 1, "s1", "wgrad_mfma_kernel<1,1,", None),
    "v1_1x1_384":     (2, 128, 384, 9, 13, 1, "s1", "wgrad_mfma_kernel<1,1,", None),
}
# fp16 x on the same values (and the same references): case -> the kernel an fp16 input goes to (v4 / v6 take bf16 only)
WGRAD_F16_X = {
    "v4_two_block": "wgrad_mfma3_kernel<1,true>",
    "v3_up":        "wgrad_mfma3_kernel<1,true>",
    "v1_s2_64":     "wgrad_mfma_kernel<3,2,",
}
# the job mix of tests/test_gpu_wgrad_v6.py::test_batched_launch_mixes_all_kernel_modes: (cin, cout, h = w), batch 3
BATCHED_JOBS = [(32, 32, 24), (64, 64, 16), (128, 128, 8), (64, 128, 12), (128, 64, 12), (32, 64, 8)]
BATCHED_N = 3
DIRECT_SIZES = [(9, 11), (13, 19)]
# (kind, n, cw, cn, h, w): the fewcin rows of tests/test_gpu_ops.py::test_wgrad_direct and its fewcout rows without prologue
WGRAD_DIRECT_CASES = [("fewcin", 2, 32, 1, 16, 16), ("fewcin", 2, 128, 4, 8, 8), ("fewcin", 1, 64, 3, 10, 12),
                      ("fewcout", 2, 32, 1, 16, 16), ("fewcout", 2, 128, 4, 8, 8)]
# (n, c, h, w): integer maps for gn_stats (16 groups), each in bf16 and fp16 storage
STATS_CASES = [(3, 64, 9, 7), (2, 32, 13, 19)]
POOL_CASE = (2, 64, 10, 6)       # pool2x2_sum: [2, 10, 6, 64] NHWC -> [2, 5, 3, 64]
STATS_GROUPS = 16


# ---- integer data ------------------------------------------------------------------------------------------------------
def ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(F64)


def ternary(gen, shape, density):
    """{-1, 0, +1} with P(+1) = P(-1) = density / 2."""
    u = torch.rand(tuple(shape), generator=gen, dtype=F64)
    return (u < density / 2).to(F64) - (u >= 1 - density / 2).to(F64)


def conv_expr(a, wt, bias, ks, mode):
    """The forward expression of each gather mode, built as tests/test_gpu_ops.py::test_conv_mfma builds it."""
    if mode == "s1":
        return F.conv2d(a, wt, bias, padding=ks // 2)
    if mode == "s2":
        return F.conv2d(F.pad(a, (0, 1, 0, 1)), wt, bias, stride=2)
    if mode == "up":
        return F.conv2d(F.interpolate(a, scale_factor=2.0, mode="nearest"), wt, bias, padding=1)
    raise ValueError(mode)


def group_sums(y, groups=STATS_GROUPS):
    """{sum, sum of squares} per (sample, group) of an integer NCHW map -> int64 [n, groups, 2], and the largest sum of
    |terms| of any of them."""
    n = y.shape[0]
    yg = y.reshape(n, groups, -1)
    s = torch.stack([yg.sum(-1), (yg * yg).sum(-1)], -1)
    bound = max(yg.abs().sum(-1).max().item(), s[..., 1].max().item())
    return s.round().to(torch.int64), bound


# ---- the asserted conditions -------------------------------------------------------------------------------------------
def check_integers(name, t):
    assert bool((t == t.round()).all()), f"{name}: not integer-valued"


def check_store16(name, ref):
    check_integers(name, ref)
    m = ref.abs().max().item()
    assert m <= LIMIT16, f"{name}: max |ref| = {m:g} > {LIMIT16:g}: a 16-bit store would round"
    return m


def check_sum32(name, abs_sum):
    m = float(abs_sum)
    assert m < LIMIT32, f"{name}: sum |terms| = {m:g} >= 2^24: an fp32 partial sum could round"
    return m


def check_density(name, wt):
    """wt [cout, cin, k, k]: the share of non-zero weights of every (tap, 32-cin block, 32-cout block)."""
    cout, cin = wt.shape[:2]
    worst = 1.0
    for co in range(0, cout, 32):
        for ci in range(0, cin, 32):
            blk = wt[co:co + 32, ci:ci + 32]
            worst = min(worst, (blk != 0).to(F64).mean((0, 1)).min().item())
    assert worst >= MIN_DENSITY, f"{name}: a (tap, cin block, cout block) has only {worst:.3f} of its weights non-zero"
    return worst


def check_zero_fraction(name, ref):
    z = (ref == 0).to(F64).mean().item()
    assert z <= MAX_ZERO, f"{name}: {z:.3f} of the reference is zero"
    return z


# ---- cases -------------------------------------------------------------------------------------------------------------
def make_case(kind, n, cin, cout, h, w, ks=3, mode="s1", seed=0, residual=False, pooled=False, wdens=0.25, xmax=2,
              wmax=1):
    """Integer tensors and float64 references (all NCHW, on the CPU), with the exactness conditions asserted.

    kind "fwd": x, w (zins: the FORWARD weight [cin, cout, 3, 3] of the stride-2 conv whose data gradient this is, to be
      packed with flip=True), bias, res -> conv (no bias), ref_bias = conv + bias, ref_full = conv + bias + res (when
      ``residual``), stats_bias / stats_full (int64 [n, 16, 2] sums of ref_bias / ref_full), pool (2x2 sums of conv, when
      ``pooled``).
    kind "wgrad": x, dy -> dw [cout, cin, ks, ks], db [cout] by float64 autograd of the same expression.
    kind "direct": the stride-1 3x3 conv of csrc/conv_direct.hip: x, w, bias -> ref (``wmax`` > 1: dense integer weights in
      [-wmax, wmax] for the few-input-channel rows, where nine sparse terms would leave too many zeros).
    ``info`` holds the measured margins (largest |ref|, largest sum |terms|, zero share, weight density)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    c = SimpleNamespace(kind=kind, n=n, cin=cin, cout=cout, h=h, w_=w, ks=ks, mode=mode, info={})
    tag = f"{kind}[{mode},k{ks},{n}x{cin}->{cout}@{h}x{w}]"
    x = ints(gen, (n, cin, h, w), -xmax, xmax)
    c.x = x
    if kind == "fwd":
        c.bias = ints(gen, (cout,), -3, 3)
        if mode == "zins":
            wf = ternary(gen, (cin, cout, 3, 3), wdens)
            xin = torch.zeros(n, cout, 2 * h, 2 * w, dtype=F64, requires_grad=True)
            F.conv2d(F.pad(xin, (0, 1, 0, 1)), wf, None, stride=2).backward(x)
            conv, c.w = xin.grad.detach(), wf
            c.info["density"] = check_density(tag, wf.permute(1, 0, 2, 3))
        else:
            c.w = ternary(gen, (cout, cin, ks, ks), wdens)
            conv = conv_expr(x, c.w, None, ks, mode)
            c.info["density"] = check_density(tag, c.w)
        c.conv = conv
        c.ref_bias = conv + c.bias.view(1, -1, 1, 1)
        outs = [conv, c.ref_bias]
        c.res = c.ref_full = None
        if residual:
            c.res = ints(gen, conv.shape, -8, 8)
            c.ref_full = c.ref_bias + c.res
            outs.append(c.ref_full)
        c.info["max16"] = max(check_store16(tag, o) for o in outs)
        c.info["zero"] = max(check_zero_fraction(tag, o) for o in outs)
        if cout % STATS_GROUPS == 0:
            c.stats_bias, b1 = group_sums(c.ref_bias)
            c.stats_full, b2 = group_sums(c.ref_full) if residual else (None, 0.0)
            c.info["sum32"] = check_sum32(tag + " statistics", max(b1, b2))
        if pooled:
            c.pool = 4.0 * F.avg_pool2d(conv, 2)
            c.info["max16"] = max(c.info["max16"], check_store16(tag + " pooled", c.pool))
            c.info["zero"] = max(c.info["zero"], check_zero_fraction(tag + " pooled", c.pool))
    elif kind == "wgrad":
        def grads(a, g):
            wt = torch.zeros(cout, cin, ks, ks, dtype=F64, requires_grad=True)
            b = torch.zeros(cout, dtype=F64, requires_grad=True)
            y = conv_expr(a, wt, b, ks, mode)
            g = g(y.shape)
            y.backward(g)
            return wt.grad, b.grad, g
        c.dw, c.db, c.dy = grads(x, lambda s: ints(gen, s, -2, 2))
        aw, ab, _ = grads(x.abs(), lambda s: c.dy.abs())          # sum |x| |dy| of every dW / dbias element
        check_integers(tag, c.dw)
        c.info["sum32"] = check_sum32(tag, max(aw.max().item(), ab.max().item()))
        c.info["zero"] = check_zero_fraction(tag, c.dw)
    elif kind == "direct":
        c.bias = ints(gen, (cout,), -3, 3)
        c.w = ints(gen, (cout, cin, 3, 3), -wmax, wmax) if wmax > 1 else ternary(gen, (cout, cin, 3, 3), wdens)
        c.ref = F.conv2d(x, c.w, c.bias, padding=1)
        c.info["density"] = check_density(tag, c.w)
        check_integers(tag, c.ref)
        c.info["max16"] = c.ref.abs().max().item()
        c.info["sum32"] = check_sum32(tag, F.conv2d(x.abs(), c.w.abs(), c.bias.abs(), padding=1).max().item())
        c.info["zero"] = check_zero_fraction(tag, c.ref)
    else:
        raise ValueError(kind)
    return c


def make_fwd_case(row):
    return make_case("fwd", row["n"], row["cin"], row["cout"], row["h"], row["w"], row["ks"], row["mode"], row["seed"],
                     row["residual"], row["pooled"], wdens=row["wdens"], xmax=row["xmax"])


def make_wgrad_case(name):
    n, cin, cout, h, w, ks, mode = WGRAD_CASES[name][:7]
    return make_case("wgrad", n, cin, cout, h, w, ks, mode, seed=len(name))


def make_batched_case(i):
    cin, cout, hw = BATCHED_JOBS[i]
    return make_case("wgrad", BATCHED_N, cin, cout, hw, hw, 3, "s1", seed=70 + i)


def direct_rows():
    """(id, n, cin, cout, h, w, input layout/dtype, output layout/dtype): the nine rows of
    tests/test_gpu_ops.py::DIRECT_CASES, all without prologue, at the two sizes of DIRECT_SIZES."""
    from test_gpu_ops import DIRECT_CASES
    rows = []
    for k, (n, cin, cout, _, _, _, il, ol) in enumerate(DIRECT_CASES):
        for h, w in DIRECT_SIZES:
            rows.append((f"row{k}-{n}x{cin}to{cout}@{h}x{w}-{il}-{ol}", n, cin, cout, h, w, il, ol))
    return rows


def make_direct_case(n, cin, cout, h, w, out16):
    """Few input channels (the wide side is the output): dense integer weights in [-3, 3]."""
    c = make_case("direct", n, cin, cout, h, w, seed=cin + cout, wmax=3 if cin <= 16 else 1)
    if out16:
        check_store16(f"direct[{cin}->{cout}@{h}x{w}]", c.ref)
    return c


def make_wgrad_direct_case(kind, n, cw, cn, h, w):
    """fewcin: y[cw] = conv(x[cn]); fewcout: y[cn] = conv(x[cw]).  -> x, dy, dw, db (float64 autograd)."""
    cin, cout = (cn, cw) if kind == "fewcin" else (cw, cn)
    return make_case("wgrad", n, cin, cout, h, w, 3, "s1", seed=cw + cn)


def make_stats_case(n, ch, h, w, seed=0):
    gen = torch.Generator().manual_seed(2000 + seed)
    x = ints(gen, (n, ch, h, w), -2, 2)
    ref, bound = group_sums(x)
    check_sum32(f"gn_stats[{n}x{ch}@{h}x{w}]", bound)
    return SimpleNamespace(x=x, ref=ref)


def make_pool_case():
    n, ch, h, w = POOL_CASE
    gen = torch.Generator().manual_seed(3000)
    x = ints(gen, (n, ch, h, w), -60, 60)
    ref = 4.0 * F.avg_pool2d(x, 2)
    check_store16("pool2x2_sum", ref)
    check_zero_fraction("pool2x2_sum", ref)
    return SimpleNamespace(x=x, ref=ref)


# ---- the comparator ----------------------------------------------------------------------------------------------------
def tile_position(y, x, h, w, tile=TILE):
    """Where pixel (y, x) of an h x w map sits in its pixel tile: 'interior', 'edge' or 'corner' of the tile, plus 'last
    row' / 'last column' of the map."""
    th, tw = tile
    on_r, on_c = y % th in (0, th - 1), x % tw in (0, tw - 1)
    where = "corner" if (on_r and on_c) else "edge" if (on_r or on_c) else "interior"
    if y == h - 1:
        where += ", last row"
    if x == w - 1:
        where += ", last column"
    return where


def mismatches(got, ref, layout="nchw", tile=TILE):
    """-> (count, [dict]) of the elements of ``got`` that differ from ``ref`` after an exact cast (NaN differs from
    everything).  layout 'nchw' / 'nhwc': 4-D maps, located as (n, y, x, channel), tile position, 32-channel block;
    'dw': [cout, cin, k, k], located as (cout, cin, tap) and their 32-channel blocks; 'flat': the raw index."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if layout == "nhwc":
        got = got.permute(0, 3, 1, 2)
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if got.dtype.is_floating_point:
        g, r = got.to(F64), ref.to(F64)            # bf16 / fp16 / fp32 -> fp64 is exact
        bad = (g != r) | torch.isnan(g)
    else:
        check_integers("reference of an integer output", ref.to(F64))
        g, r = got.to(torch.int64), ref.to(torch.int64)
        bad = g != r
    idx = torch.nonzero(bad)
    out = []
    for i in idx.tolist():
        e = dict(index=tuple(i), got=g[tuple(i)].item(), ref=r[tuple(i)].item())
        if layout in ("nchw", "nhwc") and len(i) == 4:
            n, ch, y, x = i
            e.update(n=n, y=y, x=x, channel=ch, tile=(y // tile[0], x // tile[1]), cblock=ch // 32,
                     where=tile_position(y, x, got.shape[2], got.shape[3], tile))
        elif layout == "dw" and len(i) == 4:
            co, ci, ky, kx = i
            e.update(cout=co, cin=ci, tap=ky * got.shape[3] + kx, coblock=co // 32, ciblock=ci // 32)
        out.append(e)
    return len(out), out


def assert_exact(name, got, ref, layout="nchw", tile=TILE, show=8):
    """``got`` must equal ``ref`` element for element.  The message locates the first ``show`` mismatches."""
    count, bad = mismatches(got, ref, layout, tile)
    if count == 0:
        return
    lines = [f"{name}: {count} of {ref.numel()} elements differ from the float64 reference"]
    for e in bad[:show]:
        if "where" in e:
            lines.append(f"  (n={e['n']}, y={e['y']}, x={e['x']}, channel={e['channel']}): got {e['got']:g} ref {e['ref']:g}"
                         f" -- tile {e['tile']} {e['where']}; 32-channel block {e['cblock']}")
        elif "tap" in e:
            lines.append(f"  (cout={e['cout']}, cin={e['cin']}, tap={e['tap']}): got {e['got']:g} ref {e['ref']:g}"
                         f" -- cout block {e['coblock']}, cin block {e['ciblock']}")
        else:
            lines.append(f"  index {e['index']}: got {e['got']:g} ref {e['ref']:g}")
    if count > show:
        tiles = sorted({(e["n"], e["tile"], e["cblock"]) for e in bad if "where" in e})
        if tiles:
            lines.append(f"  ... (sample, tile, 32-channel block) touched: {tiles[:16]}{' ...' if len(tiles) > 16 else ''}")
    raise AssertionError("\n".join(lines))

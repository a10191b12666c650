"""Weight gradients under tight split-K workspaces (csrc/wgrad_mfma.hip, csrc/conv_direct.hip).

Every other test lets these kernels use the 256-MB default workspace, about a hundred times what they need, so the planners'
"does not fit" branches never run: the ``S > smax`` clamp of pti_conv_wgrad_mfma_partials, the shrink loop and the per-job,
per-mode slab carving of ``w4_plan``, the ``blocks /= 2`` loop of pti_wgrad_direct, and the three "workspace too small"
refusals.  Here each route gets workspaces of exactly one slab, two slabs and one float short of three (one v3 case also
eleven, where the ``S &= ~7`` rounding behind the clamp shows), and one of four bytes less than a slab.

Layout of every run (tests/bounds_util.py): ONE flat buffer as large as the extent the default plan writes for the case plus
4096 bytes, filled with the canary value; the kernel is handed a leading view of it.  A planner that miscounts a slab
stride, or a kernel that writes one slab more than planned, lands in the canary behind the view -- inside the test's own
allocation.  The view is filled once with the canary value and once with NaN: equal results show that the reduction reads
no slab the partial launch did not write.

References are float64 CPU autograd of F.conv2d on the same bf16 values; tolerances are those of test_conv_wgrad_mfma /
test_conv_wgrad_mfma_batched / test_wgrad_direct (tests/test_gpu_ops2.py, tests/test_gpu_ops.py).  No PTI_WGRAD_* knob is
touched: the routes are the defaults', checked against ops.last_kernel_name().
"""
import pytest
import torch
import torch.nn.functional as F

import bounds_util as B
from test_gpu_ops import _gn_ref, _nhwc, _r, _report

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENT, NAN = B.CANARY_F, float("nan")
BIG_SLABS = 40        # the "large" workspace of the default-extent run: more slabs than any case here has pixel tiles / 2

# name: n, cin, cout, h, w, ksize, mode, prologue, the partial kernel the default rules pick.  Shapes: small ones, most with
# a ragged edge against the 8 x 16 pixel tile, whose DEFAULT plan takes at least three splits, so that one and two slabs
# really are tighter than what the planner wants.
SINGLE = {
    "v4_pairs":     (3, 32, 32, 24, 40, 3, "s1", 0, "wgrad_mfma4_kernel<false>"),      # Cout % 64 != 0: mode 0
    "v4_two_block": (2, 32, 64, 13, 19, 3, "s1", 0, "wgrad_mfma4_kernel<true>"),       # Cout % 64 == 0, Cin % 64 != 0: mode 1
    "v6_shape_b":   (2, 64, 64, 30, 20, 3, "s1", 0, "wgrad_mfma6_kernel<W6Cfg<2,2,2>>"),   # mode 3, shape B
    "v6_shape_a":   (2, 128, 128, 16, 32, 3, "s1", 0, "wgrad_mfma6_kernel<W6Cfg<4,2,1>>"), # mode 2, shape A
    "v3_pro2_cob2": (3, 32, 64, 24, 40, 3, "s1", 2, "wgrad_mfma3_kernel<2,false>"),
    "v3_pro2_cob1": (3, 32, 32, 24, 40, 3, "s1", 2, "wgrad_mfma3_kernel<1,false>"),
    "v3_up":        (2, 32, 32, 12, 20, 3, "up", 0, "wgrad_mfma3_kernel<1,true>"),
    "v1_s2":        (3, 32, 32, 47, 39, 3, "s2", 0, "wgrad_mfma_kernel<3,2,"),
    "v1_1x1":       (3, 32, 64, 24, 40, 1, "s1", 0, "wgrad_mfma_kernel<1,1,"),
    # 80 pixel tiles: the default plan wants 20 splits, which the v3 launch rounds down to whole rounds over the 8 XCDs
    "v3_pro2_80_tiles": (4, 32, 32, 37, 53, 3, "s1", 2, "wgrad_mfma3_kernel<1,false>"),
}
# further workspace sizes, in slabs -> the splits the launch must then take: the ``S > smax`` clamp leaves 11, and the
# ``S &= ~7`` behind it makes that 8
EXTRA_SIZES = {"v3_pro2_80_tiles": {11: 8}}
_CASES, _DEFAULT = {}, {}


def _mode(ops, mode):
    return {"s1": ops.PTI_CONV_S1, "s2": ops.PTI_CONV_S2PAD, "up": ops.PTI_CONV_UP2}[mode]


def _case(ops, dev, name):
    """Inputs on the device, float64 reference gradients on the host; built once per case and never written again."""
    if name in _CASES:
        return _CASES[name]
    n, cin, cout, h, w, ks, mode, pro, _ = SINGLE[name]
    torch.manual_seed(4)
    groups, eps = 16, 1e-6
    x = _r(torch.randn(n, cin, h, w) * 1.3 + 0.2)
    gamma = 1 + 0.2 * torch.randn(cin)
    beta = 0.1 * torch.randn(cin)
    a = (_r(_gn_ref(x, groups, gamma, beta, eps, pro == 2)) if pro else x).double()
    wt = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    if mode == "s1":
        y = F.conv2d(a, wt, b, padding=ks // 2)
    elif mode == "s2":
        y = F.conv2d(F.pad(a, (0, 1, 0, 1)), wt, b, stride=2)
    else:
        y = F.conv2d(F.interpolate(a, scale_factor=2.0, mode="nearest"), wt, b, padding=1)
    dy = _r(torch.randn(y.shape))
    y.backward(dy.double())
    xd = _nhwc(x).to(dev, torch.bfloat16)
    c = dict(x=xd, dy=_nhwc(dy).to(dev, torch.bfloat16), ref_dw=wt.grad, ref_db=b.grad, shape=(cout, cin, ks, ks),
             slab=ops.L.lib().pti_conv_wgrad_workspace_bytes(cout, cin, ks, 1) // 4,
             kw=dict(ksize=ks, mode=_mode(ops, mode), prologue=pro, in_stats=ops.gn_stats(xd, groups) if pro else None,
                     gamma=gamma.to(dev) if pro else None, beta=beta.to(dev) if pro else None, groups=groups, eps=eps))
    assert c["slab"] == ks * ks * cout * cin + cout
    _CASES[name] = c
    return c


def _launch(ops, dev, c, ws, accumulate=False, outs=None):
    dw, db = outs or (torch.full(c["shape"], NAN, device=dev), torch.full(c["shape"][:1], NAN, device=dev))
    ops.conv_wgrad_mfma(c["x"], c["dy"], dw, db, accumulate=accumulate, workspace=ws, **c["kw"])
    torch.cuda.synchronize()
    return dw, db


def _parity(tag, c, dw, db, times=1):
    rel = ((dw.double().cpu() - times * c["ref_dw"]).norm() / (times * c["ref_dw"]).norm()).item()
    _report(f"{tag} dW", dw, times * c["ref_dw"], max_frac=2e-3, l2=2e-4)
    _report(f"{tag} db", db, times * c["ref_db"], max_frac=1e-4, l2=2e-5)
    return rel


def _default_plan(ops, dev, name):
    """-> (E, route): the floats the default plan writes (a workspace far larger than it wants) and its partial kernel."""
    if name in _DEFAULT:
        return _DEFAULT[name]
    c = _case(ops, dev, name)
    h = B.with_canary(dev, (BIG_SLABS * c["slab"],), F32, SENT)
    prof = []
    ops.KERNEL_PROFILE = prof          # the two-call form (partials, then reduce) records the partial kernel's name
    try:
        dw, db = _launch(ops, dev, c, h.view)
    finally:
        ops.KERNEL_PROFILE = None
    _parity(f"{name} default plan", c, dw, db)
    assert B.intact(h)
    _DEFAULT[name] = (B.extent(h.view, SENT), prof[0][0])
    print(f"[wgrad workspace] {name}: default extent E = {_DEFAULT[name][0]} floats = "
          f"{_DEFAULT[name][0] / c['slab']:g} slabs of {c['slab']}; route {_DEFAULT[name][1]}")
    return _DEFAULT[name]


def _tight(dev, floats, total, fill):
    """A view of ``floats`` floats filled with ``fill`` at the head of a canary-filled buffer of ``total`` floats + 4096
    bytes."""
    return B.with_canary(dev, (floats,), F32, fill, extra_bytes=(total - floats) * 4 + B.PAD_BYTES)


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_form_under_tight_workspaces(dev, name):
    from pti_ldm_vae_amd import ops
    c = _case(ops, dev, name)
    slab = c["slab"]
    E, route = _default_plan(ops, dev, name)
    assert SINGLE[name][8] in route.replace(" ", ""), f"{name} went down {route}"
    # conditions on the chosen shape: the default plan wants three splits or more (and was not clamped by the big workspace)
    assert E % slab == 0 and 3 <= E // slab < BIG_SLABS, f"{name}: default extent {E} floats, slab {slab}"
    if name == "v3_pro2_80_tiles":
        assert E == 16 * slab
    exact = {k * slab: v * slab for k, v in EXTRA_SIZES.get(name, {}).items()}
    for floats in (slab, 2 * slab, 3 * slab - 1) + tuple(exact):
        tag = f"{name} ws={floats / slab:.4g} slabs"
        got = []
        for fill in (SENT, NAN):
            h = _tight(dev, floats, E, fill)
            dw, db = _launch(ops, dev, c, h.view)
            wrote = B.extent(h.view, fill)
            assert wrote % slab == 0 and 0 < wrote <= floats, f"{tag}: wrote {wrote} floats (slab {slab})"
            assert wrote < E, f"{tag}: the clamp did not bind"
            assert wrote == exact.get(floats, wrote), f"{tag}: wrote {wrote / slab:g} slabs, not {exact.get(floats, 0) / slab:g}"
            assert B.intact(h), f"{tag}: the canary behind the view was overwritten"
            rel = _parity(tag, c, dw, db)
            if floats == slab and fill == SENT:
                print(f"[wgrad workspace] {name}: one slab dW relL2 = {rel:.3e} (bound 2e-4)")
            got.append((dw, db))
        dw, db = _launch(ops, dev, c, h.view)                      # a repeat with the same view, as the kernel left it
        assert B.intact(h)
        got.append((dw, db))
        for dw, db in got[1:]:
            assert torch.equal(dw, got[0][0]) and torch.equal(db, got[0][1]), f"{tag}: runs differ bitwise"
        if name == "v4_pairs" and floats == slab:                  # accumulate=True adds on top
            _launch(ops, dev, c, h.view, accumulate=True, outs=(dw, db))
            assert B.intact(h)
            _parity(f"{tag} accumulate", c, dw, db, times=2)


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_form_refuses_less_than_one_slab(dev, name):
    """One slab minus 4 bytes: PtiError before any launch (pti_conv_wgrad_mfma_partials returns at its ``S < 1`` check,
    ahead of the v4 planner and of every PTI_LAUNCH), outputs and workspace untouched."""
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd._lib import PtiError
    c = _case(ops, dev, name)
    E, _ = _default_plan(ops, dev, name)
    h = _tight(dev, c["slab"] - 1, E, SENT)
    dw, db = torch.full(c["shape"], NAN, device=dev), torch.full(c["shape"][:1], NAN, device=dev)
    with pytest.raises(PtiError, match="workspace too small"):
        ops.conv_wgrad_mfma(c["x"], c["dy"], dw, db, workspace=h.view, **c["kw"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())
    assert B.extent(h.flat, SENT) == 0


def test_harness_sees_an_overrun(dev):
    """What the canary check is for, shown without provoking anything: the kernel gets the full default-size view (every
    write is inside it), and ``intact`` asked as if the view had ended after one slab must report the rest overwritten."""
    from pti_ldm_vae_amd import ops
    name = "v4_pairs"
    c = _case(ops, dev, name)
    E, _ = _default_plan(ops, dev, name)
    h = B.with_canary(dev, (E,), F32, SENT)
    dw, db = _launch(ops, dev, c, h.view)
    _parity(f"{name} full view", c, dw, db)
    assert B.intact(h)
    assert B.extent(h.view, SENT) == E
    assert not B.intact(h, end=c["slab"])


# ---- batched form ---------------------------------------------------------------------------------------------------
BATCH_SHAPES = [(2, 32, 32, 16, 16), (1, 64, 128, 13, 19), (3, 128, 64, 24, 16), (2, 128, 128, 8, 8), (1, 32, 64, 40, 24),
                (2, 256, 256, 8, 16), (1, 64, 64, 8, 16)]      # the jobs of test_conv_wgrad_mfma_batched: several modes


def _batch(dev):
    if "batch" in _CASES:
        return _CASES["batch"]
    torch.manual_seed(41)
    ins, refs = [], []
    for n, cin, cout, h, w in BATCH_SHAPES:
        x = _r(torch.randn(n, cin, h, w) * 1.2 + 0.1)
        wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x.double(), wt, b, padding=1)
        dy = _r(torch.randn(y.shape))
        y.backward(dy.double())
        ins.append((_nhwc(x).to(dev, torch.bfloat16), _nhwc(dy).to(dev, torch.bfloat16)))
        refs.append((wt.grad, b.grad))
    _CASES["batch"] = (ins, refs)
    return _CASES["batch"]


def _batch_launch(ops, dev, ins, ws):
    jobs = [(x, dy, torch.full((dy.shape[3] * x.shape[3] * 9,), NAN, device=dev), torch.full((dy.shape[3],), NAN, device=dev))
            for x, dy in ins]
    ops.conv_wgrad_mfma_batched(jobs, workspace=ws, accumulate=False)
    torch.cuda.synchronize()
    return jobs


def test_batched_form_under_tight_workspaces(dev):
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd._lib import PtiError
    ins, refs = _batch(dev)
    slabs = [ops.L.lib().pti_conv_wgrad_workspace_bytes(cout, cin, 3, 1) // 4 for _, cin, cout, _, _ in BATCH_SHAPES]
    modes = [ops.L.lib().pti_conv_wgrad_batched_mode(n, h, w, cin, cout) for n, cin, cout, h, w in BATCH_SHAPES]
    assert len(set(modes)) >= 3 and min(modes) >= 0, modes             # the per-mode carving has something to carve
    need = sum(slabs)
    # default extent: no job can take more splits than it has 4 x 16 pixel tiles
    big = sum(sl * n * ((h + 3) // 4) * ((w + 15) // 16) for sl, (n, _, _, h, w) in zip(slabs, BATCH_SHAPES))
    hb = B.with_canary(dev, (big,), F32, SENT)
    _batch_launch(ops, dev, ins, hb.view)
    E = B.extent(hb.view, SENT)
    print(f"[wgrad workspace] batched: modes {modes}, one slab per job = {need} floats, default extent E = {E} floats")
    assert B.intact(hb) and need < E < big, (need, E, big)
    del hb
    for floats in (need, 2 * need + 1):
        total = max(E, floats)
        got = []
        for fill in (SENT, NAN):
            h = _tight(dev, floats, total, fill)
            jobs = _batch_launch(ops, dev, ins, h.view)
            wrote = B.extent(h.view, fill)
            assert need <= wrote <= floats, f"batched ws={floats}: wrote {wrote} floats"
            assert B.intact(h), f"batched ws={floats}: the canary behind the view was overwritten"
            for (n, cin, cout, hh, ww), (_, _, dw, db), (rw, rb) in zip(BATCH_SHAPES, jobs, refs):
                _report(f"batched ws={floats} [{cin}->{cout} {hh}x{ww} b{n}] dW", dw.view(cout, cin, 3, 3), rw, max_frac=2e-3, l2=2e-4)
                _report("batched db", db, rb, max_frac=1e-4, l2=2e-5)
            got.append(jobs)
        got.append(_batch_launch(ops, dev, ins, h.view))           # a repeat with the same view
        assert B.intact(h)
        for jobs in got[1:]:
            assert all(torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) for a, b in zip(jobs, got[0])), f"ws={floats}: runs differ"
    # one float short of one slab per job: refused before the first launch (the need_all check of the entry point)
    h = _tight(dev, need - 1, E, SENT)
    jobs = [(x, dy, torch.full((dy.shape[3] * x.shape[3] * 9,), NAN, device=dev), torch.full((dy.shape[3],), NAN, device=dev))
            for x, dy in ins]
    with pytest.raises(PtiError, match="workspace too small"):
        ops.conv_wgrad_mfma_batched(jobs, workspace=h.view, accumulate=False)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(j[2]).all()) and bool(torch.isnan(j[3]).all()) for j in jobs)
    assert B.extent(h.flat, SENT) == 0


# ---- the degenerate-channel weight gradient ---------------------------------------------------------------------------
DIRECT = {
    # kind, n, cw, cn, h, w, prologue.  The first two are test_wgrad_direct's: their maps have fewer than eight 8 x 16 tiles,
    # so the default plan is ONE block and half of it must be refused; the third has 24 tiles = 6 blocks, which the
    # halving loop takes to 3 and then to 1.
    "fewcout_128x4": ("fewcout", 2, 128, 4, 8, 8, 1),
    "fewcin_64x3":   ("fewcin", 1, 64, 3, 10, 12, 0),
    "fewcin_32x3_24_tiles": ("fewcin", 2, 32, 3, 32, 48, 0),
}


def _direct_case(ops, dev, name):
    if name in _CASES:
        return _CASES[name]
    kind, n, cw, cn, h, w, pro = DIRECT[name]
    torch.manual_seed(3)
    groups, eps = 16, 1e-6
    gamma = 1 + 0.2 * torch.randn(cw)
    beta = 0.1 * torch.randn(cw)
    if kind == "fewcout":   # y[cn] = conv(P(x[cw])), wide = x, narrow = dY
        x = _r(torch.randn(n, cw, h, w) + 0.2)
        wt = torch.zeros(cn, cw, 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cn, dtype=torch.float64, requires_grad=True)
        a = _gn_ref(x, groups, gamma, beta, eps, pro == 2) if pro else x
        dy = torch.randn(n, cn, h, w)
        F.conv2d(a.double(), wt, b, padding=1).backward(dy.double())
        wide = _nhwc(x).to(dev, torch.bfloat16)
        kw = dict(sgn=1, dw_strides=(1, 9, cw * 9), prologue=pro, in_stats=ops.gn_stats(wide, groups) if pro else None,
                  gamma=gamma.to(dev) if pro else None, beta=beta.to(dev) if pro else None, groups=groups, eps=eps)
        c = dict(wide=wide, narrow=dy.to(dev), dw_shape=(cn, cw, 3, 3), db_len=cn, db_arg="dbias_narrow", kw=kw)
    else:                   # y[cw] = conv(x[cn]), wide = dY (bf16), narrow = x
        x = torch.randn(n, cn, h, w)
        wt = torch.zeros(cw, cn, 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cw, dtype=torch.float64, requires_grad=True)
        dy = _r(torch.randn(n, cw, h, w))
        F.conv2d(x.double(), wt, b, padding=1).backward(dy.double())
        c = dict(wide=_nhwc(dy).to(dev, torch.bfloat16), narrow=x.to(dev), dw_shape=(cw, cn, 3, 3), db_len=cw,
                 db_arg="dbias_wide", kw=dict(sgn=-1, dw_strides=(1, cn * 9, 9)))
    c.update(ref_dw=wt.grad, ref_db=b.grad, block=cn * (80 * (cw // 8) + 1), pro=pro,
             dims=dict(n=n, h=h, w=w, cw=cw, cn=cn, ksize=3, narrow_layout="nchw"))
    _CASES[name] = c
    return c


def _direct_launch(ops, dev, c, ws):
    dw, db = torch.zeros(c["dw_shape"], device=dev), torch.zeros(c["db_len"], device=dev)      # the call adds to them
    ops.wgrad_direct(c["wide"], c["narrow"], dw, workspace=ws, **{c["db_arg"]: db}, **c["dims"], **c["kw"])
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("name", list(DIRECT))
def test_wgrad_direct_under_tight_workspaces(dev, name):
    """The partials of pti_wgrad_direct take cn * (80 * (cw / 8) + 1) floats per block (include/pti_vae.h).  A workspace
    of at least one block's worth must do (fewer blocks, same sums); anything less must be refused with nothing touched."""
    from pti_ldm_vae_amd import ops
    from pti_ldm_vae_amd._lib import PtiError
    c = _direct_case(ops, dev, name)
    block = c["block"]
    hb = B.with_canary(dev, (64 * block,), F32, SENT)
    _direct_launch(ops, dev, c, hb.view)
    E = B.extent(hb.view, SENT)
    print(f"[wgrad workspace] wgrad_direct {name}: default extent E = {E} floats = {E / block:g} blocks of {block}")
    assert B.intact(hb) and E % block == 0 and block <= E < 64 * block
    if name == "fewcin_32x3_24_tiles":
        assert E == 6 * block
    del hb
    tol_w = dict(max_frac=2e-3, l2=1e-3) if c["pro"] else dict(max_frac=1e-4, l2=2e-5)
    for floats in sorted({E, E // 2, block, block - 1}, reverse=True):
        tag = f"wgrad_direct {name} ws={floats / block:.4g} blocks"
        if floats < block:
            h = _tight(dev, floats, E, SENT)
            dw, db = torch.full(c["dw_shape"], NAN, device=dev), torch.full((c["db_len"],), NAN, device=dev)
            with pytest.raises(PtiError, match="workspace too small"):
                ops.wgrad_direct(c["wide"], c["narrow"], dw, workspace=h.view, **{c["db_arg"]: db}, **c["dims"], **c["kw"])
            torch.cuda.synchronize()
            assert B.extent(h.flat, SENT) == 0, f"{tag}: the refused call wrote to the workspace"
            assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), f"{tag}: the refused call wrote an output"
            continue
        got = []
        for fill in (SENT, NAN):
            h = _tight(dev, floats, E, fill)
            dw, db = _direct_launch(ops, dev, c, h.view)
            wrote = B.extent(h.view, fill)
            assert wrote % block == 0 and 0 < wrote <= floats, f"{tag}: wrote {wrote} floats"
            assert B.intact(h), f"{tag}: the canary behind the view was overwritten"
            _report(f"{tag} dW", dw, c["ref_dw"], **tol_w)
            _report(f"{tag} db", db, c["ref_db"], max_frac=1e-4, l2=2e-5)
            got.append((dw, db))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), f"{tag}: runs differ bitwise"

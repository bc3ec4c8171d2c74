"""GPU: the packed rendering passes (csrc/segscan.hip) at the edges of opacity's range and on non-finite rays.

The other tests of these passes are thorough about shape and draw mid-range values.  Here the shapes are the few thousand
samples of ``render_edges_reference.edge_counts()`` and the values are the edges a trained field reaches:

1. saturation: ``sigma * delta`` of 88, 104, 1e4 and +inf (``alpha == 1`` and ``T == 0`` behind it, exactly), against the
   float64 CLOSED forms of tests/render_edges_reference.py -- autograd over a ``cumprod`` is not the contract at
   ``alpha == 1`` (the backward divides by ``max(1 - alpha, 1e-10)``), see tests/test_render_edges_cpu.py;
2. vanishing opacity and the clamp of ``rendering``'s depth normalisation;
3. thresholds: exact ties of the alpha path, and the visibility pass's exp-free band around ``-ln(early_stop_eps)``;
4. containment: one non-finite sample costs its own ray and nothing else.

Tolerances are ``seg_reference.bound`` plus the TINY floor of the variant tests; tests/test_render_edges_cpu.py shows the
float32 torch composition of the reference alone stays within half of them.  An "exact zero behind a saturating sample"
is asserted where float64 ``exp(-S)`` is below 2^-151, a quarter of float32's smallest subnormal: an ``expf`` whose
unrounded result is off by less than a factor 2 must round that to 0.  (S = 104 alone, exp(-104) = 0.486 of the smallest
subnormal, sits too close to the rounding boundary at one half and is held to the TINY floor instead.)

One expectation deliberately differs from a naive reading of "a ray of zeros has zero gradients through depth": with
opacity below eps the depth is ``sum w mid / eps``, whose derivative w.r.t. a zero density is ``g_depth mid delta / eps``,
not 0.  What IS exactly 0 below eps is opacity's share of the normalisation's gradient; both are asserted as they are.
"""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import nerfacc_amd as na
import render_edges_reference as ER
import seg_reference as SR
from nerfacc_amd import _backend as B
from nerfacc_amd import volrend
from nerfacc_amd._segments import seginfo_from_packed, seginfo_from_ray_indices
from test_kernel_variants_gpu import CallLog, check, d64, grads_like, run_pair, shifted

pytestmark = pytest.mark.gpu

WHERE = ("first", "middle", "last")
DEAD = 2.0 ** -151


def finite(**named):
    for k, t in named.items():
        assert bool(torch.isfinite(t).all()), (k, int((~torch.isfinite(t)).sum()))


def zeros_at(rows, **named):
    for k, t in named.items():
        assert bool((t[rows] == 0).all()), (k, int((t[rows] != 0).sum()))


@lru_cache(None)
def _sat(where: str, devname: str, R: int = 0, S: int = 0):
    """The saturating case on the device with its float64 forward (shared, never modified)."""
    dev = torch.device(devname)
    counts = torch.full((R,), S, dtype=torch.int64) if R else ER.edge_counts()
    c = ER.saturating(counts, where, seed=20 + WHERE.index(where))
    rays = SR.Rays(counts.to(dev))
    ts, te, sig = (c[k].to(dev) for k in ("t_starts", "t_ends", "sigmas"))
    ts64, te64, sig64 = d64(ts, te, sig)
    w64, T64, a64, x64 = ER.density_forward(rays, ts64, te64, sig64)
    S64 = rays.unpad(SR.excl_sum_rows(rays.pad(x64)))
    g = torch.Generator().manual_seed(77)
    return {"rays": rays, "ri": rays.ray_ids.clone(), "ts": ts, "te": te, "sig": sig, "ts64": ts64, "te64": te64, "sig64": sig64,
            "w64": w64, "T64": T64, "a64": a64, "dead": torch.exp(-S64) < DEAD, "inf": torch.isinf(sig),
            "sat": c["sat"].to(dev), "rgb": torch.rand(rays.n, 3, generator=g).to(dev)}


def sat_case(dev, where, R=0, S=0):
    return _sat(where, str(dev), R, S)


def float32_alphas(c):
    """The alphas of the alpha path: the float32 results of the density pass, so that alpha == 1 occurs exactly."""
    rays = c["rays"]
    with torch.no_grad():
        al = na.render_weight_from_density(c["ts"], c["te"], c["sig"], ray_indices=c["ri"], n_rays=rays.R)[2]
    sat = c["sat"][c["sat"] >= 0]
    assert bool((al[sat] == 1.0).all())
    return al.clone()


# ============================================================================= 1: saturation
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("fn", ["weight", "transmittance"])
def test_saturation_from_density(dev, monkeypatch, where, fn):
    c = sat_case(dev, where)
    rays, ri, ts, te, sig = (c[k] for k in ("rays", "ri", "ts", "te", "sig"))
    R, full = rays.R, fn == "weight"
    api = na.render_weight_from_density if full else na.render_transmittance_from_density
    f = lambda a, b, s: api(a, b, s, ray_indices=ri, n_rays=R)
    gin = grads_like([sig] * (3 if full else 2), 31)
    log = CallLog(monkeypatch)
    outs, (g_sig,) = run_pair(f, [ts, te, sig], [False, False, True], lambda o: gin, log,
                              ["nfa_render_from_density_fwd", "nfa_render_from_density_bwd"])
    gw, gt, ga = d64(*(gin if full else [None] + gin))
    w, T, a = outs if full else [None] + outs
    ts64, te64, sig64, w64, T64, a64 = (c[k] for k in ("ts64", "te64", "sig64", "w64", "T64", "a64"))
    _, gs64 = ER.density_backward(rays, ts64, te64, T64, a64, gw, gt, ga)
    s_w, s_t, s_a, s_gx = ER.density_scales(rays, ts64, te64, sig64, T64, a64, gw, gt, ga)
    finite(trans=T, alphas=a, g_sigmas=g_sig)
    check("trans", T, T64, SR.bound(rays, s_t))
    check("alphas", a, a64, SR.bound(rays, s_a))
    check("g_sigmas", g_sig, gs64, SR.bound(rays, s_gx * (te64 - ts64).abs()))
    zeros_at(c["dead"], trans=T)
    assert bool((a[c["inf"]] == 1.0).all()) and int(c["inf"].sum()) >= 5 and int(c["dead"].sum()) > 100
    if full:
        finite(weights=w)
        check("weights", w, w64, SR.bound(rays, s_w))
        zeros_at(c["dead"], weights=w)
        assert torch.equal(w[c["inf"]], T[c["inf"]])
    # no gradient arriving at alphas (an alpha behind the saturating sample still depends on its own density): every
    # gradient w.r.t. a density behind it is an exact zero, and the +inf sample's own is finite
    s = sig.clone().requires_grad_(True)
    o = f(ts, te, s)
    (g2,) = torch.autograd.grad(o[:-1], s, gin[:-1])
    finite(g_sigmas=g2)
    zeros_at(c["dead"], g_sigmas=g2)


@pytest.mark.parametrize("where", WHERE)
def test_saturation_from_alpha(dev, monkeypatch, where):
    c = sat_case(dev, where)
    rays, ri = c["rays"], c["ri"]
    al = float32_alphas(c)
    one = al == 1.0
    gin = grads_like([al] * 2, 32)
    log = CallLog(monkeypatch)
    (w, T), (g_al,) = run_pair(lambda a: na.render_weight_from_alpha(a, ray_indices=ri, n_rays=rays.R), [al], [True],
                               lambda o: gin, log, ["nfa_render_from_alpha_fwd", "nfa_render_from_alpha_bwd"])
    al64, gw, gt = d64(al, *gin)
    w64, T64 = ER.alpha_forward(rays, al64)
    ga64 = ER.alpha_backward(rays, al64, T64, gw, gt)
    s_w, s_t, s_g = ER.alpha_scales(rays, al64, T64, gw, gt)
    finite(weights=w, trans=T, g_alphas=g_al)
    check("weights", w, w64, SR.bound(rays, s_w))
    check("trans", T, T64, SR.bound(rays, s_t))
    check("g_alphas", g_al, ga64, SR.bound(rays, s_g))
    dead = T64 == 0
    assert where == "last" or int(dead.sum()) > 100
    zeros_at(dead, weights=w, trans=T, g_alphas=g_al)
    assert torch.equal(w[one], T[one])
    assert torch.equal(g_al[one], (gin[0] * T)[one])        # the clamped form at alpha == 1: g_w T - 0 / 1e-10
    # transmittance alone: the same bits, and its gradient (only g_T arrives)
    x = al.clone().requires_grad_(True)
    T2 = na.render_transmittance_from_alpha(x, ray_indices=ri, n_rays=rays.R)
    (g2,) = torch.autograd.grad(T2, x, gin[1])
    assert torch.equal(T2.detach(), T)
    finite(g_alphas=g2)
    check("g_alphas (trans)", g2, ER.alpha_backward(rays, al64, T64, None, gt), SR.bound(rays, ER.alpha_scales(rays, al64, T64, None, gt)[2]))
    zeros_at(dead, g_alphas=g2)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", ["inclusive_sum", "exclusive_sum", "inclusive_prod", "exclusive_prod"])
def test_saturation_scans(dev, monkeypatch, where, kind):
    c = sat_case(dev, where)
    rays = c["rays"]
    prod = kind.endswith("prod")
    x = (1.0 - float32_alphas(c)) if prod else c["sig"] * (c["te"] - c["ts"])     # exact zeros / +inf at the saturating samples
    pi = rays.packed_info()
    gin = grads_like([x], 33)
    log = CallLog(monkeypatch)
    (y,), (gx,) = run_pair(lambda a: (getattr(na, kind)(a, pi),), [x], [True], lambda o: gin, log,
                           ["nfa_packed_scan"] + (["nfa_packed_prod_backward"] if prod else []))
    x64, g64 = d64(x, gin[0])
    y64 = SR.scan(rays, x64, kind)
    finite(grad=gx)
    if prod:
        s_f, s_b = ER.prod_scales(rays, x64, y64, g64, kind)
        want_g = ER.prod_backward(rays, x64, y64, g64, kind)
        finite(y=y)
        zeros_at(y64 == 0, y=y)
    else:
        s_f, s_b = SR.scan_scales(rays, x64, y64, g64, kind)
        want_g = ER._suffix(rays, g64, kind.startswith("inclusive"))
    ok = torch.isfinite(y64)
    assert torch.equal(y[~ok].double(), y64[~ok])        # a sum behind +inf is +inf
    assert kind != "inclusive_sum" or int((~ok).sum()) >= 5
    check("y", y[ok], y64[ok], SR.bound(rays, s_f)[ok])
    check("grad", gx, want_g, SR.bound(rays, s_b))


def _render(mode, c, field, rgb, gl, fuse=True):
    """na.rendering on aligned and shifted views (bit-identical); returns the outputs as a dict and (g_field, g_rgb)."""
    rays, ri, ts, te = c["rays"], c["ri"], c["ts"], c["te"]
    dens, extras = mode.startswith("sigma"), not mode.endswith("colors")

    def fn(a, b, f, col):
        cb = (lambda *_: (col, f))
        kw = {"rgb_sigma_fn": cb} if dens else {"rgb_alpha_fn": cb}
        colors, opac, depth, ex = na.rendering(a, b, ri, n_rays=rays.R, **kw)
        return (colors, opac, depth) + ((ex["weights"], ex["trans"]) + ((ex["alphas"],) if dens else ()) if extras else ())

    n_out = 3 + (0 if not extras else (3 if dens else 2))
    saved = volrend.FUSE_RENDERING
    volrend.FUSE_RENDERING = fuse
    try:
        res = []
        for unaligned in (False, True):
            sh = (lambda t, k: shifted(t, k)) if unaligned else (lambda t, k: t.detach().clone())
            f, col = sh(field, 2).requires_grad_(True), sh(rgb, 1).requires_grad_(True)
            outs = fn(sh(ts, 1), sh(te, 3), f, col)
            pairs = [(o, sh(g, 1 + j % 3)) for j, (o, g) in enumerate(zip(outs, gl[:n_out])) if g is not None]
            grads = torch.autograd.grad([o for o, _ in pairs], [f, col], [g for _, g in pairs])
            res.append(([o.detach() for o in outs], grads))
    finally:
        volrend.FUSE_RENDERING = saved
    for a, b in zip(res[0][0] + list(res[0][1]), res[1][0] + list(res[1][1])):
        assert torch.equal(a, b)
    names = ("colors", "opacities", "depths", "weights", "trans", "alphas")
    return dict(zip(names, res[0][0])), res[0][1]


def _render_grads(rays, dev, seed, extras, dens):
    g = torch.Generator().manual_seed(seed)
    gl = [torch.randn(rays.R, 3, generator=g), torch.randn(rays.R, 1, generator=g), torch.randn(rays.R, 1, generator=g)]
    gl += [torch.randn(rays.n, generator=g) for _ in range((3 if dens else 2) if extras else 0)]
    return [x.to(dev) for x in gl]


def _check_rendering(c, dens, field, rgb, gl, outs, grads):
    rays = c["rays"]
    ex = tuple(d64(*(gl[3:] + [None] * 3)[:3]))
    ref = ER.rendering_reference(rays, c["ts64"], c["te64"], field.double(), rgb.double(), dens, *d64(*gl[:3]), ex,
                                 opac_own=outs["opacities"], depth_own=outs["depths"])
    got = dict(outs, g_field=grads[0], g_rgbs=grads[1])
    for k, t in got.items():
        finite(**{k: t})
        check(k, t, *ref[k])
    return ref


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("mode", ["sigma_extras", "sigma_colors", "sigma_two_pass", "alpha_extras"])
def test_saturation_rendering(dev, monkeypatch, where, mode):
    c = sat_case(dev, where)
    rays, rgb = c["rays"], c["rgb"]
    dens, fuse = mode.startswith("sigma"), mode != "sigma_two_pass"
    field = c["sig"] if dens else float32_alphas(c)
    gl = _render_grads(rays, dev, 34, not mode.endswith("colors"), dens)
    log = CallLog(monkeypatch)
    outs, grads = _render(mode, c, field, rgb, gl, fuse)
    log.assert_scalar_form(*(["nfa_render_fused_fwd", "nfa_render_fused_bwd"] if dens and fuse else
                             ["nfa_render_from_density_fwd" if dens else "nfa_render_from_alpha_fwd", "nfa_render_accumulate_fwd",
                              "nfa_render_accumulate_bwd"]))
    _check_rendering(c, dens, field, rgb, gl, outs, grads)
    dead = c["dead"] if dens else ER.alpha_forward(rays, field.double())[1] == 0
    zeros_at(dead, g_rgbs=grads[1])
    if "weights" in outs:
        zeros_at(dead, weights=outs["weights"], trans=outs["trans"])
        sat1 = c["inf"] if dens else field == 1.0
        assert torch.equal(outs["weights"][sat1], outs["trans"][sat1])
    if mode == "sigma_two_pass":     # the one-pass form computes the same bits
        fused, _ = _render("sigma_extras", c, field, rgb, gl, True)
        for k, t in outs.items():
            assert torch.equal(t, fused[k]), k


@pytest.mark.parametrize("where", WHERE)
def test_saturation_const_step_entries(dev, where):
    """The `_cs` entries (t_ends formed as t_starts + step) against their siblings that load it, on saturating densities:
    bit-identical, and the forward equals rendering()'s outputs, which test_saturation_rendering holds to float64."""
    c = sat_case(dev, where)
    rays, ts, te, sig, rgb = (c[k] for k in ("rays", "ts", "te", "sig", "rgb"))
    n, R, step = rays.n, rays.R, ER.DELTA
    assert torch.equal(ts + torch.tensor(step, dtype=torch.float32, device=dev), te)
    seg = seginfo_from_ray_indices(c["ri"], R)
    tail = (B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, R, n)
    new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)

    def forward(name, second):
        out = [new(n), new(n), new(n), new(R, 3), new(R), new(R)]
        B.call(name, B.ptr(ts), second, B.ptr(sig), B.ptr(rgb), *tail, *(B.ptr(t) for t in out), B.stream())
        return out

    fa, fb = forward("nfa_render_fused_fwd_cs", step), forward("nfa_render_fused_fwd", B.ptr(te))
    for x, y in zip(fa, fb):
        assert torch.equal(x, y)
    with torch.no_grad():
        colors, opac, _, ex = na.rendering(ts, te, c["ri"], n_rays=R, rgb_sigma_fn=lambda *_: (rgb, sig))
    for x, y in zip(fa[:5], (ex["weights"], ex["trans"], ex["alphas"], colors, opac[:, 0])):
        assert torch.equal(x, y)
    gl = _render_grads(rays, dev, 35, True, True)
    grads = [gl[0], gl[1][:, 0].contiguous(), gl[2][:, 0].contiguous()] + gl[3:]

    def backward(name, second):
        out = [new(n), new(n, 3)]
        B.call(name, B.ptr(ts), second, B.ptr(rgb), B.ptr(fa[1]), B.ptr(fa[2]), *(B.ptr(t) for t in grads), *tail,
               *(B.ptr(t) for t in out), B.stream())
        return out

    ba, bb = backward("nfa_render_fused_bwd_cs", step), backward("nfa_render_fused_bwd", B.ptr(te))
    assert torch.equal(ba[0], bb[0]) and torch.equal(ba[1], bb[1])
    finite(g_sigmas=ba[0], g_rgbs=ba[1])
    for thre in (0.0, 0.01):
        va = volrend._visibility_native(seg, ts, te, sig, None, 1e-4, thre, want_counts=True, step=step)
        vb = volrend._visibility_native(seg, ts, te, sig, None, 1e-4, thre, want_counts=True)
        assert torch.equal(va[0], vb[0]) and torch.equal(va[1], vb[1])
        want = (c["T64"] >= ER.eps32(1e-4)) & (c["a64"] >= ER.eps32(thre))     # (no class has its alpha near 0.01)
        # a sample is near the threshold when its sum S is within the float32 sum's error (plus expf's rounding) of -ln(eps)
        S = rays.unpad(SR.excl_sum_rows(rays.pad((c["sig64"] * ER.DELTA).clamp_max(ER.X_SAT32))))
        near = (S + math.log(ER.eps32(1e-4))).abs() <= SR.bound(rays, 1.0 + S)
        assert int(near.sum()) < 8 and torch.equal(va[0][~near], want[~near])
        assert not bool(va[0][c["dead"]].any())


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("alpha_thre", [0.0, 0.01])
def test_saturation_render_step_accumulate(dev, monkeypatch, where, alpha_thre):
    from nerfacc_amd import marching
    c = sat_case(dev, where)
    rays, ri, ts, te, sig, rgbs = (c[k] for k in ("rays", "ri", "ts", "te", "sig", "rgb"))
    R = rays.R
    g = torch.Generator().manual_seed(36)
    c0 = torch.rand(R, 3, generator=g).to(dev)
    o0 = (torch.rand(R, 1, generator=g) * 0.5).to(dev)
    d0 = torch.rand(R, 1, generator=g).to(dev)
    seg = seginfo_from_ray_indices(ri, R)
    log = CallLog(monkeypatch)
    res = []
    for k in (0, 1):
        sh = (lambda t, j: shifted(t, j)) if k else (lambda t, j: t.clone())
        co, o, d = c0.clone(), o0.clone(), d0.clone()
        nv = torch.zeros(marching._VISIBLE_SLOTS, dtype=torch.int64, device=dev) if alpha_thre > 0 else None
        marching._render_step_native(seg, sh(ts, 1), sh(te, 3), sh(sig, 2), sh(rgbs, 1), alpha_thre, co, o, d, nv)
        res.append((co, o, d, None if nv is None else int(nv.sum())))
    for a, b in zip(res[0], res[1]):
        assert (a == b) if not torch.is_tensor(a) else torch.equal(a, b)
    log.assert_scalar_form("nfa_render_step_accumulate")
    co, o, d, nv = res[0]
    finite(colors=co, opacity=o, depth=d)
    ts64, te64, sig64, rgb64, o64 = c["ts64"], c["te64"], c["sig64"], rgbs.double(), o0.double()
    dc, do, dd, keep = SR.render_step(rays, ts64, te64, sig64, rgb64, o64[:, 0], alpha_thre)
    _, T, a = SR.from_density(rays, ts64, te64, sig64, 1.0 - o64[ri, 0])
    s_w, _, s_a, _ = ER.density_scales(rays, ts64, te64, sig64, T, a)
    near = (a - alpha_thre).abs() <= SR.bound(rays, s_a) + ER.TINY if alpha_thre > 0 else torch.zeros_like(keep)
    assert not bool(near.any())       # no class of the generator has its alpha at the threshold
    sw1 = torch.where(keep, s_w + T * a, torch.zeros_like(s_w))
    mid = ((ts64 + te64) / 2.0).abs()
    for name, got, base, inc, sc in (("colors", co, c0, dc, SR.accumulate(rays, sw1, rgb64.abs())),
                                     ("opacity", o, o0, do, SR.accumulate(rays, sw1)),
                                     ("depth", d, d0, dd, SR.accumulate(rays, sw1, mid[:, None]))):
        check(name, got, base.double() + inc, SR.bound(rays, sc + base.double().abs(), per_ray=True, extra=1))
    if alpha_thre > 0:
        assert nv == int(keep.sum())


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("R,S", [(37, 65), (3, 257)])
def test_saturation_cdf_rows(dev, monkeypatch, where, R, S):
    from nerfacc_amd.estimators import prop_net as PN
    c = sat_case(dev, where, R, S)
    rays = c["rays"]
    ts, te, sg = (c[k].view(R, S) for k in ("ts", "te", "sig"))
    gin = [torch.randn(R, S + 1, generator=torch.Generator().manual_seed(37)).to(dev)]
    log = CallLog(monkeypatch)
    (cd,), (g_sig,) = run_pair(lambda a, b, s: (PN._cdfs_from_density(a, b, s),), [ts, te, sg], [False, False, True],
                               lambda o: gin, log, ["nfa_density_cdf_rows_fwd", "nfa_density_cdf_rows_bwd"])
    ts64, te64, sig64, T64 = c["ts64"], c["te64"], c["sig64"], c["T64"]
    gt = -gin[0].double()[:, :S].reshape(-1)
    _, gs64 = ER.density_backward(rays, ts64, te64, T64, torch.zeros_like(T64), None, gt, None)
    _, s_t, _, s_gx = ER.density_scales(rays, ts64, te64, sig64, T64, torch.zeros_like(T64), gt=gt)
    finite(cdfs=cd, g_sigmas=g_sig)
    check("cdfs", cd[:, :S].reshape(-1), 1.0 - T64, SR.bound(rays, s_t + (1.0 - T64)))
    assert bool((cd[:, S] == 1.0).all()) and bool((cd[:, :S].reshape(-1)[c["dead"]] == 1.0).all())
    check("g_sigmas", g_sig.reshape(-1), gs64, SR.bound(rays, s_gx * (te64 - ts64).abs()))
    zeros_at(c["dead"], g_sigmas=g_sig.reshape(-1))


# ============================================================================= 2: vanishing opacity, the depth clamp
@lru_cache(None)
def _van(devname: str):
    dev = torch.device(devname)
    v = ER.vanishing(ER.edge_counts(), seed=40)
    rays = SR.Rays(v["rays"].counts.to(dev))
    c = {"rays": rays, "ri": rays.ray_ids.clone(), "ts": v["t_starts"].to(dev), "te": v["t_ends"].to(dev), "sig": v["sigmas"].to(dev),
         "al": v["alphas"].to(dev), "rgb": v["rgbs"].to(dev), "kind": v["kind"].to(dev), "cls": v["cls"].to(dev)}
    c["ts64"], c["te64"] = d64(c["ts"], c["te"])
    return c


@pytest.mark.parametrize("mode", ["sigma_extras", "alpha_extras"])
def test_vanishing_opacity_and_depth_clamp(dev, mode):
    c = _van(str(dev))
    rays, rgb, kind = c["rays"], c["rgb"], c["kind"]
    dens = mode.startswith("sigma")
    field = c["sig"] if dens else c["al"]
    K = {k: kind == i for i, k in enumerate(ER.VANISHING)}
    gl = _render_grads(rays, dev, 41, False, dens)
    outs, grads = _render(mode, c, field, rgb, gl)
    ref = _check_rendering(c, dens, field, rgb, gl, outs, grads)
    opac, depth, colors = outs["opacities"], outs["depths"], outs["colors"]
    # rays of zeros (and of +-0 alphas / densities whose float32 alpha is exactly 0): exact zeros out
    for k in ("zeros", "neg_zeros", "total_0"):
        zeros_at(K[k], opacities=opac, depths=depth, colors=colors)
        zeros_at(K[k][rays.ray_ids], weights=outs["weights"], g_rgbs=grads[1])
    if not dens:     # the alpha path hits the five targets exactly
        for k, target in ER.OPACITY_TARGETS.items():
            assert bool((opac[K[k], 0] == float(np.float32(target))).all()), k
        below = K["total_subnormal"] | K["total_below_eps"] | K["subnormal"]
        assert bool((opac[below, 0] < ER.EPS_DEPTH).all()) and bool((opac[below, 0] > 0).all())
        assert bool((opac[K["total_eps"] | K["total_above_eps"], 0] >= ER.EPS_DEPTH).all())
    # only the depth's gradient arrives: within the bound of the clamped restatement, and opacity's share of the
    # normalisation is exactly 0 wherever the product's own opacity is below eps
    z = torch.zeros_like
    gd = [z(gl[0]), z(gl[1]), gl[2]]
    _, grads_d = _render(mode.replace("extras", "colors"), c, field, rgb, gd)
    ref_d = _check_rendering(c, dens, field, rgb, gd, {k: outs[k] for k in ("colors", "opacities", "depths")}, grads_d)
    share = ref_d["share"][0]
    lo = opac.double() < ER.EPS_DEPTH
    assert bool((share[lo] == 0).all()) and int(lo.sum()) > 20
    hi = ~lo & (depth != 0)
    assert bool((share[hi] != 0).all()) and (dens or int((hi[:, 0] & (K["total_eps"] | K["total_above_eps"])).sum()) >= 4)
    zeros_at(K["zeros"][rays.ray_ids] | K["neg_zeros"][rays.ray_ids], g_rgbs=grads_d[1])
    # -0.0 in place of +0.0: no NaN (checked above), the same values in those rays, the same BITS in every other ray
    plus = torch.where(field == 0, z(field), field)
    assert bool(torch.signbit(field).any()) and not bool(torch.signbit(plus).any())
    outs_p, grads_p = _render(mode, c, plus, rgb, gl)
    other = ~K["neg_zeros"]
    for k in outs:
        rows = other if outs[k].shape[0] == rays.R else other[rays.ray_ids]
        assert torch.equal(outs[k][rows], outs_p[k][rows]), k
        assert bool((outs[k][~rows] == outs_p[k][~rows]).all()), k
    for a, b in zip(grads, grads_p):
        assert torch.equal(a[other[rays.ray_ids]], b[other[rays.ray_ids]]) and bool((a == b).all())
    del ref


# ============================================================================= 3: thresholds
def _compact(seg, vis, cnt, ts, te, dev):
    R, n = seg.n_rays, vis.numel()
    m = int(cnt.sum())
    st = torch.cumsum(cnt, 0) - cnt
    o_ri = torch.full((m,), -1, dtype=torch.int64, device=dev)
    o_ts, o_te = torch.full((m,), -1.0, device=dev), torch.full((m,), -1.0, device=dev)
    B.call("nfa_compact_samples", B.ptr(vis), B.ptr(ts), B.ptr(te), B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles,
           B.ptr(st), R, n, B.ptr(o_ri), B.ptr(o_ts), B.ptr(o_te), m, B.stream())
    return o_ri, o_ts, o_te


@pytest.mark.parametrize("k", [1, 13, 64, 126, 140])
def test_alpha_path_exact_ties_of_the_transmittance(dev, k):
    """alpha = 0.5 everywhere: T = 2^-i exactly at the ray's i-th sample, so with early_stop_eps = 2^-k sample k is visible
    and sample k + 1 is not (2^-140 is a subnormal threshold)."""
    counts = torch.tensor([150, 3, 0, 149, 257, 1], dtype=torch.int64)
    rays = SR.Rays(counts.to(dev))
    n = rays.n
    al = torch.full((n,), 0.5, device=dev)
    ts = torch.arange(n, device=dev, dtype=torch.float32)
    te = ts + 0.5
    seg = seginfo_from_packed(rays.packed_info(), n)
    idx = torch.arange(n, device=dev) - rays.starts[rays.ray_ids]
    want = idx <= k
    for pf in (None, torch.ones(n, device=dev)):
        vis, cnt = volrend._visibility_native(seg, None, None, al, pf, 2.0 ** -k, 0.0, want_counts=True)
        assert torch.equal(vis, want)
        assert torch.equal(cnt, rays.counts.clamp_max(k + 1))
    assert torch.equal(na.render_visibility_from_alpha(al, packed_info=rays.packed_info(), early_stop_eps=2.0 ** -k), want)
    o_ri, o_ts, o_te = _compact(seg, vis, cnt, ts, te, dev)
    assert torch.equal(o_ri, rays.ray_ids[want]) and torch.equal(o_ts, ts[want]) and torch.equal(o_te, te[want])


def test_alpha_path_exact_tie_of_alpha_thre(dev):
    counts = ER.edge_counts()
    rays = SR.Rays(counts.to(dev))
    n = rays.n
    thre = float(np.float32(0.3))
    below = float(np.nextafter(np.float32(0.3), np.float32(0)))
    pick = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(50))
    al = torch.tensor([thre, below, 0.0], dtype=torch.float32)[pick].to(dev)
    seg = seginfo_from_packed(rays.packed_info(), n)
    want = (pick == 0).to(dev)
    vis, cnt = volrend._visibility_native(seg, None, None, al, None, 0.0, thre, want_counts=True)
    assert torch.equal(vis, want) and bool(want.any())
    assert torch.equal(cnt, torch.zeros_like(cnt).index_add_(0, rays.ray_ids, want.long()))
    ts = torch.rand(n, generator=torch.Generator().manual_seed(51)).to(dev)
    o_ri, o_ts, o_te = _compact(seg, vis, cnt, ts, ts + 1, dev)
    assert torch.equal(o_ri, rays.ray_ids[want]) and torch.equal(o_ts, ts[want]) and torch.equal(o_te, (ts + 1)[want])
    # density path: the same tie on alpha = 1 - exp(-x) is decided on the float32 alphas the passes compute themselves
    c = sat_case(dev, "middle")
    a32 = float32_alphas(c)
    t = float(a32[a32 > 0].median())
    seg = seginfo_from_ray_indices(c["ri"], c["rays"].R)
    v = volrend._visibility_native(seg, c["ts"], c["te"], c["sig"], None, 0.0, t)
    assert torch.equal(v, a32 >= t)
    v = volrend._visibility_native(seg, c["ts"], c["te"], c["sig"], None, 0.0, float(np.nextafter(np.float32(t), np.float32(1))))
    assert torch.equal(v, a32 > t)


@pytest.mark.parametrize("lead", [0, 300])
@pytest.mark.parametrize("eps", ER.EARLY_STOP_EPS)
def test_density_path_threshold_band(dev, eps, lead):
    """The visibility pass decides T >= early_stop_eps on the sum S outside a band around -ln(eps) and evaluates expf inside.
    (a) With prefix_trans = ones the pass evaluates the same expf at every sample: masks and counts must be bit-identical.
    (b) Both agree with float64 exp(-S) >= eps except on the few probes within 8 * 2^-24 relative of eps (normal eps only).
    (c) The constant-step entry gives the same mask.  lead = 300: S reaches the probed sample through the step carry."""
    S = ER.threshold_sweeps(eps)
    p = ER.probe_rays(S, lead)
    counts, probe = p["counts"].to(dev), p["probe"].to(dev)
    ts, te, sig = (p[k].to(dev) for k in ("t_starts", "t_ends", "sigmas"))
    n, R = int(ts.numel()), int(counts.numel())
    starts = torch.cumsum(counts, 0) - counts
    seg = seginfo_from_packed(torch.stack([starts, counts], -1), n)
    ri = torch.repeat_interleave(torch.arange(R, device=dev), counts)
    plain = volrend._visibility_native(seg, ts, te, sig, None, eps, 0.0, want_counts=True)
    ones = volrend._visibility_native(seg, ts, te, sig, torch.ones(n, device=dev), eps, 0.0, want_counts=True)
    cs = volrend._visibility_native(seg, ts, te, sig, None, eps, 0.0, want_counts=True, step=1.0)
    differ = plain[0][probe] != ones[0][probe]
    print(f"eps {eps:g} lead {lead}: {S.numel()} probes, band {ER.band(eps)}, {int(differ.sum())} differ from the expf-everywhere mask",
          "" if not bool(differ.any()) else f"(S from {float(S.to(dev)[differ].min())!r} to {float(S.to(dev)[differ].max())!r})")
    assert torch.equal(plain[0], ones[0]), int((plain[0] != ones[0]).sum())                         # (a)
    assert torch.equal(plain[1], ones[1])
    assert torch.equal(plain[1], torch.zeros_like(plain[1]).index_add_(0, ri, plain[0].long()))
    if ER.eps32(eps) >= ER.FLT_MIN:                                                                   # (b)
        want, amb = ER.sweep_expectation(S.to(dev), eps)
        assert int(amb.sum()) <= ER.ambiguous_cap(eps)
        assert torch.equal(plain[0][probe][~amb], want[~amb])
        if eps <= 1.0:
            lead_rows = torch.ones(n, dtype=torch.bool, device=dev)
            lead_rows[probe] = False
            assert bool(plain[0][lead_rows].all())       # in front of the probe T is 1 (and 1 >= eps)
    assert torch.equal(cs[0], plain[0]) and torch.equal(cs[1], plain[1])                              # (c)


# ============================================================================= 4: containment
NAN, INF = float("nan"), float("inf")
POISONS = [(key, v) for key in ("sig", "al", "rgb", "ts") for v in (NAN, INF, -INF)] + [("sig_inf_delta_0", INF)]


def _positions(rays):
    """(label, ray, packed index of the poisoned sample)."""
    named, st, ct = ER.edge_rays(), rays.starts.tolist(), rays.counts.tolist()
    pos = [(k, named[k], st[named[k]] + ct[named[k]] // 2) for k in ("lane", "tile_first", "tile_last", "step_end")]
    r = named["long"]
    return pos + [("long_first", r, st[r]), ("long_last", r, st[r] + ct[r] - 1)]


@lru_cache(None)
def _base(devname: str):
    dev = torch.device(devname)
    o = ER.ordinary(ER.edge_counts(), seed=60)
    rays = SR.Rays(o["rays"].counts.to(dev))
    g = torch.Generator().manual_seed(61)
    d = {"rays": rays, "ri": rays.ray_ids.clone(), "ts": o["t_starts"].to(dev), "te": o["t_ends"].to(dev), "sig": o["sigmas"].to(dev),
         "al": o["alphas"].to(dev), "rgb": o["rgbs"].to(dev)}
    d["g_n"] = [torch.randn(rays.n, generator=g).to(dev) for _ in range(3)]
    d["g_r"] = [torch.randn(rays.R, k, generator=g).to(dev) for k in (3, 1, 1, 4, 5)]
    d["ray0"] = [torch.rand(rays.R, k, generator=g).to(dev) * 0.5 for k in (3, 1, 1)]
    d["seg"] = seginfo_from_ray_indices(d["ri"], rays.R)
    return d


def _poisoned(d, key, value, p):
    q = dict(d)
    if key == "sig_inf_delta_0":
        q["sig"], q["te"] = d["sig"].clone(), d["te"].clone()
        q["sig"][p] = value
        q["te"][p] = d["ts"][p]
    else:
        q[key] = d[key].clone()
        if key == "rgb":
            q[key][p, 1] = value
        else:
            q[key][p] = value
    return q


# every op: (the inputs it reads, function of the data -> {name: (tensor, "fwd" | "sample" | "ray")})
def _op_density(d):
    R = d["rays"].R
    s = d["sig"].clone().requires_grad_(True)
    w, T, a = na.render_weight_from_density(d["ts"], d["te"], s, ray_indices=d["ri"], n_rays=R)
    (g,) = torch.autograd.grad([w, T, a], s, d["g_n"])
    T2, a2 = na.render_transmittance_from_density(d["ts"], d["te"], d["sig"], ray_indices=d["ri"], n_rays=R)
    return {"w": (w, "fwd"), "T": (T, "fwd"), "a": (a, "fwd"), "g_sigma": (g, "sample"), "T2": (T2, "fwd"), "a2": (a2, "fwd")}


def _op_alpha(d):
    R = d["rays"].R
    x = d["al"].clone().requires_grad_(True)
    w, T = na.render_weight_from_alpha(x, ray_indices=d["ri"], n_rays=R)
    (g,) = torch.autograd.grad([w, T], x, d["g_n"][:2])
    T2 = na.render_transmittance_from_alpha(d["al"], ray_indices=d["ri"], n_rays=R)
    return {"w": (w, "fwd"), "T": (T, "fwd"), "g_alpha": (g, "sample"), "T2": (T2, "fwd")}


def _op_scans(d):
    pi = d["rays"].packed_info()
    out = {}
    for kind in ("inclusive_sum", "exclusive_sum", "inclusive_prod", "exclusive_prod"):
        x = (1.0 - d["al"] if kind.endswith("prod") else d["sig"] * (d["te"] - d["ts"])).clone().requires_grad_(True)
        y = getattr(na, kind)(x, pi)
        (g,) = torch.autograd.grad(y, x, d["g_n"][0])
        out[kind] = (y, "fwd")
        out[kind + ".grad"] = (g, "sample")
    return out


def _rendering_outputs(res, f, col, d, dens):
    colors, opac, depth, ex = res
    outs = [colors, opac, depth, ex["weights"], ex["trans"]] + ([ex["alphas"]] if dens else [])
    g_f, g_c = torch.autograd.grad(outs, [f, col], d["g_r"][:3] + d["g_n"][:len(outs) - 3])
    out = {"colors": (colors, "ray"), "opacities": (opac, "ray"), "depths": (depth, "ray"), "weights": (ex["weights"], "fwd"),
           "trans": (ex["trans"], "fwd"), "g_field": (g_f, "sample"), "g_rgb": (g_c, "sample")}
    if dens:
        out["alphas"] = (ex["alphas"], "fwd")
    return out


def _op_rendering(dens, fuse=True):
    def op(d):
        f = (d["sig"] if dens else d["al"]).clone().requires_grad_(True)
        col = d["rgb"].clone().requires_grad_(True)
        kw = {"rgb_sigma_fn": lambda *_: (col, f)} if dens else {"rgb_alpha_fn": lambda *_: (col, f)}
        saved = volrend.FUSE_RENDERING
        volrend.FUSE_RENDERING = fuse
        try:
            return _rendering_outputs(na.rendering(d["ts"], d["te"], d["ri"], n_rays=d["rays"].R, **kw), f, col, d, dens)
        finally:
            volrend.FUSE_RENDERING = saved
    return op


def _op_const_step(d):
    rays, seg, dev = d["rays"], d["seg"], d["ts"].device
    n, R, step = rays.n, rays.R, ER.DELTA
    tail = (B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, R, n)
    new = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    f = [new(n), new(n), new(n), new(R, 3), new(R), new(R)]
    B.call("nfa_render_fused_fwd_cs", B.ptr(d["ts"]), step, B.ptr(d["sig"]), B.ptr(d["rgb"]), *tail, *(B.ptr(t) for t in f), B.stream())
    grads = [d["g_r"][0], d["g_r"][1][:, 0].contiguous(), d["g_r"][2][:, 0].contiguous()] + d["g_n"]
    b = [new(n), new(n, 3)]
    B.call("nfa_render_fused_bwd_cs", B.ptr(d["ts"]), step, B.ptr(d["rgb"]), B.ptr(f[1]), B.ptr(f[2]), *(B.ptr(t) for t in grads), *tail,
           *(B.ptr(t) for t in b), B.stream())
    vis, cnt = volrend._visibility_native(seg, d["ts"], d["te"], d["sig"], None, 1e-2, 0.01, want_counts=True, step=step)
    return {"w": (f[0], "fwd"), "T": (f[1], "fwd"), "a": (f[2], "fwd"), "colors": (f[3], "ray"), "opac": (f[4], "ray"), "depth": (f[5], "ray"),
            "g_sigma": (b[0], "sample"), "g_rgb": (b[1], "sample"), "vis": (vis, "fwd"), "counts": (cnt, "ray")}


def _op_render_step(d):
    from nerfacc_amd import marching
    out = {}
    for thre in (0.0, 0.01):
        c, o, dp = (t.clone() for t in d["ray0"])
        nv = torch.zeros(marching._VISIBLE_SLOTS, dtype=torch.int64, device=c.device)
        marching._render_step_native(d["seg"], d["ts"], d["te"], d["sig"], d["rgb"], thre, c, o, dp, nv if thre > 0 else None)
        out.update({f"colors{thre}": (c, "ray"), f"opacity{thre}": (o, "ray"), f"depth{thre}": (dp, "ray")})
    return out


def _op_visibility(d):
    seg, n = d["seg"], d["rays"].n
    pf = 0.5 + 0.5 * d["al"]
    out = {}
    for name, args in (("density", (d["ts"], d["te"], d["sig"])), ("alpha", (None, None, d["al"]))):
        for pname, p in (("", None), (".prefix", pf)):
            vis, cnt = volrend._visibility_native(seg, *args, p, 1e-2, 0.01, want_counts=True)
            out[name + pname + ".vis"] = (vis, "fwd")
            out[name + pname + ".counts"] = (cnt, "ray")
    return out


def _op_compact(d):
    """Compaction of a fixed mask (the base's): t_starts / t_ends are copied, so a poisoned value moves with its sample."""
    b = _base(str(d["ts"].device))
    if "vis" not in b:
        b["vis"] = volrend._visibility_native(b["seg"], b["ts"], b["te"], b["sig"], None, 1e-2, 0.0, want_counts=True)
    vis, cnt = b["vis"]
    o_ri, o_ts, o_te = _compact(d["seg"], vis, cnt, d["ts"], d["te"], d["ts"].device)
    full = lambda o: torch.zeros(d["rays"].n, dtype=o.dtype, device=o.device).masked_scatter_(vis, o)   # back at the samples' places
    return {"ray_indices": (full(o_ri), "fwd"), "t_starts": (full(o_ts), "fwd"), "t_ends": (full(o_te), "fwd")}


def _values(d, D):
    rgb = d["rgb"]
    return rgb[:, 1:2].contiguous() if D == 1 else torch.cat([rgb, rgb[:, :D - 3]], -1)


def _op_accumulate(d):
    """Weights are the densities, values are made of the colours (channel 1, the poisoned one, is in all of them)."""
    rays, ri = d["rays"], d["ri"]
    out = {}
    for D, g in ((1, d["g_r"][1]), (4, d["g_r"][3]), (5, d["g_r"][4])):
        w, v = d["sig"].clone().requires_grad_(True), _values(d, D).requires_grad_(True)
        o = na.accumulate_along_rays(w, v, ri, rays.R)
        gw, gv = torch.autograd.grad(o, [w, v], g)
        inplace = d["ray0"][0][:, :1].repeat(1, D).contiguous()
        with torch.no_grad():
            volrend.accumulate_along_rays_(d["sig"], _values(d, D), ri, inplace)
        out.update({f"out{D}": (o, "ray"), f"g_w{D}": (gw, "sample"), f"g_v{D}": (gv, "sample"), f"in_place{D}": (inplace, "ray")})
    return out


def _op_distortion(d):
    from nerfacc_amd.losses import distortion
    w, ts, te = (d[k].clone().requires_grad_(True) for k in ("al", "ts", "te"))
    loss = distortion(w, ts, te, ray_indices=d["ri"], n_rays=d["rays"].R)
    gw, gs, ge = torch.autograd.grad(loss, [w, ts, te], d["g_r"][1][:, 0].contiguous())
    return {"loss": (loss, "ray"), "g_w": (gw, "sample"), "g_ts": (gs, "sample"), "g_te": (ge, "sample")}


def _op_raw(d):
    from nerfacc_amd.rawrender import rendering_from_raw
    f, col = d["sig"].clone().requires_grad_(True), d["rgb"].clone().requires_grad_(True)
    res = rendering_from_raw(d["ts"], d["te"], col, f, d["ri"], d["rays"].R, density_activation="none", rgb_activation="sigmoid")
    return _rendering_outputs(res, f, col, d, True)


def _op_raw_exp(d):
    """raw = ln(sigma): +inf stays +inf, -inf becomes a zero density, NaN stays NaN."""
    from nerfacc_amd.rawrender import rendering_from_raw
    f = torch.where(torch.isfinite(d["sig"]), torch.log(d["sig"].clamp_min(1e-3)), d["sig"]).requires_grad_(True)
    col = d["rgb"].clone().requires_grad_(True)
    res = rendering_from_raw(d["ts"], d["te"], col, f, d["ri"], d["rays"].R, density_activation="trunc_exp", rgb_activation="none")
    return _rendering_outputs(res, f, col, d, True)


def _op_sdf(model):
    def op(d):
        from nerfacc_amd.sdfrender import rendering_from_sdf
        f = (0.05 - d["sig"] * 0.01).requires_grad_(True)       # signed distances around 0; the poison arrives through them
        col = d["rgb"].clone().requires_grad_(True)
        kw = {"model": "neus", "inv_s": 20.0, "cos": -d["al"].clamp(0.05, 1.0)} if model == "neus" else {"model": "volsdf", "beta": 0.1}
        res = rendering_from_sdf(d["ts"], d["te"], col, f, d["ri"], d["rays"].R, **kw)
        return _rendering_outputs(res, f, col, d, True)
    return op


OPS = {
    "from_density": (("sig", "ts"), _op_density), "from_alpha": (("al",), _op_alpha), "scans": (("sig", "al", "ts"), _op_scans),
    "rendering_fused": (("sig", "rgb", "ts"), _op_rendering(True)), "rendering_two_pass": (("sig", "rgb", "ts"), _op_rendering(True, False)),
    "rendering_alpha": (("al", "rgb", "ts"), _op_rendering(False)), "const_step": (("sig", "rgb", "ts"), _op_const_step),
    "render_step": (("sig", "rgb", "ts"), _op_render_step), "visibility": (("sig", "al", "ts"), _op_visibility),
    "compact": (("ts",), _op_compact), "accumulate": (("sig", "rgb"), _op_accumulate), "distortion": (("al", "ts"), _op_distortion),
    "raw": (("sig", "rgb", "ts"), _op_raw), "raw_trunc_exp": (("sig", "rgb", "ts"), _op_raw_exp),
    "sdf_neus": (("sig", "rgb", "ts", "al"), _op_sdf("neus")), "sdf_volsdf": (("sig", "rgb", "ts"), _op_sdf("volsdf")),
}


def _same_bits(a, b):
    return a.shape == b.shape and (torch.equal(a, b) if not a.is_floating_point() else torch.equal(a.view(torch.int32), b.view(torch.int32)))


@pytest.mark.parametrize("name", list(OPS))
def test_containment(dev, name):
    """One non-finite sample: every value of every OTHER ray, and the poisoned ray's forward per-sample outputs in front of
    the poisoned sample, keep the bits of the unpoisoned run.  Nothing is asserted about the rest of the poisoned ray."""
    keys, op = OPS[name]
    d = _base(str(dev))
    rays = d["rays"]
    base = {k: (t.detach().clone(), kind) for k, (t, kind) in op(d).items()}
    for k, (t, _) in base.items():
        assert not t.is_floating_point() or bool(torch.isfinite(t).all()), k
    idx, rids = torch.arange(rays.n, device=dev), torch.arange(rays.R, device=dev)
    runs = 0
    for key, value in POISONS:
        if key.split("_")[0] not in keys or (key == "sig_inf_delta_0" and "ts" not in keys):
            continue
        for label, r, p in _positions(rays):
            got = op(_poisoned(d, key, value, p))
            runs += 1
            for k, (t, kind) in got.items():
                b = base[k][0]
                rows = (rids != r) if kind == "ray" else (rays.ray_ids != r)
                if kind == "fwd":
                    rows = rows | (idx < p)
                assert _same_bits(t.detach()[rows].contiguous(), b[rows].contiguous()), (name, key, value, label, k)
    assert runs >= 18
    # the call returned every time, and a finite case run afterwards gives the base bits again
    for k, (t, _) in op(d).items():
        assert _same_bits(t.detach(), base[k][0]), k


@pytest.mark.parametrize("D", [1, 4, 5])
def test_containment_atomic_accumulate(dev, D):
    """Unsorted indices take the atomic kernel, whose order of additions varies from run to run: the other rays stay finite
    and within the order-independent bound of the float64 sums (bits cannot be compared)."""
    d = _base(str(dev))
    rays, ri = d["rays"], d["ri"]
    perm = torch.randperm(rays.n, generator=torch.Generator().manual_seed(D)).to(dev)
    w64 = d["sig"].double()
    for key, value in (("sig", NAN), ("sig", INF), ("rgb", NAN), ("rgb", -INF)):
        for label, r, p in _positions(rays):
            q = _poisoned(d, key, value, p)
            v = _values(q, D)
            out = d["ray0"][0][:, :1].repeat(1, D).contiguous()
            with torch.no_grad():
                volrend.accumulate_along_rays_(q["sig"][perm], v[perm], ri[perm], out)
            v64 = _values(d, D).double()
            want = d["ray0"][0][:, :1].double() + SR.accumulate(rays, w64, v64)
            tol = SR.bound(rays, d["ray0"][0][:, :1].double() + SR.accumulate(rays, w64, v64.abs()), per_ray=True, extra=1)
            other = torch.arange(rays.R, device=dev) != r
            check(f"{key} {value} {label}", out[other], want[other], tol[other])


@pytest.mark.parametrize("R,S", [(37, 65)])
def test_containment_cdf_rows(dev, R, S):
    from nerfacc_amd.estimators import prop_net as PN
    g = torch.Generator().manual_seed(70)
    t = torch.sort(torch.rand(R, S + 1, generator=g) * 5.0 + 0.1, -1).values.to(dev)
    ts, te = t[:, :-1].contiguous(), t[:, 1:].contiguous()
    sg = (torch.rand(R, S, generator=g) * 6.0).to(dev)
    gin = torch.randn(R, S + 1, generator=g).to(dev)

    def run(ts_, sg_):
        s = sg_.clone().requires_grad_(True)
        cd = PN._cdfs_from_density(ts_, te, s)
        (gs,) = torch.autograd.grad(cd, s, gin)
        return cd.detach(), gs

    base = run(ts, sg)
    finite(cdfs=base[0], g_sigmas=base[1])
    for key, value in [(k, v) for k in ("sig", "ts") for v in (NAN, INF, -INF)]:
        for r, col in ((0, 0), (R - 1, S - 1), (17, 31), (3, 64)):
            ts_, sg_ = ts.clone(), sg.clone()
            (sg_ if key == "sig" else ts_)[r, col] = value
            cd, gs = run(ts_, sg_)
            other = torch.arange(R, device=dev) != r
            assert _same_bits(cd[other].contiguous(), base[0][other].contiguous()), (key, value, r, col)
            assert _same_bits(gs[other].contiguous(), base[1][other].contiguous()), (key, value, r, col)
            assert _same_bits(cd[r, :col + 1].contiguous(), base[0][r, :col + 1].contiguous())      # in front of the poison
    again = run(ts, sg)
    assert _same_bits(again[0], base[0]) and _same_bits(again[1], base[1])

"""CPU: the closed forms and generators of tests/render_edges_reference.py.

* the closed-form backward of the density chain, the alpha chain and the product scans against a per-ray Python loop and
  against float64 autograd (they agree to 1e-12 wherever no alpha == 1 occurs, and the clamped alpha form DIFFERS from
  autograd at alpha == 1: that is why tests/test_render_edges_gpu.py cannot use an autograd reference);
* the generators' properties (every class and position present, the five opacity targets hit exactly, the threshold
  sweeps inside their cap of ambiguous probes);
* the reference alone against its own bounds: the float32 torch composition of the same formulas stays within half of
  ``bound(...) + TINY`` of the float64 run, for every output and gradient of every finite generator.
"""
import math

import numpy as np
import pytest
import torch

import render_edges_reference as ER
import seg_reference as SR

WHERE = ("first", "middle", "last")


def _grads(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]


def _close(a, b, tol=1e-12):
    return bool(((a - b).abs() <= tol * (1.0 + b.abs())).all())


def _midrange(seed=3):
    """Unsaturated samples: no alpha reaches 1 in float64."""
    counts = ER.edge_counts()
    rays = SR.Rays(counts)
    g = torch.Generator().manual_seed(seed)
    ts, te = ER._grid_times(rays.n, g)
    sig = torch.rand(rays.n, generator=g, dtype=torch.float64) * 20.0
    return rays, ts.double(), te.double(), sig


# ----------------------------------------------------------------------------- closed forms
def _loop_density(counts, ts, te, sig, gw, gt, ga):
    out, p = [], 0
    for c in counts.tolist():
        x = [float(sig[p + i]) * (float(te[p + i]) - float(ts[p + i])) for i in range(c)]
        S, T, a = 0.0, [], []
        for i in range(c):
            T.append(math.exp(-S)); a.append(1.0 - math.exp(-x[i])); S += x[i]
        E = 0.0
        row = [0.0] * c
        for i in range(c - 1, -1, -1):
            row[i] = (float(gw[p + i]) * T[i] + float(ga[p + i])) * (1.0 - a[i]) - E
            E += (float(gw[p + i]) * a[i] + float(gt[p + i])) * T[i]
        out += row
        p += c
    return torch.tensor(out, dtype=torch.float64)


def _loop_alpha(counts, al, gw, gt):
    out, p = [], 0
    for c in counts.tolist():
        T, t = [], 1.0
        for i in range(c):
            T.append(t); t *= 1.0 - float(al[p + i])
        E, row = 0.0, [0.0] * c
        for i in range(c - 1, -1, -1):
            row[i] = float(gw[p + i]) * T[i] - E / max(1.0 - float(al[p + i]), 1e-10)
            E += (float(gw[p + i]) * float(al[p + i]) + float(gt[p + i])) * T[i]
        out += row
        p += c
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("where", WHERE)
def test_density_closed_form(where):
    c = ER.saturating(ER.edge_counts(), where, seed=1, with_inf=False)
    rays = c["rays"]
    ts, te, sig = (c[k].double() for k in ("t_starts", "t_ends", "sigmas"))
    gw, gt, ga = _grads([(rays.n,)] * 3, 2)
    w, T, a, _ = ER.density_forward(rays, ts, te, sig)
    gx, gs = ER.density_backward(rays, ts, te, T, a, gw, gt, ga)
    assert _close(gx, _loop_density(rays.counts, ts, te, sig, gw, gt, ga))
    # the density chain has no clamp: autograd agrees everywhere, saturated or not
    s = sig.clone().requires_grad_(True)
    (ag,) = torch.autograd.grad(SR.from_density(rays, ts, te, s), s, [gw, gt, ga])
    assert _close(gs, ag) and bool((a == 1.0).any())


def test_alpha_closed_form_against_loop_and_autograd():
    rays, ts, te, sig = _midrange()
    _, _, al, _ = ER.density_forward(rays, ts, te, sig)
    assert float(al.max()) < 1.0
    gw, gt = _grads([(rays.n,)] * 2, 4)
    w, T = ER.alpha_forward(rays, al)
    ga = ER.alpha_backward(rays, al, T, gw, gt)
    assert _close(ga, _loop_alpha(rays.counts, al, gw, gt))
    x = al.clone().requires_grad_(True)
    (ag,) = torch.autograd.grad(SR.from_alpha(rays, x), x, [gw, gt])
    assert _close(ga, ag)
    s_w, s_t, s_g = ER.alpha_scales(rays, al, T, gw, gt)
    r_w, r_t, r_g = SR.alpha_scales(rays, al, T, gw, gt)
    assert _close(s_g, r_g) and _close(s_w, r_w) and _close(s_t, r_t)


@pytest.mark.parametrize("where", WHERE)
def test_alpha_closed_form_differs_from_autograd_at_alpha_one(where):
    c = ER.saturating(ER.edge_counts(), where, seed=5)
    rays = c["rays"]
    ts, te, sig = (c[k] for k in ("t_starts", "t_ends", "sigmas"))
    al = ER.density_forward(rays, ts, te, sig)[2].double()      # float32 alphas: alpha == 1 exactly at the saturating samples
    one = al == 1.0
    assert bool(one[c["sat"][c["sat"] >= 0]].all())
    gw, gt = _grads([(rays.n,)] * 2, 6)
    w, T = ER.alpha_forward(rays, al)
    ga = ER.alpha_backward(rays, al, T, gw, gt)
    assert _close(ga, _loop_alpha(rays.counts, al, gw, gt))
    x = al.clone().requires_grad_(True)
    (ag,) = torch.autograd.grad(SR.from_alpha(rays, x), x, [gw, gt])
    behind = ER._suffix(rays, one.double()) > 0                 # a sample with an alpha == 1 sample behind it ...
    clean = ~one & ~behind & (ER._suffix(rays, one.double(), True) == 0)
    front = ~one & behind
    assert _close(ga[front | clean], ag[front | clean])         # ... still has the autograd derivative: 1 - a_i > 0 there
    diff = (ga - ag).abs()[one]
    if where != "last":                                         # (behind a last sample there is nothing to differ about)
        assert float(diff.max()) > 1.0 and int((diff > 1e-3).sum()) > 10
    else:
        assert float(diff.max()) == 0.0
    assert bool((ga[one] == (gw * T)[one]).all())               # the clamped form: the chain's share is exactly 0 there
    assert bool(torch.isfinite(ga).all())


@pytest.mark.parametrize("kind", ["inclusive_prod", "exclusive_prod"])
def test_prod_backward_closed_form(kind):
    rays = SR.Rays(ER.edge_counts())
    g = torch.Generator().manual_seed(7)
    x = torch.rand(rays.n, generator=g, dtype=torch.float64) * 0.2 + 0.9
    (go,) = _grads([(rays.n,)], 8)
    y = SR.scan(rays, x, kind)
    gx = ER.prod_backward(rays, x, y, go, kind)
    xa = x.clone().requires_grad_(True)
    (ag,) = torch.autograd.grad(SR.scan(rays, xa, kind), xa, go)
    assert _close(gx, ag)
    x0 = x.clone()
    x0[rays.starts[rays.counts > 2] + 1] = 0.0                   # a zero factor: the clamp, not the derivative
    y0 = SR.scan(rays, x0, kind)
    gx0 = ER.prod_backward(rays, x0, y0, go, kind)
    xa = x0.clone().requires_grad_(True)
    (ag0,) = torch.autograd.grad(SR.scan(rays, xa, kind), xa, go)
    assert bool(torch.isfinite(gx0).all()) and not _close(gx0, ag0, 1e-6)


def test_depth_normalisation_gradient():
    eps = ER.EPS_DEPTH
    op = torch.tensor([[0.0], [1e-40], [eps * (1 - 2.0 ** -24)], [eps], [eps * (1 + 2.0 ** -23)], [0.3]], dtype=torch.float64)
    dr = torch.rand(6, 1, dtype=torch.float64) * op
    g_o, g_d = _grads([(6, 1)] * 2, 9)
    o, d = op.clone().requires_grad_(True), dr.clone().requires_grad_(True)
    depth = ER.normalise_depth(o, d)
    a_o, a_d = torch.autograd.grad([o, depth], [o, d], [g_o, g_d])
    G_o, G_d, share = ER.normalise_depth_backward(op, depth.detach(), g_o, g_d)
    assert _close(G_o, a_o) and _close(G_d, a_d)
    assert bool((share[:3] == 0).all()) and bool((share[3:] != 0).all())


# ----------------------------------------------------------------------------- generators
def test_edge_counts():
    counts = ER.edge_counts()
    c = counts.tolist()
    for k in list(range(6)) + [63, 64, 65, 255, 256, 257, 1025]:
        assert k in c
    assert c.count(1025) == 1 and sum(c) % 4 != 0 and 2000 < sum(c) < 4000
    run = max(len(s) for s in "".join("0" if k == 0 else "x" for k in c).split("x"))
    assert run >= 70
    rays, named = SR.Rays(counts), ER.edge_rays()
    st, ct = rays.starts.tolist(), c
    r = named["lane"]
    assert ct[r - 1:r + 2] == [1, 2, 3] and st[r - 1] // 4 == st[r] // 4 and (st[r] + 1) // 4 == st[r + 1] // 4
    r = named["step_end"]
    assert (st[r] + ct[r]) % ER.STEP_ELEMS == 0 and ct[r] > 0
    r = named["tile_last"]
    assert (st[r] + ct[r]) % ER.TILE_ELEMS == 0 and st[r] // ER.TILE_ELEMS == 0
    r = named["tile_first"]
    assert st[r] % ER.TILE_ELEMS == 0 and st[r] > 0 and ct[r] > 0 and ct[r + 1] == 0 and ct[r - 1] > 0
    assert ct[named["long"]] == 1025


@pytest.mark.parametrize("where", WHERE)
def test_saturating_generator(where):
    c = ER.saturating(ER.edge_counts(), where, seed=1)
    rays, cls, sat = c["rays"], c["cls"], c["sat"]
    assert sorted(set(cls.tolist())) == list(range(ER.N_BG + len(ER.SATURATING)))    # every class is present
    live = rays.counts > 0
    assert bool((sat[~live] == -1).all()) and int((cls >= ER.N_BG).sum()) == int(live.sum())   # one per ray
    pos = sat[live] - rays.starts[live]
    want = {"first": torch.zeros_like(pos), "middle": rays.counts[live] // 2, "last": rays.counts[live] - 1}[where]
    assert torch.equal(pos, want)
    x = c["sigmas"].double() * (c["t_ends"] - c["t_starts"]).double()
    for k, v in enumerate(ER.SATURATING):
        assert bool((x[cls == ER.N_BG + k] == v).all())
    for k, v in enumerate(ER.BACKGROUND):
        assert bool(((x[cls == k] - v).abs() <= 2.0 ** -23 * v).all())
    # float32: alpha == 1 exactly at the saturating samples; 1 - exp(-x) is exactly 0 below 2^-25 (at 2^-25, where
    # exp(-x) is a tie between 1 and 1 - 2^-24, it is 0 or 2^-24)
    a32 = 1.0 - torch.exp(-(c["sigmas"] * (c["t_ends"] - c["t_starts"])))
    assert bool((a32[cls >= ER.N_BG] == 1.0).all())
    k25 = ER.BACKGROUND.index(2.0 ** -25)
    assert bool((a32[cls < k25] == 0.0).all()) and bool((a32[cls > k25] > 0).all())
    assert bool(((a32[cls == k25] == 0.0) | (a32[cls == k25] == 2.0 ** -24)).all())
    # live signal in front of the saturating sample
    w = ER.density_forward(rays, c["t_starts"], c["t_ends"], c["sigmas"])[0]
    assert float((w > 0).float().mean()) > 0.04
    assert not bool(torch.isinf(ER.saturating(ER.edge_counts(), where, with_inf=False)["sigmas"]).any())


def test_vanishing_generator():
    c = ER.vanishing(ER.edge_counts(), seed=2)
    rays, kind = c["rays"], c["kind"]
    assert sorted(set(kind.tolist())) == [-1] + list(range(len(ER.VANISHING)))
    al, sig = c["alphas"], c["sigmas"]
    for dtype in (torch.float32, torch.float64):                 # the alpha path: the five targets exactly, in either type
        w, _ = ER.alpha_forward(rays, al.to(dtype))
        op = SR.accumulate(rays, w)[:, 0]
        for name, target in ER.OPACITY_TARGETS.items():
            rows = kind == ER.VANISHING.index(name)
            assert bool(rows.any()) and bool((op[rows] == torch.tensor(target, dtype=torch.float32).to(dtype)).all()), name
    t32 = lambda v: float(np.float32(v))
    assert t32(ER.OPACITY_TARGETS["total_below_eps"]) < ER.EPS_DEPTH < t32(ER.OPACITY_TARGETS["total_above_eps"])
    assert 0 < t32(ER.OPACITY_TARGETS["total_subnormal"]) < 2.0 ** -126
    z, nz, sub = (c["cls"] == ER.VANISHING.index(k) for k in ("zeros", "neg_zeros", "subnormal"))
    assert bool((sig[z] == 0).all()) and not bool(torch.signbit(sig[z]).any())
    assert bool(torch.signbit(sig[nz]).all()) and bool(torch.signbit(al[nz]).all()) and bool((sig[nz] == 0).all())
    assert bool(((sig[sub] > 0) & (sig[sub] < 2.0 ** -126)).all())
    # the density form of "total_0": non-zero densities, float32 alphas exactly 0
    t0 = c["cls"] == ER.VANISHING.index("total_0")
    a32 = ER.density_forward(rays, c["t_starts"], c["t_ends"], sig)[2]
    assert bool((sig[t0] > 0).all()) and bool((a32[t0] == 0).all())


@pytest.mark.parametrize("eps", ER.EARLY_STOP_EPS)
def test_threshold_sweeps(eps):
    S = ER.threshold_sweeps(eps)
    s_lo, s_hi = ER.band(eps)
    assert S.dtype == torch.float32 and bool((S[1:] > S[:-1]).all()) and bool((S >= 0).all()) and S.numel() < 4000
    L = -math.log(ER.eps32(eps))
    if L >= 1.0:     # consecutive float32 values over the whole band and 50 beyond each end
        bits = S.numpy().view(np.int32)
        assert np.array_equal(np.diff(bits), np.ones(len(bits) - 1, np.int32))
        assert int((S < s_lo).sum()) >= ER.N_BEYOND and int((S > s_hi).sum()) >= ER.N_BEYOND
    else:            # a grid of 2^-26 (S >= 0: what lies below 0 cannot be reached with densities >= 0)
        assert bool((torch.diff(S.double()) == ER.GRID_BELOW_1).all())
        assert int((S > s_hi).sum()) >= ER.N_BEYOND and (float(S[0]) == 0.0 or int((S < s_lo).sum()) >= ER.N_BEYOND)
    assert int(((S > s_lo) & (S < s_hi)).sum()) > 100 or s_hi <= 0
    if ER.eps32(eps) >= ER.FLT_MIN:
        want, amb = ER.sweep_expectation(S, eps)
        assert int(amb.sum()) <= ER.ambiguous_cap(eps)
        assert ER.ambiguous_cap(eps) == 8 or L < 1.0
        if eps < 1.0:
            assert bool(want.any()) and bool((~want).any())
    p = ER.probe_rays(S[:5], lead=3)
    assert p["counts"].tolist() == [5] * 5 and p["probe"].tolist() == [4, 9, 14, 19, 24]
    rays = SR.Rays(p["counts"])
    x = p["sigmas"] * (p["t_ends"] - p["t_starts"])
    assert torch.equal(rays.unpad(SR.excl_sum_rows(rays.pad(x)))[p["probe"]], S[:5])      # S arrives exactly


# ----------------------------------------------------------------------------- the reference alone against its bounds
def _ratio(v32, v64, tol):
    err = (v32.double() - v64).abs()
    assert bool(torch.isfinite(err).all()) and bool(torch.isfinite(tol).all())
    return float((err / (tol + ER.TINY)).max()) if err.numel() else 0.0


def _finite_cases():
    counts = ER.edge_counts()
    for where in WHERE:
        c = ER.saturating(counts, where, seed=11, with_inf=False)
        g = torch.Generator().manual_seed(12)
        c["rgbs"] = torch.rand(c["rays"].n, 3, generator=g)
        yield "saturating_" + where, c
    yield "vanishing", ER.vanishing(counts, seed=13)


WORST = {}


@pytest.mark.parametrize("name,c", list(_finite_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_reference_alone_stays_inside_the_bounds(name, c):
    rays = c["rays"]
    n, R = rays.n, rays.R
    ts, te, sig, rgb = (c[k] for k in ("t_starts", "t_ends", "sigmas", "rgbs"))
    gw, gt, ga = _grads([(n,)] * 3, 14)
    ratios = {}
    # weights / trans / alphas from density
    o32 = ER.density_forward(rays, ts, te, sig)
    w, T, a, _ = ER.density_forward(rays, ts.double(), te.double(), sig.double())
    s_w, s_t, s_a, s_gx = ER.density_scales(rays, ts.double(), te.double(), sig.double(), T, a, gw, gt, ga)
    for k, v32, v64, s in (("w", o32[0], w, s_w), ("T", o32[1], T, s_t), ("a", o32[2], a, s_a)):
        ratios["density." + k] = _ratio(v32, v64, SR.bound(rays, s))
    g32 = ER.density_backward(rays, ts, te, o32[1], o32[2], gw.float(), gt.float(), ga.float())[1]
    g64 = ER.density_backward(rays, ts.double(), te.double(), T, a, gw, gt, ga)[1]
    ratios["density.g_sigma"] = _ratio(g32, g64, SR.bound(rays, s_gx * (te - ts).double().abs()))
    # from alpha: the float32 alphas of the density results (alpha == 1 exactly at a saturating sample)
    al = c["alphas"] if "alphas" in c else o32[2]
    a32 = ER.alpha_forward(rays, al)
    w, T = ER.alpha_forward(rays, al.double())
    s_w, s_t, s_g = ER.alpha_scales(rays, al.double(), T, gw, gt)
    ratios["alpha.w"] = _ratio(a32[0], w, SR.bound(rays, s_w))
    ratios["alpha.T"] = _ratio(a32[1], T, SR.bound(rays, s_t))
    ratios["alpha.g_alpha"] = _ratio(ER.alpha_backward(rays, al, a32[1], gw.float(), gt.float()),
                                     ER.alpha_backward(rays, al.double(), T, gw, gt), SR.bound(rays, s_g))
    # the product scans and their backward
    x = 1.0 - al
    for kind in ("inclusive_prod", "exclusive_prod"):
        y32, y64 = SR.scan(rays, x, kind), SR.scan(rays, x.double(), kind)
        s_f, s_b = ER.prod_scales(rays, x.double(), y64, gw, kind)
        ratios[kind] = _ratio(y32, y64, SR.bound(rays, s_f))
        ratios[kind + ".grad"] = _ratio(ER.prod_backward(rays, x, y32, gw.float(), kind),
                                        ER.prod_backward(rays, x.double(), y64, gw, kind), SR.bound(rays, s_b))
    # rendering, both fields, with gradients at the extras
    g_c, g_o, g_d = _grads([(R, 3), (R, 1), (R, 1)], 15)
    for dens, field in ((True, sig), (False, al)):
        ex = (gw, gt, ga if dens else None)
        r32 = ER.rendering_reference(rays, ts, te, field, rgb, dens, g_c.float(), g_o.float(), g_d.float(),
                                     tuple(None if e is None else e.float() for e in ex))
        r64 = ER.rendering_reference(rays, ts.double(), te.double(), field.double(), rgb.double(), dens, g_c, g_o, g_d, ex,
                                     opac_own=r32["opacities"][0], depth_own=r32["depths"][0])
        for k, (v64, tol) in r64.items():
            if tol is not None:
                ratios[("sigma." if dens else "alpha.") + "rendering." + k] = _ratio(r32[k][0], v64, tol)
    worst = max(ratios, key=ratios.get)
    WORST[name] = (worst, ratios[worst])
    print(name, "worst error / tolerance:", worst, ratios[worst])
    assert ratios[worst] <= 0.5, (worst, ratios[worst])

"""GPU: ``rendering_from_raw`` on its native path (nfa_render_raw_fwd / nfa_render_raw_bwd, csrc/segscan.hip).

Every output and both gradients against the float64 restatement (tests/rawrender_reference.py) within the per-element
bounds of tests/seg_reference.py, widened only by the roundings the activations add (counted below); with every
activation off the two passes must reproduce ``rendering``'s fused passes bit for bit; the scalar form (inputs that are
not 16-byte aligned) must reproduce the vector form bit for bit; and a step is exactly two native calls.
"""
import numpy as np
import pytest
import torch

import nerfacc_amd as na
import rawrender_reference as RR
import seg_reference as SR
from nerfacc_amd import _backend as B
from nerfacc_amd._segments import seginfo_from_ray_indices
from nerfacc_amd.rawrender import rendering_from_raw

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -126 * SR.K_ROUND    # results below float32's normal range have no relative precision
BIAS = -1.0
Z_MAX = 20.0                       # |raw + bias| of the inputs below stays within it

# Roundings the activations add, in the unit of SR.bound (one rounding = 2^-23 relative, as K_ROUND counts them).
#   z = raw + bias rounds once.  Through exp that relative error of z becomes |z| times as large in the result
#   (exp(z (1 + d)) = exp(z) (1 + z d)), so it counts Z_MAX times; expf and log1pf are accurate to 1 ulp = one unit each.
#   softplus = log1pf(expf(z)): the sensitivity of log1p(e) to e is at most 1 and of softplus to z at most |z|.
#   relu and none only pass z on.
DENSITY_ROUNDINGS = {"none": 1, "relu": 1, "exp": Z_MAX + 1, "trunc_exp": Z_MAX + 1, "softplus": Z_MAX + 2}
# the derivative factor, relative: exp(min(z, 15)) as above; exp reuses the density; softplus' is 1 / (1 + expf(-z)) --
# z's rounding at most |z| times, expf, the sum, the quotient; relu's and none's are exact
DERIVATIVE_ROUNDINGS = {"none": 0, "relu": 0, "exp": Z_MAX + 1, "trunc_exp": Z_MAX + 1, "softplus": Z_MAX + 3}
# c = 1 / (1 + expf(-x)): expf, the sum, the quotient
RGB_ROUNDINGS = {"none": 0, "sigmoid": 3}
PRODUCT = 2                        # the derivative is multiplied in: two more products


def shifted(x: torch.Tensor, k: int) -> torch.Tensor:
    """The values of x as a contiguous view at a storage offset of k elements."""
    buf = torch.empty(x.numel() + 16, dtype=x.dtype, device=x.device)
    v = buf[k:k + x.numel()].view(x.shape)
    v.copy_(x.detach())
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


class CallLog:
    def __init__(self, monkeypatch):
        self.calls = []
        real = B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def names(self):
        return [n for n, _ in self.calls]


def check(name, got, want, tol):
    """|got - want| <= tol element by element (NaN fails); prints the worst ratio first."""
    err = (got.double() - want.double()).abs()
    tol = tol + TINY
    ok = err <= tol
    print(f"{name}: worst err/tol {float((err / tol).max()) if err.numel() else 0.0:.3f}")
    assert bool(ok.all()), (name, int((~ok).sum()), float((err / tol).max()))


_CASE = {}


def case(dev):
    """Ray lengths: empty rays, one sample, a wave step's edge (64 lanes x 4 elements: 255, 256, 257), a ray across the
    1024-element tiles, then 300 rays of 1-3 samples (more than RAY_CAP = 192 rays in one tile: the backward's gather
    fallback) and a trailing empty ray.  Built once and shared; the tests do not modify it."""
    if "c" in _CASE:
        return _CASE["c"]
    rng = np.random.default_rng(7)
    counts = np.concatenate([[0, 1, 3, 0, 255, 256, 257, 2500], rng.integers(1, 4, 300), [0]]).astype(np.int64)
    rays = SR.Rays(torch.from_numpy(counts).to(dev))
    g = torch.Generator().manual_seed(11)
    n = rays.n
    ts = torch.rand(n, generator=g) * 4.0
    te = ts + 0.001 + torch.rand(n, generator=g) * 0.02
    raw_sig = torch.rand(n, generator=g) * 12.0 - 6.0
    # z = raw + BIAS between 16 and 20 (trunc_exp's clamp) where it does not blank the rest of a long ray: near the end
    # of the 2500-sample ray and at the head of some short rays
    starts = np.cumsum(counts) - counts
    hot = torch.from_numpy(np.concatenate([starts[7] + [2440, 2470, 2499], starts[8::37]]))
    raw_sig[hot] = 16.0 + 4.0 * torch.rand(hot.numel(), generator=g) - BIAS
    raw_rgb = torch.rand(n, 3, generator=g) * 16.0 - 8.0
    sel = torch.rand(n, generator=g) > 0.2                           # about 20 % masked
    sel[hot[::2]] = True
    gl = {"colors": torch.randn(rays.R, 3, generator=g), "opacities": torch.randn(rays.R, 1, generator=g),
          "depths": torch.randn(rays.R, 1, generator=g), "weights": torch.randn(n, generator=g),
          "trans": torch.randn(n, generator=g), "alphas": torch.randn(n, generator=g)}
    assert float((raw_sig + BIAS).abs().max()) <= Z_MAX
    c = dict(rays=rays, ri=rays.ray_ids.clone(), ts=ts.to(dev), te=te.to(dev), raw_sig=raw_sig.to(dev), raw_rgb=raw_rgb.to(dev),
             sel=sel.to(dev), gl={k: v.to(dev) for k, v in gl.items()})
    seginfo_from_ray_indices(c["ri"], rays.R)   # cached on the tensor, as for the ray_indices sampling() returns
    _CASE["c"] = c
    return c


def run(c, dens, col, extras, bias=BIAS, sel="case", tensors=None, return_activated=False):
    """One forward and backward; returns (outputs by name, (g_raw_sigmas, g_raw_rgbs))."""
    t = tensors or {k: c[k] for k in ("ts", "te", "raw_sig", "raw_rgb", "sel")}
    rs = t["raw_sig"].detach().requires_grad_(True)
    rc = t["raw_rgb"].detach().requires_grad_(True)
    selector = t["sel"] if sel == "case" else sel
    colors, opac, depth, ex = rendering_from_raw(t["ts"], t["te"], rc, rs, c["ri"], c["rays"].R, density_activation=dens,
                                                 density_bias=bias, rgb_activation=col, selector=selector,
                                                 return_activated=return_activated)
    outs = {"colors": colors, "opacities": opac, "depths": depth, **ex}
    keys = ["colors", "opacities", "depths"] + (["weights", "trans", "alphas"] if extras else [])
    gl = t.get("gl", c["gl"])
    grads = torch.autograd.grad([outs[k] for k in keys], [rs, rc], [gl[k] for k in keys])
    return {k: v.detach() for k, v in outs.items()}, grads


def incoming(opac, depth, g_o, g_d):
    """The per-ray gradients the depth normalisation (depth_raw / opacity.clamp_min(eps)) hands to the packed pass,
    from the product's own float32 opacity and depth: (G_opacity, G_depth_raw, |G_opacity| scale)."""
    eps = torch.finfo(torch.float32).eps
    o, d = opac.double(), depth.double()
    oc = o.clamp_min(eps)
    live = (o >= eps).double()
    return g_o - live * g_d * d / oc, g_d / oc, g_o.abs() + live * (g_d * d / oc).abs()


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("dens,col", [("trunc_exp", "sigmoid"), ("exp", "none"), ("relu", "sigmoid"), ("softplus", "sigmoid"),
                                      ("none", "sigmoid"), ("trunc_exp", "none")])
def test_against_float64(dev, monkeypatch, dens, col, extras):
    c = case(dev)
    rays, ri, ts, te, gl = c["rays"], c["ri"], c["ts"], c["te"], c["gl"]
    log = CallLog(monkeypatch)
    outs, (g_sig, g_rgb) = run(c, dens, col, extras, return_activated=True)
    assert log.names() == ["nfa_render_raw_fwd", "nfa_render_raw_bwd"]
    assert (log.calls[1][1][12] is not None) == extras   # g_weights: the backward's EXTRA variant

    # float64, with the incoming per-ray gradients torch forms from the product's own outputs
    G_o, G_d, G_o_abs = incoming(outs["opacities"], outs["depths"], gl["opacities"].double(), gl["depths"].double())
    grads = {"colors": gl["colors"], "opacities": G_o, "depths_raw": G_d}
    if extras:
        grads.update({k: gl[k] for k in ("weights", "trans", "alphas")})
    ref = RR.render(rays, ts, te, c["raw_sig"], c["raw_rgb"], dens, BIAS, col, c["sel"], grads=grads)

    e_d, e_c = DENSITY_ROUNDINGS[dens], RGB_ROUNDINGS[col]
    ts64, te64 = ts.double(), te.double()
    sig, rgb, w, T, a = ref["sigmas"], ref["rgbs"], ref["weights"], ref["trans"], ref["alphas"]
    mid = ((ts64 + te64) / 2.0).abs()
    g_c = gl["colors"].double().abs()[ri]
    ex_g = [grads.get(k) for k in ("weights", "trans", "alphas")]
    gw_abs = ((g_c * rgb.abs()).sum(-1) + G_o_abs[ri, 0] + G_d.abs()[ri, 0] * mid + (0.0 if ex_g[0] is None else ex_g[0].double().abs()))
    s_w, s_t, s_a, s_gx = SR.density_scales(rays, ts64, te64, sig, T, a, gw_abs, *[None if x is None else x.double() for x in ex_g[1:]])
    sw1 = s_w + w
    s_col = SR.accumulate(rays, sw1, rgb.abs())
    s_op = SR.accumulate(rays, sw1)
    s_dr = SR.accumulate(rays, sw1, mid[:, None])
    s_dep = (s_dr + ref["depths"].abs() * s_op) / ref["opacities"].clamp_min(torch.finfo(torch.float32).eps)

    check("sigmas", outs["sigmas"], sig, (SR.K_ROUND + e_d) * SR.EPS32 * sig.abs())
    check("rgbs", outs["rgbs"], rgb, (SR.K_ROUND + e_c) * SR.EPS32 * rgb.abs())
    check("colors", outs["colors"], ref["colors"], SR.bound(rays, s_col, per_ray=True, extra=e_d + e_c))
    check("opacities", outs["opacities"], ref["opacities"], SR.bound(rays, s_op, per_ray=True, extra=e_d))
    check("depths", outs["depths"], ref["depths"], SR.bound(rays, s_dep, per_ray=True, extra=4 + e_d))
    check("weights", outs["weights"], w, SR.bound(rays, s_w, extra=e_d))
    check("trans", outs["trans"], T, SR.bound(rays, s_t, extra=e_d))
    check("alphas", outs["alphas"], a, SR.bound(rays, s_a, extra=e_d))

    # gradients: the scale of the gradient w.r.t. the activated value times the derivative factor
    s_gsig = s_gx * (te64 - ts64).abs() * ref["dsig"].abs()
    check("g_raw_sigmas", g_sig, ref["g_raw_sigmas"],
          SR.bound(rays, s_gsig, extra=e_d + e_c + DERIVATIVE_ROUNDINGS[dens] + PRODUCT))
    s_grgb = g_c * sw1[:, None]
    tol = SR.bound(rays, s_grgb * ref["drgb"].abs(), extra=e_d + e_c + PRODUCT)
    if col == "sigmoid":   # c (1 - c): the three roundings of c are an absolute error of 3 * 2^-23 * c in 1 - c
        tol = tol + 3 * SR.EPS32 * s_grgb * rgb.abs()
    check("g_raw_rgbs", g_rgb, ref["g_raw_rgbs"], tol)

    # behind the mask: exact zeros, forward and in the gradient
    off = ~c["sel"]
    for k in ("sigmas", "alphas", "weights"):
        assert not bool(outs[k][off].any()), k
    assert not bool(g_sig[off].any())


def test_trunc_exp_gradient_uses_the_clamped_exponent(dev):
    """One ray of one sample with z = 18 and of one with z = 3: d sigma / d raw is exp(15) and exp(3)."""
    dt = 2.0 ** -30
    ts = torch.zeros(2, device=dev)
    te = torch.full((2,), dt, device=dev)
    ri = torch.tensor([0, 1], device=dev)
    raw = torch.tensor([18.0, 3.0], device=dev, requires_grad=True)
    rgb = torch.zeros(2, 3, device=dev)
    _, opac, _, _ = rendering_from_raw(ts, te, rgb, raw, ri, 2, rgb_activation="none")
    (g,) = torch.autograd.grad(opac.sum(), raw)
    # opacity = 1 - exp(-sigma dt): d / d raw = dt exp(-sigma dt) * (d sigma / d raw)
    want = [dt * np.exp(-np.exp(18.0) * dt) * np.exp(15.0), dt * np.exp(-np.exp(3.0) * dt) * np.exp(3.0)]
    assert np.allclose(g.double().cpu().numpy(), want, rtol=1e-5, atol=0.0), (g, want)
    assert not np.isclose(float(g[0]), want[0] * np.exp(3.0), rtol=0.5)   # not exp(18)


def test_non_finite_values_behind_the_mask_do_not_leak(dev):
    c = case(dev)
    off = (~c["sel"]).nonzero().flatten()
    raw = c["raw_sig"].clone()
    raw[off[0::3]] = float("inf")
    raw[off[1::3]] = float("nan")
    raw[off[2::3]] = float("-inf")
    t = {**{k: c[k] for k in ("ts", "te", "raw_rgb", "sel")}, "raw_sig": raw}
    for dens in RR.DENSITY:
        clean, g_clean = run(c, dens, "sigmoid", True)
        dirty, g_dirty = run(c, dens, "sigmoid", True, tensors=t)
        for k in clean:
            assert torch.equal(clean[k], dirty[k]), (dens, k)
        assert torch.equal(g_clean[0], g_dirty[0]) and torch.equal(g_clean[1], g_dirty[1]), dens
        assert not bool(g_dirty[0][off].any())


@pytest.mark.parametrize("extras", [False, True])
def test_no_activation_is_the_existing_pass_bit_for_bit(dev, extras):
    c = case(dev)
    sig = (c["raw_sig"].abs() * 0.3).contiguous()            # densities as rendering's callback would return them
    rgb = torch.sigmoid(c["raw_rgb"])
    t = {"ts": c["ts"], "te": c["te"], "raw_sig": sig, "raw_rgb": rgb}
    got, g_got = run(c, "none", "none", extras, bias=0.0, sel=None, tensors=t)
    s2, c2 = sig.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    colors, opac, depth, ex = na.rendering(c["ts"], c["te"], c["ri"], n_rays=c["rays"].R, rgb_sigma_fn=lambda *_: (c2, s2))
    want = {"colors": colors, "opacities": opac, "depths": depth, "weights": ex["weights"], "trans": ex["trans"], "alphas": ex["alphas"]}
    keys = ["colors", "opacities", "depths"] + (["weights", "trans", "alphas"] if extras else [])
    g_want = torch.autograd.grad([want[k] for k in keys], [s2, c2], [c["gl"][k] for k in keys])
    for k, v in want.items():
        assert torch.equal(got[k], v.detach()), k
    assert torch.equal(g_got[0], g_want[0]) and torch.equal(g_got[1], g_want[1])


@pytest.mark.parametrize("extras", [False, True])
def test_scalar_form_equals_vector_form_bit_for_bit(dev, monkeypatch, extras):
    c = case(dev)
    aligned, g_aligned = run(c, "trunc_exp", "sigmoid", extras, return_activated=True)
    sel = shifted(c["sel"], 1)                               # the mask at a one-byte offset
    assert sel.data_ptr() % 4 != 0
    t = {"ts": shifted(c["ts"], 1), "te": shifted(c["te"], 3), "raw_sig": shifted(c["raw_sig"], 2),
         "raw_rgb": shifted(c["raw_rgb"], 1), "sel": sel, "gl": {k: shifted(v, 1 + i % 3) for i, (k, v) in enumerate(c["gl"].items())}}
    log = CallLog(monkeypatch)
    got, g_got = run(c, "trunc_exp", "sigmoid", extras, tensors=t, return_activated=True)
    assert log.names() == ["nfa_render_raw_fwd", "nfa_render_raw_bwd"]
    for name, a in log.calls:   # the per-sample inputs reached the entry points unaligned
        assert all(v % 16 != 0 for v in a[:4]) and a[4] % 4 != 0, name
    for k in aligned:
        assert torch.equal(aligned[k], got[k]), k
    assert torch.equal(g_aligned[0], g_got[0]) and torch.equal(g_aligned[1], g_got[1])


def test_a_step_is_two_native_calls(dev, monkeypatch):
    c = case(dev)
    log = CallLog(monkeypatch)
    outs, _ = run(c, "trunc_exp", "sigmoid", False)
    assert log.names() == ["nfa_render_raw_fwd", "nfa_render_raw_bwd"]
    assert set(outs) == {"colors", "opacities", "depths", "weights", "trans", "alphas"}   # activated values only on request
    fwd = log.calls[0][1]
    assert fwd[16] is None and fwd[17] is None   # act_sigmas, act_rgbs: not written either


def test_other_inputs_take_the_torch_composition(dev, monkeypatch):
    """t_starts that require a gradient: no nfa_render_raw_* call, same results within rounding."""
    c = case(dev)
    want, _ = run(c, "trunc_exp", "sigmoid", False)
    log = CallLog(monkeypatch)
    ts = c["ts"].clone().requires_grad_(True)
    colors, opac, _, _ = rendering_from_raw(ts, c["te"], c["raw_rgb"], c["raw_sig"], c["ri"], c["rays"].R, density_bias=BIAS,
                                            selector=c["sel"])
    assert not any(n.startswith("nfa_render_raw") for n in log.names())
    assert torch.allclose(colors, want["colors"], rtol=1e-4, atol=1e-5) and torch.allclose(opac, want["opacities"], rtol=1e-4, atol=1e-5)
    (g,) = torch.autograd.grad(opac.sum(), ts)
    assert bool(torch.isfinite(g).all())


PARTIAL_LOSSES = {"opacity": lambda colors, opac, depth: opac.sum(),
                  "depth": lambda colors, opac, depth: depth.sum(),
                  "colour_and_opacity": lambda colors, opac, depth: (colors ** 2).sum() + opac.sum()}


@pytest.mark.parametrize("loss", list(PARTIAL_LOSSES))
def test_partial_losses_give_the_same_gradients_on_all_three_paths(dev, monkeypatch, loss):
    """A gradient that arrives only at opacity, only at depth (through its normalisation: at opacity and the raw depth),
    or at colours and opacity: the passes then run without some of the per-ray gradient arrays (null pointers).  The
    fused pass, the two-pass composition and rendering_from_raw without activations must agree bit for bit."""
    c = case(dev)
    sig = (c["raw_sig"].abs() * 0.3).contiguous()
    rgb = torch.sigmoid(c["raw_rgb"])
    R = c["rays"].R
    log = CallLog(monkeypatch)

    def grads(render):
        s, r = sig.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
        colors, opac, depth = render(s, r)
        return torch.autograd.grad(PARTIAL_LOSSES[loss](colors, opac, depth), [s, r], allow_unused=True)

    def rendering(fuse):
        def render(s, r):
            na.volrend.FUSE_RENDERING = fuse
            try:
                return na.rendering(c["ts"], c["te"], c["ri"], n_rays=R, rgb_sigma_fn=lambda *_: (r, s))[:3]
            finally:
                na.volrend.FUSE_RENDERING = True
        return render

    def from_raw(s, r):
        return rendering_from_raw(c["ts"], c["te"], r, s, c["ri"], R, density_activation="none", density_bias=0.0,
                                  rgb_activation="none", selector=None)[:3]

    fused, two_pass, raw = grads(rendering(True)), grads(rendering(False)), grads(from_raw)
    names = log.names()
    assert [n for n in names if n.endswith("_bwd")] == ["nfa_render_fused_bwd", "nfa_render_accumulate_bwd",
                                                        "nfa_render_from_density_bwd", "nfa_render_raw_bwd"]
    # which per-ray gradients reached the passes: (g_colors, g_opacities, g_depths)
    present = {"opacity": (False, True, False), "depth": (False, True, True), "colour_and_opacity": (True, True, False)}[loss]
    by_name = dict(log.calls)
    for entry, first in (("nfa_render_fused_bwd", 5), ("nfa_render_accumulate_bwd", 4), ("nfa_render_raw_bwd", 9)):
        assert tuple(p is not None for p in by_name[entry][first:first + 3]) == present, entry

    def is_zero(g):
        return g is None or not bool(g.any())

    for which, a, b, d in zip(("g_sigmas", "g_rgbs"), fused, two_pass, raw):
        if any(is_zero(g) for g in (a, b, d)):
            assert is_zero(a) and is_zero(b) and is_zero(d), (loss, which)
        else:
            assert torch.equal(a, b) and torch.equal(a, d), (loss, which)
    assert not is_zero(fused[0])                             # every one of these losses depends on the densities
    assert is_zero(fused[1]) == (not present[0])             # and on the colours only through `colors`

"""CPU: ``rendering_from_raw``'s torch composition (what every input outside the native path takes), its argument
checks, and the argument checks of the two C entry points behind the native path."""
import math

import pytest
import torch

import rawrender_reference as RR
import seg_reference as SR


def _case(seed=0, masked=True):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor([0, 1, 3, 0, 17, 40, 2, 0])
    rays = SR.Rays(counts)
    n = rays.n
    ts = torch.rand(n, generator=g) * 4.0
    te = ts + 0.001 + torch.rand(n, generator=g) * 0.02
    raw_sig = torch.rand(n, generator=g) * 12.0 - 6.0
    raw_rgb = torch.rand(n, 3, generator=g) * 16.0 - 8.0
    sel = (torch.rand(n, generator=g) > 0.2) if masked else None
    gl = {"colors": torch.randn(rays.R, 3, generator=g), "opacities": torch.randn(rays.R, 1, generator=g),
          "weights": torch.randn(n, generator=g), "trans": torch.randn(n, generator=g), "alphas": torch.randn(n, generator=g)}
    return rays, ts, te, raw_sig, raw_rgb, sel, gl


def _close(name, got, want, rtol=2e-5, atol=1e-6):
    err = (got.double() - want.double()).abs()
    tol = atol + rtol * want.double().abs()
    assert bool((err <= tol).all()), (name, float((err / tol).max()))


@pytest.mark.parametrize("col", RR.RGB)
@pytest.mark.parametrize("dens", RR.DENSITY)
def test_torch_composition_matches_float64(dens, col):
    from nerfacc_amd.rawrender import rendering_from_raw
    rays, ts, te, raw_sig, raw_rgb, sel, gl = _case(1)
    bias = -1.0
    # float64 in: another dtype than the native path's, and the comparison is tight
    ts, te, raw_sig, raw_rgb = ts.double(), te.double(), raw_sig.double(), raw_rgb.double()
    gl = {k: v.double() for k, v in gl.items()}
    rs, rc = raw_sig.clone().requires_grad_(True), raw_rgb.clone().requires_grad_(True)
    colors, opac, depth, ex = rendering_from_raw(ts, te, rc, rs, rays.ray_ids, rays.R, density_activation=dens,
                                                 density_bias=bias, rgb_activation=col, selector=sel, return_activated=True)
    assert colors.shape == (rays.R, 3) and opac.shape == (rays.R, 1) and depth.shape == (rays.R, 1)
    assert set(ex) == {"weights", "trans", "alphas", "sigmas", "rgbs"}
    outs = [colors, opac, ex["weights"], ex["trans"], ex["alphas"]]
    keys = ["colors", "opacities", "weights", "trans", "alphas"]
    g_s, g_c = torch.autograd.grad(outs, [rs, rc], [gl[k] for k in keys])
    ref = RR.render(rays, ts, te, raw_sig, raw_rgb, dens, bias, col, sel, grads=gl)
    # (rendering clamps the opacity at the eps of the colours' dtype)
    ref["depths"] = SR.finish_rendering(ref["colors"], ref["opacities"], ref["depths_raw"], torch.finfo(torch.float64).eps)[2]
    for k, got in zip(keys + ["depths", "sigmas", "rgbs"], outs + [depth, ex["sigmas"], ex["rgbs"]]):
        _close(k, got.detach(), ref[k], rtol=1e-10, atol=1e-13)
    _close("g_raw_sigmas", g_s, ref["g_raw_sigmas"], rtol=1e-9, atol=1e-12 * float(ref["g_raw_sigmas"].abs().max()))
    _close("g_raw_rgbs", g_c, ref["g_raw_rgbs"], rtol=1e-9, atol=1e-12 * float(ref["g_raw_rgbs"].abs().max()))


def test_activated_values_are_returned_only_on_request():
    from nerfacc_amd.rawrender import rendering_from_raw
    rays, ts, te, raw_sig, raw_rgb, sel, _ = _case(2)
    ex = rendering_from_raw(ts, te, raw_rgb, raw_sig, rays.ray_ids, rays.R)[3]
    assert set(ex) == {"weights", "trans", "alphas"}


def test_trunc_exp_gradient_is_clamped_at_15():
    from nerfacc_amd.rawrender import activate_density
    for z, want in ((18.0, math.exp(15.0)), (3.0, math.exp(3.0))):
        x = torch.tensor([z - 0.5], dtype=torch.float64, requires_grad=True)
        s = activate_density(x, "trunc_exp", 0.5)
        assert float(s.detach()) == pytest.approx(math.exp(z), rel=1e-12)
        (g,) = torch.autograd.grad(s, x, torch.tensor([2.0], dtype=torch.float64))
        assert float(g) == pytest.approx(2.0 * want, rel=1e-12)
    # the float64 restatement states the same derivative
    z = torch.tensor([18.0, 3.0], dtype=torch.float64)
    assert torch.allclose(RR.density_grad(z, "trunc_exp"), torch.tensor([math.exp(15.0), math.exp(3.0)], dtype=torch.float64))


@pytest.mark.parametrize("dens", RR.DENSITY)
def test_masked_samples_are_exact_zeros(dens):
    from nerfacc_amd.rawrender import rendering_from_raw
    rays, ts, te, raw_sig, raw_rgb, sel, gl = _case(3)
    off = (~sel).nonzero().flatten()
    assert off.numel() >= 3
    raw_sig = raw_sig.clone()
    raw_sig[off[0]] = float("inf")
    raw_sig[off[1]] = float("-inf")
    rs, rc = raw_sig.clone().requires_grad_(True), raw_rgb.clone().requires_grad_(True)
    colors, opac, depth, ex = rendering_from_raw(ts, te, rc, rs, rays.ray_ids, rays.R, density_activation=dens,
                                                 selector=sel, return_activated=True)
    for k in ("sigmas", "alphas", "weights"):
        assert bool((ex[k][off] == 0).all()), k
    for t in (colors, opac, depth, ex["trans"]):
        assert bool(torch.isfinite(t).all())
    (g_s,) = torch.autograd.grad([colors, opac, depth, ex["trans"]], [rs],
                                 [gl["colors"], gl["opacities"], gl["opacities"], gl["trans"]])
    assert bool((g_s[off] == 0).all()) and bool(torch.isfinite(g_s).all())
    # and the samples behind the mask do not change the others' results
    ref = RR.render(rays, ts, te, raw_sig, raw_rgb, dens, 0.0, "sigmoid", sel)
    _close("colors", colors.detach(), ref["colors"])
    _close("trans", ex["trans"].detach(), ref["trans"])


def test_column_and_flat_densities_agree():
    from nerfacc_amd.rawrender import rendering_from_raw
    rays, ts, te, raw_sig, raw_rgb, sel, gl = _case(4)
    res = []
    for shape in ((rays.n,), (rays.n, 1)):
        rs = raw_sig.clone().view(shape).requires_grad_(True)
        colors, opac, depth, ex = rendering_from_raw(ts, te, raw_rgb, rs, rays.ray_ids, rays.R, selector=sel)
        (g,) = torch.autograd.grad([colors, depth], [rs], [gl["colors"], gl["opacities"]])
        assert g.shape == shape and ex["weights"].shape == (rays.n,)
        res.append((colors.detach(), opac.detach(), depth.detach(), g.view(-1)))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_render_bkgd_and_empty_input():
    from nerfacc_amd.rawrender import rendering_from_raw
    rays, ts, te, raw_sig, raw_rgb, sel, _ = _case(5)
    bk = torch.tensor([0.25, 0.5, 0.75])
    c0, o0, _, _ = rendering_from_raw(ts, te, raw_rgb, raw_sig, rays.ray_ids, rays.R)
    c1, o1, _, _ = rendering_from_raw(ts, te, raw_rgb, raw_sig, rays.ray_ids, rays.R, render_bkgd=bk)
    assert torch.equal(o0, o1) and torch.allclose(c1, c0 + bk * (1.0 - o0))
    e = torch.empty(0)
    c, o, d, ex = rendering_from_raw(e, e, torch.empty(0, 3), e, torch.empty(0, dtype=torch.long), 4)
    assert c.shape == (4, 3) and not c.any() and not o.any() and not d.any() and ex["weights"].shape == (0,)


def test_argument_errors():
    from nerfacc_amd.rawrender import rendering_from_raw
    rays, ts, te, raw_sig, raw_rgb, sel, _ = _case(6)
    ri, R, n = rays.ray_ids, rays.R, rays.n
    with pytest.raises(ValueError, match="density_activation"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig, ri, R, density_activation="gelu")
    with pytest.raises(ValueError, match="rgb_activation"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig, ri, R, rgb_activation="tanh")
    with pytest.raises(AssertionError, match="n_rays"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig, ri)
    with pytest.raises(AssertionError, match="raw_sigmas"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig[:-1], ri, R)
    with pytest.raises(AssertionError, match="raw_sigmas"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig.view(n, 1).expand(n, 2), ri, R)
    with pytest.raises(AssertionError, match="raw_rgbs"):
        rendering_from_raw(ts, te, raw_rgb[:, :2], raw_sig, ri, R)
    with pytest.raises(AssertionError, match="same shape"):
        rendering_from_raw(ts, te[:-1], raw_rgb, raw_sig, ri, R)
    with pytest.raises(AssertionError, match="selector"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig, ri, R, selector=sel.float())
    with pytest.raises(AssertionError, match="selector"):
        rendering_from_raw(ts, te, raw_rgb, raw_sig, ri, R, selector=sel[:-1])


def test_names_are_not_part_of_the_mirrored_api():
    import nerfacc_amd
    from nerfacc_amd import rawrender
    assert callable(rawrender.rendering_from_raw)
    assert "rendering_from_raw" not in nerfacc_amd.__all__ and "rawrender" not in nerfacc_amd.__all__


# ----------------------------------------------------------------------------- C ABI argument checks
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_render_raw_fwd": "t_starts t_ends raw_sigmas raw_rgbs selector density_act density_bias rgb_act packed_info tiles n_tiles "
                          "n_rays n_elems weights trans alphas act_sigmas act_rgbs colors opacities depths stream",
    "nfa_render_raw_bwd": "t_starts t_ends raw_sigmas raw_rgbs selector density_act density_bias rgb_act trans g_colors "
                          "g_opacities g_depths g_weights g_trans g_alphas packed_info tiles n_tiles n_rays n_elems "
                          "grad_raw_sigmas grad_raw_rgbs stream",
}
_SCALARS = {"density_act": 1, "density_bias": -1.0, "rgb_act": 1, "n_tiles": 1, "n_rays": 4, "n_elems": 16}
_TOO_MANY = (1 << 31) - 64


def _cases():
    cases = []
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        cases += [
            (fn, {"n_rays": -1}, f"{nm}: negative size"),
            (fn, {"n_elems": -1}, f"{nm}: negative size"),
            (fn, {"n_rays": _TOO_MANY}, f"{nm}: too many rays"),
            (fn, {"packed_info": None}, f"{nm}: packed_info/tiles is null"),
            (fn, {"tiles": None}, f"{nm}: packed_info/tiles is null"),
            (fn, {"n_tiles": 0}, f"{nm}: packed_info/tiles is null"),
            # nothing to do: accepted before any other argument is looked at
            (fn, {"n_rays": 0, "n_elems": 0, "density_act": 9, "all_null": True}, None),
            (fn, {"density_act": 5}, f"{nm}: density_act must be in 0..4 (got 5)"),
            (fn, {"density_act": -1}, f"{nm}: density_act must be in 0..4 (got -1)"),
            (fn, {"rgb_act": 2}, f"{nm}: rgb_act must be 0 or 1 (got 2)"),
            (fn, {"density_act": 7, "t_starts": None}, f"{nm}: density_act must be in 0..4 (got 7)"),
            *[(fn, {a: None}, f"{nm}: null pointer") for a in "t_starts t_ends raw_sigmas raw_rgbs".split()],
        ]
    cases += [
        ("nfa_render_raw_fwd", {"n_rays": 0, "colors": None}, None),
        *[("nfa_render_raw_fwd", {a: None}, "render_raw_fwd: null pointer") for a in "colors opacities depths".split()],
        ("nfa_render_raw_bwd", {"n_elems": 0, "t_starts": None}, None),
        ("nfa_render_raw_bwd", {"trans": None}, "render_raw_bwd: null pointer"),
        ("nfa_render_raw_bwd", {"grad_raw_sigmas": None, "grad_raw_rgbs": None}, "render_raw_bwd: null pointer"),
    ]
    return cases


def test_entry_point_argument_errors():
    """Both entry points check their arguments in a fixed order, on the host, before a launch."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn, kw, msg in _cases():
        kw = dict(kw)
        all_null = kw.pop("all_null", False)
        args = [kw[a] if a in kw else _SCALARS[a] if a in _SCALARS else (None if all_null or a == "stream" else P)
                for a in _ARGS[fn].split()]
        assert len(args) == len(B._SIGS[fn])
        lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
        rc = getattr(lib, fn)(*args)
        if msg is None:
            assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
        else:
            assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())

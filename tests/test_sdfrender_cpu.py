"""CPU: the float64 restatement of ``rendering_from_sdf`` against a per-ray loop, the torch compositions ``neus_alpha`` /
``laplace_density`` and the fallback of ``rendering_from_sdf`` against that restatement, their gradients by gradcheck,
NeuS' opacity against the published formula with its 1e-5, the mask, the argument errors, and the argument checks of the
two C entry points behind the native path."""
import math

import pytest
import torch

import sdfrender_reference as XR
import seg_reference as SR

PARAM = {"neus": 64.0, "volsdf": 0.05}
RATIO = 0.7


def _case(seed=0, masked=True, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    rays = SR.Rays(torch.tensor([0, 1, 3, 0, 17, 40, 2, 0]))
    n = rays.n
    ts = torch.rand(n, generator=g) * 4.0
    te = ts + 0.001 + torch.rand(n, generator=g) * 0.02
    sdf = torch.rand(n, generator=g) * 0.4 - 0.2
    cos = torch.rand(n, generator=g) * 2.4 - 1.2
    raw_rgb = torch.rand(n, 3, generator=g) * 16.0 - 8.0
    sel = (torch.rand(n, generator=g) > 0.2) if masked else None
    gl = {"colors": torch.randn(rays.R, 3, generator=g), "opacities": torch.randn(rays.R, 1, generator=g),
          "weights": torch.randn(n, generator=g), "trans": torch.randn(n, generator=g), "alphas": torch.randn(n, generator=g)}
    t = dict(ts=ts, te=te, sdf=sdf, cos=cos, raw_rgb=raw_rgb)
    return rays, {k: v.to(dtype) for k, v in t.items()}, sel, {k: v.to(dtype) for k, v in gl.items()}


def _away_from_kinks(sdf, cos):
    """|cos| and |cos - 1| >= 0.05, |sdf| >= 1e-3: where the conversions are not differentiable."""
    cos = torch.where(cos.abs() < 0.05, torch.full_like(cos, 0.05), cos)
    cos = torch.where((cos - 1.0).abs() < 0.05, torch.full_like(cos, 0.95), cos)
    sdf = torch.where(sdf.abs() < 1e-3, torch.full_like(sdf, 1e-3), sdf)
    return sdf, cos


def _kw(model, param, cos, **more):
    return dict(model=model, **(dict(inv_s=param, cos=cos, cos_anneal_ratio=RATIO) if model == "neus" else dict(beta=param)), **more)


def _close(name, got, want, rtol, atol):
    err = (got.double() - want.double()).abs()
    tol = atol + rtol * want.double().abs()
    assert bool((err <= tol).all()), (name, float((err / tol).max()))


@pytest.mark.parametrize("model", XR.MODELS)
def test_reference_agrees_with_a_per_ray_loop(model):
    rays, t, sel, _ = _case(1)
    ref = XR.render(rays, t["ts"], t["te"], t["sdf"], t["cos"], t["raw_rgb"], model, PARAM[model], RATIO, "sigmoid", sel)
    s, r = PARAM[model], RATIO
    i = 0
    for ray, cnt in enumerate(rays.counts.tolist()):
        S, col, op, dep = 0.0, [0.0, 0.0, 0.0], 0.0, 0.0
        for _ in range(cnt):
            sdf, cs, a, b = (float(t[k][i]) for k in ("sdf", "cos", "ts", "te"))
            d = b - a
            if not bool(sel[i]):
                x = 0.0
            elif model == "neus":
                ct = -(max(0.5 - 0.5 * cs, 0.0) * (1.0 - r) + max(-cs, 0.0) * r)
                n, p = sdf + ct * d / 2.0, sdf - ct * d / 2.0
                log_phi = lambda y: -math.log1p(math.exp(-y)) if y > 0 else y - math.log1p(math.exp(y))
                x = max(log_phi(s * p) - log_phi(s * n), 0.0)
            else:
                e = 0.5 * math.exp(-abs(sdf) / s)
                x = (e if sdf >= 0 else 1.0 - e) / s * d
            T, al = math.exp(-S), 1.0 - math.exp(-x)
            w = T * al
            assert float(ref["x"][i]) == pytest.approx(x, rel=1e-9, abs=1e-15)
            for k, v in (("trans", T), ("alphas", al), ("weights", w)):
                assert float(ref[k][i]) == pytest.approx(v, rel=1e-9, abs=1e-15), (k, i)
            c = torch.sigmoid(t["raw_rgb"][i])
            col = [col[k] + w * float(c[k]) for k in range(3)]
            op, dep, S, i = op + w, dep + w * (a + b) / 2.0, S + x, i + 1
        assert ref["colors"][ray].tolist() == pytest.approx(col, rel=1e-9, abs=1e-15)
        assert float(ref["opacities"][ray]) == pytest.approx(op, rel=1e-9, abs=1e-15)
        assert float(ref["depths_raw"][ray]) == pytest.approx(dep, rel=1e-9, abs=1e-15)
    assert i == rays.n


@pytest.mark.parametrize("model", XR.MODELS)
def test_reference_derivatives_are_those_of_autograd(model):
    rays, t, sel, gl = _case(2)
    ref = XR.render(rays, t["ts"], t["te"], t["sdf"], t["cos"], t["raw_rgb"], model, PARAM[model], RATIO, "sigmoid", sel, grads=gl)
    D = XR.derivatives(model, t["sdf"], t["cos"], t["te"] - t["ts"], PARAM[model], RATIO, sel)
    _close("sdf", ref["g_x"] * D["sdf"], ref["g_sdfs"], 1e-11, 1e-13)
    _close("param", (ref["g_x"] * D["param"]).sum(), ref["g_param"], 1e-11, 1e-13)
    if model == "neus":
        _close("cos", ref["g_x"] * D["cos"], ref["g_cos"], 1e-11, 1e-13)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", XR.MODELS)
def test_conversions_and_fallback_match_float64(model, dtype):
    from nerfacc_amd.sdfrender import laplace_density, neus_alpha, rendering_from_sdf
    rays, t, sel, gl = _case(3, dtype=dtype)
    f64 = dtype == torch.float64
    # float32: a few hundred roundings' worth; the tight comparison of float32 results is the GPU test's
    rtol, atol = (1e-9, 1e-12) if f64 else (2e-4, 2e-5)
    par = PARAM[model]
    ref = XR.render(rays, t["ts"], t["te"], t["sdf"], t["cos"], t["raw_rgb"], model, par, RATIO, "sigmoid", sel, grads=gl)
    ref["depths"] = SR.finish_rendering(ref["colors"], ref["opacities"], ref["depths_raw"], torch.finfo(dtype).eps)[2]

    # the conversions alone, without the mask
    d = t["te"] - t["ts"]
    x = XR.convert(model, t["sdf"].double(), t["cos"].double(), d.double(), par, RATIO)
    if model == "neus":
        _close("neus_alpha", neus_alpha(t["sdf"], t["cos"], d, par, RATIO), 1.0 - torch.exp(-x), rtol, atol)
        _close("neus_alpha", neus_alpha(t["sdf"], t["cos"], d, torch.tensor([par], dtype=dtype), RATIO), 1.0 - torch.exp(-x), rtol, atol)
    else:
        _close("laplace_density", laplace_density(t["sdf"], par), x / d.double(), rtol, atol)

    sd, cs, rc = (t[k].clone().requires_grad_(True) for k in ("sdf", "cos", "raw_rgb"))
    p = torch.tensor([par], dtype=dtype, requires_grad=True)
    colors, opac, depth, ex = rendering_from_sdf(t["ts"], t["te"], rc, sd, rays.ray_ids, rays.R, **_kw(model, p, cs, selector=sel))
    assert colors.shape == (rays.R, 3) and opac.shape == (rays.R, 1) and depth.shape == (rays.R, 1)
    assert set(ex) == {"weights", "trans", "alphas"} and colors.dtype == dtype
    outs = [colors, opac, ex["weights"], ex["trans"], ex["alphas"]]
    keys = ["colors", "opacities", "weights", "trans", "alphas"]
    ins = [sd, rc, p] + ([cs] if model == "neus" else [])
    g = torch.autograd.grad(outs, ins, [gl[k] for k in keys])
    for k, got in zip(keys + ["depths"], outs + [depth]):
        _close(k, got.detach(), ref[k], rtol, atol)
    for k, got in zip(["g_sdfs", "g_raw_rgbs", "g_param"] + (["g_cos"] if model == "neus" else []), g):
        assert got.shape == (p.shape if k == "g_param" else ref[k].shape)
        _close(k, got.reshape(ref[k].shape), ref[k], rtol, atol * max(1.0, float(ref[k].abs().max())))


def test_column_sdfs_and_float_parameters_agree_with_tensors():
    from nerfacc_amd.sdfrender import rendering_from_sdf
    rays, t, sel, _ = _case(4)
    for model in XR.MODELS:
        par = PARAM[model]
        a = rendering_from_sdf(t["ts"], t["te"], t["raw_rgb"], t["sdf"], rays.ray_ids, rays.R, **_kw(model, par, t["cos"], selector=sel))
        b = rendering_from_sdf(t["ts"], t["te"], t["raw_rgb"], t["sdf"].view(-1, 1), rays.ray_ids, rays.R,
                               **_kw(model, torch.tensor(par, dtype=torch.float64), t["cos"], selector=sel))
        for u, v in zip(a[:3], b[:3]):
            assert torch.equal(u, v)
        assert b[3]["weights"].shape == (rays.n,)


@pytest.mark.parametrize("model", XR.MODELS)
def test_gradcheck(model):
    from nerfacc_amd.sdfrender import laplace_density, neus_alpha, rendering_from_sdf
    rays, t, sel, _ = _case(5)
    sdf, cos = _away_from_kinks(t["sdf"], t["cos"])
    d = t["te"] - t["ts"]
    par = torch.tensor([PARAM[model]], dtype=torch.float64, requires_grad=True)
    sdf, cos = sdf.clone().requires_grad_(True), cos.clone().requires_grad_(True)
    if model == "neus":
        assert torch.autograd.gradcheck(lambda s, c, p: neus_alpha(s, c, d, p, RATIO), (sdf, cos, par), eps=1e-7, atol=1e-6)
    else:
        assert torch.autograd.gradcheck(lambda s, p: laplace_density(s, p), (sdf, par), eps=1e-7, atol=1e-5)

    def render(s, c, p):
        colors, opac, depth, ex = rendering_from_sdf(t["ts"], t["te"], t["raw_rgb"], s, rays.ray_ids, rays.R,
                                                     **_kw(model, p, c, selector=sel))
        return colors, opac, ex["weights"], ex["trans"], ex["alphas"]

    assert torch.autograd.gradcheck(render, (sdf, cos, par), eps=1e-7, atol=1e-5)


def test_neus_alpha_is_within_1e_5_over_phi_of_the_published_formula():
    from nerfacc_amd.sdfrender import neus_alpha
    g = torch.Generator().manual_seed(6)
    n = 20000
    sdf = (torch.rand(n, generator=g, dtype=torch.float64) * 0.6 - 0.3)
    cos = torch.rand(n, generator=g, dtype=torch.float64) * 2.4 - 1.2
    d = 0.001 + torch.rand(n, generator=g, dtype=torch.float64) * 0.05
    for inv_s, r in ((64.0, 1.0), (3.0, 0.0), (300.0, 0.4)):
        # the published block (NeuS, models/renderer.py), restated
        iter_cos = -(torch.relu(-cos * 0.5 + 0.5) * (1.0 - r) + torch.relu(-cos) * r)
        nxt, prv = sdf + iter_cos * d * 0.5, sdf - iter_cos * d * 0.5
        prev_cdf, next_cdf = torch.sigmoid(prv * inv_s), torch.sigmoid(nxt * inv_s)
        published = ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).clip(0.0, 1.0)
        got = neus_alpha(sdf, cos, d, inv_s, r)
        bound = 1e-5 / prev_cdf
        assert bool(((got - published).abs() <= bound * (1.0 + 1e-9) + 1e-15).all()), float(((got - published).abs() / bound).max())


@pytest.mark.parametrize("model", XR.MODELS)
def test_masked_samples_are_exact_zeros(model):
    from nerfacc_amd.sdfrender import rendering_from_sdf
    rays, t, sel, gl = _case(7, dtype=torch.float32)
    off = (~sel).nonzero().flatten()
    assert off.numel() >= 3
    sdf = t["sdf"].clone()
    sdf[off[0]] = float("nan")
    sdf[off[1]] = float("inf")
    cos = t["cos"].clone()
    cos[off[2]] = float("nan")
    sd, cs, rc = sdf.clone().requires_grad_(True), cos.clone().requires_grad_(True), t["raw_rgb"].clone().requires_grad_(True)
    p = torch.tensor([PARAM[model]], requires_grad=True)
    colors, opac, depth, ex = rendering_from_sdf(t["ts"], t["te"], rc, sd, rays.ray_ids, rays.R, **_kw(model, p, cs, selector=sel))
    for k in ("alphas", "weights"):
        assert bool((ex[k][off] == 0).all()), k
    for v in (colors, opac, depth, ex["trans"]):
        assert bool(torch.isfinite(v).all())
    g = torch.autograd.grad([colors, opac, depth, ex["trans"], ex["weights"]], [sd, cs, rc, p],
                            [gl["colors"], gl["opacities"], gl["opacities"], gl["trans"], gl["weights"]], allow_unused=True)
    assert bool((g[0][off] == 0).all()) and bool((g[2][off] == 0).all())
    assert all(v is None or bool(torch.isfinite(v).all()) for v in g)
    if model == "neus":
        assert bool((g[1][off] == 0).all())
    # and the samples behind the mask do not change the others' results
    ref = XR.render(rays, t["ts"], t["te"], t["sdf"], t["cos"], t["raw_rgb"], model, PARAM[model], RATIO, "sigmoid", sel)
    _close("colors", colors.detach(), ref["colors"], 2e-4, 2e-5)
    _close("trans", ex["trans"].detach(), ref["trans"], 2e-4, 2e-5)


def test_cos_at_or_above_one_gives_alpha_exactly_zero():
    from nerfacc_amd.sdfrender import neus_alpha
    for dtype in (torch.float32, torch.float64):
        sdf = torch.tensor([-0.2, -0.01, 0.0, 0.03, 0.2], dtype=dtype)
        d = torch.full_like(sdf, 0.01)
        for c in (1.0, 1.2):
            for r in (0.0, 0.3, 1.0):
                s = sdf.clone().requires_grad_(True)
                a = neus_alpha(s, torch.full_like(sdf, c), d, 64.0, r)
                assert bool((a == 0).all()), (c, r, a)
                (g,) = torch.autograd.grad(a.sum(), s)
                assert bool((g == 0).all())


def test_render_bkgd_and_empty_input():
    from nerfacc_amd.sdfrender import rendering_from_sdf
    rays, t, sel, _ = _case(8, dtype=torch.float32)
    bk = torch.tensor([0.25, 0.5, 0.75])
    args = (t["ts"], t["te"], t["raw_rgb"], t["sdf"], rays.ray_ids, rays.R)
    c0, o0, _, _ = rendering_from_sdf(*args, model="volsdf", beta=0.05)
    c1, o1, _, _ = rendering_from_sdf(*args, model="volsdf", beta=0.05, render_bkgd=bk)
    assert torch.equal(o0, o1) and torch.allclose(c1, c0 + bk * (1.0 - o0))
    e = torch.empty(0)
    for kw in (dict(model="neus", inv_s=64.0, cos=e), dict(model="volsdf", beta=0.05)):
        c, o, d, ex = rendering_from_sdf(e, e, torch.empty(0, 3), e, torch.empty(0, dtype=torch.long), 4, **kw)
        assert c.shape == (4, 3) and not c.any() and not o.any() and not d.any() and ex["weights"].shape == (0,)


def test_argument_errors():
    from nerfacc_amd.sdfrender import rendering_from_sdf
    rays, t, sel, _ = _case(9, dtype=torch.float32)
    args = (t["ts"], t["te"], t["raw_rgb"], t["sdf"], rays.ray_ids, rays.R)
    cos = t["cos"]
    with pytest.raises(ValueError, match="model"):
        rendering_from_sdf(*args, model="unisurf", inv_s=64.0, cos=cos)
    with pytest.raises(ValueError, match="rgb_activation"):
        rendering_from_sdf(*args, model="neus", inv_s=64.0, cos=cos, rgb_activation="tanh")
    with pytest.raises(ValueError, match="inv_s"):
        rendering_from_sdf(*args, model="neus", cos=cos)
    with pytest.raises(ValueError, match="cos"):
        rendering_from_sdf(*args, model="neus", inv_s=64.0)
    with pytest.raises(ValueError, match="beta"):
        rendering_from_sdf(*args, model="volsdf")
    with pytest.raises(ValueError, match="beta"):
        rendering_from_sdf(*args, model="volsdf", inv_s=64.0)
    for bad in (0.0, -0.05, float("nan")):
        with pytest.raises(ValueError, match="beta must be > 0"):
            rendering_from_sdf(*args, model="volsdf", beta=bad)
        with pytest.raises(ValueError, match="inv_s must be > 0"):
            rendering_from_sdf(*args, model="neus", inv_s=bad, cos=cos)
    with pytest.raises(ValueError, match="1-element"):
        rendering_from_sdf(*args, model="volsdf", beta=torch.full((rays.n,), 0.05))
    with pytest.raises(AssertionError, match="n_rays"):
        rendering_from_sdf(*args[:5], model="volsdf", beta=0.05)
    with pytest.raises(AssertionError, match="sdfs"):
        rendering_from_sdf(t["ts"], t["te"], t["raw_rgb"], t["sdf"][:-1], rays.ray_ids, rays.R, model="volsdf", beta=0.05)
    with pytest.raises(AssertionError, match="cos"):
        rendering_from_sdf(*args, model="neus", inv_s=64.0, cos=cos[:-1])
    with pytest.raises(AssertionError, match="selector"):
        rendering_from_sdf(*args, model="volsdf", beta=0.05, selector=sel.float())


def test_names_are_not_part_of_the_mirrored_api():
    import nerfacc_amd
    from nerfacc_amd import sdfrender
    assert callable(sdfrender.rendering_from_sdf) and callable(sdfrender.neus_alpha) and callable(sdfrender.laplace_density)
    for name in ("rendering_from_sdf", "neus_alpha", "laplace_density", "sdfrender"):
        assert name not in nerfacc_amd.__all__


# ----------------------------------------------------------------------------- C ABI argument checks
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_render_sdf_fwd": "t_starts t_ends sdfs cos raw_rgbs selector model param cos_anneal_ratio rgb_act packed_info tiles n_tiles "
                          "n_rays n_elems weights trans alphas colors opacities depths stream",
    "nfa_render_sdf_bwd": "t_starts t_ends sdfs cos raw_rgbs selector model param cos_anneal_ratio rgb_act trans g_colors "
                          "g_opacities g_depths g_weights g_trans g_alphas packed_info tiles n_tiles n_rays n_elems "
                          "grad_sdfs grad_cos grad_param grad_raw_rgbs stream",
}
_SCALARS = {"model": 0, "cos_anneal_ratio": 1.0, "rgb_act": 1, "n_tiles": 1, "n_rays": 4, "n_elems": 16}
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
            (fn, {"n_rays": 0, "n_elems": 0, "model": 9, "all_null": True}, None),
            (fn, {"model": 2}, f"{nm}: model must be 0 or 1 (got 2)"),
            (fn, {"model": -1}, f"{nm}: model must be 0 or 1 (got -1)"),
            (fn, {"rgb_act": 2}, f"{nm}: rgb_act must be 0 or 1 (got 2)"),
            (fn, {"model": 7, "t_starts": None}, f"{nm}: model must be 0 or 1 (got 7)"),
            *[(fn, {a: None}, f"{nm}: null pointer") for a in "t_starts t_ends sdfs raw_rgbs".split()],
            (fn, {"cos": None}, f"{nm}: cos is null (NFA_SDF_NEUS)"),
            (fn, {"param": None}, f"{nm}: param is null"),
            (fn, {"cos": None, "param": None}, f"{nm}: cos is null (NFA_SDF_NEUS)"),
            (fn, {"model": 1, "cos": None, "param": None, "grad_cos": None}, f"{nm}: param is null"),
        ]
    cases += [
        ("nfa_render_sdf_fwd", {"n_rays": 0, "colors": None}, None),
        *[("nfa_render_sdf_fwd", {a: None}, "render_sdf_fwd: null pointer") for a in "colors opacities depths".split()],
        ("nfa_render_sdf_bwd", {"n_elems": 0, "t_starts": None}, None),
        ("nfa_render_sdf_bwd", {"trans": None}, "render_sdf_bwd: null pointer"),
        ("nfa_render_sdf_bwd", {"grad_sdfs": None, "grad_cos": None, "grad_param": None, "grad_raw_rgbs": None},
         "render_sdf_bwd: null pointer"),
        ("nfa_render_sdf_bwd", {"model": 1, "cos": None}, "render_sdf_bwd: grad_cos given with NFA_SDF_VOLSDF"),
    ]
    return cases


def test_entry_point_argument_errors():
    """Both entry points check their arguments in a fixed order, on the host, before a launch."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn, kw, msg in _cases():
        kw = dict(kw)
        all_null = kw.pop("all_null", False)
        names = _ARGS[fn].split()
        kw = {k: v for k, v in kw.items() if k in names}
        args = [kw[a] if a in kw else _SCALARS[a] if a in _SCALARS else (None if all_null or a == "stream" else P) for a in names]
        assert len(args) == len(B._SIGS[fn])
        lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
        rc = getattr(lib, fn)(*args)
        if msg is None:
            assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
        else:
            assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())

"""GPU: ``rendering_from_sdf`` on its native path (nfa_render_sdf_fwd / nfa_render_sdf_bwd, csrc/segscan.hip).

Every output and every gradient -- the scalar parameter's included -- against the float64 restatement
(tests/sdfrender_reference.py) within the per-element bounds of tests/seg_reference.py, widened only by the roundings the
conversions add (counted below); the scalar form (inputs that are not 16-byte aligned) must reproduce the vector form
bit for bit; two runs give the same bits; masked samples are exact zeros; and a step is exactly two native calls that
never wait for the device.
"""
import numpy as np
import pytest
import torch

import sdfrender_reference as XR
import seg_reference as SR
from nerfacc_amd import _backend as B
from nerfacc_amd._segments import seginfo_from_ray_indices
from nerfacc_amd.sdfrender import rendering_from_sdf

pytestmark = pytest.mark.gpu

EPS = SR.EPS32
TINY = 2.0 ** -126 * SR.K_ROUND    # results below float32's normal range have no relative precision
INV_S, BETA, RATIO = 64.0, 0.05, 0.7
PARAM = {"neus": INV_S, "volsdf": BETA}
SDF_MAX, DELTA_MAX, COS_MAX = 0.2, 0.021, 1.2

# Roundings the conversions add.  One rounding = 2^-23 (EPS), as SR.K_ROUND counts them; expf, log1pf and a division are
# taken as one unit each, as in test_rawrender_gpu.py.
#
# NeuS.  ct = -(relu(0.5 - 0.5 cos) (1 - r) + relu(-cos) r): the difference, 1 - r, two products, the sum = 5 relative
# roundings (both terms have one sign); h = ct (d 0.5) adds d = t_end - t_start and the product: 7, relative to |h|.
# n = sdf + h and y = -s n round once each, relative to |y|.  So y is off by at most (2 |y| + 7 s |h|) EPS.
H_ROUNDINGS = 7
Y_ROUNDINGS = 2
#   sp(y) = max(y, 0) + log1pf(expf(-|y|)) has slope sigmoid(y) <= 1, |y| sigmoid(y) <= max(sp(y), 1), and the inputs below
#   keep s |h| <= 1 (asserted in case()): y's error costs at most (2 + 7) max(sp(y), 1) EPS; expf, log1pf and the sum are 3
#   more, relative to sp(y).  x = sp(y_n) - sp(y_p) CANCELS, so its error is absolute: both softplus values and the
#   difference, in the unit EPS max(sp(y_n), 1)  (sp(y_n) >= sp(y_p)).
SP_ROUNDINGS = 3
NEUS_X_ROUNDINGS = 2 * (Y_ROUNDINGS + H_ROUNDINGS + SP_ROUNDINGS) + 1
#   sn = 1 / (1 + expf(s n)) has slope sn (1 - sn) <= min(sn, 1/4) and |y| sn (1 - sn) <= 0.224: y's error costs at most
#   (2 * 0.224 + 7 / 4) EPS, and relative to sn at most (2 |y| + 7) EPS; expf, the sum and the quotient are 3 EPS sn.  The
#   smaller of the two: 5.2 EPS, counted as 6, absolute, or (2 |y| + 7 + 3) EPS sn.
LOGISTIC_ABS = 6
LOGISTIC_REL = 3


def logistic_error(y, sig):
    return EPS * torch.minimum(torch.full_like(sig, LOGISTIC_ABS), (Y_ROUNDINGS * y.abs() + H_ROUNDINGS + LOGISTIC_REL) * sig)


#   dx/dcos = -(s (d 0.5)) (sn + sq) dct, relative: d and s (d 0.5) 2, dct = 0.5 (1 - r) [..] + r [..] 2, two products 2
NEUS_D_COS_RELATIVE = 6
# VolSDF, all relative.  y = -|sdf| / beta rounds once and |y| <= Y_MAX: through expf that is Y_MAX + 1 on e; psi = 1 - e
# (e <= psi there) one more; sigma = psi / beta one more.  (d and the product sigma d are in K_ROUND.)
Y_MAX = SDF_MAX / BETA
VOLSDF_X_ROUNDINGS = Y_MAX + 3
#   dx/dsdf = d (-e / (s s)): e, s s, the quotient, d and the product
VOLSDF_D_SDF = (Y_MAX + 1) + 4
#   dx/ds = d (-psi / (s s) + e sdf / (s s s)): the larger count of the two terms (e, e sdf, s s, (s s) s, the quotient: Y_MAX + 5),
#   their sum, d and the product; in the unit EPS d (psi / s^2 + e |sdf| / s^3)
VOLSDF_D_PAR = (Y_MAX + 5) + 3
RGB_ROUNDINGS = 3                  # c = 1 / (1 + expf(-x)): expf, the sum, the quotient
PRODUCT = 1                        # dL/dx times the derivative


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
    """The ray lengths of test_rawrender_gpu.py: empty rays, one sample, a wave step's edge (255, 256, 257), a ray across
    the 1024-element tiles, then 300 rays of 1-3 samples (more than RAY_CAP = 192 rays in one tile: the backward's gather
    fallback) and a trailing empty ray.  inv_s |sdf| <= 12.8 and inv_s |h| <= 1.  Built once and shared; the tests do not
    modify it.

    cos is kept 1e-3 away from 0 and from 1, where ct (and with it h and x) goes to 0: a float32 x that rounds to 0 where
    the float64 one is a tiny positive number has, by the contract, gradients of exactly 0 where the reference's dx/dcos
    is not small at all -- a discontinuity of the function, not an error to bound."""
    if "c" in _CASE:
        return _CASE["c"]
    rng = np.random.default_rng(7)
    counts = np.concatenate([[0, 1, 3, 0, 255, 256, 257, 2500], rng.integers(1, 4, 300), [0]]).astype(np.int64)
    rays = SR.Rays(torch.from_numpy(counts).to(dev))
    g = torch.Generator().manual_seed(13)
    n = rays.n
    ts = torch.rand(n, generator=g) * 4.0
    te = ts + 0.001 + torch.rand(n, generator=g) * 0.02
    sdf = torch.rand(n, generator=g) * (2 * SDF_MAX) - SDF_MAX
    cos = torch.rand(n, generator=g) * (2 * COS_MAX) - COS_MAX
    cos = torch.where(cos.abs() < 1e-3, torch.full_like(cos, -1e-3), cos)
    cos = torch.where((cos - 1.0).abs() < 1e-3, torch.full_like(cos, 1.0 - 1e-3), cos)
    raw_rgb = torch.rand(n, 3, generator=g) * 16.0 - 8.0
    sel = torch.rand(n, generator=g) > 0.2                           # about 20 % masked
    gl = {"colors": torch.randn(rays.R, 3, generator=g), "opacities": torch.randn(rays.R, 1, generator=g),
          "depths": torch.randn(rays.R, 1, generator=g), "weights": torch.randn(n, generator=g),
          "trans": torch.randn(n, generator=g), "alphas": torch.randn(n, generator=g)}
    assert float(sdf.abs().max()) <= SDF_MAX and float((te - ts).max()) <= DELTA_MAX and float(cos.abs().max()) <= COS_MAX
    assert INV_S * COS_MAX * DELTA_MAX / 2.0 <= 1.0                  # s |h| <= 1, as the counts above assume
    c = dict(rays=rays, ri=rays.ray_ids.clone(), ts=ts.to(dev), te=te.to(dev), sdf=sdf.to(dev), cos=cos.to(dev),
             raw_rgb=raw_rgb.to(dev), sel=sel.to(dev), gl={k: v.to(dev) for k, v in gl.items()})
    seginfo_from_ray_indices(c["ri"], rays.R)   # cached on the tensor, as for the ray_indices sampling() returns
    _CASE["c"] = c
    return c


def run(c, model, extras, tensors=None, param=None, param_grad=True, sel="case"):
    """One forward and backward; returns (outputs by name, gradients by name)."""
    t = tensors or {k: c[k] for k in ("ts", "te", "sdf", "cos", "raw_rgb", "sel")}
    sd = t["sdf"].detach().requires_grad_(True)
    cs = t["cos"].detach().requires_grad_(True)
    rc = t["raw_rgb"].detach().requires_grad_(True)
    if param is None:
        param = torch.full((1,), PARAM[model], device=sd.device)
    p = param.detach().requires_grad_(param_grad)
    selector = t["sel"] if sel == "case" else sel
    kw = dict(inv_s=p, cos=cs, cos_anneal_ratio=RATIO) if model == "neus" else dict(beta=p)
    colors, opac, depth, ex = rendering_from_sdf(t["ts"], t["te"], rc, sd, c["ri"], c["rays"].R, model=model, selector=selector, **kw)
    assert set(ex) == {"weights", "trans", "alphas"}
    outs = {"colors": colors, "opacities": opac, "depths": depth, **ex}
    keys = ["colors", "opacities", "depths"] + (["weights", "trans", "alphas"] if extras else [])
    gl = t.get("gl", c["gl"])
    ins = {"g_sdfs": sd, "g_raw_rgbs": rc}
    if model == "neus":
        ins["g_cos"] = cs
    if param_grad:
        ins["g_param"] = p
    grads = torch.autograd.grad([outs[k] for k in keys], list(ins.values()), [gl[k] for k in keys])
    return {k: v.detach() for k, v in outs.items()}, dict(zip(ins, grads))


def incoming(opac, depth, g_o, g_d):
    """The per-ray gradients the depth normalisation (depth_raw / opacity.clamp_min(eps)) hands to the packed pass,
    from the product's own float32 opacity and depth: (G_opacity, G_depth_raw, |G_opacity| scale)."""
    eps = torch.finfo(torch.float32).eps
    o, d = opac.double(), depth.double()
    oc = o.clamp_min(eps)
    live = (o >= eps).double()
    return g_o - live * g_d * d / oc, g_d / oc, g_o.abs() + live * (g_d * d / oc).abs()


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("model", XR.MODELS)
def test_against_float64(dev, monkeypatch, model, extras):
    c = case(dev)
    rays, ri, ts, te, gl, sel = c["rays"], c["ri"], c["ts"], c["te"], c["gl"], c["sel"]
    log = CallLog(monkeypatch)
    outs, g = run(c, model, extras)
    assert log.names() == ["nfa_render_sdf_fwd", "nfa_render_sdf_bwd"]
    assert (log.calls[1][1][14] is not None) == extras   # g_weights: the backward's EXTRA variant
    assert g["g_param"].shape == (1,)

    # float64, with the incoming per-ray gradients torch forms from the product's own outputs
    G_o, G_d, G_o_abs = incoming(outs["opacities"], outs["depths"], gl["opacities"].double(), gl["depths"].double())
    grads = {"colors": gl["colors"], "opacities": G_o, "depths_raw": G_d}
    if extras:
        grads.update({k: gl[k] for k in ("weights", "trans", "alphas")})
    par = PARAM[model]
    ref = XR.render(rays, ts, te, c["sdf"], c["cos"], c["raw_rgb"], model, par, RATIO, "sigmoid", sel, grads=grads)
    ts64, te64 = ts.double(), te.double()
    d64 = te64 - ts64
    D = XR.derivatives(model, c["sdf"], c["cos"], d64, par, RATIO, sel)
    live = sel.double()

    # x's error: absolute, e per sample.  NeuS in the unit EPS max(sp(y_n), 1); VolSDF relative to x.  The passes' own
    # roundings behind x are SR.density_scales' bounds as ever; what x's error does on top is XR.propagate_x_error's.
    if model == "neus":
        e = NEUS_X_ROUNDINGS * EPS * live * D["sp_n"].clamp_min(1.0)
    else:
        e = VOLSDF_X_ROUNDINGS * EPS * ref["x"]
    e_c = RGB_ROUNDINGS
    x, rgb, w, T, a = ref["x"], ref["rgbs"], ref["weights"], ref["trans"], ref["alphas"]
    mid = ((ts64 + te64) / 2.0).abs()
    g_c = gl["colors"].double().abs()[ri]
    ex_g = [grads.get(k) for k in ("weights", "trans", "alphas")]
    gw_abs = ((g_c * rgb.abs()).sum(-1) + G_o_abs[ri, 0] + G_d.abs()[ri, 0] * mid + (0.0 if ex_g[0] is None else ex_g[0].double().abs()))
    ex_t = [None if v is None else v.double() for v in ex_g[1:]]
    s_w, s_t, s_a, s_gx = SR.density_scales(rays, torch.zeros_like(x), torch.ones_like(x), x, T, a, gw_abs, *ex_t)   # (x = sigma delta with delta = 1)
    dT, da, dw, dgx = XR.propagate_x_error(rays, e, T, a, gw_abs, *ex_t)
    sw1 = s_w + w
    eps32 = torch.finfo(torch.float32).eps
    oc = ref["opacities"].clamp_min(eps32)
    s_col, d_col = SR.accumulate(rays, sw1, rgb.abs()), SR.accumulate(rays, dw, rgb.abs())
    s_op, d_op = SR.accumulate(rays, sw1), SR.accumulate(rays, dw)
    s_dr, d_dr = SR.accumulate(rays, sw1, mid[:, None]), SR.accumulate(rays, dw, mid[:, None])
    s_dep, d_dep = (s_dr + ref["depths"].abs() * s_op) / oc, (d_dr + ref["depths"].abs() * d_op) / oc

    check("colors", outs["colors"], ref["colors"], SR.bound(rays, s_col, per_ray=True, extra=e_c) + d_col)
    check("opacities", outs["opacities"], ref["opacities"], SR.bound(rays, s_op, per_ray=True) + d_op)
    check("depths", outs["depths"], ref["depths"], SR.bound(rays, s_dep, per_ray=True, extra=4) + d_dep)
    check("weights", outs["weights"], w, SR.bound(rays, s_w) + dw)
    check("trans", outs["trans"], T, SR.bound(rays, s_t) + dT)
    check("alphas", outs["alphas"], a, SR.bound(rays, s_a) + da)

    # gradients: dL/dx (value ref["g_x"], bound t_gx) times a derivative factor D with its own error dD
    if model == "neus":
        s, hd, sn, sq = INV_S, d64 / 2.0, D["sn"], D["sq"]
        d_sn, d_sq = logistic_error(s * D["n"], sn), logistic_error(s * D["p"], sq)
        dD = {"sdf": s * (d_sn + d_sq) + 2 * EPS * D["sdf"].abs(),                      # the difference and the product
              "cos": s * hd * D["dct"] * ((NEUS_D_COS_RELATIVE + 1) * EPS * (sn + sq) + d_sn + d_sq),   # (+ 1: the sum sn + sq)
              # p's (n's) own rounding, the product, the difference: 3; h's roundings reach both products
              "param": D["p"].abs() * d_sq + D["n"].abs() * d_sn + 3 * EPS * (D["p"].abs() * sq + D["n"].abs() * sn)
                       + H_ROUNDINGS * EPS * D["h"].abs() * (sn + sq)}
    else:
        s, sdf64 = BETA, c["sdf"].double()
        dD = {"sdf": VOLSDF_D_SDF * EPS * D["sdf"].abs(),
              "param": VOLSDF_D_PAR * EPS * d64 * (D["psi"] / s ** 2 + D["e"] * sdf64.abs() / s ** 3)}
    t_gx = SR.bound(rays, s_gx, extra=e_c) + dgx
    # (where x is exactly 0 -- cos >= 1, in float32 as in float64 -- the factors are exactly 0 on both sides)
    varies = live * (x > 0).double() if model == "neus" else live

    def tol(k):
        return SR.bound(rays, s_gx * D[k].abs(), extra=e_c + PRODUCT) + dgx * D[k].abs() + (ref["g_x"].abs() + t_gx) * dD[k] * varies

    check("g_sdfs", g["g_sdfs"], ref["g_sdfs"], tol("sdf"))
    if model == "neus":
        check("g_cos", g["g_cos"], ref["g_cos"], tol("cos"))
    # the parameter: the sum of its samples' bounds.  (The float32 sum of the stream adds its own roundings; every sample's
    # bound holds m + K + ... >= 10 units of its term, more than a reduction tree's depth in half-units.)
    check("g_param", g["g_param"][0], ref["g_param"], tol("param").sum())
    s_grgb = g_c * sw1[:, None]
    t_rgb = SR.bound(rays, s_grgb * ref["drgb"].abs(), extra=e_c + 2) + g_c * dw[:, None] * ref["drgb"].abs()
    t_rgb = t_rgb + 3 * EPS * s_grgb * rgb.abs()   # c (1 - c): the three roundings of c are an absolute error of 3 * 2^-23 * c in 1 - c
    check("g_raw_rgbs", g["g_raw_rgbs"], ref["g_raw_rgbs"], t_rgb)

    # behind the mask: exact zeros, forward and in every gradient
    off = ~sel
    for k in ("alphas", "weights"):
        assert not bool(outs[k][off].any()), k
    for k in ("g_sdfs", "g_cos"):
        assert k not in g or not bool(g[k][off].any()), k


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("model", XR.MODELS)
def test_scalar_form_equals_vector_form_bit_for_bit(dev, monkeypatch, model, extras):
    c = case(dev)
    aligned, g_aligned = run(c, model, extras)
    sel = shifted(c["sel"], 1)                               # the mask at a one-byte offset
    assert sel.data_ptr() % 4 != 0
    t = {"ts": shifted(c["ts"], 1), "te": shifted(c["te"], 3), "sdf": shifted(c["sdf"], 2), "cos": shifted(c["cos"], 3),
         "raw_rgb": shifted(c["raw_rgb"], 1), "sel": sel, "gl": {k: shifted(v, 1 + i % 3) for i, (k, v) in enumerate(c["gl"].items())}}
    log = CallLog(monkeypatch)
    got, g_got = run(c, model, extras, tensors=t)
    assert log.names() == ["nfa_render_sdf_fwd", "nfa_render_sdf_bwd"]
    for name, a in log.calls:   # the per-sample inputs reached the entry points unaligned
        per_sample = [a[0], a[1], a[2], a[4]] + ([a[3]] if model == "neus" else [])
        assert all(v % 16 != 0 for v in per_sample) and a[5] % 4 != 0, name
    for k in aligned:
        assert torch.equal(aligned[k], got[k]), k
    assert set(g_aligned) == set(g_got)
    for k in g_aligned:
        assert torch.equal(g_aligned[k], g_got[k]), k


@pytest.mark.parametrize("model", XR.MODELS)
def test_two_runs_give_the_same_bits(dev, model):
    c = case(dev)
    a, g_a = run(c, model, True)
    b, g_b = run(c, model, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert "g_param" in g_a and bool(g_a["g_param"].abs() > 0)
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k


@pytest.mark.parametrize("model", XR.MODELS)
def test_masked_samples_are_exact_zeros_whatever_they_hold(dev, model):
    c = case(dev)
    off = (~c["sel"]).nonzero().flatten()
    sdf = c["sdf"].clone()
    sdf[off[0::3]] = float("inf")
    sdf[off[1::3]] = float("nan")
    sdf[off[2::3]] = float("-inf")
    t = {**{k: c[k] for k in ("ts", "te", "cos", "raw_rgb", "sel")}, "sdf": sdf}
    clean, g_clean = run(c, model, True)
    dirty, g_dirty = run(c, model, True, tensors=t)
    for k in clean:
        assert torch.equal(clean[k], dirty[k]), k
    for k in g_clean:
        assert torch.equal(g_clean[k], g_dirty[k]), k
    for k in ("alphas", "weights"):
        assert not bool(dirty[k][off].any()), k
    for k in ("g_sdfs", "g_cos", "g_raw_rgbs"):   # (the colour's: the weight behind the mask is 0)
        assert k not in g_dirty or not bool(g_dirty[k][off].any()), k
    # The fourth gradient is the parameter's per-sample stream, which rendering_from_sdf hands to torch.sum and drops:
    # the backward entry point once more, writing that stream alone into a buffer of our own.
    seg = seginfo_from_ray_indices(c["ri"], c["rays"].R)
    gl = c["gl"]
    p = torch.full((1,), PARAM[model], device=dev)
    streams = []
    for values in (c["sdf"], sdf):
        out = torch.full_like(sdf, float("nan"))
        with torch.cuda.device(dev):
            B.call("nfa_render_sdf_bwd", B.ptr(c["ts"]), B.ptr(c["te"]), B.ptr(values), B.ptr(c["cos"]) if model == "neus" else None,
                   B.ptr(c["raw_rgb"]), B.ptr(c["sel"]), XR.MODELS.index(model), B.ptr(p), RATIO, 1, B.ptr(clean["trans"]),
                   B.ptr(gl["colors"]), B.ptr(gl["opacities"]), B.ptr(gl["depths"]), B.ptr(gl["weights"]), B.ptr(gl["trans"]),
                   B.ptr(gl["alphas"]), B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, c["rays"].R, c["rays"].n,
                   None, None, B.ptr(out), None, B.stream())
        streams.append(out)
    assert torch.equal(streams[0], streams[1])
    assert not bool(streams[1][off].any()) and bool(torch.isfinite(streams[1]).all()) and bool(streams[1].any())


@pytest.mark.parametrize("model", XR.MODELS)
def test_empty_inputs(dev, model):
    kw = (lambda n: dict(model="neus", inv_s=INV_S, cos=torch.full((n,), -0.8, device=dev))) if model == "neus" else (lambda n: dict(model="volsdf", beta=BETA))
    e = torch.empty(0, device=dev)
    ri = torch.empty(0, dtype=torch.long, device=dev)
    # n = 0 with rays (all of them empty), and no rays at all
    for R in (5, 300, 0):
        sd = e.clone().requires_grad_(True)
        p = torch.full((1,), PARAM[model], device=dev, requires_grad=True)
        k = kw(0)
        k["inv_s" if model == "neus" else "beta"] = p
        colors, opac, depth, ex = rendering_from_sdf(e, e, torch.empty(0, 3, device=dev), sd, ri, R, **k)
        assert colors.shape == (R, 3) and opac.shape == (R, 1) and depth.shape == (R, 1) and ex["weights"].shape == (0,)
        assert not colors.any() and not opac.any() and not depth.any()
        g_sd, g_p = torch.autograd.grad(colors.sum() + opac.sum(), [sd, p])
        assert g_sd.shape == (0,) and g_p.shape == (1,) and float(g_p) == 0.0
    # samples in one ray among empty ones
    counts = torch.tensor([0, 0, 3, 0, 0], device=dev)
    rays = SR.Rays(counts)
    ts = torch.tensor([0.1, 0.2, 0.3], device=dev)
    te = ts + 0.01
    sdf = torch.tensor([0.05, -0.01, -0.1], device=dev)
    colors, opac, _, _ = rendering_from_sdf(ts, te, torch.zeros(3, 3, device=dev), sdf, rays.ray_ids, 5, **kw(3))
    assert not opac[[0, 1, 3, 4]].any() and float(opac[2]) > 0 and not colors[[0, 1, 3, 4]].any()


def test_a_step_is_two_native_calls_that_never_wait(dev, monkeypatch):
    """inv_s an nn.Parameter on the device: it reaches both passes by pointer, nothing reads it on the host."""
    c = case(dev)
    inv_s = torch.nn.Parameter(torch.full((1,), INV_S, device=dev))
    sd = c["sdf"].clone().requires_grad_(True)
    cs = c["cos"].clone().requires_grad_(True)
    rc = c["raw_rgb"].clone().requires_grad_(True)

    def step():
        colors, opac, depth, ex = rendering_from_sdf(c["ts"], c["te"], rc, sd, c["ri"], c["rays"].R, model="neus", inv_s=inv_s,
                                                     cos=cs, cos_anneal_ratio=RATIO, selector=c["sel"])
        return torch.autograd.grad([colors, opac, depth], [sd, cs, rc, inv_s], [c["gl"][k] for k in ("colors", "opacities", "depths")])

    want = step()   # (libraries loaded, allocator warm)
    log = CallLog(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert log.names() == ["nfa_render_sdf_fwd", "nfa_render_sdf_bwd"]
    for name, a in log.calls:
        assert a[7] == inv_s.data_ptr(), name
    for u, v in zip(want, got):
        assert torch.equal(u, v)
    assert got[3].shape == inv_s.shape


@pytest.mark.parametrize("model", XR.MODELS)
def test_a_parameter_without_gradient_gets_no_stream(dev, monkeypatch, model):
    c = case(dev)
    _, g_with = run(c, model, False)
    log = CallLog(monkeypatch)
    _, g = run(c, model, False, param_grad=False)
    assert log.names() == ["nfa_render_sdf_fwd", "nfa_render_sdf_bwd"]
    bwd = log.calls[1][1]
    assert bwd[24] is None and bwd[22] is not None and bwd[25] is not None          # grad_param; grad_sdfs, grad_raw_rgbs
    assert (bwd[23] is not None) == (model == "neus")                               # grad_cos
    for k in g:
        assert torch.equal(g[k], g_with[k]), k
    # a Python float: a 1-element device tensor, no gradient stream either
    log.calls.clear()
    sd = c["sdf"].clone().requires_grad_(True)
    kw = dict(model="neus", inv_s=INV_S, cos=c["cos"], cos_anneal_ratio=RATIO) if model == "neus" else dict(model="volsdf", beta=BETA)
    _, opac, _, _ = rendering_from_sdf(c["ts"], c["te"], c["raw_rgb"], sd, c["ri"], c["rays"].R, selector=c["sel"], **kw)
    (g_sd,) = torch.autograd.grad(opac.sum(), sd)
    assert log.names() == ["nfa_render_sdf_fwd", "nfa_render_sdf_bwd"]
    bwd = log.calls[1][1]
    assert bwd[24] is None and bwd[23] is None and bwd[25] is None and bwd[11] is None   # only g_opacities in, only grad_sdfs out
    assert bool(torch.isfinite(g_sd).all()) and bool(g_sd.any())


@pytest.mark.parametrize("model", XR.MODELS)
def test_other_inputs_take_the_torch_composition(dev, monkeypatch, model):
    """t_starts that require a gradient: no nfa_render_sdf_* call, same results within rounding."""
    c = case(dev)
    want, _ = run(c, model, False)
    log = CallLog(monkeypatch)
    ts = c["ts"].clone().requires_grad_(True)
    kw = dict(model="neus", inv_s=INV_S, cos=c["cos"], cos_anneal_ratio=RATIO) if model == "neus" else dict(model="volsdf", beta=BETA)
    colors, opac, _, ex = rendering_from_sdf(ts, c["te"], c["raw_rgb"], c["sdf"], c["ri"], c["rays"].R, selector=c["sel"], **kw)
    assert not any(n.startswith("nfa_render_sdf") for n in log.names())
    assert set(ex) == {"weights", "trans", "alphas"}
    assert torch.allclose(colors, want["colors"], rtol=1e-4, atol=1e-5) and torch.allclose(opac, want["opacities"], rtol=1e-4, atol=1e-5)
    (g,) = torch.autograd.grad(opac.sum(), ts)
    assert bool(torch.isfinite(g).all())

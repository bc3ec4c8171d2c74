"""Float64 restatement of ``rendering_from_sdf`` on the padded table of tests/seg_reference.py.

Nothing from nerfacc_amd is used here.  The SDF-to-opacity conversions of NeuS and VolSDF are written out in float64 torch
and composed with the padded scans of seg_reference; every reference gradient -- the scalar parameter's included -- is
torch autograd over that composition.  The conversion's own derivatives are also written out (``derivatives``): the tests
build their error scales from them, and tests/test_sdfrender_cpu.py checks them against autograd.
"""
from __future__ import annotations

import torch

import rawrender_reference as RR
import seg_reference as SR

MODELS = ("neus", "volsdf")


def softplus(y: torch.Tensor) -> torch.Tensor:
    return torch.logaddexp(y, torch.zeros_like(y))


def neus_terms(sdf, cos, d, inv_s, r: float):
    """(ct, h, n, p) of NeuS: the cosine term (<= 0), the half step along it, the SDF at the sample's far and near end."""
    ct = -(torch.relu(0.5 - 0.5 * cos) * (1.0 - r) + torch.relu(-cos) * r)
    h = ct * d / 2.0
    return ct, h, sdf + h, sdf - h


def neus_x(sdf, cos, d, inv_s, r: float):
    """x = log Phi(inv_s p) - log Phi(inv_s n) >= 0, Phi the logistic function; alpha = 1 - exp(-x)."""
    _, _, n, p = neus_terms(sdf, cos, d, inv_s, r)
    return torch.relu(softplus(-inv_s * n) - softplus(-inv_s * p))


def volsdf_sigma(sdf, beta):
    e = 0.5 * torch.exp(-sdf.abs() / beta)
    return torch.where(sdf >= 0, e, 1.0 - e) / beta


def convert(model: str, sdf, cos, d, param, r: float, selector=None):
    """x of every sample (float64); exactly 0 behind a false selector, whatever the sample holds."""
    if selector is not None:
        sdf = torch.where(selector, sdf, torch.zeros_like(sdf))
        if cos is not None:
            cos = torch.where(selector, cos, torch.zeros_like(cos))
    if model == "neus":
        x = neus_x(sdf, cos, d, param, r)
    else:
        assert model == "volsdf", model
        x = volsdf_sigma(sdf, param) * d
    return x if selector is None else torch.where(selector, x, torch.zeros_like(x))


def derivatives(model: str, sdf, cos, d, param, r: float, selector=None):
    """The written-out derivatives of x: dict with ``sdf``, ``cos`` (NeuS), ``param``; all 0 behind a false selector and,
    for NeuS, where x is 0.  Also the pieces the error scales need (see test_sdfrender_gpu.py)."""
    sdf, d = sdf.double(), d.double()
    s = float(param)
    out = {}
    if model == "neus":
        cos = cos.double()
        ct, h, n, p = neus_terms(sdf, cos, d, s, r)
        sn, sq = torch.sigmoid(-s * n), torch.sigmoid(-s * p)
        dct = 0.5 * (1.0 - r) * (cos < 1).double() + r * (cos < 0).double()
        on = (neus_x(sdf, cos, d, s, r) > 0).double()
        out = {"sdf": on * s * (sq - sn), "cos": on * -(s * d / 2.0) * (sn + sq) * dct, "param": on * (p * sq - n * sn),
               "sp_n": softplus(-s * n), "h": h, "n": n, "p": p, "dct": dct, "sn": sn, "sq": sq}
    else:
        e = 0.5 * torch.exp(-sdf.abs() / s)
        psi = torch.where(sdf >= 0, e, 1.0 - e)
        out = {"sdf": d * (-e / s ** 2), "param": d * (-psi / s ** 2 + e * sdf / s ** 3), "e": e, "psi": psi}
    if selector is not None:
        for k in ("sdf", "cos", "param"):
            if k in out:
                out[k] = torch.where(selector, out[k], torch.zeros_like(out[k]))
    return out


def propagate_x_error(rays: SR.Rays, e, trans, alphas, gw_abs, gt=None, ga=None):
    """What an error of x does to everything behind it.  ``e`` (n,) bounds |x32 - x| per sample; ``trans`` / ``alphas`` are
    the exact T and alpha; ``gw_abs`` bounds the magnitude of the total gradient arriving at every weight (the incoming
    one and what the per-ray outputs hand down), ``gt`` / ``ga`` are the incoming gradients of trans / alphas.

    Returns bounds (dT, da, dw, dgx) of the changes of T, alpha, w and dL/dx, to be ADDED to the bounds of the passes'
    own roundings.  With E the sum of e in front of a sample: T = exp(-S) moves by at most T expm1(E), alpha by
    (1 - alpha) expm1(e), w = T alpha by the product rule with its cross term, and
        dL/dx_i = (gw_i T_i + ga_i)(1 - a_i) - sum_{j > i} (gw_j a_j + gt_j) T_j
    term by term.  No first-order truncation: expm1 and the cross terms are kept.
    """
    T, a = trans.abs(), alphas.abs()
    z = torch.zeros_like(T)
    gt = z if gt is None else gt.abs()
    ga = z if ga is None else ga.abs()
    E = rays.unpad(SR.excl_sum_rows(rays.pad(e)))
    dT = T * torch.expm1(E)
    da = (1.0 - a) * torch.expm1(e)
    dw = a * dT + T * da + dT * da
    direct = gw_abs * (1.0 - a) * dT + (gw_abs * (T + dT) + ga) * da
    chain = rays.unpad(SR.rev_sum_rows(rays.pad(gw_abs * dw + gt * dT), False))
    return dT, da, dw, direct + chain


def render(rays: SR.Rays, ts, te, sdf, cos, raw_rgb, model: str, param: float, r: float = 1.0, col: str = "sigmoid",
           selector=None, grads=None):
    """The float64 rendering of an SDF field.

    Returns a dict with ``x``, the activated ``rgbs`` and their derivative factor ``drgb``, the per-sample ``weights`` /
    ``trans`` / ``alphas``, the un-normalised ``colors`` / ``opacities`` / ``depths_raw`` and the normalised ``depths``.
    With ``grads`` -- a dict of incoming gradients for any of ``colors``, ``opacities``, ``depths_raw``, ``weights``,
    ``trans``, ``alphas`` -- also ``g_sdfs``, ``g_cos`` (NeuS), ``g_param``, ``g_raw_rgbs`` and ``g_x`` (dL/dx), all from
    autograd over the padded table.
    """
    ts, te = ts.double(), te.double()
    d = te - ts
    sdf_l = sdf.double().detach().requires_grad_(True)
    cos_l = None if cos is None or model != "neus" else cos.double().detach().requires_grad_(True)
    par_l = torch.tensor(float(param), dtype=torch.float64, device=ts.device, requires_grad=True)
    raw_l = raw_rgb.double().detach().requires_grad_(True)
    x = convert(model, sdf_l, cos_l, d, par_l, r, selector)
    x.retain_grad()
    c = RR.rgb(raw_l, col)
    S = rays.unpad(SR.excl_sum_rows(rays.pad(x)))
    T = torch.exp(-S)
    a = 1.0 - torch.exp(-x)
    w = T * a
    col_r, op_r, dep_r = SR.render_accumulate(rays, w, c, ts, te)
    out = {"x": x.detach(), "rgbs": c.detach(), "drgb": RR.rgb_grad(raw_l.detach(), col), "weights": w.detach(),
           "trans": T.detach(), "alphas": a.detach(), "colors": col_r.detach(), "opacities": op_r.detach(),
           "depths_raw": dep_r.detach()}
    out["depths"] = SR.finish_rendering(out["colors"], out["opacities"], out["depths_raw"])[2]
    if grads:
        named = {"colors": col_r, "opacities": op_r, "depths_raw": dep_r, "weights": w, "trans": T, "alphas": a}
        keys = [k for k in named if grads.get(k) is not None]
        leaves = [sdf_l, par_l, raw_l, x] + ([cos_l] if cos_l is not None else [])
        g = torch.autograd.grad([named[k] for k in keys], leaves, [grads[k].double() for k in keys], allow_unused=True)
        zero = lambda t, like: torch.zeros_like(like) if t is None else t
        out["g_sdfs"], out["g_param"], out["g_raw_rgbs"], out["g_x"] = (zero(t, l) for t, l in zip(g[:4], leaves[:4]))
        if cos_l is not None:
            out["g_cos"] = zero(g[4], cos_l)
    return out

"""Float64 restatements of the field activations ``rendering_from_raw`` fuses, composed with tests/seg_reference.py.

Nothing from nerfacc_amd is used here.  The activations are written out with their derivatives (``trunc_exp``'s is
the custom one of examples/radiance_fields/ngp.py:23-36: ``exp(min(z, 15))``, not ``exp(z)``), so the reference
gradients are the chain rule through these, not whatever torch differentiates.
"""
from __future__ import annotations

import torch

import seg_reference as SR

DENSITY = ("none", "trunc_exp", "exp", "relu", "softplus")
RGB = ("none", "sigmoid")


def density(z: torch.Tensor, kind: str) -> torch.Tensor:
    if kind in ("trunc_exp", "exp"):
        return torch.exp(z)
    if kind == "relu":
        return torch.clamp(z, min=0.0)
    if kind == "softplus":   # torch's defaults: beta 1, threshold 20
        return torch.where(z > 20.0, z, torch.log1p(torch.exp(torch.clamp(z, max=20.0))))
    assert kind == "none", kind
    return z


def density_grad(z: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "trunc_exp":
        return torch.exp(torch.clamp(z, max=15.0))
    if kind == "exp":
        return torch.exp(z)
    if kind == "relu":
        return (z > 0).to(z.dtype)
    if kind == "softplus":
        return torch.where(z > 20.0, torch.ones_like(z), torch.sigmoid(z))
    assert kind == "none", kind
    return torch.ones_like(z)


def rgb(x: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "sigmoid":
        return torch.sigmoid(x)
    assert kind == "none", kind
    return x


def rgb_grad(x: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "sigmoid":
        c = torch.sigmoid(x)
        return c * (1.0 - c)
    return torch.ones_like(x)


def activate(raw_sig, raw_rgb, dens: str, bias: float, col: str, selector=None):
    """(sigma, d sigma / d raw, c, d c / d raw), all float64; under a false selector sigma and its derivative are 0
    whatever the raw value."""
    z = raw_sig.double() + bias
    if selector is not None:
        z = torch.where(selector, z, torch.zeros_like(z))
    s, ds = density(z, dens), density_grad(z, dens)
    if selector is not None:
        s = torch.where(selector, s, torch.zeros_like(s))
        ds = torch.where(selector, ds, torch.zeros_like(ds))
    x = raw_rgb.double()
    return s, ds, rgb(x, col), rgb_grad(x, col)


def render(rays: SR.Rays, ts, te, raw_sig, raw_rgb, dens: str, bias: float, col: str, selector=None, grads=None):
    """The float64 rendering from raw values.

    Returns a dict with the activated ``sigmas`` / ``rgbs`` and their derivative factors ``dsig`` / ``drgb``, the
    per-sample ``weights`` / ``trans`` / ``alphas``, the un-normalised ``colors`` / ``opacities`` / ``depths_raw`` and the
    normalised ``depths``.  With ``grads`` -- a dict of incoming gradients for any of ``colors``, ``opacities``,
    ``depths_raw``, ``weights``, ``trans``, ``alphas`` -- also ``g_raw_sigmas`` / ``g_raw_rgbs``: autograd through the
    rendering as a function of the ACTIVATED values, times the derivative factors above.
    """
    ts, te = ts.double(), te.double()
    s, ds, c, dc = activate(raw_sig, raw_rgb, dens, bias, col, selector)
    s = s.detach().requires_grad_(True)
    c = c.detach().requires_grad_(True)
    w, T, a = SR.from_density(rays, ts, te, s)
    col_r, op_r, dep_r = SR.render_accumulate(rays, w, c, ts, te)
    out = {"sigmas": s.detach(), "rgbs": c.detach(), "dsig": ds, "drgb": dc, "weights": w.detach(), "trans": T.detach(),
           "alphas": a.detach(), "colors": col_r.detach(), "opacities": op_r.detach(), "depths_raw": dep_r.detach()}
    out["depths"] = SR.finish_rendering(out["colors"], out["opacities"], out["depths_raw"])[2]
    if grads:
        named = {"colors": col_r, "opacities": op_r, "depths_raw": dep_r, "weights": w, "trans": T, "alphas": a}
        keys = [k for k in named if grads.get(k) is not None]
        g_s, g_c = torch.autograd.grad([named[k] for k in keys], [s, c], [grads[k].double() for k in keys])
        out["g_sigmas"], out["g_rgbs"] = g_s, g_c
        out["g_raw_sigmas"], out["g_raw_rgbs"] = g_s * ds, g_c * dc
    return out

"""``rendering`` of signed-distance fields: the SDF-to-opacity conversion of NeuS and VolSDF fused into the two rendering
passes.

A surface model turns its SDF into an opacity before it can render: NeuS (Wang et al. 2021) with the logistic CDF of the
SDF at the two ends of a sample, VolSDF (Yariv et al. 2021) with the Laplace CDF of the SDF times ``1 / beta``.  In torch
that is about fifteen elementwise passes over the samples each way, in front of ``render_weight_from_alpha`` plus three
accumulations, or of ``rendering``.  :func:`rendering_from_sdf` takes the SDF itself: on the native path the forward pass
converts it as it loads a sample (csrc/segscan.hip: RenderSdfFwdOp) and the backward pass forms the conversion again from
the raw values and multiplies its derivatives in (RenderSdfBwdOp), one native call each way.  :func:`neus_alpha` and
:func:`laplace_density` are the same conversions in torch: the fallback of :func:`rendering_from_sdf`, and usable alone.
An extension: the reference has no counterpart, so the names are not in ``nerfacc_amd.__all__``.

Arithmetic (float32 on the native path; the torch functions below restate it operation for operation in the dtype of
their inputs), with ``d = t_end - t_start`` and ``r = cos_anneal_ratio``::

    NeuS    ct = -(relu(0.5 - 0.5 cos) (1 - r) + relu(-cos) r)                     (<= 0)
            h  = ct (d 0.5);  n = sdf + h;  p = sdf - h                            (next, previous; n <= p)
            sp(y) = max(y, 0) + log1p(exp(-|y|))                                   (softplus, stable)
            x  = max(sp(-inv_s n) - sp(-inv_s p), 0)                               (= log Phi(p) - log Phi(n), Phi = sigmoid)
    VolSDF  e = 0.5 exp(-|sdf| / beta);  psi = sdf >= 0 ? e : 1 - e;  sigma = psi / beta;  x = sigma d
    alpha = 1 - exp(-x),  T = exp(-sum of x in front of the sample),  w = T alpha

NeuS' ``x`` is the limit eps -> 0 of the published ``((Phi(p) - Phi(n) + 1e-5) / (Phi(p) + 1e-5)).clip(0, 1)``: the two
alphas differ by at most ``1e-5 / Phi(p)``.  It has no division and no eps, and it is what the passes sum along a ray.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from ._segments import SegInfo, seginfo_from_ray_indices
from .rawrender import RGB_ACTIVATIONS, _rendering_torch, activate_rgb
from .volrend import _f32c, _finish_rendering, rendering

# include/nerfacc_hip.h: NFA_SDF_*
SDF_MODELS = {"neus": 0, "volsdf": 1}

Scalar = Union[Tensor, float]


def _softplus(y: Tensor) -> Tensor:
    return torch.clamp(y, min=0.0) + torch.log1p(torch.exp(-torch.abs(y)))


def _neus_x(sdfs: Tensor, cos: Tensor, dists: Tensor, inv_s: Scalar, cos_anneal_ratio: float) -> Tensor:
    r = float(cos_anneal_ratio)
    ct = -(F.relu(0.5 - 0.5 * cos) * (1.0 - r) + F.relu(-cos) * r)
    h = ct * (dists * 0.5)
    n, p = sdfs + h, sdfs - h
    # (relu, not clamp: where the difference is not positive, x and every gradient are exactly 0)
    return F.relu(_softplus(-inv_s * n) - _softplus(-inv_s * p))


def neus_alpha(sdfs: Tensor, cos: Tensor, dists: Tensor, inv_s: Scalar, cos_anneal_ratio: float = 1.0) -> Tensor:
    """NeuS' opacity of a sample of length ``dists`` from the SDF at its midpoint, in torch.

    ``sdfs``, ``cos`` (the user's ``(dirs * normals).sum(-1)``) and ``dists`` share a shape; ``inv_s`` is a 1-element
    tensor or a float.  ``alpha = 1 - exp(-x)`` with the ``x`` of the module docstring: the published
    ``((Phi(p) - Phi(n) + 1e-5) / (Phi(p) + 1e-5)).clip(0, 1)`` without its 1e-5 (within ``1e-5 / Phi(p)`` of it).
    ``cos >= 1`` gives exactly 0.  Differentiable to ``sdfs``, ``cos``, ``dists`` and ``inv_s``.
    """
    return 1.0 - torch.exp(-_neus_x(sdfs, cos, dists, inv_s, cos_anneal_ratio))


def laplace_density(sdfs: Tensor, beta: Scalar) -> Tensor:
    """VolSDF's density ``Psi_beta(-sdf) / beta`` in torch, ``Psi`` the CDF of the Laplace distribution with scale
    ``beta`` (a 1-element tensor or a float, > 0).  Differentiable to ``sdfs`` and ``beta``."""
    e = 0.5 * torch.exp(-torch.abs(sdfs) / beta)
    psi = torch.where(sdfs >= 0, e, 1.0 - e)
    return psi / beta


class _RenderSdf(torch.autograd.Function):
    """One forward and one backward pass over the samples; saves the inputs and ``trans`` only.  ``param`` is the
    1-element device tensor of ``inv_s`` / ``beta``: the kernels read it through its pointer."""

    @staticmethod
    def forward(ctx, t_starts, t_ends, sdfs, cos, raw_rgbs, param, selector, seg: SegInfo, model: int, ratio: float, col: int):
        ctx.set_materialize_grads(False)  # unused outputs arrive as None, not as zero tensors
        ts, te, sd, c = _f32c(t_starts), _f32c(t_ends), _f32c(sdfs), _f32c(raw_rgbs)
        cs = None if cos is None else _f32c(cos)
        p = param.detach().reshape(1)
        sel = None if selector is None else selector.contiguous()
        dev = B.require_device(ts, te, sd, cs, c, p, sel)
        R, n = seg.n_rays, sd.numel()
        weights, trans, alphas = torch.empty_like(ts), torch.empty_like(ts), torch.empty_like(ts)
        colors = torch.empty((R, 3), dtype=torch.float32, device=dev)
        opac = torch.empty((R, 1), dtype=torch.float32, device=dev)
        depth = torch.empty((R, 1), dtype=torch.float32, device=dev)
        if R:
            with torch.cuda.device(dev):
                B.call("nfa_render_sdf_fwd", B.ptr(ts), B.ptr(te), B.ptr(sd), B.ptr(cs), B.ptr(c), B.ptr(sel), model, B.ptr(p),
                       ratio, col, B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, R, n, B.ptr(weights), B.ptr(trans),
                       B.ptr(alphas), B.ptr(colors), B.ptr(opac), B.ptr(depth), B.stream())
        ctx.seg, ctx.conv, ctx.has_sel, ctx.has_cos, ctx.param_shape = seg, (model, ratio, col), sel is not None, cs is not None, param.shape
        none = trans.new_empty(0)
        ctx.save_for_backward(ts, te, sd, cs if cs is not None else none, c, p, trans, sel if sel is not None else none)
        return colors, opac, depth, weights, trans, alphas

    @staticmethod
    @once_differentiable
    def backward(ctx, g_c, g_o, g_d, g_w, g_t, g_a):
        ts, te, sd, cs, c, p, trans, sel = ctx.saved_tensors
        sel = sel if ctx.has_sel else None
        cs = cs if ctx.has_cos else None
        seg = ctx.seg
        model, ratio, col = ctx.conv
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise NotImplementedError("nerfacc_amd: rendering_from_sdf is not differentiable w.r.t. t_starts / t_ends "
                                      "(same contract as rendering)")
        need_sd, need_cos, need_c, need_p = (ctx.needs_input_grad[i] for i in (2, 3, 4, 5))
        need_cos = need_cos and cs is not None
        g_sd = torch.empty_like(sd) if need_sd else None
        g_cos = torch.empty_like(cs) if need_cos else None
        g_rgb = torch.empty_like(c) if need_c else None
        g_ps = torch.empty_like(sd) if need_p else None     # per sample; the parameter's gradient is its sum
        if trans.numel() and (need_sd or need_cos or need_c or need_p):
            with torch.cuda.device(trans.device):
                B.call("nfa_render_sdf_bwd", B.ptr(ts), B.ptr(te), B.ptr(sd), B.ptr(cs), B.ptr(c), B.ptr(sel), model, B.ptr(p),
                       ratio, col, B.ptr(trans), B.ptr(_f32c(g_c)), B.ptr(_f32c(g_o)), B.ptr(_f32c(g_d)), B.ptr(_f32c(g_w)),
                       B.ptr(_f32c(g_t)), B.ptr(_f32c(g_a)), B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles,
                       seg.n_rays, trans.numel(), B.ptr(g_sd), B.ptr(g_cos), B.ptr(g_ps), B.ptr(g_rgb), B.stream())
        g_p = torch.sum(g_ps).reshape(ctx.param_shape) if need_p else None
        return None, None, g_sd, g_cos, g_rgb, g_p, None, None, None, None, None


def _as_param(value: Scalar, name: str, like: Tensor) -> Tensor:
    """``inv_s`` / ``beta`` as the caller's tensor, or a float as a 1-element tensor beside ``like``."""
    if isinstance(value, Tensor):
        if value.numel() != 1:
            raise ValueError(f"{name} must be a 1-element tensor or a float, got shape {tuple(value.shape)}")
        return value
    value = float(value)
    if not value > 0.0:
        raise ValueError(f"{name} must be > 0, got {value}")
    return torch.full((1,), value, dtype=like.dtype if like.is_floating_point() else torch.float32, device=like.device)


def rendering_from_sdf(
    t_starts: Tensor,
    t_ends: Tensor,
    raw_rgbs: Tensor,
    sdfs: Tensor,
    ray_indices: Tensor,
    n_rays: Optional[int] = None,
    *,
    model: str = "neus",
    inv_s: Optional[Scalar] = None,
    cos: Optional[Tensor] = None,
    cos_anneal_ratio: float = 1.0,
    beta: Optional[Scalar] = None,
    rgb_activation: str = "sigmoid",
    selector: Optional[Tensor] = None,
    render_bkgd: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Tensor, Dict]:
    """``rendering`` of flattened samples of a signed-distance field.

    ``sdfs`` (N,) or (N, 1) is the field's SDF at the samples and ``raw_rgbs`` (N, 3) its colour output before
    ``rgb_activation`` (``"sigmoid"`` or ``"none"``).  ``model="neus"`` needs ``inv_s`` and ``cos`` (N,), the user's
    ``(dirs * normals).sum(-1)``, and takes ``cos_anneal_ratio``; ``model="volsdf"`` needs ``beta``.  ``inv_s`` / ``beta``
    are a 1-element tensor -- typically an ``nn.Parameter`` or a function of one -- or a Python float; they must be > 0
    (a float is checked, a tensor is not: it is never read on the host).  The opacity of a sample is that of the module
    docstring.  Where the optional bool ``selector`` (N,) is false the sample contributes exactly 0 and every one of its
    gradients is exactly 0 (a select: a non-finite ``sdfs`` there has no effect).

    Returns ``(colors (n_rays, 3), opacities (n_rays, 1), depths (n_rays, 1), extras)`` as ``rendering`` does;
    ``extras`` holds ``weights``, ``trans`` and ``alphas``.  Differentiable to ``raw_rgbs``, ``sdfs``, ``cos`` and
    ``inv_s`` / ``beta``; not to ``t_starts``, ``t_ends``, ``selector`` or ``cos_anneal_ratio``.

    CUDA float32 inputs on one device with ray-sorted ``ray_indices`` and ``t_starts`` / ``t_ends`` that need no gradient
    take one native pass each way.  A tensor ``inv_s`` / ``beta`` is passed by its device pointer and read by the kernel;
    a float becomes a 1-element device tensor.  The parameter's gradient is the ``torch.sum`` of a per-sample stream the
    backward pass writes (no float atomics: two runs give the same bits); the stream exists only when the parameter
    requires a gradient.  Everything else -- CPU tensors, other dtypes (half inputs included: they are out of scope
    here), unsorted indices -- takes :func:`neus_alpha` followed by ``rendering(rgb_alpha_fn=...)`` or
    :func:`laplace_density` followed by ``rendering``'s formulas in torch.  A per-sample ``inv_s`` and a constant-step
    form that does not read ``t_ends`` are out of scope as well: compose :func:`neus_alpha` with ``rendering`` for the
    former.
    """
    if model not in SDF_MODELS:
        raise ValueError(f"model must be one of {sorted(SDF_MODELS)}, got {model!r}")
    if rgb_activation not in RGB_ACTIVATIONS:
        raise ValueError(f"rgb_activation must be one of {sorted(RGB_ACTIVATIONS)}, got {rgb_activation!r}")
    neus = model == "neus"
    if neus and inv_s is None:
        raise ValueError("model='neus' needs inv_s")
    if neus and cos is None:
        raise ValueError("model='neus' needs cos")
    if not neus and beta is None:
        raise ValueError("model='volsdf' needs beta")
    assert n_rays is not None, "n_rays must be provided"
    assert t_starts.dim() == 1 and t_starts.shape == t_ends.shape == ray_indices.shape, \
        "t_starts, t_ends and ray_indices must have the same shape (N,)"
    n = t_starts.shape[0]
    assert sdfs.shape in ((n,), (n, 1)), "sdfs must have shape (N,) or (N, 1)! Got {}".format(sdfs.shape)
    assert raw_rgbs.shape == (n, 3), "raw_rgbs must have shape (N, 3)! Got {}".format(raw_rgbs.shape)
    if neus:
        assert cos.shape == (n,), "cos must have shape (N,)! Got {}".format(cos.shape)
    if selector is not None:
        assert selector.dtype == torch.bool and selector.shape == (n,), "selector must be a bool tensor of shape (N,)"
    sdfs = sdfs.reshape(n)
    param = _as_param(inv_s, "inv_s", sdfs) if neus else _as_param(beta, "beta", sdfs)
    cos = cos if neus else None
    ratio = float(cos_anneal_ratio)

    per_sample = [t for t in (t_starts, t_ends, sdfs, raw_rgbs, cos) if t is not None]
    all_f32_cuda = all(t.is_cuda and t.dtype == torch.float32 and t.device == sdfs.device for t in per_sample)
    native = (all_f32_cuda and param.is_cuda and param.dtype == torch.float32 and param.device == sdfs.device
              and not ((t_starts.requires_grad or t_ends.requires_grad) and torch.is_grad_enabled()))
    if native:
        seg = seginfo_from_ray_indices(ray_indices, n_rays)
        native = seg.contiguous and seg.sorted_indices
    if native:
        colors, opacities, depths, weights, trans, alphas = _RenderSdf.apply(
            t_starts, t_ends, sdfs, cos, raw_rgbs, param, selector, seg, SDF_MODELS[model], ratio, RGB_ACTIVATIONS[rgb_activation])
        extras = {"weights": weights, "alphas": alphas, "trans": trans}
        return _finish_rendering(colors, opacities, depths, extras, colors, render_bkgd)   # (float32's eps)

    # the torch composition.  Behind a false selector the conversion sees sdf = 0 and its result is replaced by 0: no
    # value and no gradient of such a sample gets through, whatever it holds.
    if param.device != sdfs.device:
        param = param.to(sdfs.device)
    z = sdfs if selector is None else torch.where(selector, sdfs, torch.zeros_like(sdfs))
    rgbs = activate_rgb(raw_rgbs, rgb_activation)
    if neus:
        cz = cos if selector is None else torch.where(selector, cos, torch.zeros_like(cos))
        if all_f32_cuda:
            alphas = neus_alpha(z, cz, t_ends - t_starts, param.reshape(()), ratio)
            if selector is not None:
                alphas = torch.where(selector, alphas, torch.zeros_like(alphas))
            colors, opacities, depths, extras = rendering(t_starts, t_ends, ray_indices, n_rays=n_rays,
                                                          rgb_alpha_fn=lambda *_: (rgbs, alphas), render_bkgd=render_bkgd)
        else:   # rendering's packed ops exist for float32 on the device only
            x = _neus_x(z, cz, t_ends - t_starts, param.reshape(()), ratio)
            if selector is not None:
                x = torch.where(selector, x, torch.zeros_like(x))
            colors, opacities, depths, extras = _rendering_x_torch(t_starts, t_ends, x, rgbs, ray_indices, n_rays, render_bkgd)
    else:
        sigmas = laplace_density(z, param.reshape(()))
        if selector is not None:
            sigmas = torch.where(selector, sigmas, torch.zeros_like(sigmas))
        if all_f32_cuda:
            colors, opacities, depths, extras = rendering(t_starts, t_ends, ray_indices, n_rays=n_rays,
                                                          rgb_sigma_fn=lambda *_: (rgbs, sigmas), render_bkgd=render_bkgd)
        else:
            colors, opacities, depths, extras = _rendering_torch(t_starts, t_ends, sigmas, rgbs, ray_indices, n_rays, render_bkgd)
    return colors, opacities, depths, {k: extras[k] for k in ("weights", "trans", "alphas")}


def _rendering_x_torch(t_starts, t_ends, x, rgbs, ray_indices, n_rays, render_bkgd):
    """rawrender._rendering_torch for samples whose summand ``x`` (its ``sigma * delta``) is given: ``rendering``'s
    formulas for flattened samples in plain torch, any device and dtype."""
    ids, idx = torch.sort(ray_indices.to(torch.int64), stable=True)
    counts = torch.bincount(ids, minlength=n_rays)
    first = (torch.cumsum(counts, 0) - counts)[ids]
    xs = x[idx].to(torch.float64)
    c = torch.cumsum(xs, 0)
    base = torch.where(first > 0, c[(first - 1).clamp_min(0)], torch.zeros_like(c))
    S = torch.empty_like(xs).index_copy_(0, idx, c - xs - base).to(x.dtype)
    trans = torch.exp(-S)
    alphas = 1.0 - torch.exp(-x)
    weights = trans * alphas
    mid = (t_starts + t_ends)[:, None] / 2.0

    def accumulate(src):
        return torch.zeros((n_rays, src.shape[-1]), device=src.device, dtype=src.dtype).index_add_(0, ray_indices.to(torch.int64), src)

    colors, opacities, depths = accumulate(weights[:, None] * rgbs), accumulate(weights[:, None]), accumulate(weights[:, None] * mid)
    extras = {"weights": weights, "alphas": alphas, "trans": trans}
    return _finish_rendering(colors, opacities, depths, extras, rgbs, render_bkgd)

"""``rendering`` from the field's raw outputs: the last activations of the field fused into the two rendering passes.

The example fields end every step with an elementwise chain on every sample -- ``trunc_exp(x - 1) * selector`` on the
density and ``sigmoid`` on the colour (examples/radiance_fields/ngp.py:23-36,174-175,196; ``relu`` / ``sigmoid`` in
mlp.py:245) -- and autograd runs its backward twins behind the rendering backward.  :func:`rendering_from_raw` takes the
MLP's outputs BEFORE those activations: on the native path the forward pass applies them as it loads a sample
(csrc/segscan.hip: RenderRawFwdOp) and the backward pass forms them again from the raw values and multiplies their
derivatives in (RenderRawBwdOp), one native call each way.  An extension: the reference has no counterpart, so the name is
not in ``nerfacc_amd.__all__``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from ._segments import SegInfo, seginfo_from_ray_indices
from .volrend import _f32c, _finish_rendering, rendering

# include/nerfacc_hip.h: NFA_ACT_* / NFA_RGB_ACT_*
DENSITY_ACTIVATIONS = {"none": 0, "trunc_exp": 1, "exp": 2, "relu": 3, "softplus": 4}
RGB_ACTIVATIONS = {"none": 0, "sigmoid": 1}


class _TruncExp(torch.autograd.Function):
    """exp(x) whose derivative is exp(min(x, 15)) (ref: examples/radiance_fields/ngp.py:23-36)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


def activate_density(raw_sigmas: Tensor, activation: str, bias: float = 0.0, selector: Optional[Tensor] = None) -> Tensor:
    """The torch composition of the density activation: ``act(raw + bias)`` where ``selector`` is true, exactly 0 (with
    a gradient of exactly 0, whatever the raw value) elsewhere."""
    z = raw_sigmas + bias
    if selector is not None:
        z = torch.where(selector, z, torch.zeros_like(z))   # a non-finite raw value behind the mask reaches no exp
    if activation == "trunc_exp":
        s = _TruncExp.apply(z)
    elif activation == "exp":
        s = torch.exp(z)
    elif activation == "relu":
        s = F.relu(z)
    elif activation == "softplus":
        s = F.softplus(z)
    else:
        s = z
    if selector is not None:
        s = torch.where(selector, s, torch.zeros_like(s))
    return s


def activate_rgb(raw_rgbs: Tensor, activation: str) -> Tensor:
    return torch.sigmoid(raw_rgbs) if activation == "sigmoid" else raw_rgbs


_HALF = (torch.float16, torch.bfloat16)


def _raw_entry(name: str, dtype: torch.dtype):
    """(entry point, leading arguments) for raw streams of ``dtype``: float32 calls the unsuffixed entry as ever, fp16 and
    bf16 the ``_t`` one with its element-type code."""
    return (name, ()) if dtype == torch.float32 else (name + "_t", (B.ELEM_CODES[dtype],))


class _RenderRaw(torch.autograd.Function):
    """One forward and one backward pass over the samples; saves the inputs and ``trans`` only.  ``raw_sigmas`` and
    ``raw_rgbs`` share one dtype, float32, fp16 or bf16: the activated values and both gradients are written in it,
    everything else is float32."""

    @staticmethod
    def forward(ctx, t_starts, t_ends, raw_sigmas, raw_rgbs, selector, seg: SegInfo, dens: int, bias: float, col: int,
                return_activated: bool):
        ctx.set_materialize_grads(False)  # unused outputs arrive as None, not as zero tensors
        ts, te = _f32c(t_starts), _f32c(t_ends)
        if raw_sigmas.dtype in _HALF and raw_rgbs.dtype == raw_sigmas.dtype:
            sg, c = raw_sigmas.contiguous(), raw_rgbs.contiguous()
        else:
            sg, c = _f32c(raw_sigmas), _f32c(raw_rgbs)
        sel = None if selector is None else selector.contiguous()
        dev = B.require_device(ts, te, sg, c, sel)
        R, n = seg.n_rays, sg.numel()
        weights, trans, alphas = torch.empty_like(ts), torch.empty_like(ts), torch.empty_like(ts)
        a_sig = torch.empty_like(sg) if return_activated else None
        a_rgb = torch.empty_like(c) if return_activated else None
        colors = torch.empty((R, 3), dtype=torch.float32, device=dev)
        opac = torch.empty((R, 1), dtype=torch.float32, device=dev)
        depth = torch.empty((R, 1), dtype=torch.float32, device=dev)
        if R:
            with torch.cuda.device(dev):
                entry, elem = _raw_entry("nfa_render_raw_fwd", sg.dtype)
                B.call(entry, *elem, B.ptr(ts), B.ptr(te), B.ptr(sg), B.ptr(c), B.ptr(sel), dens, bias, col,
                       B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, R, n, B.ptr(weights), B.ptr(trans),
                       B.ptr(alphas), B.ptr(a_sig), B.ptr(a_rgb), B.ptr(colors), B.ptr(opac), B.ptr(depth), B.stream())
        ctx.seg, ctx.act, ctx.has_sel = seg, (dens, bias, col), sel is not None
        ctx.save_for_backward(ts, te, sg, c, trans, sel if sel is not None else trans.new_empty(0))
        if not return_activated:
            a_sig, a_rgb = trans.new_empty(0), trans.new_empty(0)
        ctx.mark_non_differentiable(a_sig, a_rgb)
        return colors, opac, depth, weights, trans, alphas, a_sig, a_rgb

    @staticmethod
    @once_differentiable
    def backward(ctx, g_c, g_o, g_d, g_w, g_t, g_a, _g_sig, _g_rgb):
        ts, te, sg, c, trans, sel = ctx.saved_tensors
        sel = sel if ctx.has_sel else None
        seg = ctx.seg
        dens, bias, col = ctx.act
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise NotImplementedError("nerfacc_amd: rendering_from_raw is not differentiable w.r.t. t_starts / t_ends "
                                      "(same contract as rendering)")
        need_sg, need_c = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        g_sig = torch.empty_like(sg) if need_sg else None
        g_rgb = torch.empty_like(c) if need_c else None
        if trans.numel() and (need_sg or need_c):
            with torch.cuda.device(trans.device):
                entry, elem = _raw_entry("nfa_render_raw_bwd", sg.dtype)
                B.call(entry, *elem, B.ptr(ts), B.ptr(te), B.ptr(sg), B.ptr(c), B.ptr(sel), dens, bias, col,
                       B.ptr(trans), B.ptr(_f32c(g_c)), B.ptr(_f32c(g_o)), B.ptr(_f32c(g_d)), B.ptr(_f32c(g_w)),
                       B.ptr(_f32c(g_t)), B.ptr(_f32c(g_a)), B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles,
                       seg.n_rays, trans.numel(), B.ptr(g_sig), B.ptr(g_rgb), B.stream())
        return None, None, g_sig, g_rgb, None, None, None, None, None, None


def rendering_from_raw(
    t_starts: Tensor,
    t_ends: Tensor,
    raw_rgbs: Tensor,
    raw_sigmas: Tensor,
    ray_indices: Tensor,
    n_rays: Optional[int] = None,
    *,
    density_activation: str = "trunc_exp",
    density_bias: float = 0.0,
    rgb_activation: str = "sigmoid",
    selector: Optional[Tensor] = None,
    render_bkgd: Optional[Tensor] = None,
    return_activated: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Dict]:
    """``rendering`` of flattened samples from the field's outputs BEFORE their last activations.

    ``raw_sigmas`` (N,) or (N, 1) and ``raw_rgbs`` (N, 3) are the MLP's outputs; the density is
    ``density_activation(raw_sigmas + density_bias)`` with ``density_activation`` one of ``"trunc_exp"`` (``exp`` whose
    derivative is ``exp(min(z, 15))``), ``"exp"``, ``"relu"``, ``"softplus"`` (beta 1, threshold 20) and ``"none"``, the
    colour ``rgb_activation(raw_rgbs)`` with ``"sigmoid"`` or ``"none"``.  Where the optional bool ``selector`` (N,) --
    e.g. the one ``sample_positions(..., selector=True)`` returns -- is false, the density is exactly 0 and so is its
    gradient (a select, not a product: a non-finite raw density there has no effect).

    Returns ``(colors (n_rays, 3), opacities (n_rays, 1), depths (n_rays, 1), extras)`` as ``rendering`` does;
    ``extras`` holds ``weights``, ``trans`` and ``alphas``.  The activated ``sigmas`` and ``rgbs`` are in ``extras`` only
    with ``return_activated=True``: the native path never materialises them otherwise, so by default (``False``) the two
    keys are absent.  Differentiable to ``raw_rgbs`` and ``raw_sigmas``; not to ``t_starts``, ``t_ends``, ``selector``
    or ``density_bias`` (the contract of ``rendering``).

    CUDA float32 inputs with ray-sorted ``ray_indices`` take one native pass each way (there the activated values, when
    asked for, carry no gradient).  So do ``raw_rgbs`` and ``raw_sigmas`` that are both fp16 or both bf16 (a field run
    under ``torch.autocast``) next to float32 ``t_starts`` / ``t_ends``: the passes load the halves directly and compute
    in float32; ``colors``, ``opacities``, ``depths``, ``weights``, ``trans`` and ``alphas`` are float32, the activated
    values and the gradients are in the raw dtype (each the float32 result rounded once).  Everything else takes the
    same activations in torch, followed by ``rendering`` (CUDA float32: unsorted indices, ``t_starts`` / ``t_ends`` that
    require a gradient) or, where ``rendering`` has no packed ops (CPU tensors, other dtypes, one half and one float32
    raw input, half ``t_starts`` / ``t_ends``), by its formulas in plain torch.
    """
    if density_activation not in DENSITY_ACTIVATIONS:
        raise ValueError(f"density_activation must be one of {sorted(DENSITY_ACTIVATIONS)}, got {density_activation!r}")
    if rgb_activation not in RGB_ACTIVATIONS:
        raise ValueError(f"rgb_activation must be one of {sorted(RGB_ACTIVATIONS)}, got {rgb_activation!r}")
    assert n_rays is not None, "n_rays must be provided"
    assert t_starts.dim() == 1 and t_starts.shape == t_ends.shape == ray_indices.shape, \
        "t_starts, t_ends and ray_indices must have the same shape (N,)"
    n = t_starts.shape[0]
    assert raw_sigmas.shape in ((n,), (n, 1)), "raw_sigmas must have shape (N,) or (N, 1)! Got {}".format(raw_sigmas.shape)
    assert raw_rgbs.shape == (n, 3), "raw_rgbs must have shape (N, 3)! Got {}".format(raw_rgbs.shape)
    if selector is not None:
        assert selector.dtype == torch.bool and selector.shape == (n,), "selector must be a bool tensor of shape (N,)"
    raw_sigmas = raw_sigmas.reshape(n)
    density_bias = float(density_bias)

    all_f32_cuda = all(t.is_cuda and t.dtype == torch.float32 for t in (t_starts, t_ends, raw_sigmas, raw_rgbs))
    half_raw = (all(t.is_cuda and t.dtype == torch.float32 for t in (t_starts, t_ends)) and raw_sigmas.is_cuda
                and raw_rgbs.is_cuda and raw_sigmas.dtype in _HALF and raw_rgbs.dtype == raw_sigmas.dtype
                and t_starts.device == t_ends.device == raw_sigmas.device == raw_rgbs.device)
    native = (all_f32_cuda or half_raw) and not ((t_starts.requires_grad or t_ends.requires_grad) and torch.is_grad_enabled())
    if native:
        seg = seginfo_from_ray_indices(ray_indices, n_rays)
        native = seg.contiguous and seg.sorted_indices
    if native:
        colors, opacities, depths, weights, trans, alphas, a_sig, a_rgb = _RenderRaw.apply(
            t_starts, t_ends, raw_sigmas, raw_rgbs, selector, seg, DENSITY_ACTIVATIONS[density_activation], density_bias,
            RGB_ACTIVATIONS[rgb_activation], bool(return_activated))
        extras = {"weights": weights, "alphas": alphas, "trans": trans}
        if return_activated:
            extras.update(sigmas=a_sig, rgbs=a_rgb)
        return _finish_rendering(colors, opacities, depths, extras, colors, render_bkgd)   # (float32's eps)

    sigmas = activate_density(raw_sigmas, density_activation, density_bias, selector)
    rgbs = activate_rgb(raw_rgbs, rgb_activation)
    if all_f32_cuda:
        colors, opacities, depths, extras = rendering(t_starts, t_ends, ray_indices, n_rays=n_rays,
                                                      rgb_sigma_fn=lambda *_: (rgbs, sigmas), render_bkgd=render_bkgd)
    else:   # rendering's packed ops exist for float32 on the device only
        colors, opacities, depths, extras = _rendering_torch(t_starts, t_ends, sigmas, rgbs, ray_indices, n_rays, render_bkgd)
    if not return_activated:
        extras = {k: v for k, v in extras.items() if k not in ("sigmas", "rgbs")}
    return colors, opacities, depths, extras


def _rendering_torch(t_starts, t_ends, sigmas, rgbs, ray_indices, n_rays, render_bkgd):
    """``rendering``'s formulas (ref: volrend.py:109-158) for flattened samples in plain torch, any device and dtype.
    The per-ray exclusive sum is a flat cumsum minus its value at the ray's start, in float64."""
    ids, idx = torch.sort(ray_indices.to(torch.int64), stable=True)   # samples grouped by ray (a no-op when sorted)
    counts = torch.bincount(ids, minlength=n_rays)
    first = (torch.cumsum(counts, 0) - counts)[ids]
    sdt = sigmas * (t_ends - t_starts)
    x = sdt[idx].to(torch.float64)
    c = torch.cumsum(x, 0)
    base = torch.where(first > 0, c[(first - 1).clamp_min(0)], torch.zeros_like(c))
    S = torch.empty_like(x).index_copy_(0, idx, c - x - base).to(sdt.dtype)
    trans = torch.exp(-S)
    alphas = 1.0 - torch.exp(-sdt)
    weights = trans * alphas
    mid = (t_starts + t_ends)[:, None] / 2.0

    def accumulate(src):
        return torch.zeros((n_rays, src.shape[-1]), device=src.device, dtype=src.dtype).index_add_(0, ray_indices.to(torch.int64), src)

    colors, opacities, depths = accumulate(weights[:, None] * rgbs), accumulate(weights[:, None]), accumulate(weights[:, None] * mid)
    extras = {"weights": weights, "alphas": alphas, "trans": trans, "sigmas": sigmas, "rgbs": rgbs}
    return _finish_rendering(colors, opacities, depths, extras, rgbs, render_bkgd)

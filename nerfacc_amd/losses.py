"""Regularisers over packed samples (native kernels: csrc/segscan.hip, ``DistortionFwdOp`` / ``DistortionBwdOp``).

``distortion`` is the Mip-NeRF 360 distortion loss (Barron et al. 2022, eq. 15), the other half of the proposal-sampling
recipe ``PropNetEstimator`` implements.  Earlier nerfacc releases shipped a packed version; 0.5 dropped it.

Not part of ``nerfacc_amd.__all__`` (that list mirrors the reference's exactly); import the module.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from ._segments import SegInfo, batched_native, resolve

__all__ = ["distortion"]


class _Distortion(torch.autograd.Function):
    """Per-ray loss in one forward pass; its gradients in one reverse pass (``nfa_distortion_fwd`` / ``_bwd``)."""

    @staticmethod
    def forward(ctx, weights, t_starts, t_ends, seg: SegInfo):
        ctx.set_materialize_grads(False)
        w, ts, te = weights.contiguous(), t_starts.contiguous(), t_ends.contiguous()
        dev = B.require_device(w, ts, te)
        R, n = seg.n_rays, w.numel()
        loss, w_tot, s_tot = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(3))
        if R:
            with torch.cuda.device(dev):
                B.call("nfa_distortion_fwd", B.ptr(w), B.ptr(ts), B.ptr(te), B.ptr(seg.packed_info), B.ptr(seg.tiles),
                       seg.n_tiles, R, n, B.ptr(loss), B.ptr(w_tot), B.ptr(s_tot), B.stream())
        ctx.seg = seg
        ctx.save_for_backward(w, ts, te, w_tot, s_tot)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss):
        need_w, need_ts, need_te = ctx.needs_input_grad[:3]
        if g_loss is None or not (need_w or need_ts or need_te):
            return None, None, None, None
        w, ts, te, w_tot, s_tot = ctx.saved_tensors
        seg = ctx.seg
        g = g_loss.to(torch.float32).contiguous()
        g_w = torch.empty_like(w) if need_w else None
        g_ts = torch.empty_like(w) if need_ts else None
        g_te = torch.empty_like(w) if need_te else None
        if w.numel():
            with torch.cuda.device(w.device):
                B.call("nfa_distortion_bwd", B.ptr(w), B.ptr(ts), B.ptr(te), B.ptr(w_tot), B.ptr(s_tot), B.ptr(g),
                       B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, seg.n_rays, w.numel(), B.ptr(g_w),
                       B.ptr(g_ts), B.ptr(g_te), B.stream())
        return g_w, g_ts, g_te, None


def _distortion_torch(weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_ids: Tensor, n_rays: int) -> Tensor:
    """The same O(n) formula in torch, for samples grouped by ray (``ray_ids`` non-decreasing).  Sums run in float64:
    a flat cumsum minus its value at each ray's start is then exact enough for any ray."""
    w = weights.to(torch.float64)
    m = (t_starts.to(torch.float64) + t_ends.to(torch.float64)) / 2.0
    s = t_ends.to(torch.float64) - t_starts.to(torch.float64)
    counts = torch.bincount(ray_ids, minlength=n_rays)
    starts = torch.cumsum(counts, 0) - counts
    first = starts[ray_ids]
    d = m - m[first]  # the loss is shift-invariant; as on the native path

    def excl(x):  # exclusive prefix sum within each ray
        c = torch.cumsum(x, 0)
        base = torch.where(first > 0, c[(first - 1).clamp_min(0)], torch.zeros_like(c))
        return c - x - base

    wd = w * d
    term = 2.0 * w * (d * excl(w) - excl(wd)) + w * w * s / 3.0
    loss = torch.zeros(n_rays, dtype=torch.float64, device=w.device).index_add(0, ray_ids, term)
    return loss.to(weights.dtype)


def _packed_gather(packed_info: Tensor, n_elems: int):
    """(element index, ray id) of every sample a ``packed_info`` covers, in ray order."""
    pi = packed_info.to(torch.int64)
    starts, counts = pi[:, 0], pi[:, 1].clamp_min(0)
    ray_ids = torch.repeat_interleave(torch.arange(pi.shape[0], device=pi.device), counts)
    offs = torch.arange(ray_ids.numel(), device=pi.device) - torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
    idx = starts[ray_ids] + offs
    assert idx.numel() == 0 or (int(idx.min()) >= 0 and int(idx.max()) < n_elems), "packed_info exceeds the samples"
    return idx, ray_ids


def _native_ok(*tensors: Tensor) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 for t in tensors)


def distortion(
    weights: Tensor,
    t_starts: Tensor,
    t_ends: Tensor,
    ray_indices: Optional[Tensor] = None,
    n_rays: Optional[int] = None,
    packed_info: Optional[Tensor] = None,
) -> Tensor:
    """Mip-NeRF 360 distortion loss per ray (Barron et al. 2022, eq. 15):

        loss[r] = sum_{i,j in r} w_i w_j |m_i - m_j| + 1/3 sum_{i in r} w_i^2 (t_end_i - t_start_i),  m = (t_start + t_end) / 2

    Args:
        weights, t_starts, t_ends: packed ``(n_samples,)`` with ``ray_indices`` / ``packed_info``, or batched
            ``(..., n_samples)`` without either.
        ray_indices: ray of every packed sample.  Unsorted indices are grouped by ray (stably) first.
        n_rays: number of rays (default: ``ray_indices.max() + 1``).
        packed_info: ``(n_rays, 2)`` {start, count} per ray; wins over ``ray_indices`` as in ``nerfacc`` 0.5.

    Returns:
        The loss per ray: ``(n_rays,)`` for packed input, ``weights.shape[:-1]`` for batched input.  Differentiable
        w.r.t. ``weights``, ``t_starts`` and ``t_ends``.

    Samples are expected in non-decreasing midpoint order within each ray (both estimators' ``sampling()`` produce it);
    the loss is then computed in O(n) from per-ray prefix sums.  Input out of that order gets what that O(n) form gives
    (it is not detected); tied midpoints take the subgradient of the given order.  CUDA float32 input runs on
    libnerfacc_hip.so; anything else (CPU, other dtypes) runs the same formula in torch.
    """
    assert weights.shape == t_starts.shape == t_ends.shape, "weights, t_starts and t_ends must have the same shape"
    if packed_info is None and ray_indices is None:  # batched (..., n_samples)
        assert weights.dim() >= 1, "batched input must have a samples dimension"
        shape = weights.shape[:-1]
        useg = batched_native(weights, t_starts, t_ends)
        if useg is not None:
            flat = [t.contiguous().view(-1) for t in (weights, t_starts, t_ends)]
            return _Distortion.apply(*flat, useg).view(shape)
        R, S = math.prod(shape), weights.shape[-1]
        ids = torch.arange(R, device=weights.device).repeat_interleave(S)
        flat = [t.reshape(-1) for t in (weights, t_starts, t_ends)]
        return _distortion_torch(*flat, ids, R).view(shape)

    assert weights.dim() == 1, "packed input must be 1-D with shape (n_samples,)"
    n = weights.numel()
    if packed_info is None and n_rays is None:
        n_rays = int(ray_indices.max().item()) + 1 if ray_indices.numel() else 0
    index = packed_info if packed_info is not None else ray_indices
    if _native_ok(weights, t_starts, t_ends) and index.device == weights.device:
        seg = resolve(n, packed_info, ray_indices, n_rays)
        if seg.contiguous and seg.sorted_indices:
            return _Distortion.apply(weights, t_starts, t_ends, seg)
    # torch: group the samples by ray, then the same formula
    if packed_info is not None:
        idx, ids = _packed_gather(packed_info, n)
        R = packed_info.shape[0]
    else:
        ids, idx = torch.sort(ray_indices.to(torch.int64), stable=True)
        R = n_rays
    return _distortion_torch(weights[idx], t_starts[idx], t_ends[idx], ids, R)

"""Regularisers over packed samples (native kernels: csrc/segscan.hip, ``DistortionFwdOp`` / ``DistortionBwdOp``), over
the tables of a plane grid (csrc/planereg.hip), of a VM grid (csrc/vmreg.hip) and of a dense voxel grid (csrc/voxreg.hip).

``distortion`` is the Mip-NeRF 360 distortion loss (Barron et al. 2022, eq. 15), the other half of the proposal-sampling
recipe ``PropNetEstimator`` implements.  Earlier nerfacc releases shipped a packed version; 0.5 dropped it.

``plane_terms`` / ``plane_regularization`` are the regularisers K-Planes (Fridovich-Keil et al. 2023) adds to every step, over
the planes of a :class:`~nerfacc_amd.encodings.PlaneGridEncoding`: total variation in space, the second difference along
time and the L1 pull of the space-time planes towards 1, as one native pass each way.

``vm_terms`` / ``vm_regularization`` are the regularisers TensoRF (Chen et al. 2022) adds to a step, over the planes and lines
of a :class:`~nerfacc_amd.encodings.VMGridEncoding`: total variation, the L1 pull towards 0 and the orthogonality penalty on
the line components, as two launches forward and one backward.

``voxel_terms`` / ``voxel_regularization`` / ``voxel_tv_add_grad_`` are the regularisers DVGO (Sun et al. 2022) and TiNeuVox
put on a :class:`~nerfacc_amd.encodings.VoxelGridEncoding`'s table (csrc/voxreg.hip): total variation along the three axes
under an l2, l1 or Huber penalty and the L1 pull towards 0, as two launches forward and one backward, and as one in-place
launch that adds the gradient straight into ``params.grad``.

Not part of ``nerfacc_amd.__all__`` (that list mirrors the reference's exactly); import the module.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from ._segments import SegInfo, batched_native, resolve
from .encodings import _aligned16

__all__ = ["distortion", "plane_terms", "plane_regularization", "vm_terms", "vm_regularization", "voxel_terms", "voxel_regularization",
           "voxel_tv_add_grad_"]


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


# ----------------------------------------------------------------------------- plane regularisers (csrc/planereg.hip)
def _plane_shapes(table):
    """(offset, size, H, W, is_time) of every plane of a ``PlaneTable``, in table order."""
    return [(table.offsets[s][k], table.sizes[s][k], res[b], res[a], b == 3)
            for s, res in enumerate(table.res) for k, (a, b) in enumerate(table.planes)]


def _plane_counts(H: int, W: int, F: int, time: bool):
    """The number of summands of (tv_h, tv_w, smooth, l1) on an ``[H, W, F]`` plane; 0: the term does not exist."""
    return (F * (H - 1) * W, F * H * (W - 1), F * (H - 2) * W if time else 0, F * H * W if time else 0)


def _plane_terms_torch(params: Tensor, table) -> Tensor:
    """The four terms per plane by slicing, in ``params``' dtype; differentiated by autograd."""
    F, rows = table.n_features, []
    for off, size, H, W, time in _plane_shapes(table):
        p = params[off: off + size].view(H, W, F)
        n_h, n_w, n_s, n_l = _plane_counts(H, W, F, time)
        dh = p[1:] - p[:-1]
        dw = p[:, 1:] - p[:, :-1]
        zero = params.new_zeros(())
        smooth = ((dh[1:] - dh[:-1]) ** 2).sum() / n_s if n_s else zero
        l1 = (1.0 - p).abs().sum() / n_l if n_l else zero
        rows.append(torch.stack([(dh ** 2).sum() / n_h, (dw ** 2).sum() / n_w, smooth, l1]))
    return torch.stack(rows).view(len(table.res), len(table.planes), 4)


def _sign0(v: Tensor) -> Tensor:
    """1, -1, and ``v`` itself where it is neither above nor below 0 (0 at 0; NaN stays NaN): csrc/plane_tiles.h's ``sign0``."""
    return torch.where(v > 0, torch.ones_like(v), torch.where(v < 0, -torch.ones_like(v), v))


def _tv_stencils(p: Tensor):
    """``(gh, gw)`` of an ``[H, W, F]`` plane as csrc/plane_tiles.h's backward row walk forms them: ``A - B`` of the
    differences towards the previous and the next row (node), a literal 0 where that row (node) does not exist."""
    H, W, F = p.shape
    zr, zc = p.new_zeros(1, W, F), p.new_zeros(H, 1, F)
    dh = p[1:] - p[:-1]
    dw = p[:, 1:] - p[:, :-1]
    return torch.cat([zr, dh]) - torch.cat([dh, zr]), torch.cat([zc, dw], 1) - torch.cat([dw, zc], 1)


def _plane_terms_grad_torch(params: Tensor, grad_terms: Tensor, table) -> Tensor:
    """``d (grad_terms . terms) / d params`` in float32, operation for operation as ``nfa_planereg_bwd`` forms it (the
    stencils and their order: csrc/planereg.hip's header), so the two agree bit for bit."""
    F = table.n_features
    p32, g32 = params.detach().to(torch.float32), grad_terms.detach().to(torch.float32).reshape(-1, 4)
    out = torch.empty_like(p32)
    for n, (off, size, H, W, time) in enumerate(_plane_shapes(table)):
        p = p32[off: off + size].view(H, W, F)
        inv = torch.tensor([1.0 / c if c else 0.0 for c in _plane_counts(H, W, F, time)], dtype=torch.float32, device=p.device)
        c = g32[n] * inv
        gh, gw = _tv_stencils(p)
        g = (2.0 * c[0]) * gh + (2.0 * c[1]) * gw
        if time:
            zr, dh = p.new_zeros(1, W, F), p[1:] - p[:-1]
            d2 = dh[1:] - dh[:-1]
            gs = (torch.cat([zr, zr, d2]) - 2.0 * torch.cat([zr, d2, zr])) + torch.cat([d2, zr, zr])
            g = (g + (2.0 * c[2]) * gs) + c[3] * _sign0(p - 1.0)
        out[off: off + size] = g.reshape(-1)
    return out


def _planereg_args(enc):
    return enc.n_scales, enc.n_features, enc.table.c_res


class _PlaneTermsFn(torch.autograd.Function):
    """``terms`` in two launches (``nfa_planereg_fwd``); the table gradient through :class:`_PlaneTermsBwdFn`."""

    @staticmethod
    def forward(ctx, params, enc):
        dev = B.require_device(params)
        p = _aligned16(params)
        n_partials = B.load().nfa_planereg_partials(enc.n_input_dims, *_planereg_args(enc))   # (host arithmetic on the shape)
        partials = torch.empty(n_partials, 4, dtype=torch.float32, device=dev)
        terms = torch.empty(enc.n_scales, len(enc.table.planes), 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            B.call("nfa_planereg_fwd", enc.n_input_dims, B.ptr(p), *_planereg_args(enc), B.ptr(partials), n_partials,
                   B.ptr(terms), B.stream())
        ctx.enc = enc
        ctx.save_for_backward(p)
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        if g_terms is None or not ctx.needs_input_grad[0]:
            return None, None
        (p,) = ctx.saved_tensors
        return _PlaneTermsBwdFn.apply(p, g_terms.to(torch.float32).contiguous(), ctx.enc), None


class _PlaneTermsBwdFn(torch.autograd.Function):
    """The backward as a function ``(params, g_terms) -> g_params`` of its own, so that differentiating it again fails with
    a message that names ``plane_terms`` instead of a missing ``grad_fn`` (as ``encodings._GridBwdFn`` does)."""

    @staticmethod
    def forward(ctx, p, g, enc):
        g_p = torch.empty_like(p)   # (every element is written)
        with torch.cuda.device(p.device):
            B.call("nfa_planereg_bwd", enc.n_input_dims, B.ptr(p), *_planereg_args(enc), B.ptr(g), B.ptr(g_p), B.stream())
        return g_p

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_p):
        raise NotImplementedError("plane_terms: the second order (differentiating dL/dparams again) is not implemented on the "
                                  "native path; the torch path on CPU tensors is differentiated by autograd")


def plane_terms(enc) -> Tensor:
    """The four regularisation terms of every plane of a :class:`~nerfacc_amd.encodings.PlaneGridEncoding`:
    ``[n_scales, n_planes, 4]`` float32 on ``enc.params``' device, ``(tv_h, tv_w, smooth, l1)`` per plane.  With plane
    ``(s, k)`` seen as ``p[j, i, f]`` (``enc.plane(s, k)``: ``j < H`` rows, ``i < W``, ``f < F``), each a mean:

        tv_h   = sum (p[j+1,i,f] - p[j,i,f])^2 / (F (H-1) W)
        tv_w   = sum (p[j,i+1,f] - p[j,i,f])^2 / (F H (W-1))
        smooth = sum ((p[j+2,i,f] - p[j+1,i,f]) - (p[j+1,i,f] - p[j,i,f]))^2 / (F (H-2) W)
        l1     = sum |1 - p[j,i,f]| / (F H W)

    ``smooth`` and ``l1`` exist on the time planes only (those whose rows are the time axis: ``k`` = 2, 4, 5 at D = 4); on
    a spatial plane they are exactly 0, and ``smooth`` is 0 (with zero gradient) when the time axis has 2 nodes.  The
    derivative of ``|1 - p|`` is ``sign(p - 1)``, 0 at ``p == 1``.

    In terms of K-Planes' regularisers, up to weights: its ``compute_plane_tv`` of a plane is ``2 (tv_h + tv_w)``, its
    ``compute_plane_smoothness`` is ``smooth`` and its ``L1TimePlanes`` sums ``l1``; its ``PlaneTV`` counts the spatial planes
    twice.

    Differentiable once towards ``enc.params``.  CUDA float32 parameters run on libnerfacc_hip.so (csrc/planereg.hip: two
    launches forward, one backward, no atomics, nothing read back from the device: the same bits on every run); anything
    else (CPU tensors, other dtypes) runs the same formulas in torch and is differentiated by autograd."""
    params = enc.params
    if params.is_cuda and params.dtype == torch.float32:
        return _PlaneTermsFn.apply(params, enc)
    dt = torch.promote_types(params.dtype, torch.float32)
    return _plane_terms_torch(params.to(dt), enc.table).to(torch.float32)


_REG_WEIGHTS: dict = {}   # (n_dims, n_scales, the four weights, device) -> [n_scales, n_planes, 4]


def _reg_weights(enc, tv: float, tv_time: float, time_smoothness: float, l1_time: float) -> Tensor:
    key = (enc.n_input_dims, enc.n_scales, tv, tv_time, time_smoothness, l1_time, enc.params.device)
    w = _REG_WEIGHTS.get(key)
    if w is None:
        row = [[tv_time, tv_time, time_smoothness, l1_time] if b == 3 else [tv, tv, 0.0, 0.0] for _, b in enc.table.planes]
        w = _REG_WEIGHTS[key] = torch.tensor([row] * enc.n_scales, dtype=torch.float32, device=enc.params.device)
    return w


def plane_regularization(enc, tv: float = 0.0, tv_time: Optional[float] = None, time_smoothness: float = 0.0,
                         l1_time: float = 0.0) -> Tensor:
    """The weighted sum of :func:`plane_terms` over the scales and planes of ``enc``, a scalar:

        sum_s [ tv sum_{spatial k} (tv_h + tv_w) + tv_time sum_{time k} (tv_h + tv_w)
                + time_smoothness sum_{time k} smooth + l1_time sum_{time k} l1 ]

    ``tv_time=None`` means ``tv``.  A non-zero ``time_smoothness`` on an encoding whose time axis has fewer than 3 nodes
    raises ``ValueError`` (there is no second difference to penalise).  Example: K-Planes' ``PlaneTV(w)`` is
    ``plane_regularization(enc, tv=4 * w, tv_time=2 * w)``: K-Planes counts the spatial planes twice and its per-plane value
    is ``2 (tv_h + tv_w)``.

    It is ``plane_terms(enc)`` dotted with a constant weight tensor that is built once per (shape, weights, device) and
    kept, so a call makes no host-to-device copy after the first."""
    tv, time_smoothness, l1_time = float(tv), float(time_smoothness), float(l1_time)
    tv_time = tv if tv_time is None else float(tv_time)
    if time_smoothness != 0.0 and enc.n_input_dims == 4 and min(r[3] for r in enc.table.res) < 3:
        raise ValueError("plane_regularization: time_smoothness needs at least 3 nodes along the time axis "
                         f"(got {min(r[3] for r in enc.table.res)})")
    return (plane_terms(enc) * _reg_weights(enc, tv, tv_time, time_smoothness, l1_time)).sum()


# ----------------------------------------------------------------------------- VM-grid regularisers (csrc/vmreg.hip)
def _vm_counts(H: int, W: int, R: int, C: int):
    """The number of summands of (tv_h, tv_w, l1_plane, tv_line, l1_line, ortho) of a mode; every one positive."""
    return (C * (H - 1) * W, C * H * (W - 1), C * H * W, C * (R - 1), C * R, C * (C - 1) // 2)


def _vm_terms_torch(params: Tensor, table) -> Tensor:
    """The six terms per mode by slicing (and the Gram matrix by a matmul), in ``params``' dtype; differentiated by
    autograd."""
    C, rows = table.n_components, []
    for m in range(3):
        p, l = table.plane(params, m), table.line(params, m)
        n = _vm_counts(p.shape[0], p.shape[1], l.shape[0], C)
        gram = torch.triu(l.t() @ l, diagonal=1)
        rows.append(torch.stack([((p[1:] - p[:-1]) ** 2).sum() / n[0], ((p[:, 1:] - p[:, :-1]) ** 2).sum() / n[1],
                                 p.abs().sum() / n[2], ((l[1:] - l[:-1]) ** 2).sum() / n[3], l.abs().sum() / n[4],
                                 gram.abs().sum() / n[5]]))
    return torch.stack(rows)


def _vm_terms_grad_torch(params: Tensor, grad_terms: Tensor, table) -> Tensor:
    """``d (grad_terms . terms) / d params`` in float32, operation for operation as ``nfa_vmreg_bwd`` forms it from the
    signs ``nfa_vmreg_fwd`` leaves (the stencils and their order: csrc/vmreg.hip's header), so the two agree bit for bit.
    The Gram matrix is summed over ``r`` ascending from 0, ``go`` over ``j`` ascending from 0; the term ``j == i`` is skipped
    (not multiplied by a zero sign), as in the kernel."""
    C = table.n_components
    p32, g32 = params.detach().to(torch.float32), grad_terms.detach().to(torch.float32).reshape(3, 6)
    out = torch.empty_like(p32)
    comp = torch.arange(C, device=p32.device)
    for m in range(3):
        p, l = table.plane(p32, m), table.line(p32, m)
        H, W, R = p.shape[0], p.shape[1], l.shape[0]
        inv = torch.tensor([1.0 / n for n in _vm_counts(H, W, R, C)], dtype=torch.float32, device=p.device)
        c = g32[m] * inv
        gh, gw = _tv_stencils(p)
        g_plane = ((2.0 * c[0]) * gh + (2.0 * c[1]) * gw) + c[2] * _sign0(p)
        dt = l[1:] - l[:-1]
        zl = p.new_zeros(1, C)
        gt = torch.cat([zl, dt]) - torch.cat([dt, zl])
        gram = p.new_zeros(C, C)
        for r in range(R):
            gram = gram + l[r][:, None] * l[r][None, :]
        s = _sign0(gram)
        go = p.new_zeros(R, C)
        for j in range(C):
            go = torch.where(comp != j, go + s[:, j][None, :] * l[:, j][:, None], go)
        g_line = ((2.0 * c[3]) * gt + c[4] * _sign0(l)) + c[5] * go
        table.plane(out, m).copy_(g_plane)
        table.line(out, m).copy_(g_line)
    return out


def _vmreg_args(enc):
    return enc.n_components, enc.table.c_res


class _VMTermsFn(torch.autograd.Function):
    """``terms`` in two launches (``nfa_vmreg_fwd``); the table gradient through :class:`_VMTermsBwdFn`, which reads the
    Gram matrix's signs this pass leaves."""

    @staticmethod
    def forward(ctx, params, enc):
        dev = B.require_device(params)
        p = _aligned16(params)
        C = enc.n_components
        n_partials = B.load().nfa_vmreg_partials(*_vmreg_args(enc))   # (host arithmetic on the shape)
        partials = torch.empty(n_partials, 4, dtype=torch.float32, device=dev)
        signs = torch.empty(3, C, C, dtype=torch.float32, device=dev)
        terms = torch.empty(3, 6, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            B.call("nfa_vmreg_fwd", B.ptr(p), *_vmreg_args(enc), B.ptr(partials), n_partials, B.ptr(signs), B.ptr(terms),
                   B.stream())
        ctx.enc = enc
        ctx.save_for_backward(p, signs)
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        if g_terms is None or not ctx.needs_input_grad[0]:
            return None, None
        p, signs = ctx.saved_tensors
        return _VMTermsBwdFn.apply(p, g_terms.to(torch.float32).contiguous(), signs, ctx.enc), None


class _VMTermsBwdFn(torch.autograd.Function):
    """The backward as a function ``(params, g_terms, signs) -> g_params`` of its own, so that differentiating it again
    fails with a message that names ``vm_terms`` instead of a missing ``grad_fn`` (as ``_PlaneTermsBwdFn`` does)."""

    @staticmethod
    def forward(ctx, p, g, signs, enc):
        g_p = torch.empty_like(p)   # (every element is written)
        with torch.cuda.device(p.device):
            B.call("nfa_vmreg_bwd", B.ptr(p), *_vmreg_args(enc), B.ptr(g), B.ptr(signs), B.ptr(g_p), B.stream())
        return g_p

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_p):
        raise NotImplementedError("vm_terms: the second order (differentiating dL/dparams again) is not implemented on the "
                                  "native path; the torch path on CPU tensors is differentiated by autograd")


def vm_terms(enc) -> Tensor:
    """The six regularisation terms of every mode of a :class:`~nerfacc_amd.encodings.VMGridEncoding`: ``[3, 6]`` float32 on
    ``enc.params``' device, ``(tv_h, tv_w, l1_plane, tv_line, l1_line, ortho)`` per mode.  With mode ``m``'s plane seen as
    ``p[j, i, k]`` (``enc.plane(m)``: ``j < H`` rows, ``i < W``, ``k < C``) and its line as ``l[r, k]`` (``enc.line(m)``:
    ``r < R``), each a mean:

        tv_h     = sum (p[j+1,i,k] - p[j,i,k])^2 / (C (H-1) W)
        tv_w     = sum (p[j,i+1,k] - p[j,i,k])^2 / (C H (W-1))
        l1_plane = sum |p[j,i,k]| / (C H W)
        tv_line  = sum (l[r+1,k] - l[r,k])^2 / (C (R-1))
        l1_line  = sum |l[r,k]| / (C R)
        ortho    = sum_{i<j} |G_ij| / (C (C-1) / 2),   G_ij = sum_r l[r,i] l[r,j]

    The derivative of ``|v|`` is ``sign(v)``, 0 at ``v == 0``; that of ``ortho`` towards ``l[r,i]`` is
    ``sum_{j != i} sign(G_ij) l[r,j] / (C (C-1) / 2)``.

    In terms of TensoRF's ``TensorVMSplit``, on the ``[1, C, H, W]`` / ``[1, C, R, 1]`` views
    (``plane(m).permute(2, 0, 1)[None]``, ``line(m).t()[None, :, :, None]``): ``TVLoss()`` of a plane is
    ``2 (tv_h + tv_w)``, ``density_L1`` is ``sum_m (l1_plane + l1_line)`` and ``vector_comp_diffs`` is ``sum_m ortho`` (the
    mean over the ordered off-diagonal pairs equals the mean over ``i < j``).  ``tv_line`` is this library's own term.
    Nothing beyond these formulas is claimed.

    Differentiable once towards ``enc.params``.  CUDA float32 parameters run on libnerfacc_hip.so (csrc/vmreg.hip: two
    launches forward, one backward, no atomics, nothing read back from the device: the same bits on every run); anything
    else (CPU tensors, other dtypes) runs the same formulas in torch and is differentiated by autograd."""
    params = enc.params
    if params.is_cuda and params.dtype == torch.float32:
        return _VMTermsFn.apply(params, enc)
    dt = torch.promote_types(params.dtype, torch.float32)
    return _vm_terms_torch(params.to(dt), enc.table).to(torch.float32)


_VM_WEIGHTS: dict = {}   # (the four weights, device) -> [3, 6]


def _vm_weights(enc, tv: float, l1: float, tv_line: float, ortho: float) -> Tensor:
    key = (tv, l1, tv_line, ortho, enc.params.device)
    w = _VM_WEIGHTS.get(key)
    if w is None:
        w = _VM_WEIGHTS[key] = torch.tensor([[tv, tv, l1, tv_line, l1, ortho]] * 3, dtype=torch.float32, device=enc.params.device)
    return w


def vm_regularization(enc, tv: float = 0.0, l1: float = 0.0, tv_line: float = 0.0, ortho: float = 0.0) -> Tensor:
    """The weighted sum of :func:`vm_terms` over the modes of ``enc``, a scalar:

        sum_m [ tv (tv_h + tv_w) + l1 (l1_plane + l1_line) + tv_line tv_line + ortho ortho ]

    In TensoRF's training loop, for a weight ``w`` each: ``TV_loss_density(TVLoss()) * w`` (and ``TV_loss_app``) is
    ``tv = 0.02 * w``, because TensoRF multiplies the per-plane value by 1e-2 and that value is ``2 (tv_h + tv_w)``;
    ``density_L1() * w`` is ``l1 = w``; ``vector_comp_diffs() * w`` is ``ortho = w`` -- each on the grid (density or
    appearance) TensoRF applies it to.

    It is ``vm_terms(enc)`` dotted with a constant weight tensor that is built once per (weights, device) and kept, so a call
    makes no host-to-device copy after the first."""
    return (vm_terms(enc) * _vm_weights(enc, float(tv), float(l1), float(tv_line), float(ortho))).sum()


# ----------------------------------------------------------------------------- voxel-grid regularisers (csrc/voxreg.hip)
def _voxel_check(fn: str, enc, kind: str, reduction: str) -> None:
    from .encodings import VoxelGridEncoding
    if not isinstance(enc, VoxelGridEncoding):
        raise ValueError(f"{fn}: enc must be a VoxelGridEncoding (got {type(enc).__name__})")
    if kind not in B.VOXREG_KIND_CODES:
        raise ValueError(f"{fn}: kind must be 'l2', 'l1' or 'huber' (got {kind!r})")
    if reduction not in B.VOXREG_REDUCTION_CODES:
        raise ValueError(f"{fn}: reduction must be 'mean' or 'sum' (got {reduction!r})")


def _voxel_counts(res, C: int):
    """The number of summands of (tv_x, tv_y, tv_z, l1) on a ``[R_z, R_y, R_x, C]`` table; every one positive."""
    Rx, Ry, Rz = res
    return (C * Rz * Ry * (Rx - 1), C * Rz * (Ry - 1) * Rx, C * (Rz - 1) * Ry * Rx, C * Rz * Ry * Rx)


def _voxel_rho(d: Tensor, kind: str) -> Tensor:
    if kind == "l2":
        return d * d
    a = d.abs()
    return a if kind == "l1" else torch.where(a <= 1.0, 0.5 * (d * d), a - 0.5)


def _voxel_p(d: Tensor, kind: str) -> Tensor:
    """``P`` of csrc/voxreg.hip's backward: the identity for l2 (its factor 2 is in ``k_t``), ``rho'`` otherwise."""
    if kind == "l2":
        return d
    if kind == "l1":
        return _sign0(d)
    one = torch.ones_like(d)
    return torch.where(d < -1.0, -one, torch.where(d > 1.0, one, d))


def _voxel_diffs(g: Tensor):
    """The differences of ``g[z, y, x, c]`` towards the next node along x, y and z."""
    return g[:, :, 1:] - g[:, :, :-1], g[:, 1:] - g[:, :-1], g[1:] - g[:-1]


def _voxel_terms_torch(params: Tensor, res, C: int, kind: str, reduction: str) -> Tensor:
    """The four terms by slicing, in ``params``' dtype; differentiated by autograd."""
    g = params.view(res[2], res[1], res[0], C)
    n = _voxel_counts(res, C) if reduction == "mean" else (1, 1, 1, 1)
    sums = [_voxel_rho(d, kind).sum() for d in _voxel_diffs(g)] + [g.abs().sum()]
    return torch.stack([s / c for s, c in zip(sums, n)])


def _voxel_terms_grad_torch(params: Tensor, grad_terms: Tensor, res, C: int, kind: str, reduction: str) -> Tensor:
    """``d (grad_terms . terms) / d params`` in float32, operation for operation as ``nfa_voxreg_bwd`` forms it (the stencils
    and their order: csrc/voxreg.hip's header), so the two agree bit for bit: with ``c_t = grad_terms[t] * (float)(1 / n_t)``
    (``* 1`` with ``"sum"``), ``k_t = 2 c_t`` for l2 and ``c_t`` otherwise,

        gx = (x >= 1 ? P(g - g[x-1]) : 0) - (x + 1 < R_x ? P(g[x+1] - g) : 0)          likewise gy, gz
        v  = k_x gx;   v = v + k_y gy;   v = v + k_z gz;   v = v + c_l sign0(g)"""
    p32, g32 = params.detach().to(torch.float32), grad_terms.detach().to(torch.float32).reshape(4)
    g = p32.view(res[2], res[1], res[0], C)
    scale = [1.0 / n if reduction == "mean" else 1.0 for n in _voxel_counts(res, C)]
    c = g32 * torch.tensor(scale, dtype=torch.float32, device=g.device)
    k = 2.0 * c if kind == "l2" else c
    v = None
    for t, (dim, d) in enumerate(zip((2, 1, 0), _voxel_diffs(g))):
        pd = _voxel_p(d, kind)
        zero = torch.zeros_like(pd.narrow(dim, 0, 1))
        part = k[t] * (torch.cat([zero, pd], dim) - torch.cat([pd, zero], dim))
        v = part if v is None else v + part
    return (v + c[3] * _sign0(g)).reshape(-1)


def _voxreg_args(enc, kind: str, reduction: str):
    return enc.n_features, enc.table.c_res, B.VOXREG_KIND_CODES[kind], B.VOXREG_REDUCTION_CODES[reduction]


class _VoxelTermsFn(torch.autograd.Function):
    """``terms`` in two launches (``nfa_voxreg_fwd``); the table gradient through :class:`_VoxelTermsBwdFn`."""

    @staticmethod
    def forward(ctx, params, enc, kind, reduction):
        dev = B.require_device(params)
        p = _aligned16(params)
        n_partials = B.load().nfa_voxreg_partials(enc.n_features, enc.table.c_res)   # (host arithmetic on the shape)
        partials = torch.empty(n_partials, 4, dtype=torch.float32, device=dev)
        terms = torch.empty(4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            B.call("nfa_voxreg_fwd", B.ptr(p), *_voxreg_args(enc, kind, reduction), B.ptr(partials), n_partials, B.ptr(terms), B.stream())
        ctx.enc, ctx.kind, ctx.reduction = enc, kind, reduction
        ctx.save_for_backward(p)
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        if g_terms is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        (p,) = ctx.saved_tensors
        return _VoxelTermsBwdFn.apply(p, g_terms.to(torch.float32).contiguous(), ctx.enc, ctx.kind, ctx.reduction), None, None, None


class _VoxelTermsBwdFn(torch.autograd.Function):
    """The backward as a function ``(params, g_terms) -> g_params`` of its own, so that differentiating it again fails with
    a message that names ``voxel_terms`` instead of a missing ``grad_fn`` (as ``_VMTermsBwdFn`` does)."""

    @staticmethod
    def forward(ctx, p, g, enc, kind, reduction):
        g_p = torch.empty_like(p)   # (every element is written)
        with torch.cuda.device(p.device):
            B.call("nfa_voxreg_bwd", B.ptr(p), *_voxreg_args(enc, kind, reduction), B.ptr(g), B.ptr(g_p), B.stream())
        return g_p

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_p):
        raise NotImplementedError("voxel_terms: the second order (differentiating dL/dparams again) is not implemented on the "
                                  "native path; the torch path on CPU tensors is differentiated by autograd")


def voxel_terms(enc, kind: str = "l2", reduction: str = "mean") -> Tensor:
    """The four regularisation terms of a :class:`~nerfacc_amd.encodings.VoxelGridEncoding`'s table: ``[4]`` float32 on
    ``enc.params``' device, ``(tv_x, tv_y, tv_z, l1)``.  With the table seen as ``g[z, y, x, c]`` (``enc.grid()``; the base
    table, whatever ``strides``) of resolution ``(R_x, R_y, R_z)`` with ``C`` features:

        tv_x = sum rho(g[z,y,x+1,c] - g[z,y,x,c]) / (C R_z R_y (R_x-1))
        tv_y = sum rho(g[z,y+1,x,c] - g[z,y,x,c]) / (C R_z (R_y-1) R_x)
        tv_z = sum rho(g[z+1,y,x,c] - g[z,y,x,c]) / (C (R_z-1) R_y R_x)
        l1   = sum |g| / (C R_z R_y R_x)

    ``kind`` picks the penalty: ``"l2"``: ``rho(d) = d^2``; ``"l1"``: ``|d|`` (derivative ``sign(d)``, 0 at 0); ``"huber"``:
    ``d^2 / 2`` for ``|d| <= 1``, else ``|d| - 1/2`` (``F.smooth_l1_loss`` with ``beta=1``; derivative ``clamp(d, -1, 1)``).
    ``reduction="sum"`` leaves the divisions out.  The derivative of ``|g|`` is ``sign(g)``, 0 at 0.

    These are the terms DVGO and TiNeuVox build their total variation from (on the ``[1, C, N_x, N_y, N_z]`` view
    ``grid().permute(3, 2, 1, 0)[None]``, the differences along dims 2, 3, 4 are those along x, y, z here); nothing beyond
    these formulas is claimed.

    Differentiable once towards ``enc.params``.  CUDA float32 parameters run on libnerfacc_hip.so (csrc/voxreg.hip: two
    launches forward, one backward, no atomics, nothing read back from the device: the same bits on every run); anything
    else (CPU tensors, other dtypes) runs the same formulas in torch and is differentiated by autograd."""
    _voxel_check("voxel_terms", enc, kind, reduction)
    params = enc.params
    if params.is_cuda and params.dtype == torch.float32:
        return _VoxelTermsFn.apply(params, enc, kind, reduction)
    dt = torch.promote_types(params.dtype, torch.float32)
    return _voxel_terms_torch(params.to(dt), enc.resolution, enc.n_features, kind, reduction).to(torch.float32)


_VOXEL_WEIGHTS: dict = {}   # (the four weights, device) -> [4]


def _voxel_weights(enc, wx: float, wy: float, wz: float, l1: float) -> Tensor:
    key = (wx, wy, wz, l1, enc.params.device)
    w = _VOXEL_WEIGHTS.get(key)
    if w is None:
        w = _VOXEL_WEIGHTS[key] = torch.tensor([wx, wy, wz, l1], dtype=torch.float32, device=enc.params.device)
    return w


def voxel_regularization(enc, tv: float = 0.0, l1: float = 0.0, kind: str = "l2", tv_xyz=None, reduction: str = "mean") -> Tensor:
    """The weighted sum of :func:`voxel_terms`, a scalar:

        tv (tv_x + tv_y + tv_z) + l1 l1          or, with tv_xyz = (wx, wy, wz):    wx tv_x + wy tv_y + wz tv_z + l1 l1

    It is ``voxel_terms(enc, kind, reduction)`` dotted with a constant weight tensor that is built once per (weights, device)
    and kept, so a call makes no host-to-device copy after the first."""
    wx, wy, wz = (float(tv),) * 3 if tv_xyz is None else (float(w) for w in tv_xyz)
    return (voxel_terms(enc, kind, reduction) * _voxel_weights(enc, wx, wy, wz, float(l1))).sum()


@torch.no_grad()
def voxel_tv_add_grad_(enc, wx: float, wy: float, wz: float, l1: float = 0.0, kind: str = "huber", dense: bool = True,
                       reduction: str = "sum") -> None:
    """Adds the gradient of ``wx tv_x + wy tv_y + wz tv_z + l1 l1`` (:func:`voxel_terms`' terms) into ``enc.params.grad`` in
    place, without building the loss: one launch, no allocation.  Per element, with ``c_t`` the weight times ``1 / n_t``
    (times 1 with ``reduction="sum"``), ``k_t = 2 c_t`` and ``P(d) = d`` for ``"l2"``, ``k_t = c_t`` and ``P = rho'`` otherwise:

        gx = (x >= 1 ? P(g - g[x-1]) : 0) - (x + 1 < R_x ? P(g[x+1] - g) : 0)          likewise gy, gz
        grad += ((k_x gx + k_y gy) + k_z gz) + c_l sign(g)

    ``dense=True`` adds everywhere (``grad is None``: zeros are allocated first).  ``dense=False`` adds only where the gradient
    is not exactly 0 (a NaN is not 0) and writes nothing elsewhere (``grad is None``: nothing happens): exactly-zero gradients
    stay exactly zero, so ``FusedAdam(skip_zero_grad=True)`` still skips the voxels no ray touched.

    ``reduction="sum", kind="huber"`` with ``wx = wy = wz = w / 6`` is the form of DVGO's in-place total variation
    (``total_variation_add_grad``: the clamped differences towards the six neighbours, early in training everywhere,
    afterwards only where the data term left a gradient).  The ``1/6`` and the clamp are from memory of DVGO's extension,
    which was not at hand: the formulas above are what is computed, nothing beyond them is claimed.

    CUDA float32 parameters with a contiguous, 16-byte-aligned float32 gradient run on libnerfacc_hip.so
    (``nfa_voxreg_add_grad``); anything else runs :func:`_voxel_terms_grad_torch` and a masked add in torch, with the same bits."""
    _voxel_check("voxel_tv_add_grad_", enc, kind, reduction)
    p = enc.params
    if p.grad is None:
        if not dense:
            return
        p.grad = torch.zeros_like(p)
    grad = p.grad
    w = [float(wx), float(wy), float(wz), float(l1)]
    if (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() % 16 == 0 and grad.dtype == torch.float32
            and grad.device == p.device and not grad.is_sparse and grad.is_contiguous() and grad.data_ptr() % 16 == 0):
        with torch.cuda.device(p.device):
            B.call("nfa_voxreg_add_grad", B.ptr(p), *_voxreg_args(enc, kind, reduction), (ctypes.c_float * 4)(*w), int(bool(dense)),
                   B.ptr(grad), B.stream())
        return
    G = _voxel_terms_grad_torch(p, torch.tensor(w, dtype=torch.float32, device=p.device), enc.resolution, enc.n_features, kind, reduction)
    g32 = grad.to(torch.float32)
    total = g32 + G
    grad.copy_(total if dense else torch.where(g32 != 0, total, g32))

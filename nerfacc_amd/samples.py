"""Sample positions for a field (native kernels: csrc/samples.hip, and ``SamplePosBwdOp`` of csrc/segscan.hip).

``sample_positions`` is the glue every user of ``sampling()`` writes between the estimator and the field: the midpoint
of each sample on its ray (the reference's ``examples/utils.py:83-85``), normalised to the scene box or contracted for
unbounded scenes, the per-sample view directions and the inside-the-box selector (``examples/radiance_fields/ngp.py``
:42-66, :158-164, :185).  As torch expressions that is about ten gather / elementwise launches; here it is one pass
forward and one pass backward, and the gradients towards ``rays_o`` / ``rays_d`` (camera-pose optimisation) are per-ray
sums made by the segmented engine: no float atomics, the same bits every run.

Its outputs are what ``nerfacc_amd.encodings`` expects: ``HashGridEncoding`` takes ``positions`` in [0, 1]^3 (``aabb=``),
``SphericalHarmonicsEncoding`` takes ``dirs="unit"``.

Not part of ``nerfacc_amd.__all__`` (that list mirrors the reference's exactly); import the module.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Union

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from ._segments import SegInfo, seginfo_from_ray_indices, uniform_seginfo

__all__ = ["sample_positions", "SamplePositions"]


class SamplePositions(NamedTuple):
    positions: Tensor            # (..., 3): p, or x in the box's coordinates when ``aabb`` is given
    dirs: Optional[Tensor]       # (..., 3), with ``dirs=``
    selector: Optional[Tensor]   # (...,) bool, with ``selector=True``


_CONTRACTIONS = {None: 0, "sphere": 1, "cube": 2}
_DIRS = {None: 0, "raw": 1, "unit": 2}


class _Box:
    """The aabb as the native calls take it: six host floats passed by value, or -- for a box that lives on the device --
    its address (reading it back would synchronise and could not be captured)."""

    def __init__(self, aabb, device):
        self.host = self.dev = None
        if aabb is None:
            return
        if isinstance(aabb, Tensor) and aabb.is_cuda:
            self.dev = aabb.detach().to(device=device, dtype=torch.float32).contiguous().view(-1)
        else:
            vals = [float(v) for v in (aabb.detach().reshape(-1).tolist() if isinstance(aabb, Tensor) else aabb)]
            self.host = (ctypes.c_float * 6)(*vals)

    def args(self):
        return self.host, B.ptr(self.dev)


class _SamplePositionsFn(torch.autograd.Function):
    """``nfa_sample_positions_fwd`` / ``_bwd``.  Nothing per sample is saved beyond the inputs."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, t_starts, t_ends, ray_indices, box: _Box, contraction: int, dirs_mode: int,
                selector: bool, seg: Optional[SegInfo]):
        ctx.set_materialize_grads(False)
        o, d, ts, te = rays_o.contiguous(), rays_d.contiguous(), t_starts.contiguous(), t_ends.contiguous()
        dev = B.require_device(o, d, ts, te, ray_indices)
        n, n_rays = ts.numel(), o.shape[0]
        S = 0 if ray_indices is not None else ts.shape[-1]
        pos = torch.empty((*ts.shape, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty((*ts.shape, 3), dtype=torch.float32, device=dev) if dirs_mode else None
        sel = torch.empty(ts.shape, dtype=torch.bool, device=dev) if selector else None
        if n:
            with torch.cuda.device(dev):
                B.call("nfa_sample_positions_fwd", B.ptr(o), B.ptr(d), B.ptr(ts), B.ptr(te), B.ptr(ray_indices), n_rays, n, S,
                       *box.args(), contraction, dirs_mode, B.ptr(pos), B.ptr(dirs), B.ptr(sel), B.stream())
        ctx.save_for_backward(o, d, ts, te, ray_indices)
        ctx.box, ctx.contraction, ctx.dirs_mode, ctx.seg, ctx.S = box, contraction, dirs_mode, seg, S
        if sel is not None:
            ctx.mark_non_differentiable(sel)
        return pos, dirs, sel

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pos, g_dirs, _g_sel):
        need_o, need_d, need_ts, need_te = ctx.needs_input_grad[:4]
        none = (None,) * 10
        if (g_pos is None and g_dirs is None) or not (need_o or need_d or need_ts or need_te):
            return none
        o, d, ts, te, ri = ctx.saved_tensors
        dev, n, n_rays, seg = o.device, ts.numel(), o.shape[0], ctx.seg
        g_pos = None if g_pos is None else g_pos.to(torch.float32).contiguous()
        g_dirs = None if g_dirs is None else g_dirs.to(torch.float32).contiguous()
        per_ray = need_o or need_d
        engine = per_ray and seg is not None and seg.contiguous and seg.sorted_indices
        # (two tensors although their values are equal: autograd may hand each to its leaf as .grad)
        g_ts = torch.empty_like(ts) if need_ts else None
        g_te = torch.empty_like(te) if need_te else None
        if g_pos is None:   # the gradient arrived at dirs only: nothing flows through the positions
            g_ts = None if g_ts is None else g_ts.zero_()
            g_te = None if g_te is None else g_te.zero_()
        g_o = g_d = None

        def call(**kw):
            a = dict(g_dirs=None, packed_info=None, tiles=None, n_tiles=0, grad_rays_o=None, grad_rays_d=None, grad_p=None)
            a.update(kw)
            t_out = (g_ts, g_te) if g_pos is not None else (None, None)
            with torch.cuda.device(dev):
                B.call("nfa_sample_positions_bwd", B.ptr(o), B.ptr(d), B.ptr(ts), B.ptr(te), B.ptr(ri), B.ptr(g_pos),
                       B.ptr(a["g_dirs"]), B.ptr(a["packed_info"]), B.ptr(a["tiles"]), a["n_tiles"], n_rays, n, ctx.S,
                       *ctx.box.args(), ctx.contraction, ctx.dirs_mode, B.ptr(a["grad_rays_o"]), B.ptr(a["grad_rays_d"]),
                       B.ptr(t_out[0]), B.ptr(t_out[1]), B.ptr(a["grad_p"]), B.stream())

        if engine:
            g_o = torch.empty_like(o) if need_o else None
            g_d = torch.empty_like(d) if need_d else None
            call(g_dirs=g_dirs, packed_info=seg.packed_info, tiles=seg.tiles, n_tiles=seg.n_tiles, grad_rays_o=g_o, grad_rays_d=g_d)
            return (g_o, g_d, g_ts, g_te) + (None,) * 6
        # ray indices in any order (or no per-ray gradient wanted): g_p per sample from the flat form of the same arithmetic,
        # reduced over rays with index_add_
        g_p = torch.empty((n, 3), dtype=torch.float32, device=dev) if per_ray and g_pos is not None else None
        if n and g_pos is not None:
            call(grad_p=g_p)
        if per_ray:
            rows = ri if ri is not None else torch.arange(n_rays, device=dev).repeat_interleave(ctx.S)
            if need_o:
                g_o = torch.zeros_like(o)
                if g_p is not None:
                    g_o.index_add_(0, rows, g_p)
            if need_d:
                g_d = torch.zeros_like(d)
                term = None if g_p is None else ((ts + te) / 2.0).reshape(-1, 1) * g_p
                if g_dirs is not None:
                    via_dirs = g_dirs.reshape(-1, 3) * (0.5 if ctx.dirs_mode == 2 else 1.0)
                    term = via_dirs if term is None else term + via_dirs
                if term is not None:
                    g_d.index_add_(0, rows, term)
        return (g_o, g_d, g_ts, g_te) + (None,) * 6


def _contract_torch(x: Tensor, contraction: int) -> Tensor:
    u = x * 2 - 1
    if contraction == 1:
        mag = torch.linalg.norm(u, dim=-1, keepdim=True)
    else:   # |u|_inf through its first argmax: the subgradient of that coordinate at ties
        a = u.abs()
        mag = a.gather(-1, a.argmax(dim=-1, keepdim=True))
    safe = torch.where(mag > 1, mag, torch.ones_like(mag))
    u = torch.where(mag > 1, (2 - 1 / safe) * (u / safe), u)
    return u / 4 + 0.5


def _sample_positions_torch(rays_o, rays_d, t_starts, t_ends, ray_indices, aabb, contraction, dirs_mode, selector):
    """The same formulas as torch expressions (CPU tensors, other dtypes); autograd differentiates them."""
    if ray_indices is not None:
        t_origins, t_dirs = rays_o[ray_indices], rays_d[ray_indices]
    else:
        t_origins, t_dirs = rays_o[:, None, :], rays_d[:, None, :].expand(*t_starts.shape, 3)
    x = t_origins + t_dirs * (t_starts + t_ends)[..., None] / 2.0
    if aabb is not None:
        box = torch.as_tensor(aabb, dtype=x.dtype, device=x.device).reshape(-1)
        lo, hi = box[:3], box[3:]
        x = (x - lo) / (hi - lo)
        if contraction:
            x = _contract_torch(x, contraction)
    dirs = None if not dirs_mode else (t_dirs.contiguous() if dirs_mode == 1 else (t_dirs + 1) / 2)
    sel = ((x > 0) & (x < 1)).all(dim=-1) if selector else None
    return SamplePositions(x, dirs, sel)


def sample_positions(
    rays_o: Tensor,
    rays_d: Tensor,
    t_starts: Tensor,
    t_ends: Tensor,
    ray_indices: Optional[Tensor] = None,
    *,
    aabb: Union[None, Tensor, Sequence[float]] = None,
    contraction: Optional[str] = None,
    dirs: Optional[str] = None,
    selector: bool = False,
) -> SamplePositions:
    """Positions of ray samples, ready for a field.

        p = rays_o[r] + (rays_d[r] * (t_starts + t_ends)) / 2

    Args:
        rays_o, rays_d: ``(n_rays, 3)``.
        t_starts, t_ends: packed ``(n,)`` with ``ray_indices`` ``(n,)`` (in any order), or batched ``(n_rays, S)`` without
            it: the ray of an element is then its row.
        aabb: ``{min xyz, max xyz}``, a tensor or six floats: positions become ``x = (p - min) / (max - min)``.
        contraction: ``None``, ``"sphere"`` or ``"cube"`` (needs ``aabb``): the scene contraction of unbounded scenes with
            the 2-norm or the infinity norm: ``u = 2x - 1``; where ``m = |u| > 1``, ``u <- (2 - 1/m) (u / m)``;
            ``x = u / 4 + 0.5``.  The box lands on [0.25, 0.75]^3, everything else inside [0, 1]^3.
        dirs: ``None``, ``"raw"`` (``rays_d[r]`` per sample) or ``"unit"`` (``(rays_d[r] + 1) / 2``, the input of
            ``SphericalHarmonicsEncoding``).
        selector: also return ``((x > 0) & (x < 1)).all(-1)`` (needs ``aabb``).

    Returns:
        ``SamplePositions(positions, dirs, selector)``; fields not asked for are ``None``.  Shapes ``(n, 3)`` / ``(n,)``
        for packed input, ``(n_rays, S, 3)`` / ``(n_rays, S)`` for batched input.

    Differentiable w.r.t. ``rays_o``, ``rays_d``, ``t_starts`` and ``t_ends`` through ``positions`` and ``dirs``.  CUDA
    float32 input runs on libnerfacc_hip.so: without ``aabb`` the positions are bit-identical to the torch expression;
    the gradients of ``rays_o`` / ``rays_d`` are deterministic per-ray sums when ``ray_indices`` is sorted by ray (what
    ``sampling()`` returns), and an ``index_add_`` otherwise.  Neither direction reads from the device (the one exception
    is the sortedness check of ``ray_indices`` this package did not produce, made once per tensor when ``rays_o`` or
    ``rays_d`` needs a gradient).  Anything else (CPU, other dtypes) runs the same formulas in torch.
    """
    if contraction not in _CONTRACTIONS:
        raise ValueError(f"contraction must be None, 'sphere' or 'cube', got {contraction!r}")
    if dirs not in _DIRS:
        raise ValueError(f"dirs must be None, 'raw' or 'unit', got {dirs!r}")
    if aabb is None and contraction is not None:
        raise ValueError("contraction needs an aabb")
    if aabb is None and selector:
        raise ValueError("selector=True needs an aabb")
    if aabb is not None and (aabb.numel() if isinstance(aabb, Tensor) else len(aabb)) != 6:
        raise ValueError("aabb must hold 6 values: min xyz, max xyz")
    assert rays_o.dim() == 2 and rays_o.shape[-1] == 3 and rays_o.shape == rays_d.shape, "rays_o and rays_d must be (n_rays, 3)"
    assert t_starts.shape == t_ends.shape, "t_starts and t_ends must have the same shape"
    if ray_indices is not None:
        assert t_starts.dim() == 1 and ray_indices.shape == t_starts.shape, "packed input must be 1-D with shape (n_samples,)"
    else:
        assert t_starts.dim() == 2 and t_starts.shape[0] == rays_o.shape[0], "batched input must be (n_rays, n_samples)"
    c, dm = _CONTRACTIONS[contraction], _DIRS[dirs]
    tensors = (rays_o, rays_d, t_starts, t_ends)
    native = all(t.is_cuda and t.dtype == torch.float32 and t.device == rays_o.device for t in tensors) and \
        (ray_indices is None or ray_indices.device == rays_o.device)
    if not native:
        return _sample_positions_torch(rays_o, rays_d, t_starts, t_ends, ray_indices, aabb, c, dm, selector)
    ri = ray_indices
    if ri is not None and (ri.dtype != torch.int64 or not ri.is_contiguous()):
        ri = ri.to(torch.int64).contiguous()
    seg = None
    if t_starts.numel() and torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad):
        if ray_indices is None:
            seg = uniform_seginfo(rays_o.shape[0], t_starts.shape[-1], rays_o.device)
        else:
            seg = seginfo_from_ray_indices(ray_indices, rays_o.shape[0])   # cached on the tensor; sampling() pre-tags its own
    out = _SamplePositionsFn.apply(rays_o, rays_d, t_starts, t_ends, ri, _Box(aabb, rays_o.device), c, dm, bool(selector), seg)
    return SamplePositions(*out)

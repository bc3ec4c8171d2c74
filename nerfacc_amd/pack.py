"""``pack_info`` (ref: nerfacc/pack.py:10-49), and nerfacc 0.3's ``unpack_info`` / ``unpack_data`` / ``pack_data``.

The last three convert between the two sample layouts the ops take: packed ``(all_samples, ...)`` with ``packed_info``
``(n_rays, 2)``, and padded ``(n_rays, n_samples, ...)``.  nerfacc 0.5 removed them ("temporally", CHANGELOG 0.5.0); they
are attributes of ``nerfacc_amd`` but not part of ``__all__``, which mirrors 0.5's names.  Native kernels:
csrc/pack.hip (``nfa_unpack_rows`` / ``nfa_pack_rows`` / ``nfa_mask_row_counts``) and ``nfa_fill_ray_indices``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from ._segments import _ATTR, SegInfo, pack_info_native, tag_ray_indices, tag_trusted


@torch.no_grad()
def pack_info(ray_indices: Tensor, n_rays: Optional[int] = None) -> Tensor:
    """Pack ``ray_indices`` to ``packed_info`` = (start, count) per ray, LongTensor (n_rays, 2).

    >>> pack_info(tensor([0, 0, 1, 1, 1, 2, 2, 2, 2]), n_rays=3)
    tensor([[0, 2], [2, 3], [5, 4]])

    Like the reference this needs a device tensor (pack.py:47-48 raises on CPU).  The histogram
    uses one atomic per run of equal indices instead of ``index_add_`` per sample.
    """
    assert ray_indices.dim() == 1, "ray_indices must be a 1D tensor with shape (n_samples)."
    if not ray_indices.is_cuda:
        raise NotImplementedError("Only support cuda inputs.")
    if n_rays is None:
        n_rays = int(ray_indices.max().item()) + 1 if ray_indices.numel() else 0
    packed, _ = pack_info_native(ray_indices, n_rays)
    tag_trusted(packed, ray_indices.numel())
    if ray_indices.dtype != torch.int64:
        packed = packed.to(ray_indices.dtype)  # the reference keeps the dtype of ray_indices
    return packed


# --------------------------------------------------------------------------- packed <-> padded


def _as_pairs(packed_info: Tensor) -> Tensor:
    if packed_info.dim() != 2 or packed_info.shape[-1] != 2:
        raise ValueError(f"packed_info must have shape (n_rays, 2), got {tuple(packed_info.shape)}")
    if packed_info.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"packed_info must be int32 or int64, got {packed_info.dtype}")
    return packed_info.to(torch.int64).contiguous()


def _trusted(packed_info: Tensor, n: int) -> Optional[SegInfo]:
    """The SegInfo of a ``packed_info`` this package produced for ``n`` samples (its chunks tile [0, n)), else None."""
    cached = getattr(packed_info, _ATTR, None)
    if cached is not None and cached[0] == packed_info._version and cached[1] == n and cached[2].trusted:
        return cached[2]
    return None


def _check_chunks(pi: Tensor, n: int) -> Tuple[bool, bool, bool, int]:
    """(in range, disjoint, tiling [0, n) in ray order, largest count) of foreign chunks, by torch reductions and ONE
    read-back; nothing is launched on foreign data before this."""
    if pi.shape[0] == 0:
        return True, True, n == 0, 0
    starts, cnts = pi[:, 0], pi[:, 1]
    ends = starts + cnts
    in_range = ((starts >= 0) & (cnts >= 0) & (ends <= n)).all()
    s_sorted, order = torch.sort(starts, stable=True)
    reach = torch.cummax(ends[order], 0).values                    # furthest end among chunks that start no later
    overlap = ((s_sorted[1:] < reach[:-1]) & (cnts[order][1:] > 0)).any()
    tiling = (starts == torch.cumsum(cnts, 0) - cnts).all() & (cnts.sum() == n)
    ok, no_overlap, tiles, cmax = torch.stack([in_range.long(), (~overlap).long(), tiling.long(), cnts.max()]).tolist()
    return bool(ok), bool(no_overlap), bool(tiles), int(cmax)


def _pad_bytes(pad_value, dtype: torch.dtype) -> bytes:
    return torch.full((1,), pad_value, dtype=dtype).view(torch.uint8).numpy().tobytes()


def _row_bytes(t: Tensor, lead: int) -> int:
    return math.prod(t.shape[lead:]) * t.element_size()


def _unpack_info_torch(pi: Tensor) -> Tensor:
    return torch.repeat_interleave(torch.arange(pi.shape[0], device=pi.device), pi[:, 1])


def _unpack_data_torch(pi: Tensor, data: Tensor, S: int, pad_value) -> Tensor:
    R = pi.shape[0]
    keep = pi[:, 1].clamp(max=S)
    rows = torch.repeat_interleave(torch.arange(R, device=pi.device), keep)
    slot = torch.arange(rows.numel(), device=pi.device) - (torch.cumsum(keep, 0) - keep)[rows]
    out = data.new_full((R, S, *data.shape[1:]), pad_value)
    return out.index_put((rows, slot), data[pi[rows, 0] + slot])


def _pack_data_torch(data: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
    cnts = mask.sum(1, dtype=torch.int64)
    return data[mask], torch.stack([torch.cumsum(cnts, 0) - cnts, cnts], dim=-1)


class _UnpackData(torch.autograd.Function):
    """packed -> padded by counts (``nfa_unpack_rows``); the backward is the reverse gather (``nfa_pack_rows``)."""

    @staticmethod
    def forward(ctx, data, pi, S: int, pad_value, tiles: bool):
        d = data.contiguous()
        dev = B.require_device(d, pi)
        R, N, rb = pi.shape[0], d.shape[0], _row_bytes(d, 1)
        out = torch.empty((R, S, *d.shape[1:]), dtype=d.dtype, device=dev)
        pad = _pad_bytes(pad_value, d.dtype) if pad_value != 0 else b""
        buf = C.create_string_buffer(pad, max(len(pad), 1))
        if out.numel():
            with torch.cuda.device(dev):
                B.call("nfa_unpack_rows", B.ptr(d), B.ptr(pi), None, R, S, N, rb, C.addressof(buf) if pad else None,
                       len(pad), B.ptr(out), B.stream())
        ctx.save_for_backward(pi)
        ctx.meta = (N, S, rb, tiles, d.shape[1:])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        (pi,) = ctx.saved_tensors
        N, S, rb, tiles, feat = ctx.meta
        g = g_out.contiguous()
        # every packed row is written when the chunks tile [0, N) and S > 0 (dropped samples get zeros); else zero-fill
        g_data = (torch.empty if tiles and S > 0 else torch.zeros)((N, *feat), dtype=g.dtype, device=g.device)
        if g.numel() and N:
            with torch.cuda.device(g.device):
                B.call("nfa_pack_rows", B.ptr(g), B.ptr(pi), None, pi.shape[0], S, N, rb, B.ptr(g_data), B.stream())
        return g_data, None, None, None, None


class _PackData(torch.autograd.Function):
    """padded -> packed by a mask (``nfa_mask_row_counts`` + ``nfa_exclusive_cumsum_pairs_i64`` + ``nfa_pack_rows``); the
    backward scatters back with zeros at unset slots (``nfa_unpack_rows``)."""

    @staticmethod
    def forward(ctx, data, mask):
        d, m = data.contiguous(), mask.contiguous()
        dev = B.require_device(d, m)
        R, S, rb = m.shape[0], m.shape[1], _row_bytes(d, 2)
        pi = torch.zeros((R, 2), dtype=torch.int64, device=dev)
        N = 0
        if R:
            with torch.cuda.device(dev):
                cnts = torch.empty(R, dtype=torch.int64, device=dev)
                total = torch.empty(1, dtype=torch.int64, device=dev)
                scratch = B.cumsum_scratch(R, dev)
                B.call("nfa_mask_row_counts", B.ptr(m), R, S, B.ptr(cnts), B.stream())
                B.call("nfa_exclusive_cumsum_pairs_i64", B.ptr(cnts), R, B.ptr(pi), B.ptr(total), B.ptr(scratch), B.stream())
                N = int(total.item())   # sizes the output, as data[mask] does
        out = torch.empty((N, *d.shape[2:]), dtype=d.dtype, device=dev)
        if out.numel():
            with torch.cuda.device(dev):
                B.call("nfa_pack_rows", B.ptr(d), B.ptr(pi), B.ptr(m), R, S, N, rb, B.ptr(out), B.stream())
        ctx.mark_non_differentiable(pi)
        ctx.save_for_backward(m, pi)
        ctx.meta = (N, rb, d.shape)
        return out, pi

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_pi):
        m, pi = ctx.saved_tensors
        N, rb, shape = ctx.meta
        if g_out is None:
            return None, None
        g = g_out.contiguous()
        g_data = torch.empty(shape, dtype=g.dtype, device=g.device)
        if g_data.numel():
            with torch.cuda.device(g.device):
                B.call("nfa_unpack_rows", B.ptr(g), B.ptr(pi), B.ptr(m), shape[0], shape[1], N, rb, None, 0, B.ptr(g_data),
                       B.stream())
        return g_data, None


@torch.no_grad()
def unpack_info(packed_info: Tensor, n_samples: int) -> Tensor:
    """Ray index of every packed sample (nerfacc 0.3): LongTensor ``(n_samples,)``.

    >>> unpack_info(tensor([[0, 2], [2, 3], [5, 0]]), 5)
    tensor([0, 0, 1, 1, 1])

    Args:
        packed_info: ``(n_rays, 2)`` {start, count} per ray, int32 or int64.  Its chunks must tile ``[0, n_samples)`` in
            ray order (``pack_info``, ``sampling`` and ``pack_data`` produce that); anything else raises ``ValueError``.
        n_samples: the total number of packed samples.

    The result carries its segment bookkeeping, so ``rendering(..., ray_indices=unpack_info(pi, n), n_rays=R)`` runs no
    ``pack_info`` and no read-back.  CUDA input runs ``nfa_fill_ray_indices``; CPU input the same in torch.
    """
    pi = _as_pairs(packed_info)
    n = int(n_samples)
    if _trusted(packed_info, n) is None and _trusted(pi, n) is None:
        ok, _, tiles, _ = _check_chunks(pi, n)
        if not (ok and tiles):
            raise ValueError(f"unpack_info: the chunks of packed_info must tile [0, {n}) in ray order")
    if not pi.is_cuda:
        return _unpack_info_torch(pi)
    R = pi.shape[0]
    ray_indices = torch.empty(n, dtype=torch.int64, device=pi.device)
    if n:
        with torch.cuda.device(pi.device):
            B.call("nfa_fill_ray_indices", R, B.ptr(pi), B.ptr(ray_indices), B.stream())
    tag_ray_indices(ray_indices, R, tag_trusted(pi, n))
    return ray_indices


def unpack_data(packed_info: Tensor, data: Tensor, n_samples: Optional[int] = None, pad_value=0) -> Tensor:
    """Packed samples to padded rows (nerfacc 0.3): ``data (N, D)`` -> ``(n_rays, S, D)``; 1-D ``data (N,)`` -> ``(n_rays, S)``.

    Args:
        packed_info: ``(n_rays, 2)`` {start, count} per ray, int32 or int64.  Any chunks with ``start >= 0``,
            ``count >= 0`` and ``start + count <= N`` that do not overlap, with gaps and in any order; anything else
            raises ``ValueError`` (checked with torch reductions before any kernel runs).
        data: packed samples, ``(N, ...)``, any dtype.
        n_samples: ``S``, the padded row length.  Default: the largest count (one read-back, as in 0.3).
        pad_value: the value of slots without a sample, cast to ``data.dtype``.

    Returns:
        ``(n_rays, S, ...)``: row ``r`` holds the ray's samples ``0 .. min(count_r, S) - 1`` in order, then ``pad_value``.
        Samples past ``S`` are dropped and get zero gradient; so do packed samples no chunk covers.  Differentiable w.r.t.
        ``data``.

    CUDA tensors run csrc/pack.hip for every dtype; CPU tensors run the same in torch.
    """
    if data.dim() < 1:
        raise ValueError("data must have a samples dimension")
    pi = _as_pairs(packed_info)
    N = data.shape[0]
    info = _trusted(packed_info, N) or _trusted(pi, N)
    if info is not None:
        tiles = True
        if n_samples is None:
            n_samples = int(pi[:, 1].max()) if pi.shape[0] else 0
    else:
        ok, disjoint, tiles, cmax = _check_chunks(pi, N)
        if not ok:
            raise ValueError(f"unpack_data: packed_info needs start >= 0, count >= 0 and start + count <= {N}")
        if not disjoint:
            raise ValueError("unpack_data: the chunks of packed_info overlap")
        if n_samples is None:
            n_samples = cmax
    S = int(n_samples)
    if S < 0:
        raise ValueError("n_samples must be >= 0")
    if not data.is_cuda:
        return _unpack_data_torch(pi, data, S, pad_value)
    return _UnpackData.apply(data, pi, S, pad_value, tiles)


def pack_data(data: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
    """Padded rows to packed samples (nerfacc 0.3): ``data (n_rays, S, D)`` (or ``(n_rays, S)``) and a bool ``mask (n_rays, S)``
    give ``packed_data (N, D)``, the set samples in row-major order (``data[mask]``), and ``packed_info (n_rays, 2)``.

    ``packed_info`` is int64 (nerfacc 0.3 returned int32; int64 is what every op here takes) and carries its segment
    bookkeeping.  Differentiable w.r.t. ``data``; unset slots get zero gradient.  One read-back sizes the output, as
    ``data[mask]`` needs.  CUDA tensors run csrc/pack.hip for every dtype; CPU tensors run the same in torch.
    """
    if mask.dim() != 2 or mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor of shape (n_rays, S), got {mask.dtype} {tuple(mask.shape)}")
    if data.dim() < 2 or data.shape[:2] != mask.shape:
        raise ValueError(f"data {tuple(data.shape)} must start with the mask's shape {tuple(mask.shape)}")
    if not data.is_cuda:
        return _pack_data_torch(data, mask)
    packed, pi = _PackData.apply(data, mask)
    tag_trusted(pi, packed.shape[0])
    return packed, pi

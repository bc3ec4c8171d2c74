"""Input encodings of Instant-NGP radiance fields (native kernels: csrc/encoding.hip).

``HashGridEncoding`` and ``SphericalHarmonicsEncoding`` stand for tiny-cuda-nn's ``HashGrid`` (2-D, 3-D or 4-D input, linear
or smoothstep interpolation) and ``SphericalHarmonics`` encodings, the two encodings nerfacc's example radiance fields
(``examples/radiance_fields/ngp.py``: ``NGPRadianceField``, ``NGPDensityField``) are built on; the MLPs around them are
plain ``torch.nn`` layers.  ``encoding_from_tcnn_config`` builds them from the config dicts those examples pass to tcnn.
Parameter layout compatibility with tcnn checkpoints is not a goal.

``PlaneGridEncoding`` is the plane-factorised multiscale encoding of K-Planes (3-D: tri-planes, 4-D: the six planes of a
dynamic scene) as one native pass each way (csrc/planes.hip); it shares ``out_dtype`` and the device rules below.
``VMGridEncoding`` is TensoRF's vector-matrix decomposition (three plane x line modes, concatenated for the appearance or
summed for the density) with its grid resampling (csrc/vmgrid.hip), under the same rules.
``VoxelGridEncoding`` is the dense voxel grid of DVGO and TiNeuVox (trilinear samples of one ``[R_z, R_y, R_x, C]`` table at
up to four node strides, TiNeuVox's multi-distance interpolation) with its resampling (csrc/voxgrid.hip), under the same rules.
``SinusoidalEncoding`` is NeRF's positional encoding, the front end of the reference's MLP fields
(``examples/radiance_fields/mlp.py``: ``SinusoidalEncoder``), with one native pass each for the forward, the backward and the
second order (csrc/sinenc.hip); it has no parameters and is not reachable through ``encoding_from_tcnn_config``.

CUDA float32 tensors run on libnerfacc_hip.so; CPU tensors and other dtypes run the same formulas in torch (the hash grid's
torch path reproduces the native forward bit for bit).  Under ``torch.autocast`` both encodings run in float32, as tcnn's
do.  Neither direction reads from the device, so a step that uses them can be captured (``CapturedStep``).

``out_dtype`` (``None``: float32) makes an encoding write fp16 or bf16 activations, as tcnn's do by default, and take
the gradient in that dtype: the arithmetic stays float32, the kernels convert each value once as they store or load it, so
the output equals ``float32_output.to(out_dtype)`` bit for bit and no cast pass runs next to a mixed-precision MLP.
``"autocast"`` follows the active autocast dtype.  Parameters, inputs and their gradients are float32 either way.

Not part of ``nerfacc_amd.__all__`` (that list mirrors the reference's exactly); import the module.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import itertools
import math

import numpy as np
import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _backend as B

__all__ = ["HashGridEncoding", "SphericalHarmonicsEncoding", "PlaneGridEncoding", "VMGridEncoding", "VoxelGridEncoding", "SinusoidalEncoding",
           "barf_window", "encoding_from_tcnn_config"]

_M32 = 0xFFFFFFFF
_PRIMES = (1, 2654435761, 805459861, 3674653429)   # tcnn's hash primes of dimensions 0..3
GRID_DIMS = (2, 3, 4)   # input dimensions of the native hash grid

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp2f.restype = ctypes.c_float
_libm.exp2f.argtypes = [ctypes.c_float]
_libm.log2f.restype = ctypes.c_float
_libm.log2f.argtypes = [ctypes.c_float]


class LevelTable:
    """Per-level constants of a hash grid, computed once on the host in float32 (the C library's exp2f / log2f):

        scale_l = exp2f(l * log2f(per_level_scale)) * base_resolution - 1,   res_l = ceil(scale_l) + 1,
        size_l = min(roundup8(res_l^D), 2^log2_hashmap_size) (hashed when the dense size is larger), D = n_dims,
        offset_l = sum of the sizes of the levels before l.

    ``scale_l`` and ``res_l`` do not depend on ``n_dims``; ``res_l^D`` is a Python int (no overflow).
    """

    def __init__(self, n_levels: int, log2_hashmap_size: int, base_resolution: float, per_level_scale: float,
                 n_dims: int = 3):
        f32 = np.float32
        self.n_dims = int(n_dims)
        lg = f32(_libm.log2f(float(f32(per_level_scale))))
        self.scales, self.resolutions, self.sizes, self.offsets, self.hashed = [], [], [], [], []
        table, offset = 1 << int(log2_hashmap_size), 0
        for l in range(int(n_levels)):
            e = f32(f32(l) * lg)
            s = f32(f32(_libm.exp2f(float(e))) * f32(base_resolution)) - f32(1.0)
            r = int(math.ceil(float(s))) + 1
            dense = (r ** self.n_dims + 7) // 8 * 8
            self.scales.append(float(s))
            self.resolutions.append(r)
            self.sizes.append(min(dense, table))
            self.hashed.append(dense > table)
            self.offsets.append(offset)
            offset += self.sizes[-1]
        self.n_entries = offset
        self.log2_hashmap_size = int(log2_hashmap_size)
        # host arrays handed to nfa_hashgrid_{fwd,bwd} (read synchronously by each call)
        self.c_scales = (ctypes.c_float * len(self.scales))(*self.scales)
        self.c_res = (ctypes.c_int32 * len(self.scales))(*[min(r, 1 << 30) for r in self.resolutions])
        self.c_sizes = (ctypes.c_int32 * len(self.scales))(*self.sizes)


def _hashgrid_torch(x: Tensor, params: Tensor, t: LevelTable, n_features: int, interp: int = 0) -> Tensor:
    """The hash grid in torch, op for op as csrc/encoding.hip computes it (x [N, D], D = ``t.n_dims``, and params in one
    float dtype); ``interp``: a ``B.INTERP_CODES`` value."""
    F, D = n_features, t.n_dims
    table = params.view(-1, F)
    outs = []
    for l in range(len(t.scales)):
        p = x * t.scales[l] + 0.5   # (a float32 value: exact in x's dtype)
        fl = torch.floor(p)
        f = p - fl
        if interp == B.INTERP_CODES["Smoothstep"]:
            f = (f * f) * (3.0 - 2.0 * f)   # S(f) takes the fraction's place in the corner weights
        g = fl.detach().clamp(-2147483648.0, 2147483520.0).to(torch.int64) & _M32
        lvl = table[t.offsets[l]: t.offsets[l] + t.sizes[l]]
        size, res = t.sizes[l], t.resolutions[l]
        acc = torch.zeros(x.shape[0], F, dtype=x.dtype, device=x.device)
        for c in range(1 << D):
            b = [(c >> d) & 1 for d in range(D)]
            q = [(g[:, d] + b[d]) & _M32 for d in range(D)]
            if t.hashed[l]:
                idx = q[0]
                for d in range(1, D):
                    idx = idx ^ ((q[d] * _PRIMES[d]) & _M32)
                idx = idx & (size - 1)
            else:
                idx, power = q[0], res   # (sum_d q_d res^d mod 2^32: the powers wrap, every partial sum is reduced)
                for d in range(1, D):
                    idx = (idx + q[d] * power) & _M32
                    power = (power * res) & _M32
                idx = idx % size
            w = [f[:, d] if b[d] else 1.0 - f[:, d] for d in range(D)]
            wc = w[0]
            for d in range(1, D):
                wc = wc * w[d]
            acc = acc + wc[:, None] * lvl[idx]
        outs.append(acc)
    return torch.cat(outs, -1)


def _aligned16(t: Tensor) -> Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


_HALF = (torch.float16, torch.bfloat16)


def _check_out_dtype(out_dtype):
    if out_dtype is None or out_dtype == "autocast" or out_dtype in _HALF:   # (a str never equals a torch.dtype)
        return out_dtype
    if out_dtype == torch.float32:
        return None
    raise ValueError(f"out_dtype must be None, torch.float32, torch.float16, torch.bfloat16 or 'autocast' (got {out_dtype!r})")


def _resolve_out_dtype(out_dtype, x: Tensor) -> torch.dtype:
    """The dtype an encoding returns for input ``x``; call before autocast is switched off."""
    if out_dtype is None:
        return torch.float32
    if out_dtype == "autocast":
        dt = x.device.type
        if torch.is_autocast_enabled(dt) and torch.get_autocast_dtype(dt) in _HALF:
            return torch.get_autocast_dtype(dt)
        return torch.float32
    return out_dtype


def _entry(name: str, dtype: torch.dtype, interp: int = 0, n_dims: int = 3):
    """(entry point, leading arguments): float32 calls the unsuffixed entry as ever, fp16 / bf16 the ``_t`` one, and an
    interpolation other than Linear the ``_i`` one.  The ``_sorted`` entries always take the element code.  A hash grid of
    2 or 4 input dimensions calls the ``_d`` entry, which takes all three codes."""
    if n_dims != 3:
        return name + "_d", (n_dims, interp, B.ELEM_CODES[dtype])
    if interp:
        return name + "_i", (interp, B.ELEM_CODES[dtype])
    if name.endswith("_sorted"):
        return name, (B.ELEM_CODES[dtype],)
    return (name, ()) if dtype == torch.float32 else (name + "_t", (B.ELEM_CODES[dtype],))


def _table_args(enc: "HashGridEncoding", n_points: int, params: Tensor):
    """The grid description every ``nfa_hashgrid_*`` entry takes after its tensors."""
    t = enc.table
    return (n_points, enc.n_levels, enc.n_features_per_level, t.log2_hashmap_size, t.c_scales, t.c_res, t.c_sizes,
            params.numel())


SORTED_MAX_POINTS = (1 << 29) - 1   # nfa_hashgrid_*_sorted: the item id 8 n + c is 32 bits wide (3-D)


def sorted_max_points(n_dims: int) -> int:
    """The most points one ``deterministic=True`` call takes: the item id ``2^D n + c`` is 32 bits wide."""
    return (1 << (32 - n_dims)) - 1


def _sorted_scratch(enc: "HashGridEncoding", n_points: int, device) -> Tensor:
    """The scratch of one ``nfa_hashgrid_*_sorted`` call: a byte tensor from torch's allocator (under graph capture: the
    graph's pool), sized by the library."""
    D = enc.n_input_dims
    if n_points > sorted_max_points(D):
        raise ValueError(f"HashGridEncoding(deterministic=True): {n_points} points in one call (at most 2^{32 - D} - 1 = "
                         f"{sorted_max_points(D)}: the sorted table gradient numbers its {1 << D} * n_points items in 32 bits)")
    if D == 3:
        nbytes = B.load().nfa_hashgrid_sorted_scratch_bytes(n_points, enc.n_levels, enc.table.log2_hashmap_size)
    else:
        nbytes = B.load().nfa_hashgrid_sorted_scratch_bytes_d(D, n_points, enc.n_levels, enc.table.log2_hashmap_size)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _grad_as(g: Tensor, dtype: torch.dtype) -> Tensor:
    """The incoming gradient as the backward kernels read it: contiguous, 16-byte aligned, in the output's dtype (autograd
    delivers it in that dtype, so a half gradient is handed over as it is, never widened)."""
    return _aligned16(g if g.dtype == dtype else g.to(dtype))


class _HashGridFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, enc: "HashGridEncoding", dtype: torch.dtype):
        B.require_device(x, params)
        N = x.shape[0]
        y = torch.empty(N, enc.n_levels * enc.n_features_per_level, dtype=dtype, device=x.device)
        if N:
            with torch.cuda.device(x.device):
                entry, lead = _entry("nfa_hashgrid_fwd", dtype, enc.interp, enc.n_input_dims)
                B.call(entry, *lead, B.ptr(x), B.ptr(params), *_table_args(enc, N, params), B.ptr(y), B.stream())
        ctx.enc, ctx.dtype = enc, dtype
        ctx.save_for_backward(x, params)
        return y

    @staticmethod
    def backward(ctx, g_y):
        need_x, need_p = ctx.needs_input_grad[:2]
        if g_y is None or not (need_x or need_p):
            return None, None, None, None
        x, params = ctx.saved_tensors
        g_x, g_p = _HashGridBwdFn.apply(x, params, _grad_as(g_y, ctx.dtype), ctx.enc, ctx.dtype, need_x, need_p)
        return g_x, g_p, None, None


class _HashGridBwdFn(torch.autograd.Function):
    """The hash grid's backward as a function ``(x, params, g_y) -> (g_x, g_params)``, so that ``g_x`` can be differentiated
    again (``create_graph=True``: Eikonal terms, normals).  Its own backward is one ``nfa_hashgrid_bwd_bwd[_t|_i]`` call."""

    @staticmethod
    def forward(ctx, x, params, g, enc: "HashGridEncoding", dtype: torch.dtype, need_x: bool, need_p: bool):
        g_p = torch.zeros_like(params) if need_p else None
        g_x = torch.empty_like(x) if need_x else None
        if x.shape[0]:
            with torch.cuda.device(x.device):
                args = (B.ptr(x), B.ptr(params), B.ptr(g), *_table_args(enc, x.shape[0], params), B.ptr(g_p), B.ptr(g_x))
                if enc.deterministic and need_p:
                    scratch = _sorted_scratch(enc, x.shape[0], x.device)
                    entry, lead = _entry("nfa_hashgrid_bwd_sorted", dtype, enc.interp, enc.n_input_dims)
                    B.call(entry, *lead, *args, B.ptr(scratch), scratch.numel(), B.stream())
                else:
                    entry, lead = _entry("nfa_hashgrid_bwd", dtype, enc.interp, enc.n_input_dims)
                    B.call(entry, *lead, *args, B.stream())
        ctx.enc, ctx.dtype = enc, dtype
        ctx.save_for_backward(x, params, g)
        ctx.set_materialize_grads(False)
        return g_x, g_p

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_x, gg_p):
        if ctx.enc.n_input_dims != 3 and gg_x is not None:
            raise NotImplementedError(f"HashGridEncoding: the second order (differentiating dL/dx again) is implemented for 3 "
                                      f"input dimensions only (this grid has {ctx.enc.n_input_dims})")
        if gg_p is not None:
            raise NotImplementedError("HashGridEncoding: the derivative of the table gradient (dL/dparams) is not "
                                      "implemented; only dL/dx can be differentiated again")
        need_x, need_p, need_g = ctx.needs_input_grad[:3]
        if gg_x is None or not (need_x or need_p or need_g):
            return (None,) * 7
        x, params, g = ctx.saved_tensors
        enc = ctx.enc
        v = gg_x.to(torch.float32).contiguous()
        x2 = torch.empty_like(x) if need_x else None
        g2_p = torch.zeros_like(params) if need_p else None
        gg_y = torch.empty_like(g) if need_g else None
        if x.shape[0]:
            with torch.cuda.device(x.device):
                args = (B.ptr(x), B.ptr(params), B.ptr(g), B.ptr(v), *_table_args(enc, x.shape[0], params), B.ptr(gg_y),
                        B.ptr(g2_p), B.ptr(x2))
                if enc.deterministic and need_p:
                    scratch = _sorted_scratch(enc, x.shape[0], x.device)
                    entry, lead = _entry("nfa_hashgrid_bwd_bwd_sorted", ctx.dtype, enc.interp)
                    B.call(entry, *lead, *args, B.ptr(scratch), scratch.numel(), B.stream())
                else:
                    entry, lead = _entry("nfa_hashgrid_bwd_bwd", ctx.dtype, enc.interp)
                    B.call(entry, *lead, *args, B.stream())
        return x2, g2_p, gg_y, None, None, None, None


class _SHFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, degree: int, dtype: torch.dtype):
        B.require_device(dirs)
        N = dirs.shape[0]
        out = torch.empty(N, degree * degree, dtype=dtype, device=dirs.device)
        if N:
            with torch.cuda.device(dirs.device):
                entry, elem = _entry("nfa_sh_fwd", dtype)
                B.call(entry, *elem, B.ptr(dirs), N, degree, B.ptr(out), B.stream())
        ctx.degree, ctx.dtype = degree, dtype
        ctx.save_for_backward(dirs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        if g_out is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (dirs,) = ctx.saved_tensors
        g = _grad_as(g_out, ctx.dtype)
        g_d = torch.empty_like(dirs)
        if dirs.shape[0]:
            with torch.cuda.device(dirs.device):
                entry, elem = _entry("nfa_sh_bwd", ctx.dtype)
                B.call(entry, *elem, B.ptr(dirs), B.ptr(g), dirs.shape[0], ctx.degree, B.ptr(g_d), B.stream())
        return g_d, None, None


def _autocast_off(x: Tensor):
    """(x as the encodings see it, a context that disables autocast): float32 inputs under autocast, like tcnn's
    ``custom_fwd(cast_inputs=torch.float32)``."""
    dt = x.device.type
    if torch.is_autocast_enabled(dt) and x.is_floating_point():
        x = x.float()
    return x, torch.autocast(dt, enabled=False)


class HashGridEncoding(nn.Module):
    """tiny-cuda-nn's ``HashGrid`` encoding with 2-D, 3-D or 4-D input (``n_input_dims`` = D) and linear or smoothstep
    interpolation: ``forward(x[..., D]) -> [..., n_levels * n_features_per_level]``, level-major (output ``l * F + j`` is
    feature ``j`` of level ``l``).

    ``n_input_dims``: 2 (image-space and tri-plane / K-Planes style fields), 3, or 4 ((x, y, z, t) of a dynamic scene).  A
    level has ``min(roundup8(res^D), 2^log2_hashmap_size)`` entries, the cell has ``2^D`` corners, and the hash uses
    tcnn's primes of the first D dimensions (csrc/encoding.hip, "Other dimensions").  For D = 2 and 4 the forward, the
    first-order backward (``dL/dparams`` in both modes, ``dL/dx``), both interpolations and every ``out_dtype`` are native
    kernels; differentiating ``dL/dx`` again (``create_graph=True``) raises ``NotImplementedError`` there: the second
    order is 3-D only (the torch path on CPU tensors is differentiated by autograd to any order).  ``deterministic=True``
    takes at most ``2^(32 - D) - 1`` points per call.  What follows is true of every D unless it says 3-D.

    ``params`` is one flat float32 table of ``sum(sizes) * F`` values laid out ``[level][entry][feature]``, initialised
    uniform in +-1e-4.  ``scales``, ``resolutions``, ``offsets`` and ``sizes`` are the per-level constants
    (:class:`LevelTable`).  Inputs outside [0, 1] are legal (every index wraps into its level); results for non-finite
    inputs are unspecified.  Differentiable w.r.t. ``params`` and ``x``, and twice where the first derivative taken is the
    one w.r.t. ``x``: ``torch.autograd.grad(y, x, g, create_graph=True)`` gives a ``dL/dx`` that can be differentiated
    w.r.t. ``params``, ``x`` and ``g`` (one native pass; what an Eikonal term, analytic normals or any regulariser of the
    field's spatial gradient needs).  With linear interpolation the second derivative w.r.t. ``x`` has mixed partials only;
    with ``interpolation="Smoothstep"`` it has the pure second partials along each axis as well.  ``floor`` contributes
    nothing on either.  Differentiating ``dL/dparams`` again raises ``NotImplementedError``; there is no
    third order.

    ``out_dtype``: ``None`` (float32 output, also under autocast), ``torch.float16`` / ``torch.bfloat16`` (the float32
    result rounded once to nearest even, written by the kernel itself; the gradient arrives and is read in that dtype),
    or ``"autocast"`` (the active autocast dtype of the input's device when that is fp16 or bf16, else float32).

    ``deterministic``: by default the native table gradient (``dL/dparams``, at first and at second order) is scattered
    with float atomics, so its last bits change from run to run.  ``True`` forms it by a stable sort of the (point,
    corner) contributions by table entry and a segmented sum in a fixed order (``nfa_hashgrid_bwd_sorted``,
    ``nfa_hashgrid_bwd_bwd_sorted``; the order is stated in csrc/encoding.hip): the same inputs give the same bits on
    every run, at the price of a scratch tensor per call (at most 512 MiB unless one level alone needs more) and at most
    2^29 - 1 points per call at D = 3, ``2^(32 - D) - 1`` in general (``ValueError`` above).  Every other result is the same on both settings.  The torch path
    (CPU tensors, other dtypes) ignores the flag: its reproducibility is torch's own (``index`` backward, see
    ``torch.use_deterministic_algorithms``).

    ``interpolation``: ``"Linear"`` or ``"Smoothstep"`` (case-insensitive; tcnn's ``"interpolation"``).  Smoothstep forms the
    corner weights from ``S(f) = f^2 (3 - 2 f)`` instead of the cell fraction ``f``: the encoding becomes C^1 (``dL/dx`` is
    continuous, and zero along an axis on that axis' cell faces, so analytic normals are not faceted) and its second
    derivative gains the curvature along each axis.  All three native passes, both table-gradient modes and every
    ``out_dtype`` take it; parameters, ``state_dict``, the level table and the initialisation do not depend on it.
    tcnn's ``"Nearest"`` is not provided.
    """

    def __init__(self, n_input_dims: int = 3, n_levels: int = 16, n_features_per_level: int = 2,
                 log2_hashmap_size: int = 19, base_resolution: float = 16, per_level_scale: float = 2.0, out_dtype=None,
                 deterministic: bool = False, interpolation: str = "Linear"):
        super().__init__()
        self.out_dtype = _check_out_dtype(out_dtype)
        self.deterministic = bool(deterministic)
        names = {k.lower(): k for k in B.INTERP_CODES}
        if not isinstance(interpolation, str) or interpolation.lower() not in names:
            raise ValueError(f"HashGridEncoding: interpolation must be 'Linear' or 'Smoothstep' (got {interpolation!r})")
        self.interpolation = names[interpolation.lower()]
        self.interp = B.INTERP_CODES[self.interpolation]   # NFA_INTERP_*
        if n_input_dims not in GRID_DIMS:
            raise ValueError(f"HashGridEncoding: n_input_dims must be 2, 3 or 4 (got {n_input_dims})")
        if n_features_per_level not in (1, 2, 4, 8):
            raise ValueError(f"HashGridEncoding: n_features_per_level must be 1, 2, 4 or 8 (got {n_features_per_level})")
        if not 1 <= n_levels <= 32:
            raise ValueError(f"HashGridEncoding: n_levels must be in 1..32 (got {n_levels})")
        if not 10 <= log2_hashmap_size <= 24:
            raise ValueError(f"HashGridEncoding: log2_hashmap_size must be in 10..24 (got {log2_hashmap_size})")
        if not (base_resolution >= 1 and per_level_scale >= 1):
            raise ValueError("HashGridEncoding: base_resolution and per_level_scale must be >= 1")
        self.n_input_dims = int(n_input_dims)
        self.n_levels, self.n_features_per_level = int(n_levels), int(n_features_per_level)
        self.log2_hashmap_size = int(log2_hashmap_size)
        self.base_resolution, self.per_level_scale = base_resolution, float(per_level_scale)
        self.n_output_dims = self.n_levels * self.n_features_per_level
        self.table = LevelTable(n_levels, log2_hashmap_size, base_resolution, per_level_scale, self.n_input_dims)
        n_params = self.table.n_entries * self.n_features_per_level
        if n_params >= 1 << 31:
            raise ValueError(f"HashGridEncoding: {n_params} parameters (at most 2^31 - 1)")
        self.params = nn.Parameter(torch.empty(n_params, dtype=torch.float32).uniform_(-1e-4, 1e-4))

    scales = property(lambda self: list(self.table.scales))
    resolutions = property(lambda self: list(self.table.resolutions))
    offsets = property(lambda self: list(self.table.offsets))
    sizes = property(lambda self: list(self.table.sizes))

    def forward(self, x: Tensor) -> Tensor:
        D = self.n_input_dims
        assert x.shape[-1] == D, f"HashGridEncoding: x must have shape (..., {D})"
        out = _resolve_out_dtype(self.out_dtype, x)
        x, ctx = _autocast_off(x)
        with ctx:
            lead = x.shape[:-1]
            x2 = x.reshape(-1, D)
            p = self.params
            if x2.is_cuda and x2.dtype == torch.float32 and p.dtype == torch.float32 and p.device == x2.device:
                # (2-D and 4-D points are moved as one 8- or 16-byte vector: 16-byte aligned)
                y = _HashGridFn.apply(x2.contiguous() if D == 3 else _aligned16(x2), p, self, out)
            else:
                dt = torch.promote_types(x2.dtype, p.dtype)
                y = _hashgrid_torch(x2.to(dt), p.to(dt), self.table, self.n_features_per_level, self.interp)
                if self.out_dtype is not None:
                    y = y.to(out)
            return y.view(*lead, self.n_output_dims)

    def extra_repr(self) -> str:
        return ((f"n_input_dims={self.n_input_dims}, " if self.n_input_dims != 3 else "")
                + f"n_levels={self.n_levels}, n_features_per_level={self.n_features_per_level}, "
                f"log2_hashmap_size={self.log2_hashmap_size}, base_resolution={self.base_resolution}, "
                f"per_level_scale={self.per_level_scale}") + ((f", out_dtype={self.out_dtype}" if self.out_dtype is not None else "")
                + (", deterministic=True" if self.deterministic else "")
                + (f", interpolation={self.interpolation}" if self.interp else ""))


# Instant-NGP's real spherical-harmonics basis (tcnn's constants)
_SH = dict(c0=0.28209479177387814, c1=0.48860251190291987, c2a=1.0925484305920792, c2b=0.94617469575755997,
           c2c=0.31539156525251999, c2d=0.54627421529603959, c3a=0.59004358992664352, c3b=2.8906114426405538,
           c3c=0.45704579946446572, c3d=0.3731763325901154, c3e=1.4453057213202769)


def _sh_torch(d: Tensor, degree: int) -> Tensor:
    u = 2.0 * d - 1.0
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    k = _SH
    out = [torch.full_like(x, k["c0"])]
    if degree > 1:
        out += [-k["c1"] * y, k["c1"] * z, -k["c1"] * x]
    if degree > 2:
        x2, y2, z2 = x * x, y * y, z * z
        out += [k["c2a"] * x * y, -k["c2a"] * y * z, k["c2b"] * z2 - k["c2c"], -k["c2a"] * x * z, k["c2d"] * (x2 - y2)]
        if degree > 3:
            out += [k["c3a"] * y * (-3.0 * x2 + y2), k["c3b"] * x * y * z, k["c3c"] * y * (1.0 - 5.0 * z2),
                    k["c3d"] * z * (5.0 * z2 - 3.0), k["c3c"] * x * (1.0 - 5.0 * z2), k["c3e"] * z * (x2 - y2),
                    k["c3a"] * x * (-x2 + 3.0 * y2)]
    return torch.stack(out, -1)


class SphericalHarmonicsEncoding(nn.Module):
    """tiny-cuda-nn's ``SphericalHarmonics`` encoding: directions in [0, 1]^3 (``u = 2 d - 1``, not renormalised), ``degree``
    1..4, ``forward(d[..., 3]) -> [..., degree^2]``.  Differentiable w.r.t. the directions.  ``out_dtype`` as for
    :class:`HashGridEncoding`."""

    def __init__(self, n_input_dims: int = 3, degree: int = 4, out_dtype=None):
        super().__init__()
        self.out_dtype = _check_out_dtype(out_dtype)
        if n_input_dims != 3:
            raise ValueError(f"SphericalHarmonicsEncoding: only 3 input dimensions are supported (got {n_input_dims})")
        if not 1 <= degree <= 4:
            raise ValueError(f"SphericalHarmonicsEncoding: degree must be in 1..4 (got {degree})")
        self.n_input_dims, self.degree = 3, int(degree)
        self.n_output_dims = self.degree * self.degree

    def forward(self, d: Tensor) -> Tensor:
        assert d.shape[-1] == 3, "SphericalHarmonicsEncoding: directions must have shape (..., 3)"
        out = _resolve_out_dtype(self.out_dtype, d)
        d, ctx = _autocast_off(d)
        with ctx:
            lead = d.shape[:-1]
            d2 = d.reshape(-1, 3)
            if d2.is_cuda and d2.dtype == torch.float32:
                y = _SHFn.apply(d2.contiguous(), self.degree, out)
            else:
                y = _sh_torch(d2, self.degree)
                if self.out_dtype is not None:
                    y = y.to(out)
            return y.view(*lead, self.n_output_dims)

    def extra_repr(self) -> str:
        return f"degree={self.degree}" + (f", out_dtype={self.out_dtype}" if self.out_dtype is not None else "")


PLANE_DIMS = (3, 4)   # input dimensions of the native plane grid


class PlaneTable:
    """The planes of a plane grid, computed once on the host: ``planes`` (the axis pairs ``(a, b)``, ``a < b``, in
    ``itertools.combinations`` order), ``res[s][d] = R_d * m_s`` for the spatial axes ``d < 3`` and ``R_3`` for the time
    axis, and, per scale ``s`` and plane ``k``, ``offsets[s][k]`` / ``sizes[s][k]`` in floats: plane ``(s, k)`` is the
    row-major ``[R_b, R_a, F]`` block at ``offsets[s][k]``, the blocks in scale-major, then plane order without gaps."""

    def __init__(self, n_dims: int, resolution, multiscale_res, n_features: int):
        D = self.n_dims = int(n_dims)
        self.n_features = int(n_features)
        self.planes = list(itertools.combinations(range(D), 2))
        self.res = [[int(resolution[d]) * int(m) if d < 3 else int(resolution[d]) for d in range(D)] for m in multiscale_res]
        self.offsets, self.sizes, offset = [], [], 0
        for r in self.res:
            self.sizes.append([r[a] * r[b] * self.n_features for a, b in self.planes])
            self.offsets.append([offset + sum(self.sizes[-1][:k]) for k in range(len(self.planes))])
            offset += sum(self.sizes[-1])
        self.n_params = offset
        # host array handed to nfa_planegrid_{fwd,bwd} (read synchronously by each call)
        flat = [min(v, (1 << 31) - 1) for r in self.res for v in r]
        self.c_res = (ctypes.c_int32 * len(flat))(*flat)


def _locate_nodes(p: Tensor, R: int):
    """axis.h's locate_pos for node coordinates ``p`` among ``R`` nodes: (i, f), i int64 in [0, R - 2], f in [0, 1]."""
    rm1 = float(R - 1)
    q = torch.where(p >= 0, p, torch.zeros_like(p))        # (NaN gives 0: `where`, not `maximum`)
    q = torch.where(q <= rm1, q, torch.full_like(q, rm1))
    i = torch.floor(q.detach()).to(torch.int64).clamp(max=R - 2)
    return i, q - i.to(q.dtype)


def _plane_value(plane: Tensor, Ra: int, ia, fa, ib, fb) -> Tensor:
    """axis.h's plane_value, the 4-tap sum of csrc/planes.hip and csrc/vmgrid.hip, on a ``[R_b * R_a, C]`` plane: corner
    order, from 0."""
    row = ib * Ra + ia
    v = torch.zeros(ia.shape[0], plane.shape[1], dtype=plane.dtype, device=plane.device)
    for k in range(4):
        ka, kb = k & 1, k >> 1
        w = (fa if ka else 1.0 - fa) * (fb if kb else 1.0 - fb)
        v = v + w[:, None] * plane[row + (kb * Ra + ka)]
    return v


def _planegrid_torch(x: Tensor, params: Tensor, t: PlaneTable, reduce: int = 0) -> Tensor:
    """The plane grid in torch, op for op as csrc/planes.hip computes it (x [N, D], D = ``t.n_dims``, and params in one
    float dtype); ``reduce``: a ``B.PLANE_REDUCE_CODES`` value."""
    F = t.n_features
    outs = []
    for s, res in enumerate(t.res):
        cell = [_locate_nodes(x[:, d] * float(res[d] - 1), res[d]) for d in range(t.n_dims)]
        out = None
        for k, (a, b) in enumerate(t.planes):
            plane = params[t.offsets[s][k]: t.offsets[s][k] + t.sizes[s][k]].view(-1, F)
            v = _plane_value(plane, res[a], *cell[a], *cell[b])
            out = v if out is None else (out + v if reduce else out * v)
        outs.append(out)
    return torch.cat(outs, -1)


class _GridFn(torch.autograd.Function):
    """The native pass of a :class:`PlaneGridEncoding` or a :class:`VMGridEncoding`: ``enc._entries`` names its forward
    and backward entry, ``enc._lead`` / ``enc._table_args`` give their arguments around the pointers."""

    @staticmethod
    def forward(ctx, x, params, enc, dtype: torch.dtype):
        B.require_device(x, params)
        N = x.shape[0]
        y = torch.empty(N, enc.n_output_dims, dtype=dtype, device=x.device)
        if N:
            with torch.cuda.device(x.device):
                B.call(enc._entries[0], *enc._lead(dtype), B.ptr(x), B.ptr(params), *enc._table_args(N), B.ptr(y), B.stream())
        ctx.enc, ctx.dtype = enc, dtype
        ctx.save_for_backward(x, params)
        return y

    @staticmethod
    def backward(ctx, g_y):
        need_x, need_p = ctx.needs_input_grad[:2]
        if g_y is None or not (need_x or need_p):
            return None, None, None, None
        x, params = ctx.saved_tensors
        g_x, g_p = _GridBwdFn.apply(x, params, _grad_as(g_y, ctx.dtype), ctx.enc, ctx.dtype, need_x, need_p)
        return g_x, g_p, None, None


class _GridBwdFn(torch.autograd.Function):
    """The grid's backward as a function ``(x, params, g_y) -> (g_x, g_params)`` of its own, so that differentiating it
    again (``create_graph=True``) fails with a message that names the encoding instead of a missing ``grad_fn``."""

    @staticmethod
    def forward(ctx, x, params, g, enc, dtype: torch.dtype, need_x: bool, need_p: bool):
        g_p = torch.zeros_like(params) if need_p else None
        g_x = torch.empty_like(x) if need_x else None
        if x.shape[0]:
            with torch.cuda.device(x.device):
                B.call(enc._entries[1], *enc._lead(dtype), B.ptr(x), B.ptr(params), B.ptr(g), *enc._table_args(x.shape[0]),
                       B.ptr(g_p), B.ptr(g_x), B.stream())
        ctx.enc = enc
        ctx.set_materialize_grads(False)
        return g_x, g_p

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_x, gg_p):
        raise NotImplementedError(f"{type(ctx.enc).__name__}: the second order (differentiating dL/dx or dL/dparams again) is "
                                  "not implemented on the native path; the torch path on CPU tensors is differentiated by "
                                  "autograd")


class PlaneGridEncoding(nn.Module):
    """The plane-factorised multiscale encoding of K-Planes (Fridovich-Keil et al. 2023): its ``interpolate_ms_features``
    with ``concat_features=True`` as one native pass each way (csrc/planes.hip).  ``forward(x[..., D]) -> [..., S * F]`` for
    ``x`` in [0, 1]^D (K-Planes' ``u`` in [-1, 1] is ``x = (u + 1) / 2``), scale ``s`` at columns ``s F .. s F + F - 1``.

    ``n_input_dims`` D: 3 (a static scene: 3 planes per scale) or 4 ((x, y, z, t): 6 planes).  The planes are the axis
    pairs ``(a, b)``, ``a < b``, in ``itertools.combinations(range(D), 2)`` order.  ``resolution`` ``(R_0, .., R_{D-1})``
    and ``multiscale_res`` ``(m_0, .., m_{S-1})`` (S in 1..8): scale ``s`` has ``R_d m_s`` nodes along a spatial axis and
    ``R_3`` along the time axis, every one at least 2.  ``n_features`` F: 4, 8, 16 or 32 per plane.

    ``params`` is one flat float32 table (fewer than 2^31 values): plane ``(s, k)`` is the row-major ``[R_b, R_a, F]`` block
    at ``offsets[s][k]``, scale-major, then plane order; ``plane(s, k)`` is that view and ``plane(s, k).permute(2, 0, 1)[None]``
    the ``[1, F, H, W]`` tensor K-Planes hands to ``grid_sample``.  A plane is sampled as ``F.grid_sample(mode="bilinear",
    padding_mode="border", align_corners=True)`` samples it; ``reduce`` is ``"product"`` (K-Planes) or ``"sum"``
    (EG3D-style tri-planes) over the planes of a scale.  Initialised as K-Planes: uniform in ``init = (0.1, 0.5)``, planes
    that contain the time axis ones when ``reduce="product"``.

    Every input is legal: a coordinate outside [0, 1] samples the border, NaN samples node 0, and ``dL/dx`` is zero on such
    an axis.  Differentiable once w.r.t. ``params`` (float atomics: the last bits change from run to run) and ``x`` (bitwise
    reproducible); the torch path (CPU tensors, other dtypes) is differentiated by autograd.  On a grid node the native
    ``dL/dx`` is the derivative towards the upper cell (the lower one at x = 1).  ``out_dtype`` as for
    :class:`HashGridEncoding`."""

    def __init__(self, n_input_dims: int, resolution, multiscale_res=(1,), n_features: int = 32, reduce: str = "product",
                 init=(0.1, 0.5), out_dtype=None):
        super().__init__()
        self.out_dtype = _check_out_dtype(out_dtype)
        if n_input_dims not in PLANE_DIMS:
            raise ValueError(f"PlaneGridEncoding: n_input_dims must be 3 or 4 (got {n_input_dims})")
        if n_features not in (4, 8, 16, 32):
            raise ValueError(f"PlaneGridEncoding: n_features must be 4, 8, 16 or 32 (got {n_features})")
        if reduce not in B.PLANE_REDUCE_CODES:
            raise ValueError(f"PlaneGridEncoding: reduce must be 'product' or 'sum' (got {reduce!r})")
        resolution, multiscale_res = tuple(int(r) for r in resolution), tuple(int(m) for m in multiscale_res)
        if len(resolution) != n_input_dims:
            raise ValueError(f"PlaneGridEncoding: resolution must have {n_input_dims} entries (got {len(resolution)})")
        if not 1 <= len(multiscale_res) <= 8:
            raise ValueError(f"PlaneGridEncoding: multiscale_res must have 1..8 entries (got {len(multiscale_res)})")
        self.n_input_dims, self.n_features, self.reduce = int(n_input_dims), int(n_features), reduce
        self.resolution, self.multiscale_res = resolution, multiscale_res
        self.table = PlaneTable(n_input_dims, resolution, multiscale_res, n_features)
        for s, r in enumerate(self.table.res):
            if min(r) < 2:
                raise ValueError(f"PlaneGridEncoding: every resolution must be at least 2 (scale {s} has {tuple(r)})")
        if self.table.n_params >= 1 << 31:
            raise ValueError(f"PlaneGridEncoding: {self.table.n_params} parameters (at most 2^31 - 1)")
        self.n_scales = len(multiscale_res)
        self.n_output_dims = self.n_scales * self.n_features
        self.init = (float(init[0]), float(init[1]))
        self.params = nn.Parameter(torch.empty(self.table.n_params, dtype=torch.float32).uniform_(*self.init))
        if reduce == "product":
            with torch.no_grad():
                for s in range(self.n_scales):
                    for k, (a, b) in enumerate(self.table.planes):
                        if b == 3:
                            self.plane(s, k).fill_(1.0)

    planes = property(lambda self: list(self.table.planes))
    resolutions = property(lambda self: [list(r) for r in self.table.res])
    offsets = property(lambda self: [list(o) for o in self.table.offsets])
    sizes = property(lambda self: [list(z) for z in self.table.sizes])

    _entries = ("nfa_planegrid_fwd", "nfa_planegrid_bwd")

    def plane(self, s: int, k: int) -> Tensor:
        """Plane ``k`` of scale ``s`` as a ``[R_b, R_a, F]`` view of ``params``."""
        t = self.table
        a, b = t.planes[k]
        return self.params[t.offsets[s][k]: t.offsets[s][k] + t.sizes[s][k]].view(t.res[s][b], t.res[s][a], self.n_features)

    def _lead(self, dtype: torch.dtype):
        return self.n_input_dims, B.PLANE_REDUCE_CODES[self.reduce], B.ELEM_CODES[dtype]

    def _table_args(self, n_points: int):
        return n_points, self.n_scales, self.n_features, self.table.c_res

    def forward(self, x: Tensor) -> Tensor:
        D = self.n_input_dims
        assert x.shape[-1] == D, f"PlaneGridEncoding: x must have shape (..., {D})"
        out = _resolve_out_dtype(self.out_dtype, x)
        x, ctx = _autocast_off(x)
        with ctx:
            lead = x.shape[:-1]
            x2 = x.reshape(-1, D)
            p = self.params
            if x2.is_cuda and x2.dtype == torch.float32 and p.dtype == torch.float32 and p.device == x2.device:
                y = _GridFn.apply(x2.contiguous(), p, self, out)   # (element-wise access: no alignment beyond 4 bytes)
            else:
                dt = torch.promote_types(x2.dtype, p.dtype)
                y = _planegrid_torch(x2.to(dt), p.to(dt), self.table, B.PLANE_REDUCE_CODES[self.reduce])
                if self.out_dtype is not None:
                    y = y.to(out)
            return y.view(*lead, self.n_output_dims)

    def extra_repr(self) -> str:
        return (f"n_input_dims={self.n_input_dims}, resolution={self.resolution}, multiscale_res={self.multiscale_res}, "
                f"n_features={self.n_features}, reduce={self.reduce!r}"
                + (f", init={self.init}" if self.init != (0.1, 0.5) else "")
                + (f", out_dtype={self.out_dtype}" if self.out_dtype is not None else ""))


VM_MODES = ((0, 1, 2), (0, 2, 1), (1, 2, 0))   # (a, b, c) per mode: TensoRF's matMode (plane axes) and vecMode (line axis)


def _vm_lanes(n_components: int) -> int:
    """The lane-group width of csrc/vmgrid.hip: the largest power of two <= 32 that divides C."""
    return next(w for w in (32, 16, 8, 4) if n_components % w == 0)


class VMTable:
    """The blocks of a VM grid, computed once on the host: per mode ``m`` with axes ``(a, b, c) = VM_MODES[m]`` the plane,
    a row-major ``[R_b, R_a, C]`` block at ``plane_offsets[m]``, then the line, a ``[R_c, C]`` block at ``line_offsets[m]``,
    the modes in order without gaps (sizes in floats)."""

    def __init__(self, resolution, n_components: int):
        self.res = [int(r) for r in resolution]
        C = self.n_components = int(n_components)
        self.plane_offsets, self.plane_sizes, self.line_offsets, self.line_sizes, offset = [], [], [], [], 0
        for a, b, c in VM_MODES:
            self.plane_offsets.append(offset)
            self.plane_sizes.append(self.res[a] * self.res[b] * C)
            offset += self.plane_sizes[-1]
            self.line_offsets.append(offset)
            self.line_sizes.append(self.res[c] * C)
            offset += self.line_sizes[-1]
        self.n_params = offset
        # host array handed to nfa_vmgrid_{fwd,bwd,resample} (read synchronously by each call)
        self.c_res = (ctypes.c_int32 * 3)(*[min(r, (1 << 31) - 1) for r in self.res])

    def plane(self, params: Tensor, m: int) -> Tensor:
        a, b, _ = VM_MODES[m]
        o = self.plane_offsets[m]
        return params[o: o + self.plane_sizes[m]].view(self.res[b], self.res[a], self.n_components)

    def line(self, params: Tensor, m: int) -> Tensor:
        o = self.line_offsets[m]
        return params[o: o + self.line_sizes[m]].view(self.res[VM_MODES[m][2]], self.n_components)


def _vm_line_value(line: Tensor, ic, fc) -> Tensor:
    """``(0 + (1 - f) L[i]) + f L[i + 1]`` on a ``[R_c, C]`` line."""
    v = torch.zeros(ic.shape[0], line.shape[1], dtype=line.dtype, device=line.device)
    v = v + (1.0 - fc)[:, None] * line[ic]
    return v + fc[:, None] * line[ic + 1]


def _vmgrid_torch(x: Tensor, params: Tensor, t: VMTable, reduce: int = 0) -> Tensor:
    """The VM grid in torch, op for op as csrc/vmgrid.hip computes it, the lane sums and the xor butterfly of ``"sum"``
    included (x [N, 3] and params in one float dtype); ``reduce``: a ``B.VM_REDUCE_CODES`` value."""
    C = t.n_components
    cell = [_locate_nodes(x[:, d] * float(t.res[d] - 1), t.res[d]) for d in range(3)]
    terms = []
    for m, (a, b, c) in enumerate(VM_MODES):
        pv = _plane_value(t.plane(params, m).view(-1, C), t.res[a], *cell[a], *cell[b])
        terms.append(pv * _vm_line_value(t.line(params, m), *cell[c]))
    if not reduce:
        return torch.cat(terms, -1)
    L = _vm_lanes(C)
    lanes = torch.zeros(x.shape[0], L, dtype=x.dtype, device=x.device)
    for term in terms:
        for r in range(C // L):
            lanes = lanes + term[:, r * L: (r + 1) * L]
    lane = torch.arange(L, device=x.device)
    off = L // 2
    while off:
        lanes = lanes + lanes[:, lane ^ off]
        off //= 2
    return lanes[:, :1]


def _vm_resample_torch(params: Tensor, src: VMTable, dst: VMTable) -> Tensor:
    """``nfa_vmgrid_resample`` in torch, op for op (TensoRF's ``up_sampling_VM``): the table of ``dst`` whose every node is
    the sample of ``src``'s block at ``i' * ((R - 1) / (R' - 1))`` per axis, the quotient and the product in params' dtype."""
    C, dt, dev = src.n_components, params.dtype, params.device

    def nodes(d):
        scale = torch.tensor(src.res[d] - 1, dtype=dt) / torch.tensor(dst.res[d] - 1, dtype=dt)
        return _locate_nodes(torch.arange(dst.res[d], dtype=dt, device=dev) * scale.to(dev), src.res[d])

    cell = [nodes(d) for d in range(3)]
    out = []
    for m, (a, b, c) in enumerate(VM_MODES):
        ia, fa = (v.repeat(dst.res[b]) for v in cell[a])               # node (i'_b, i'_a), row-major: a runs fastest
        ib, fb = (v.repeat_interleave(dst.res[a]) for v in cell[b])
        out.append(_plane_value(src.plane(params, m).view(-1, C), src.res[a], ia, fa, ib, fb).reshape(-1))
        out.append(_vm_line_value(src.line(params, m), *cell[c]).reshape(-1))
    return torch.cat(out)


class VMGridEncoding(nn.Module):
    """The vector-matrix (VM) decomposition of TensoRF (Chen et al. 2022), ``TensorVMSplit``'s feature grids, as one native
    pass each way (csrc/vmgrid.hip).  ``forward(x[..., 3])`` for ``x`` in [0, 1]^3 (TensoRF's ``u`` in [-1, 1] is
    ``x = (u + 1) / 2``) gives ``[..., 3 C]`` with ``reduce="concat"`` (mode ``m`` at columns ``m C .. m C + C - 1``:
    ``compute_appfeature`` before ``basis_mat``) or ``[..., 1]`` with ``reduce="sum"`` (``compute_densityfeature``).

    Mode ``m`` has the axes ``(a, b, c) = VM_MODES[m]``: the plane over ``matMode = (0,1) (0,2) (1,2)``, the line along
    ``vecMode = 2, 1, 0``.  ``resolution`` ``(R_0, R_1, R_2)``, every one at least 2; ``n_components`` C per mode, a multiple
    of 4 in 4..96 (TensoRF: 16 for the density, 48 for the appearance).

    ``params`` is one flat float32 table (fewer than 2^31 values): per mode the plane, then the line, without gaps
    (``offsets`` / ``sizes``: ``[[plane, line]]`` per mode, in floats).  ``plane(m)`` is the ``[R_b, R_a, C]`` view and
    ``plane(m).permute(2, 0, 1)[None]`` the ``[1, C, H, W]`` tensor TensoRF keeps in ``density_plane[m]`` / ``app_plane[m]``;
    ``line(m)`` is the ``[R_c, C]`` view and ``line(m).t()[None, :, :, None]`` TensoRF's ``[1, C, R, 1]`` line.  Both are
    sampled as ``F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True)`` samples them (TensoRF pads
    with zeros, which differs outside the box only) and multiplied.  Initialised as TensoRF: ``init_scale * randn``.

    Every input is legal: a coordinate outside [0, 1] samples the border, NaN samples node 0, and ``dL/dx`` is zero on such
    an axis.  Differentiable once w.r.t. ``params`` (float atomics: the last bits change from run to run) and ``x`` (bitwise
    reproducible); the torch path (CPU tensors, other dtypes) is differentiated by autograd.  ``out_dtype`` as for
    :class:`HashGridEncoding`.  ``resampled(resolution)`` is TensoRF's ``up_sampling_VM``."""

    def __init__(self, resolution, n_components: int = 16, reduce: str = "concat", init_scale: float = 0.1, out_dtype=None):
        super().__init__()
        self._configure(resolution, n_components, reduce, init_scale, out_dtype)
        self.params = nn.Parameter(torch.randn(self.table.n_params, dtype=torch.float32) * self.init_scale)

    def _configure(self, resolution, n_components, reduce, init_scale, out_dtype):
        """The checks and everything of the module but ``params`` (``resampled`` fills those itself)."""
        self.out_dtype = _check_out_dtype(out_dtype)
        if not (isinstance(n_components, int) and 4 <= n_components <= 96 and n_components % 4 == 0):
            raise ValueError(f"VMGridEncoding: n_components must be a multiple of 4 in 4..96 (got {n_components})")
        if reduce not in B.VM_REDUCE_CODES:
            raise ValueError(f"VMGridEncoding: reduce must be 'concat' or 'sum' (got {reduce!r})")
        resolution = tuple(int(r) for r in resolution)
        if len(resolution) != 3:
            raise ValueError(f"VMGridEncoding: resolution must have 3 entries (got {len(resolution)})")
        if min(resolution) < 2:
            raise ValueError(f"VMGridEncoding: every resolution must be at least 2 (got {resolution})")
        self.n_input_dims, self.n_components, self.reduce, self.resolution = 3, n_components, reduce, resolution
        self.table = VMTable(resolution, n_components)
        if self.table.n_params >= 1 << 31:
            raise ValueError(f"VMGridEncoding: {self.table.n_params} parameters (at most 2^31 - 1)")
        self.n_output_dims = 3 * n_components if reduce == "concat" else 1
        self.init_scale = float(init_scale)

    modes = property(lambda self: list(VM_MODES))
    offsets = property(lambda self: [[p, l] for p, l in zip(self.table.plane_offsets, self.table.line_offsets)])
    sizes = property(lambda self: [[p, l] for p, l in zip(self.table.plane_sizes, self.table.line_sizes)])

    _entries = ("nfa_vmgrid_fwd", "nfa_vmgrid_bwd")

    def plane(self, m: int) -> Tensor:
        """The plane of mode ``m`` as a ``[R_b, R_a, C]`` view of ``params``."""
        return self.table.plane(self.params, m)

    def line(self, m: int) -> Tensor:
        """The line of mode ``m`` as a ``[R_c, C]`` view of ``params``."""
        return self.table.line(self.params, m)

    def _lead(self, dtype: torch.dtype):
        return B.VM_REDUCE_CODES[self.reduce], B.ELEM_CODES[dtype]

    def _table_args(self, n_points: int):
        return n_points, self.n_components, self.table.c_res

    def forward(self, x: Tensor) -> Tensor:
        assert x.shape[-1] == 3, "VMGridEncoding: x must have shape (..., 3)"
        out = _resolve_out_dtype(self.out_dtype, x)
        x, ctx = _autocast_off(x)
        with ctx:
            lead = x.shape[:-1]
            x2 = x.reshape(-1, 3)
            p = self.params
            if x2.is_cuda and x2.dtype == torch.float32 and p.dtype == torch.float32 and p.device == x2.device:
                y = _GridFn.apply(x2.contiguous(), p, self, out)   # (element-wise access: no alignment beyond 4 bytes)
            else:
                dt = torch.promote_types(x2.dtype, p.dtype)
                y = _vmgrid_torch(x2.to(dt), p.to(dt), self.table, B.VM_REDUCE_CODES[self.reduce])
                if self.out_dtype is not None:
                    y = y.to(out)
            return y.view(*lead, self.n_output_dims)

    @torch.no_grad()
    def resampled(self, resolution) -> "VMGridEncoding":
        """A new module on the same device whose planes and lines are these resampled to ``resolution`` (each axis up, down
        or unchanged): ``F.interpolate(mode="bilinear", align_corners=True)`` of every block, TensoRF's ``up_sampling_VM``.
        The same resolution copies the table bit for bit (finite values).  Optimiser state does not follow: build a new
        optimiser, as TensoRF does."""
        new = VMGridEncoding.__new__(VMGridEncoding)   # (no random table is drawn for a module that gets this one's samples)
        nn.Module.__init__(new)
        new._configure(resolution, self.n_components, self.reduce, self.init_scale, self.out_dtype)
        p = self.params.detach()
        if p.is_cuda and p.dtype == torch.float32:
            q = torch.empty(new.table.n_params, dtype=torch.float32, device=p.device)
            with torch.cuda.device(p.device):
                B.call("nfa_vmgrid_resample", B.ptr(p), self.table.c_res, B.ptr(q), new.table.c_res, self.n_components, B.stream())
        else:
            q = _vm_resample_torch(p, self.table, new.table)
        new.params = nn.Parameter(q, requires_grad=self.params.requires_grad)
        return new

    def extra_repr(self) -> str:
        return (f"resolution={self.resolution}, n_components={self.n_components}, reduce={self.reduce!r}"
                + (f", init_scale={self.init_scale}" if self.init_scale != 0.1 else "")
                + (f", out_dtype={self.out_dtype}" if self.out_dtype is not None else ""))


VOXEL_MAX_STRIDES = 4


class VoxelTable:
    """The shape of a dense voxel grid, computed once on the host: ``res`` ``(R_x, R_y, R_z)``, ``n_features`` C, ``strides``
    and, per stride ``s``, ``nodes[k][d] = ceil(R_d / s)``; the table is one row-major ``[R_z, R_y, R_x, C]`` block."""

    def __init__(self, resolution, n_features: int, strides=(1,)):
        self.res = [int(r) for r in resolution]
        self.n_features = int(n_features)
        self.strides = [int(s) for s in strides]
        self.nodes = [[-(-r // s) for r in self.res] for s in self.strides]
        self.n_params = self.res[0] * self.res[1] * self.res[2] * self.n_features
        # host arrays handed to nfa_voxgrid_{fwd,bwd,resample} (read synchronously by each call)
        self.c_res = (ctypes.c_int32 * 3)(*[min(r, (1 << 31) - 1) for r in self.res])
        self.c_strides = (ctypes.c_int32 * len(self.strides))(*self.strides)


def _volume_value(table: Tensor, Rx: int, Ry: int, s: int, cx, cy, cz) -> Tensor:
    """axis.h's volume_value, the 8-tap sum of csrc/voxgrid.hip, on a ``[R_z * R_y * R_x, C]`` table whose sampled nodes are
    ``s`` apart: ``c* = (i, f)`` per axis, corners ``k = k_x + 2 k_y + 4 k_z`` in order, from 0, weights ``(w_x w_y) w_z``."""
    (ix, fx), (iy, fy), (iz, fz) = cx, cy, cz
    row = ((iz * s) * Ry + iy * s) * Rx + ix * s
    v = torch.zeros(ix.shape[0], table.shape[1], dtype=table.dtype, device=table.device)
    for k in range(8):
        kx, ky, kz = k & 1, (k >> 1) & 1, k >> 2
        w = ((fx if kx else 1.0 - fx) * (fy if ky else 1.0 - fy)) * (fz if kz else 1.0 - fz)
        v = v + w[:, None] * table[row + ((kz * s * Ry + ky * s) * Rx + kx * s)]
    return v


def _voxgrid_torch(x: Tensor, params: Tensor, t: VoxelTable) -> Tensor:
    """The voxel grid in torch, op for op as csrc/voxgrid.hip computes it (x [N, 3] and params in one float dtype), with int64
    gathers."""
    table = params.view(-1, t.n_features)
    outs = []
    for s, n in zip(t.strides, t.nodes):
        cell = [_locate_nodes(x[:, d] * float(n[d] - 1), n[d]) for d in range(3)]
        outs.append(_volume_value(table, t.res[0], t.res[1], s, *cell))
    return torch.cat(outs, -1)


def _voxel_resample_torch(params: Tensor, src: VoxelTable, dst: VoxelTable) -> Tensor:
    """``nfa_voxgrid_resample`` in torch, op for op (DVGO's ``scale_volume_grid``): the table of ``dst`` whose every node is
    the sample of ``src``'s table at ``i' * ((R - 1) / (R' - 1))`` per axis, the quotient and the product in params' dtype."""
    dt, dev = params.dtype, params.device

    def nodes(d):
        scale = torch.tensor(src.res[d] - 1, dtype=dt) / torch.tensor(dst.res[d] - 1, dtype=dt)
        return _locate_nodes(torch.arange(dst.res[d], dtype=dt, device=dev) * scale.to(dev), src.res[d])

    Wx, Wy, Wz = dst.res
    cx = tuple(v.repeat(Wy * Wz) for v in nodes(0))                          # node (i'_z, i'_y, i'_x), row-major: x runs fastest
    cy = tuple(v.repeat_interleave(Wx).repeat(Wz) for v in nodes(1))
    cz = tuple(v.repeat_interleave(Wx * Wy) for v in nodes(2))
    return _volume_value(params.view(-1, src.n_features), src.res[0], src.res[1], 1, cx, cy, cz).reshape(-1)


class VoxelGridEncoding(nn.Module):
    """A dense 3-D feature grid sampled trilinearly, as one native pass each way (csrc/voxgrid.hip): DVGO's density grid
    (``n_features=1``) and ``k0`` feature grid (12), TiNeuVox's feature volume with its multi-distance interpolation
    (``strides=(1, 2, 4)`` is ``mult_dist_interp``), ReLU-Fields-style grids.  ``forward(x[..., 3])`` for ``x`` in [0, 1]^3
    (DVGO's and TiNeuVox's ``u`` in [-1, 1] is ``x = (u + 1) / 2``) gives ``[..., C * len(strides)]``, the k-th stride at the
    columns ``k C .. k C + C - 1``.

    ``resolution`` ``(R_x, R_y, R_z)``, every one at least 2; ``n_features`` C: 1, 2 or a multiple of 4 up to 64.  ``strides``:
    at most 4, each in 1..8.  Stride ``s`` has its nodes at the table indices ``0, s, 2s, ..`` per axis, ``ceil(R / s)`` of them
    (at least 2 on every axis), the last one at ``s (ceil(R / s) - 1)``: it is sampled as ``F.grid_sample(mode="bilinear",
    padding_mode="border", align_corners=True)`` samples the view ``grid[:, :, ::s, ::s, ::s]``.  (TiNeuVox pads its grid so
    that ``R - 1`` is a multiple of 4 and all levels span the same box; here any ``R`` is legal.)

    ``params`` is one flat float32 table (fewer than 2^31 values), a row-major ``[R_z, R_y, R_x, C]`` block: x runs fastest
    among the nodes and a node's channels are contiguous.  ``grid()`` is that 4-D view, and ``grid().permute(3, 2, 1, 0)[None]``
    the ``[1, C, N_x, N_y, N_z]`` tensor DVGO and TiNeuVox keep and hand to ``grid_sample`` with flipped coordinates;
    ``load_grid`` copies such a tensor in.  Initialised as ``init_scale * randn``.

    Every input is legal: a coordinate outside [0, 1] samples the border (``grid_sample``'s zero padding differs outside the
    box only), NaN samples node 0, and ``dL/dx`` is zero on such an axis.  Differentiable once w.r.t. ``params`` (float atomics:
    the last bits change from run to run) and ``x`` (bitwise reproducible); the torch path (CPU tensors, other dtypes) is
    differentiated by autograd.  ``out_dtype`` as for :class:`HashGridEncoding`.  ``resampled(resolution)`` is DVGO's
    ``scale_volume_grid``."""

    def __init__(self, resolution, n_features: int = 12, strides=(1,), init_scale: float = 0.1, out_dtype=None):
        super().__init__()
        self._configure(resolution, n_features, strides, init_scale, out_dtype)
        self.params = nn.Parameter(torch.randn(self.table.n_params, dtype=torch.float32) * self.init_scale)

    def _configure(self, resolution, n_features, strides, init_scale, out_dtype):
        """The checks and everything of the module but ``params`` (``resampled`` fills those itself)."""
        self.out_dtype = _check_out_dtype(out_dtype)
        if not (isinstance(n_features, int) and (n_features in (1, 2) or (4 <= n_features <= 64 and n_features % 4 == 0))):
            raise ValueError(f"VoxelGridEncoding: n_features must be 1, 2 or a multiple of 4 up to 64 (got {n_features})")
        resolution, strides = tuple(int(r) for r in resolution), tuple(int(s) for s in strides)
        if len(resolution) != 3:
            raise ValueError(f"VoxelGridEncoding: resolution must have 3 entries (got {len(resolution)})")
        if min(resolution) < 2:
            raise ValueError(f"VoxelGridEncoding: every resolution must be at least 2 (got {resolution})")
        if not 1 <= len(strides) <= VOXEL_MAX_STRIDES:
            raise ValueError(f"VoxelGridEncoding: strides must have 1..{VOXEL_MAX_STRIDES} entries (got {len(strides)})")
        for s in strides:
            if not 1 <= s <= 8:
                raise ValueError(f"VoxelGridEncoding: every stride must be in 1..8 (got {strides})")
            if min(-(-r // s) for r in resolution) < 2:
                raise ValueError(f"VoxelGridEncoding: stride {s} leaves fewer than 2 nodes along an axis of resolution {resolution}")
        self.n_input_dims, self.n_features, self.strides, self.resolution = 3, n_features, strides, resolution
        self.table = VoxelTable(resolution, n_features, strides)
        if self.table.n_params >= 1 << 31:
            raise ValueError(f"VoxelGridEncoding: {self.table.n_params} parameters (at most 2^31 - 1)")
        self.n_output_dims = n_features * len(strides)
        self.init_scale = float(init_scale)

    _entries = ("nfa_voxgrid_fwd", "nfa_voxgrid_bwd")

    def grid(self) -> Tensor:
        """The table as a ``[R_z, R_y, R_x, C]`` view of ``params``."""
        Rx, Ry, Rz = self.resolution
        return self.params.view(Rz, Ry, Rx, self.n_features)

    @torch.no_grad()
    def load_grid(self, t: Tensor) -> None:
        """Copy a DVGO / TiNeuVox grid, ``[1, C, N_x, N_y, N_z]`` or ``[C, N_x, N_y, N_z]``, into ``params``."""
        if t.dim() == 5 and t.shape[0] == 1:
            t = t[0]
        want = (self.n_features, *self.resolution)
        if tuple(t.shape) != want:
            raise ValueError(f"VoxelGridEncoding.load_grid: the grid must have shape {(1, *want)} or {want} (got {tuple(t.shape)})")
        self.grid().copy_(t.permute(3, 2, 1, 0))

    def _lead(self, dtype: torch.dtype):
        return (B.ELEM_CODES[dtype],)

    def _table_args(self, n_points: int):
        return n_points, self.n_features, self.table.c_res, len(self.strides), self.table.c_strides

    def forward(self, x: Tensor) -> Tensor:
        assert x.shape[-1] == 3, "VoxelGridEncoding: x must have shape (..., 3)"
        out = _resolve_out_dtype(self.out_dtype, x)
        x, ctx = _autocast_off(x)
        with ctx:
            lead = x.shape[:-1]
            x2 = x.reshape(-1, 3)
            p = self.params
            if x2.is_cuda and x2.dtype == torch.float32 and p.dtype == torch.float32 and p.device == x2.device:
                y = _GridFn.apply(x2.contiguous(), p, self, out)   # (element-wise access: no alignment beyond 4 bytes)
            else:
                dt = torch.promote_types(x2.dtype, p.dtype)
                y = _voxgrid_torch(x2.to(dt), p.to(dt), self.table)
                if self.out_dtype is not None:
                    y = y.to(out)
            return y.view(*lead, self.n_output_dims)

    @torch.no_grad()
    def resampled(self, resolution) -> "VoxelGridEncoding":
        """A new module on the same device whose table is this one resampled to ``resolution`` (each axis up, down or
        unchanged) in one launch: ``F.interpolate(mode="trilinear", align_corners=True)``, DVGO's ``scale_volume_grid``.  The
        same resolution copies the table bit for bit (finite values).  ``strides`` carry over and must fit the new resolution.
        Optimiser state does not follow: build a new optimiser, as DVGO does."""
        new = VoxelGridEncoding.__new__(VoxelGridEncoding)   # (no random table is drawn for a module that gets this one's samples)
        nn.Module.__init__(new)
        new._configure(resolution, self.n_features, self.strides, self.init_scale, self.out_dtype)
        p = self.params.detach()
        if p.is_cuda and p.dtype == torch.float32:
            q = torch.empty(new.table.n_params, dtype=torch.float32, device=p.device)
            with torch.cuda.device(p.device):
                B.call("nfa_voxgrid_resample", B.ptr(p), self.table.c_res, B.ptr(q), new.table.c_res, self.n_features, B.stream())
        else:
            q = _voxel_resample_torch(p, self.table, new.table)
        new.params = nn.Parameter(q, requires_grad=self.params.requires_grad)
        return new

    def extra_repr(self) -> str:
        return (f"resolution={self.resolution}, n_features={self.n_features}, strides={self.strides}"
                + (f", init_scale={self.init_scale}" if self.init_scale != 0.1 else "")
                + (f", out_dtype={self.out_dtype}" if self.out_dtype is not None else ""))


SIN_DIMS = (1, 2, 3, 4)   # input dimensions of the native sinusoidal encoding
SIN_MAX_FREQS = 16


def barf_window(alpha, n_freqs: int) -> Tensor:
    """BARF's coarse-to-fine weights of ``n_freqs`` frequencies at progress ``alpha`` in [0, n_freqs] (Lin et al. 2021, eq. 14;
    the Nerfies window is the same curve): ``w_k = (1 - cos(pi * clamp(alpha - k, 0, 1))) / 2`` as a float32 tensor, on
    ``alpha``'s device when that is a tensor.  Hand it to ``SinusoidalEncoding.forward(..., freq_weights=w)``."""
    alpha = torch.as_tensor(alpha, dtype=torch.float32)
    k = torch.arange(int(n_freqs), dtype=torch.float32, device=alpha.device)
    return (1.0 - torch.cos(math.pi * torch.clamp(alpha - k, 0.0, 1.0))) / 2.0


def _sinusoidal_torch(x: Tensor, min_deg: int, max_deg: int, use_identity: bool = True, var: Tensor | None = None,
                      freq_weights: Tensor | None = None) -> Tensor:
    """The sinusoidal encoding in torch: the reference's formula literally (``sin`` of ``cat([xb, xb + 0.5 * pi])``; bit for
    bit its ``SinusoidalEncoder`` without ``var`` and ``freq_weights``), both blocks times ``a = w_k exp(-0.5 s_k^2 var_d)``
    where those are given."""
    if max_deg == min_deg:
        return x
    L, D = max_deg - min_deg, x.shape[-1]
    scales = torch.tensor([2.0 ** i for i in range(min_deg, max_deg)], dtype=x.dtype, device=x.device)
    xb = torch.reshape(x[..., None, :] * scales[:, None], list(x.shape[:-1]) + [L * D])
    latent = torch.sin(torch.cat([xb, xb + 0.5 * math.pi], dim=-1))
    if var is not None or freq_weights is not None:
        a = torch.ones(L, 1, dtype=x.dtype, device=x.device) if freq_weights is None else freq_weights.to(x.dtype)[:, None]
        if var is not None:
            a = a * torch.exp((-0.5 * (scales * scales))[:, None] * var[..., None, :])
        a = torch.reshape(a.expand(*x.shape[:-1], L, D), list(x.shape[:-1]) + [L * D])
        latent = latent * torch.cat([a, a], dim=-1)
    if use_identity:
        latent = torch.cat([x, latent], dim=-1)
    return latent


class _SinEncFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, var, fw, enc: "SinusoidalEncoding", dtype: torch.dtype):
        B.require_device(x, var, fw)
        N = x.shape[0]
        y = torch.empty(N, enc.n_output_dims, dtype=dtype, device=x.device)
        if N:
            with torch.cuda.device(x.device):
                B.call("nfa_sinenc_fwd", B.ELEM_CODES[dtype], B.ptr(x), B.ptr(var), B.ptr(fw), *enc._args(N), B.ptr(y), B.stream())
        ctx.enc, ctx.dtype, ctx.has_var, ctx.has_fw = enc, dtype, var is not None, fw is not None
        ctx.save_for_backward(x, *(t for t in (var, fw) if t is not None))
        return y

    @staticmethod
    def backward(ctx, g_y):
        need_x, need_v = ctx.needs_input_grad[:2]
        if g_y is None or not (need_x or need_v):
            return None, None, None, None, None
        x, *rest = ctx.saved_tensors
        var = rest.pop(0) if ctx.has_var else None
        fw = rest.pop(0) if ctx.has_fw else None
        g_x, g_v = _SinEncBwdFn.apply(x, var, fw, _grad_as(g_y, ctx.dtype), ctx.enc, ctx.dtype, need_x, need_v)
        return g_x, g_v, None, None, None


class _SinEncBwdFn(torch.autograd.Function):
    """The sinusoidal encoding's backward as a function ``(x, var, g_y) -> (g_x, g_var)``, so that ``g_x`` can be
    differentiated again (``create_graph=True``: the Eikonal term of an SDF MLP).  Its own backward is one
    ``nfa_sinenc_bwd_bwd`` call; with ``var`` there is no second order."""

    @staticmethod
    def forward(ctx, x, var, fw, g, enc: "SinusoidalEncoding", dtype: torch.dtype, need_x: bool, need_v: bool):
        g_x = torch.empty_like(x) if need_x else None
        g_v = torch.empty_like(var) if need_v else None
        if x.shape[0]:
            with torch.cuda.device(x.device):
                B.call("nfa_sinenc_bwd", B.ELEM_CODES[dtype], B.ptr(x), B.ptr(var), B.ptr(fw), B.ptr(g), *enc._args(x.shape[0]),
                       B.ptr(g_x), B.ptr(g_v), B.stream())
        ctx.enc, ctx.dtype, ctx.has_var, ctx.has_fw = enc, dtype, var is not None, fw is not None
        ctx.save_for_backward(x, g, *((fw,) if fw is not None else ()))
        ctx.set_materialize_grads(False)
        return g_x, g_v

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_x, gg_v):
        if gg_x is None and gg_v is None:
            return (None,) * 8
        if ctx.has_var or gg_v is not None:
            raise NotImplementedError("SinusoidalEncoding: the second order (differentiating dL/dx or dL/dvar again) is not "
                                      "implemented with var; the torch path on CPU tensors is differentiated by autograd")
        need_x, need_g = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        if not (need_x or need_g):
            return (None,) * 8
        x, g, *rest = ctx.saved_tensors
        fw = rest[0] if ctx.has_fw else None
        v = gg_x.to(torch.float32).contiguous()
        x2 = torch.empty_like(x) if need_x else None
        gg_y = torch.empty_like(g) if need_g else None
        if x.shape[0]:
            with torch.cuda.device(x.device):
                B.call("nfa_sinenc_bwd_bwd", B.ELEM_CODES[ctx.dtype], B.ptr(x), B.ptr(fw), B.ptr(g), B.ptr(v),
                       *ctx.enc._args(x.shape[0]), B.ptr(gg_y), B.ptr(x2), B.stream())
        return x2, None, None, gg_y, None, None, None, None


class SinusoidalEncoding(nn.Module):
    """NeRF's sinusoidal (positional) encoding, the reference's ``SinusoidalEncoder(x_dim, min_deg, max_deg, use_identity)``
    (``examples/radiance_fields/mlp.py``) as one native pass each way (csrc/sinenc.hip):
    ``forward(x[..., D]) -> [..., latent_dim]``, ``latent_dim = n_output_dims = (int(use_identity) + 2 L) D``,
    ``L = max_deg - min_deg``.  Columns in the reference's order: ``x`` (when ``use_identity``; bitwise copies), then
    ``sin(2^k x_d)`` at column ``(k - min_deg) D + d`` of the sine block, then the cosine block in the same order.
    ``L == 0`` returns ``x`` itself whatever ``use_identity`` is, as the reference does.

    ``n_input_dims`` D in 1..4, L in 0..16, ``-16 <= min_deg <= max_deg <= 32``.  No parameters.

    ``forward(x, var=None, freq_weights=None)``.  ``freq_weights``: a float32 tensor of L per-frequency weights on ``x``'s
    device; both blocks of frequency ``k`` are multiplied by ``w_k`` (BARF's coarse-to-fine schedule, see
    :func:`barf_window`; the Nerfies window; FreeNeRF's frequency mask).  It is read through its pointer when the pass runs,
    so a training loop can update it in place, also inside a captured step; it gets no gradient.  ``var``: a ``[..., D]``
    diagonal variance in ``x``'s shape; both blocks are multiplied by ``exp(-0.5 4^k var_d)``, mip-NeRF's integrated
    positional encoding (the identity columns are untouched).

    CUDA float32 inputs run the native passes: float32 arithmetic with the device library's accurate ``sincosf`` / ``expf``,
    the cosine evaluated itself (the reference's ``sin(x_b + pi/2)`` rounds the phase; the two differ by at most that
    rounding, ``2^-22 max(1, |2^k x|)``).  Differentiable w.r.t. ``x`` and ``var``, bitwise reproducible, and w.r.t. ``x`` a
    second time: ``torch.autograd.grad(y, x, g, create_graph=True)`` gives a ``dL/dx`` that can be differentiated towards
    ``x`` and ``g`` (one native pass).  With ``var`` the second order raises ``NotImplementedError``.  CPU tensors and other
    dtypes take the torch path, the reference's formula literally (bit for bit the reference), differentiated by autograd.
    ``out_dtype`` as for :class:`HashGridEncoding`."""

    def __init__(self, n_input_dims: int, min_deg: int, max_deg: int, use_identity: bool = True, out_dtype=None):
        super().__init__()
        self.out_dtype = _check_out_dtype(out_dtype)
        if n_input_dims not in SIN_DIMS:
            raise ValueError(f"SinusoidalEncoding: n_input_dims must be in 1..4 (got {n_input_dims})")
        if not (isinstance(min_deg, int) and isinstance(max_deg, int) and -16 <= min_deg <= max_deg <= 32):
            raise ValueError(f"SinusoidalEncoding: need integers -16 <= min_deg <= max_deg <= 32 (got min_deg={min_deg}, "
                             f"max_deg={max_deg})")
        if max_deg - min_deg > SIN_MAX_FREQS:
            raise ValueError(f"SinusoidalEncoding: at most {SIN_MAX_FREQS} frequencies (got max_deg - min_deg = {max_deg - min_deg})")
        self.n_input_dims, self.min_deg, self.max_deg = int(n_input_dims), min_deg, max_deg
        self.use_identity = bool(use_identity)
        self.n_freqs = max_deg - min_deg
        self.n_output_dims = (int(self.use_identity) + 2 * self.n_freqs) * self.n_input_dims

    latent_dim = property(lambda self: self.n_output_dims)

    def _args(self, n_points: int):
        return n_points, self.n_input_dims, self.min_deg, self.n_freqs, int(self.use_identity)

    def forward(self, x: Tensor, var: Tensor | None = None, freq_weights: Tensor | None = None) -> Tensor:
        D, L = self.n_input_dims, self.n_freqs
        if x.shape[-1] != D:
            raise ValueError(f"SinusoidalEncoding: x must have shape (..., {D}) (got {tuple(x.shape)})")
        if var is not None and var.shape != x.shape:
            raise ValueError(f"SinusoidalEncoding: var must have x's shape {tuple(x.shape)} (got {tuple(var.shape)})")
        if freq_weights is not None:
            if freq_weights.shape != (L,) or freq_weights.dtype != torch.float32:
                raise ValueError(f"SinusoidalEncoding: freq_weights must be a float32 tensor of shape ({L},) (got "
                                 f"{tuple(freq_weights.shape)}, {freq_weights.dtype})")
            if freq_weights.device != x.device:
                raise ValueError(f"SinusoidalEncoding: freq_weights must be on x's device {x.device} (got {freq_weights.device})")
        if L == 0:
            return x
        out = _resolve_out_dtype(self.out_dtype, x)
        x, ctx = _autocast_off(x)
        with ctx:
            lead = x.shape[:-1]
            x2 = x.reshape(-1, D)
            v2 = None if var is None else var.reshape(-1, D)
            if x2.is_cuda and x2.dtype == torch.float32 and (v2 is None or (v2.dtype == torch.float32 and v2.device == x2.device)):
                fw = None if freq_weights is None else freq_weights.detach().contiguous()
                y = _SinEncFn.apply(x2.contiguous(), None if v2 is None else v2.contiguous(), fw, self, out)
            else:
                if v2 is not None:
                    v2 = v2.to(x2.dtype)
                y = _sinusoidal_torch(x2, self.min_deg, self.max_deg, self.use_identity, v2,
                                      None if freq_weights is None else freq_weights.detach())
                if self.out_dtype is not None:
                    y = y.to(out)
            return y.view(*lead, self.n_output_dims)

    def extra_repr(self) -> str:
        return (f"n_input_dims={self.n_input_dims}, min_deg={self.min_deg}, max_deg={self.max_deg}"
                + ("" if self.use_identity else ", use_identity=False")
                + (f", out_dtype={self.out_dtype}" if self.out_dtype is not None else ""))


def encoding_from_tcnn_config(n_input_dims: int, config: dict, out_dtype=None, deterministic: bool = False) -> nn.Module:
    """The encoding a tiny-cuda-nn encoding config describes: ``HashGrid`` (linear interpolation), ``SphericalHarmonics``,
    or ``Composite`` with ONE nested encoding over all input dimensions (as ``ngp.py`` builds its direction encoding).
    Anything else raises ``ValueError``.  ``out_dtype`` is handed to the encoding built, ``deterministic`` to a hash grid.
    ``"interpolation": "Smoothstep"`` is still refused here; build it with ``HashGridEncoding(..., interpolation="Smoothstep")``.
    A ``HashGrid`` of other than 3 input dimensions is refused here too (``only 3 input dimensions``); build a 2-D or 4-D grid
    with ``HashGridEncoding(n_input_dims=2 or 4, ...)``."""
    if not isinstance(config, dict) or "otype" not in config:
        raise ValueError(f"not a tcnn encoding config: {config!r}")
    otype = config["otype"]
    if otype == "HashGrid":
        interp = config.get("interpolation", "Linear")
        if interp != "Linear":
            raise ValueError(f"HashGrid: only linear interpolation is supported (got {interp!r})")
        if n_input_dims != 3:
            raise ValueError(f"HashGrid: only 3 input dimensions are supported here (got {n_input_dims}); "
                             f"HashGridEncoding(n_input_dims=...) takes 2, 3 or 4")
        return HashGridEncoding(n_input_dims, n_levels=int(config.get("n_levels", 16)),
                                n_features_per_level=int(config.get("n_features_per_level", 2)),
                                log2_hashmap_size=int(config.get("log2_hashmap_size", 19)),
                                base_resolution=config.get("base_resolution", 16),
                                per_level_scale=float(config.get("per_level_scale", 2.0)), out_dtype=out_dtype,
                                deterministic=deterministic)
    if otype == "SphericalHarmonics":
        return SphericalHarmonicsEncoding(n_input_dims, degree=int(config.get("degree", 4)), out_dtype=out_dtype)
    if otype == "Composite":
        nested = config.get("nested", [])
        if len(nested) != 1:
            raise ValueError(f"Composite: exactly one nested encoding is supported (got {len(nested)})")
        inner = dict(nested[0])
        dims = inner.pop("n_dims_to_encode", n_input_dims)
        if dims != n_input_dims:
            raise ValueError(f"Composite: the nested encoding must cover all {n_input_dims} dimensions (got {dims})")
        return encoding_from_tcnn_config(n_input_dims, inner, out_dtype, deterministic)
    raise ValueError(f"unsupported tcnn encoding {otype!r} (supported: HashGrid, SphericalHarmonics, Composite)")

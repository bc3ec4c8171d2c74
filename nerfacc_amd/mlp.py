"""The field's network as fused half-precision MFMA passes (csrc/mlp.hip): tiny-cuda-nn's ``FullyFusedMLP``, and with
``bias=`` / ``skip_layer=`` the reference's own ``MLP`` class (ref: examples/radiance_fields/mlp.py) up to 128 neurons.  Wider and
deeper networks -- 128 or 256 neurons, up to 8 hidden layers: the reference's ``NerfMLP`` -- are :class:`StreamedMLP` and
:class:`NerfMLP` at the end of this module (csrc/mlp_stream.hip: the packed weights stream through the LDS).

The reference's NGP fields put ``tcnn.Network(otype="FullyFusedMLP")`` between the encodings and the renderer (ref:
examples/radiance_fields/ngp.py:131-135, 150-154, 255-259): 64 neurons, 1 or 2 hidden layers, ReLU, no biases, no output
activation (the output activations live in :func:`nerfacc_amd.rendering_from_raw`).  :class:`FusedMLP` is that component:
the encodings hand it fp16 / bf16 activations (``out_dtype=``), it hands the renderer fp16 / bf16 raw outputs, and the
gradients travel back the same way, with no cast pass and no ``torch.autocast`` in between.

Not part of ``nerfacc_amd.__all__`` (nerfacc has no such module): ``from nerfacc_amd.mlp import FusedMLP``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _backend as B

WIDTHS = (64, 128)
MAX_HIDDEN_LAYERS = 4
MAX_INPUT_DIMS = 256
MAX_OUTPUT_DIMS = 32
LDS_BUDGET = 160 * 1024          # bytes of LDS per compute unit
STAGE_BYTES = 4 * 32 * 33 * 4    # the four waves' store staging tiles (csrc/mlp.hip: STAGE_BYTES)
# include/nerfacc_hip.h: NFA_MLP_WGRAD_MIN_SLICE, NFA_MLP_WGRAD_MAX_SLICES
WGRAD_MIN_SLICE = 256
WGRAD_MAX_SLICES = 256
MAX_CAT_DIMS = 256               # n_input_dims + n_neurons of a network with a skip: the weight gradient's staging of one layer


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def skip_mask_of(skip_layer: Optional[int], n_hidden: int) -> int:
    """Bit ``l`` set: layer ``l`` takes ``[H_{l-1}, x]``.  The reference's rule (ref: examples/radiance_fields/mlp.py:50-57,
    92-97): the input is appended after hidden layer ``i`` when ``i > 0 and i % skip_layer == 0``, so layer ``i + 1`` sees it."""
    if skip_layer is None:
        return 0
    return sum(1 << (i + 1) for i in range(1, n_hidden) if i % skip_layer == 0)


def layer_dims(n_in: int, n_out: int, width: int, n_hidden: int, skip_mask: int = 0) -> List[tuple]:
    """``[(out_l, in_l)]`` of the ``n_hidden + 1`` matrices; a layer of ``skip_mask`` has ``width + n_in`` inputs."""
    ins = [n_in] + [width + (n_in if (skip_mask >> l) & 1 else 0) for l in range(1, n_hidden + 1)]
    outs = [width] * n_hidden + [n_out]
    return list(zip(outs, ins))


def image_elems(n_in: int, n_out: int, width: int, n_hidden: int, skip_mask: int = 0) -> tuple:
    """Elements of the packed forward and backward weight images (include/nerfacc_hip.h: nfa_mlp_pack_weights,
    nfa_mlp_desc): the x part of a cat layer starts on a k-step of its own."""
    dims = layer_dims(n_in, n_out, width, n_hidden, skip_mask)
    kq = [_cdiv(width, 16) + _cdiv(n_in, 16) if (skip_mask >> l) & 1 else _cdiv(i, 16) for l, (o, i) in enumerate(dims)]
    fwd = sum(_cdiv(o, 32) * q * 512 for (o, i), q in zip(dims, kq))
    bwd = sum(_cdiv(i, 32) * _cdiv(o, 16) * 512 for o, i in dims)
    return fwd, bwd


def lds_bias_bytes(width: int, n_hidden: int, bias: bool) -> int:
    """Bytes of the float32 biases as the forward pass holds them beside its image (the output layer padded to 32 rows)."""
    return (n_hidden * width + 32) * 4 if bias else 0


def wgrad_slices(n_points: int) -> int:
    """Slices the weight gradient cuts ``n_points`` into (include/nerfacc_hip.h: nfa_mlp_bwd_weights)."""
    s = min(max(_cdiv(n_points, WGRAD_MIN_SLICE), 1), WGRAD_MAX_SLICES)
    slice_len = _cdiv(_cdiv(n_points, s), 64) * 64
    return _cdiv(n_points, slice_len)


# ---------------------------------------------------------------- the arithmetic restated in torch (CPU tensors)

def _cat_input(h: Tensor, x0: Tensor, l: int, skip_mask: int) -> Tensor:
    """The input of layer ``l``: ``[h, x0]`` at a cat layer, ``x0`` the rounded network input (or tangent input)."""
    return torch.cat([h, x0], dim=1) if (skip_mask >> l) & 1 else h


ACTIVATIONS = ("None", "ReLU", "LeakyReLU", "Sigmoid", "Tanh", "Softplus", "Exponential")   # tiny-cuda-nn's names; B.ACT_CODES
UNSUPPORTED_ACTIVATIONS = ("Sine", "Squareplus")   # tcnn's other two: Sine's derivative needs the pre-activation, which no pass stores
CURVED_ACTIVATIONS = ("Sigmoid", "Tanh", "Softplus", "Exponential")   # rho = f'' / f' is not identically zero
LEAKY_SLOPE = 0.009999999776482582   # 0.01f
DEFAULT_ACT = ("ReLU", "None", 10.0)


def check_activation(who: str, what: str, name) -> str:
    if name is None:
        name = "None"
    if name in UNSUPPORTED_ACTIVATIONS:
        raise ValueError(f"{who}: {what} {name!r} is not supported ({' and '.join(UNSUPPORTED_ACTIVATIONS)} stay refused: Sine's derivative "
                         f"needs the pre-activation, which no pass stores); one of {', '.join(ACTIVATIONS)}")
    if name not in ACTIVATIONS:
        raise ValueError(f"{who}: {what} {name!r}: one of {', '.join(ACTIVATIONS)}")
    return name


def _act(name: str, z: Tensor, beta: float) -> Tensor:
    """``f(z)`` in ``z``'s own precision (float32 where the kernels are restated), unrounded."""
    if name == "ReLU":
        return torch.relu(z)
    if name == "LeakyReLU":
        return torch.where(z > 0, z, z * LEAKY_SLOPE)
    if name == "Sigmoid":
        return 1.0 / (1.0 + torch.exp(-z))
    if name == "Tanh":
        return torch.tanh(z)
    if name == "Softplus":
        return torch.where(z > 0, z, torch.zeros_like(z)) + torch.log1p(torch.exp(-beta * z.abs())) / beta
    if name == "Exponential":
        return torch.exp(z)
    return z


def _times_deriv(name: str, d: Tensor, y: Tensor, beta: float) -> Tensor:
    """``d * f'(y)`` with ``f'`` formed from the stored ``y``; ReLU and LeakyReLU select."""
    if name == "ReLU":
        return torch.where(y > 0, d, torch.zeros_like(d))
    if name == "LeakyReLU":
        return torch.where(y > 0, d, d * LEAKY_SLOPE)
    if name == "Sigmoid":
        return d * (y * (1.0 - y))
    if name == "Tanh":
        return d * (1.0 - y * y)
    if name == "Softplus":
        return d * (1.0 - torch.exp(-beta * y))
    if name == "Exponential":
        return d * y
    return d


def _curvature_term(name: str, a: Tensor, y: Tensor, dz: Tensor, beta: float) -> Tensor:
    """``R = (rho(y) dZ) A``, an exact zero where ``rho`` is identically zero."""
    if name == "Sigmoid":
        rho = 1.0 - 2.0 * y
    elif name == "Tanh":
        rho = -2.0 * y
    elif name == "Softplus":
        rho = beta * torch.exp(-beta * y)
    elif name == "Exponential":
        rho = torch.ones_like(y)
    else:
        return torch.zeros_like(a)
    return (rho * dz) * a


def _rnd(t: Tensor, dtype: torch.dtype) -> Tensor:
    """``t`` rounded once to ``dtype`` and widened to float32 again.  ``dtype=torch.float64`` is the unrounded form of the
    restatements: nothing rounds and every sum is float64 (what the tests compare with ``torch.autograd``)."""
    return t.double() if dtype == torch.float64 else t.to(dtype).float()


def _wide(t: Tensor, dtype: torch.dtype) -> Tensor:
    return t.double() if dtype == torch.float64 else t.float()


def _forward_torch(x: Tensor, weights: Sequence[Tensor], dtype: torch.dtype, out_f32: bool, biases: Optional[Sequence[Tensor]] = None,
                   skip_mask: int = 0, act: tuple = DEFAULT_ACT):
    """(y, hidden): float32 sums of exact products, rounded where the kernels round (x, W, every hidden activation, y).  A
    bias is added in float32 and never rounded; a cat layer takes ``cat([h, x rounded])``.  ``act``: (hidden activation,
    output activation, beta); the activation is evaluated in float32 and rounded once."""
    hid, out, beta = act
    x0 = _rnd(x, dtype)
    h, hidden = x0, []
    for l, w in enumerate(weights):
        z = _cat_input(h, x0, l, skip_mask) @ _rnd(w, dtype).t()
        if biases is not None:
            z = z + _wide(biases[l], dtype)
        if l < len(weights) - 1:
            h = _rnd(_act(hid, z, beta), dtype)
            hidden.append(h)
    z = _act(out, z, beta)
    return (z if out_f32 else z.to(dtype)), hidden


def _backward_torch(x: Tensor, weights: Sequence[Tensor], hidden: Sequence[Tensor], g: Tensor, dtype: torch.dtype,
                    need_x: bool, need_p: bool, bias: bool = False, skip_mask: int = 0, act: tuple = DEFAULT_ACT,
                    y: Optional[Tensor] = None, inject: Optional[Sequence[Tensor]] = None):
    """(dL/dx in x's dtype, dL/dparams flat float32: matrices, then biases, [dZ_l]) with dZ_l rounded as the kernels round it:
    ``dZ_L = rnd(g * f_out'(y))``, ``dZ_l = rnd(dH_l * f'(H_l))``.  dL/dx is the float32 sum of layer 0's product and the skip
    columns' products of every cat layer, rounded once.  With ``inject`` (the tangent's ``[R_0 .. R_{L-1}]``; ``g`` is then
    ``R_L`` and takes no output derivative) this is the curvature pass: ``E_l = rnd(dH_l * f'(H_l) + R_l)``."""
    hid, out, beta = act
    x0 = _rnd(x, dtype)
    W = weights[0].shape[0]
    if out == "None" or inject is not None:
        dz = _rnd(g, dtype)
    else:
        dz = _rnd(_times_deriv(out, _wide(g, dtype), _wide(y, dtype), beta), dtype)
    dzs, g_w, g_b = [dz], [], []
    g_x, skips = None, []
    for l in range(len(weights) - 1, -1, -1):
        h_prev = hidden[l - 1] if l > 0 else x0
        if need_p:
            g_w.append(dz.t() @ _cat_input(h_prev, x0, l, skip_mask))
            g_b.append(dz.sum(0))
        if l == 0 and not need_x:
            break
        dh = dz @ _rnd(weights[l], dtype)
        if l > 0:
            if (skip_mask >> l) & 1:
                skips.append(dh[:, W:])
                dh = dh[:, :W]
            dz = _times_deriv(hid, dh, h_prev, beta)   # ReLU: a select
            if inject is not None:
                dz = dz + inject[l - 1]
            dz = _rnd(dz, dtype)
            dzs.append(dz)
        else:
            for s in reversed(skips):   # ascending layers, as the kernel adds them
                dh = dh + s
            g_x = dh.to(x.dtype)
    g_p = torch.cat([w.reshape(-1) for w in reversed(g_w)] + (list(reversed(g_b)) if bias else [])) if need_p else None
    return g_x, g_p, dzs[::-1]


def _tangent_torch(v: Tensor, weights: Sequence[Tensor], hidden: Sequence[Tensor], dzs: Sequence[Tensor], dtype: torch.dtype,
                   need_p: bool, bias: bool = False, skip_mask: int = 0, act: tuple = DEFAULT_ACT, y: Optional[Tensor] = None):
    """:func:`_tangent_terms` without the curvature cotangents: (u, ds/dparams, [T_l])."""
    return _tangent_terms(v, weights, hidden, dzs, dtype, need_p, bias, skip_mask, act, y)[:3]


def _tangent_terms(v: Tensor, weights: Sequence[Tensor], hidden: Sequence[Tensor], dzs: Sequence[Tensor], dtype: torch.dtype,
                   need_p: bool, bias: bool = False, skip_mask: int = 0, act: tuple = DEFAULT_ACT, y: Optional[Tensor] = None):
    """The second order: (u float32 unrounded, ds/dparams flat float32, [T_{-1}, T_0 .. T_{L-1}], [R_0 .. R_L]) for the cotangent
    ``v`` of dL/dx.  The derivative of the network along ``v`` with the SAVED activations (``f'`` from ``hidden``, never an
    activation of the tangent): ``T_l = rnd(A_l * f'(H_l))``, ``u = f_out'(y) * A_L``; ``ds/dW_l = dZ_l^T T_{l-1}`` with the
    first backward's ``dZ_l`` is the part of the parameter gradient returned here, whose bias segment is zero; a cat layer sees
    ``[T_{l-1}, v]``.  ``R_l = rnd((rho(H_l) dZ_l) A_l)`` are the cotangents the curvature pass injects (zeros where ``rho`` is)."""
    hid, out, beta = act
    t0 = _rnd(v, dtype)
    t, ts, rs = t0, [t0], []
    for l, w in enumerate(weights):
        z = _cat_input(t, t0, l, skip_mask) @ _rnd(w, dtype).t()
        if l < len(weights) - 1:
            rs.append(_rnd(_curvature_term(hid, z, hidden[l], dzs[l], beta), dtype))
            t = _rnd(_times_deriv(hid, z, hidden[l], beta), dtype)
            ts.append(t)
    if out != "None":
        rs.append(_rnd(_curvature_term(out, z, _wide(y, dtype), dzs[-1], beta), dtype))
        z = _times_deriv(out, z, _wide(y, dtype), beta)
    else:
        rs.append(torch.zeros_like(z))
    g_p = None
    if need_p:
        g_p = torch.cat([(dz.t() @ _cat_input(t, t0, l, skip_mask)).reshape(-1) for l, (dz, t) in enumerate(zip(dzs, ts))] +
                        ([torch.zeros(sum(w.shape[0] for w in weights))] if bias else []))
    return z, g_p, ts, rs


def _curvature_torch(x: Tensor, weights: Sequence[Tensor], hidden: Sequence[Tensor], rs: Sequence[Tensor], dtype: torch.dtype,
                     need_x: bool, need_p: bool, bias: bool = False, skip_mask: int = 0, act: tuple = DEFAULT_ACT):
    """The curvature pass: (ds/dx in x's dtype, the second part of ds/dparams: ``E_l^T [H_{l-1}(, x)]`` and ``sum_p E_l[p]``,
    [E_0 .. E_L]) with ``E_L = R_L``, ``E_{l-1} = rnd((W_l^T E_l)[:W] * f'(H_{l-1}) + R_{l-1})``: the data gradient's chain
    and the weight gradient on ``(x, H, E)``."""
    return _backward_torch(x, weights, hidden, rs[-1], dtype, need_x, need_p, bias, skip_mask, act, None, inject=rs[:-1])


# ---------------------------------------------------------------- autograd

class _MLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, params: Tensor, mlp: "FusedMLP"):
        N = x.shape[0]
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out_f32 = mlp.out_dtype == torch.float32
        ctx.mlp = mlp
        if N == 0:
            ctx.save_for_backward(x, params)
            return torch.empty(0, mlp.n_output_dims, dtype=mlp.out_dtype, device=x.device)
        if not x.is_cuda:
            y, hidden = _forward_torch(x, mlp._views(params), mlp.dtype, out_f32, mlp._bias_views(params), mlp.skip_mask, mlp._act_names)
            ctx.save_for_backward(x, params, *hidden, *([y] if mlp._out_act else []))
            return y
        B.require_device(x, params)
        elem = B.ELEM_CODES[mlp.dtype]
        fwd_img, bwd_img = mlp._images(params)
        y = torch.empty(N, mlp.n_output_dims, dtype=mlp.out_dtype, device=x.device)
        hidden = torch.empty(mlp.n_hidden_layers, N, mlp.n_neurons, dtype=mlp.dtype, device=x.device) if need_grad else None
        with torch.cuda.device(x.device):
            if mlp._plain:
                B.call("nfa_mlp_fwd", elem, B.ptr(x), B.ELEM_CODES[x.dtype], B.ptr(fwd_img), N, *mlp._shape, B.ptr(y),
                       B.ELEM_CODES[y.dtype], B.ptr(hidden), int(need_grad), B.stream())
            elif mlp._act is not None:
                B.call("nfa_mlp_act_fwd", elem, mlp._desc, mlp._act, B.ptr(x), B.ELEM_CODES[x.dtype], B.ptr(fwd_img),
                       mlp._bias_ptr(params), N, B.ptr(y), B.ELEM_CODES[y.dtype], B.ptr(hidden), int(need_grad), B.stream())
            else:
                B.call(mlp._entry("fwd"), elem, mlp._desc, B.ptr(x), B.ELEM_CODES[x.dtype], B.ptr(fwd_img), mlp._bias_ptr(params), N,
                       B.ptr(y), B.ELEM_CODES[y.dtype], B.ptr(hidden), int(need_grad), B.stream())
        if need_grad:   # the second order runs the chain again on the forward image
            ctx.save_for_backward(x, params, hidden, bwd_img, *([fwd_img] if mlp.second_order else []), *([y] if mlp._out_act else []))
        return y

    @staticmethod
    def backward(ctx, g_y):
        need_x, need_p = ctx.needs_input_grad[:2]
        if g_y is None or not (need_x or need_p):
            return None, None, None
        x, params, *saved = ctx.saved_tensors
        # y (saved for an output activation) is this function's own output: detached, or the second backward would come back
        # through here with a zero cotangent.  What dL/dx owes to y is in the second order's own formulas (R_L).
        g_x, g_p = _MLPBwdFn.apply(x, params, g_y, ctx.mlp, need_x, need_p, *[t.detach() for t in saved])
        return g_x, g_p, None


class _MLPBwdFn(torch.autograd.Function):
    """The backward as a function ``(x, params, g_y) -> (g_x, g_params)`` of its own, so that differentiating it again
    (``create_graph=True``) fails with a message that names the module instead of a missing ``grad_fn``, or, for a module
    with ``second_order=True``, runs the tangent pass: with ``v`` the cotangent of ``g_x`` and ``s = <v, g_x>``,
    ``T_{-1} = v``, ``T_l = M_l * (W_l T_{l-1})``, ``ds/dg_y = W_L T_{L-1}``, ``ds/dW_l = dZ_l^T T_{l-1}``, ``ds/dx = 0``.  With an
    activation that has curvature the tangent pass also writes ``R_l``, the curvature pass turns them into ``E_l`` and ``ds/dx``,
    and ``ds/dparams`` gains the weight gradient on ``(x, H, E)``: the two float32 results are added with one torch add."""

    @staticmethod
    def forward(ctx, x: Tensor, params: Tensor, g: Tensor, mlp: "FusedMLP", need_x: bool, need_p: bool, *saved):
        ctx.set_materialize_grads(False)
        saved = list(saved)
        ctx.mlp, ctx.g_dtype, ctx.g_shape, ctx.n_saved = mlp, g.dtype, g.shape, len(saved)
        N = x.shape[0]
        if N == 0:
            return (torch.empty_like(x) if need_x else None), (torch.zeros_like(params) if need_p else None)
        if g.dtype not in (torch.float32, mlp.dtype):
            g = g.float()
        g = g.contiguous()
        if not x.is_cuda:
            hidden_cpu, y = (saved[:-1], saved[-1]) if mlp._out_act else (saved, None)
            with torch.autocast("cpu", enabled=False):   # a backward called under autocast must not round the float32 sums
                g_x, g_p, dzs = _backward_torch(x, mlp._views(params), hidden_cpu, g, mlp.dtype, need_x, need_p, mlp.bias_enabled,
                                                mlp.skip_mask, mlp._act_names, y)
            if mlp.second_order:   # retained only under create_graph=True: a plain backward runs this in no-grad mode
                ctx.save_for_backward(params, *hidden_cpu, *dzs, *([x] if mlp._act is not None else []), *([y] if mlp._out_act else []))
            return g_x, g_p
        y = saved.pop() if mlp._out_act else None
        hidden, bwd_img, *fwd_img = saved
        elem, dev = B.ELEM_CODES[mlp.dtype], x.device
        dz = torch.empty(mlp.n_hidden_layers, N, mlp.n_neurons, dtype=mlp.dtype, device=dev)
        dz_out = g if g.dtype == mlp.dtype and not mlp._out_act else torch.empty(N, mlp.n_output_dims, dtype=mlp.dtype, device=dev)
        g_x = torch.empty_like(x) if need_x else None
        g_p = None
        with torch.cuda.device(dev):
            if mlp._plain:
                B.call("nfa_mlp_bwd_data", elem, B.ptr(g), B.ELEM_CODES[g.dtype], B.ptr(hidden), B.ptr(bwd_img), N, *mlp._shape,
                       B.ptr(dz), None if dz_out is g else B.ptr(dz_out), B.ptr(g_x), B.ELEM_CODES[x.dtype], B.stream())
            elif mlp._act is not None:
                B.call("nfa_mlp_act_bwd_data", elem, mlp._desc, mlp._act, B.ptr(g), B.ELEM_CODES[g.dtype], B.ptr(y),
                       B.ELEM_CODES[mlp.out_dtype], B.ptr(hidden), B.ptr(bwd_img), N, B.ptr(dz), None if dz_out is g else B.ptr(dz_out),
                       B.ptr(g_x), B.ELEM_CODES[x.dtype], B.stream())
            else:
                B.call(mlp._entry("bwd_data"), elem, mlp._desc, B.ptr(g), B.ELEM_CODES[g.dtype], B.ptr(hidden), B.ptr(bwd_img), N,
                       B.ptr(dz), None if dz_out is g else B.ptr(dz_out), B.ptr(g_x), B.ELEM_CODES[x.dtype], B.stream())
            if need_p:
                P = params.numel()
                partials = torch.empty(mlp._slices(N) * P, dtype=torch.float32, device=dev)
                g_p = torch.empty(P, dtype=torch.float32, device=dev)
                mlp._weight_gradient(elem, x, hidden, dz, dz_out, N, partials, g_p, zero_bias=False)
        if mlp.second_order:   # retained only under create_graph=True: a plain backward runs this in no-grad mode
            ctx.save_for_backward(hidden, dz, dz_out, *fwd_img, *([x, bwd_img] if mlp._act is not None else []), *([y] if mlp._out_act else []))
        return g_x, g_p

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_x, gg_p):
        mlp = ctx.mlp
        if isinstance(mlp, StreamedMLP):
            raise NotImplementedError("StreamedMLP: the second order (differentiating dL/dx or dL/dparams again, create_graph=True) is "
                                      "not implemented for the streamed network; FusedMLP(second_order=True) holds up to 128 neurons")
        if not mlp.second_order:
            raise NotImplementedError("FusedMLP: the second order (differentiating dL/dx or dL/dparams again, create_graph=True) is not "
                                      "enabled for this module: construct it with second_order=True (that of dL/dx, which an "
                                      "Eikonal term needs)")
        if gg_p is not None:
            raise NotImplementedError("FusedMLP: the second order of dL/dparams (a cotangent for dL/dparams) is not implemented, "
                                      "only that of dL/dx")
        need_p, need_g = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_x = ctx.needs_input_grad[0] and mlp._curved   # ds/dx is zero (None) when no activation has curvature
        none = (None,) * (6 + ctx.n_saved)
        if gg_x is None or not (need_p or need_g or need_x):
            return none
        N, P = gg_x.shape[0], mlp._bias_offsets[-1]   # all parameters: matrices, then biases
        v = gg_x.contiguous()
        u_dtype = ctx.g_dtype if ctx.g_dtype in (torch.float32, mlp.dtype) else torch.float32
        if N == 0:
            u = torch.empty(ctx.g_shape, dtype=ctx.g_dtype, device=v.device) if need_g else None
            return (torch.zeros_like(v) if need_x else None, torch.zeros(P, dtype=torch.float32, device=v.device) if need_p else None,
                    u) + none[3:]
        L = mlp.n_hidden_layers
        if not v.is_cuda:
            params, *saved = ctx.saved_tensors
            y = saved.pop() if mlp._out_act else None
            x = saved.pop() if mlp._act is not None else None
            hidden, dzs = saved[:L], saved[L:]
            s_x = None
            with torch.autocast("cpu", enabled=False):
                ws = mlp._views(params)
                u, g_p, _, rs = _tangent_terms(v, ws, hidden, dzs, mlp.dtype, need_p, mlp.bias_enabled, mlp.skip_mask, mlp._act_names, y)
                if mlp._curved and (need_p or need_x):
                    s_x, g_p2, _ = _curvature_torch(x, ws, hidden, rs, mlp.dtype, need_x, need_p, mlp.bias_enabled, mlp.skip_mask,
                                                    mlp._act_names)
                    if need_p:
                        g_p = g_p + g_p2
            return (s_x, g_p, u.to(ctx.g_dtype) if need_g else None) + none[3:]
        if mlp._act is not None:
            return _MLPBwdFn._backward_act(ctx, v, u_dtype, need_x, need_p, need_g) + none[3:]
        hidden, dz, dz_out, fwd_img = ctx.saved_tensors
        elem, dev = B.ELEM_CODES[mlp.dtype], v.device
        tangent = torch.empty(L, N, mlp.n_neurons, dtype=mlp.dtype, device=dev) if need_p else None
        u = torch.empty(N, mlp.n_output_dims, dtype=u_dtype, device=dev)
        g_p = None
        with torch.cuda.device(dev):
            if mlp._plain:
                B.call("nfa_mlp_tangent", elem, B.ptr(v), B.ELEM_CODES[v.dtype], B.ptr(hidden), B.ptr(fwd_img), N, *mlp._shape,
                       B.ptr(tangent), B.ptr(u), B.ELEM_CODES[u_dtype], B.stream())
            else:
                B.call("nfa_mlp_net_tangent", elem, mlp._desc, B.ptr(v), B.ELEM_CODES[v.dtype], B.ptr(hidden), B.ptr(fwd_img), N,
                       B.ptr(tangent), B.ptr(u), B.ELEM_CODES[u_dtype], B.stream())
            if need_p:   # ds/dW_l = dZ_l^T [T_{l-1}(, v)]: the weight gradient pass on (v, T) in the place of (x, H); ds/db = 0
                partials = torch.empty(wgrad_slices(N) * P, dtype=torch.float32, device=dev)
                g_p = torch.empty(P, dtype=torch.float32, device=dev)
                mlp._weight_gradient(elem, v, tangent, dz, dz_out, N, partials, g_p, zero_bias=True)
        return (None, g_p, (u if u.dtype == ctx.g_dtype else u.to(ctx.g_dtype)) if need_g else None) + none[3:]

    @staticmethod
    def _backward_act(ctx, v: Tensor, u_dtype: torch.dtype, need_x: bool, need_p: bool, need_g: bool):
        """The second order of a module with activations on the device: the tangent pass (which also writes ``R_l``), the
        curvature pass and the weight gradient pass twice.  Returns (ds/dx, ds/dparams, ds/dg)."""
        mlp = ctx.mlp
        saved = list(ctx.saved_tensors)
        y = saved.pop() if mlp._out_act else None
        hidden, dz, dz_out, fwd_img, x, bwd_img = saved
        N, P, L = v.shape[0], mlp._bias_offsets[-1], mlp.n_hidden_layers
        elem, dev = B.ELEM_CODES[mlp.dtype], v.device
        curved = mlp._curved and (need_p or need_x)
        half = lambda *shape: torch.empty(*shape, dtype=mlp.dtype, device=dev)
        tangent = half(L, N, mlp.n_neurons) if need_p else None
        r, r_out = (half(L, N, mlp.n_neurons), half(N, mlp.n_output_dims)) if curved else (None, None)
        u = torch.empty(N, mlp.n_output_dims, dtype=u_dtype, device=dev)
        s_x = g_p = None
        with torch.cuda.device(dev):
            B.call("nfa_mlp_act_tangent", elem, mlp._desc, mlp._act, B.ptr(v), B.ELEM_CODES[v.dtype], B.ptr(y), B.ELEM_CODES[mlp.out_dtype],
                   B.ptr(hidden), B.ptr(dz), B.ptr(dz_out), B.ptr(fwd_img), N, B.ptr(tangent), B.ptr(r), B.ptr(r_out), B.ptr(u),
                   B.ELEM_CODES[u_dtype], B.stream())
            if curved:
                e = half(L, N, mlp.n_neurons)
                s_x = torch.empty_like(x) if need_x else None
                B.call("nfa_mlp_act_curvature", elem, mlp._desc, mlp._act, B.ptr(r_out), B.ptr(hidden), B.ptr(r), B.ptr(bwd_img), N,
                       B.ptr(e), B.ptr(s_x), B.ELEM_CODES[x.dtype], B.stream())
            if need_p:
                partials = torch.empty(wgrad_slices(N) * P, dtype=torch.float32, device=dev)
                g_p = torch.empty(P, dtype=torch.float32, device=dev)
                mlp._weight_gradient(elem, v, tangent, dz, dz_out, N, partials, g_p, zero_bias=True)
                if curved:   # + E_l^T [H_{l-1}(, x)] and sum_p E_l: the same pass on (x, H, E); one torch add of two P-vectors
                    g_p2 = torch.empty(P, dtype=torch.float32, device=dev)
                    mlp._weight_gradient(elem, x, hidden, e, r_out, N, partials, g_p2, zero_bias=False)
                    g_p = g_p + g_p2
        return s_x, g_p, (u if u.dtype == ctx.g_dtype else u.to(ctx.g_dtype)) if need_g else None


class FusedMLP(nn.Module):
    """tiny-cuda-nn's ``FullyFusedMLP``: ``n_hidden_layers + 1`` weight matrices, by default no biases, ReLU on the hidden
    layers and no output activation, as one native launch forward and three backward (and, on request, three for the second
    order, six with an activation that has curvature).

    ``n_neurons`` 64 or 128, ``n_hidden_layers`` 1..4, ``n_input_dims`` 1..256, ``n_output_dims`` 1..32; a configuration
    whose packed weights do not fit the 160 KiB of LDS of a compute unit is refused here, with the sizes in the message.
    ``dtype`` (fp16 or bf16) is the type of the weights as the kernels see them, of the hidden activations and of the
    gradients between the layers; sums are float32.  The parameters are float32 masters in ONE flat ``nn.Parameter``
    (``params``), each matrix in torch's ``Linear`` layout ``[out, in]``: :meth:`weight` is a view of one,
    :meth:`linear_weights` / :meth:`load_linear_weights` exchange them with ``nn.Linear(bias=False)`` layers.  They are
    initialised as tcnn does: Xavier uniform per matrix, drawn from ``generator`` (default: a generator seeded 1337).

    ``forward(x)``: ``x [N, n_input_dims]`` float32 or ``dtype``, contiguous; a float32 ``x`` is rounded to ``dtype`` as
    the kernel loads it.  Returns ``[N, n_output_dims]`` in ``dtype``, or with ``out_dtype=torch.float32`` the float32
    accumulators unrounded.  ``dL/dx`` comes back in ``x``'s dtype, ``dL/dparams`` float32 without atomics: the same bits
    on every run.  ``torch.autocast`` changes nothing: the module handles its own precision.  CPU tensors take a torch
    restatement with the same rounding points.

    ``second_order=True`` makes ``dL/dx`` differentiable once more (``create_graph=True``: an Eikonal term on an SDF field's
    normals): one more fused launch, the tangent pass, and the weight gradient passes again.  For a network whose activations
    are piecewise linear (``None``, ``ReLU``, ``LeakyReLU``) this is exact: ``dL/dx`` is linear in ``dL/dy`` and in each matrix
    and its derivative factors are piecewise constant, so the gradient of ``<v, dL/dx>`` towards ``x`` is zero (``None``),
    towards ``dL/dy`` it is the network's derivative along ``v`` and towards the masters a weight gradient with the tangent
    activations in the place of the activations; float32, without atomics, the same bits on every run.  With an activation that
    has curvature (below) it is exact too, by one more fused launch, the curvature pass: the gradient towards ``x`` is then a
    tensor of ``x``'s dtype, which an encoding's own second order receives through autograd.  It costs memory only under ``create_graph=True``, where the graph keeps the ``dZ_l`` alive.
    The derivative of ``dL/dparams`` and a third order raise.  Without it (the default) differentiating the gradients again
    raises ``NotImplementedError``.

    ``bias=True`` and ``skip_layer=`` make it the reference's own ``MLP`` class (ref: examples/radiance_fields/mlp.py), in
    the same launches.  ``bias``: every layer ``l`` has a float32 bias ``b_l [out_l]``, ``z_l = b_l + W_l in_l``; the bias is
    never rounded to ``dtype`` (it is the float32 value the layer's sum starts from) and ``dL/db_l = sum_p dZ_l[p]`` is float32,
    without atomics.  ``skip_layer``: the reference's rule, after hidden layer ``i`` with ``i > 0 and i % skip_layer == 0`` the
    network input is appended, ``in_{i+1} = cat([H_i, x])`` in this column order, and the next matrix (which may be the output
    matrix) is ``[out, n_neurons + n_input_dims]``; a ``skip_layer`` that selects no layer is the plain chain bit for bit.
    ``params`` then holds all matrices in layer order, each ``[out, in_l]`` row-major, and behind them all biases in layer
    order, initialised to zero (:meth:`bias` is a view of one); without either argument offsets, random draws and values are
    unchanged, and Xavier uses each matrix's true fan-in.  With the second order ``T_l`` at such a layer sees ``[T_{l-1}, v]``,
    and the gradient of ``<v, dL/dx>`` towards the biases is exactly zero (the bias segment of the flat gradient).
    Limits besides those above: with a skip ``n_input_dims + n_neurons <= 256`` (what the weight gradient stages for one
    layer), and the LDS budget counts the longer images and, for the forward pass, ``(n_hidden_layers n_neurons + 32) * 4``
    bytes of biases.  :func:`reference_mlp` builds the module from the reference's argument names and
    :meth:`load_reference_state_dict` takes its state dict.

    ``activation`` (all hidden layers) and ``output_activation``: tiny-cuda-nn's ``None``, ``ReLU``, ``LeakyReLU`` (slope
    0.01), ``Sigmoid``, ``Tanh``, ``Softplus`` (``max(z, 0) + log1p(exp(-beta |z|)) / beta`` with ``beta = activation_beta``:
    10 is tiny-cuda-nn's constant, NeuS' SDF network uses 100) and ``Exponential``, in the same launches (the ``nfa_mlp_act_*``
    entries; the default pair calls the entries it always called).  ``Sine`` and ``Squareplus`` raise ``ValueError``.  The
    activation is evaluated in float32 and rounded once to ``dtype``; every derivative is formed from the stored, rounded
    activation (Sigmoid ``y (1 - y)``, Tanh ``1 - y^2``, Softplus ``1 - exp(-beta y)``, Exponential ``y``), as tiny-cuda-nn's
    fused network forms it, so the forward hands ``y`` to the backward when there is an output activation.  With
    ``second_order=True`` and Sigmoid, Tanh, Softplus or Exponential anywhere, the tangent pass also writes the cotangents
    ``R_l = (f''/f')(H_l) dZ_l A_l`` that the activation's second derivative puts into every layer, the curvature pass (the data
    gradient's chain with ``R_l`` injected) turns them into ``E_l`` and the gradient of ``<v, dL/dx>`` towards ``x``, and the
    gradient towards the masters is the weight gradient pass run twice, on ``(v, T, dZ)`` and on ``(x, H, E)``: the two float32
    results are added with one torch add of two ``P``-vectors, the only torch pass; the bias segment is then ``sum_p E_l[p]``,
    no longer zero.
    """

    def __init__(self, n_input_dims: int, n_output_dims: int, n_neurons: int = 64, n_hidden_layers: int = 2,
                 dtype: torch.dtype = torch.float16, out_dtype: Optional[torch.dtype] = None,
                 generator: Optional[torch.Generator] = None, second_order: bool = False, bias: bool = False,
                 skip_layer: Optional[int] = None, activation: str = "ReLU", output_activation: str = "None",
                 activation_beta: float = 10.0):
        super().__init__()
        activation = check_activation("FusedMLP", "activation", activation)
        output_activation = check_activation("FusedMLP", "output_activation", output_activation)
        if not (isinstance(activation_beta, (int, float)) and activation_beta > 0 and math.isfinite(activation_beta)):
            raise ValueError(f"FusedMLP: activation_beta {activation_beta!r}: a positive number (Softplus' beta)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"FusedMLP: dtype {dtype}: torch.float16 or torch.bfloat16")
        if out_dtype not in (None, dtype, torch.float32):
            raise ValueError(f"FusedMLP: out_dtype {out_dtype}: None, dtype ({dtype}) or torch.float32")
        if n_neurons not in WIDTHS:
            raise ValueError(f"FusedMLP: n_neurons {n_neurons}: one of {WIDTHS} (wider networks stay torch)")
        if not 1 <= n_hidden_layers <= MAX_HIDDEN_LAYERS:
            raise ValueError(f"FusedMLP: n_hidden_layers {n_hidden_layers}: 1 to {MAX_HIDDEN_LAYERS}")
        if not 1 <= n_input_dims <= MAX_INPUT_DIMS:
            raise ValueError(f"FusedMLP: n_input_dims {n_input_dims}: 1 to {MAX_INPUT_DIMS}")
        if not 1 <= n_output_dims <= MAX_OUTPUT_DIMS:
            raise ValueError(f"FusedMLP: n_output_dims {n_output_dims}: 1 to {MAX_OUTPUT_DIMS}")
        if skip_layer is not None and not (isinstance(skip_layer, int) and skip_layer >= 1):
            raise ValueError(f"FusedMLP: skip_layer {skip_layer!r}: None or a positive integer")
        skip_mask = skip_mask_of(skip_layer, n_hidden_layers)
        if skip_mask and n_input_dims + n_neurons > MAX_CAT_DIMS:
            raise ValueError(f"FusedMLP: n_input_dims {n_input_dims} + n_neurons {n_neurons} = {n_input_dims + n_neurons}: a layer that "
                             f"takes [H, x] (skip_layer {skip_layer}) holds at most {MAX_CAT_DIMS} inputs")
        fwd, bwd = image_elems(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, skip_mask)
        bias_bytes = lds_bias_bytes(n_neurons, n_hidden_layers, bool(bias))
        if max(fwd * 2 + bias_bytes, bwd * 2) + STAGE_BYTES > LDS_BUDGET:
            raise ValueError(f"FusedMLP: the packed weights do not fit the LDS: forward image {fwd * 2} B"
                             + (f" with {bias_bytes} B of biases" if bias else "") + f", backward image {bwd * 2} B, "
                             f"each with {STAGE_BYTES} B of store staging, against {LDS_BUDGET} B per compute unit "
                             f"(n_input_dims {n_input_dims}, n_output_dims {n_output_dims}, n_neurons {n_neurons}, "
                             f"n_hidden_layers {n_hidden_layers}" + (f", bias {bool(bias)}, skip_layer {skip_layer}" if bias or skip_mask else "")
                             + ")")
        self._setup(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, dtype, out_dtype, generator, second_order, bias,
                    skip_layer, skip_mask, (fwd, bwd), (activation, output_activation, float(activation_beta)))

    _NAME = "FusedMLP"

    def _entry(self, name: str) -> str:
        """The C entry of a pass of a network with a descriptor."""
        return "nfa_mlp_net_" + name

    _slices = staticmethod(wgrad_slices)

    def _setup(self, n_input_dims, n_output_dims, n_neurons, n_hidden_layers, dtype, out_dtype, generator, second_order, bias,
               skip_layer, skip_mask, image_elems_, act: tuple = DEFAULT_ACT) -> None:
        """The module's state and its initial parameters, once the constructor has accepted the configuration."""
        fwd, bwd = image_elems_
        self.activation, self.output_activation, self.activation_beta = act
        self._act_names = act
        self._out_act = act[1] != "None"                                   # the backward needs y
        self._curved = act[0] in CURVED_ACTIVATIONS or act[1] in CURVED_ACTIVATIONS   # the second order has a curvature pass
        self.n_input_dims, self.n_output_dims = n_input_dims, n_output_dims
        self.n_neurons, self.n_hidden_layers = n_neurons, n_hidden_layers
        self.dtype, self.out_dtype = dtype, out_dtype or dtype
        self.second_order = bool(second_order)
        self.bias_enabled, self.skip_layer, self.skip_mask = bool(bias), skip_layer, skip_mask
        self._shape = (n_input_dims, n_output_dims, n_neurons, n_hidden_layers)
        self._dims = layer_dims(*self._shape, skip_mask)
        self._offsets = [0]   # of the matrices; the last one is where the biases start
        for o, i in self._dims:
            self._offsets.append(self._offsets[-1] + o * i)
        self._bias_offsets = [self._offsets[-1]]
        for o, _ in self._dims:
            self._bias_offsets.append(self._bias_offsets[-1] + (o if self.bias_enabled else 0))
        self._image_elems = (fwd, bwd)
        self._packed = None   # (key, forward image, backward image)
        if generator is None:
            generator = torch.Generator().manual_seed(1337)
        init = []
        for o, i in self._dims:
            bound = math.sqrt(6.0 / (i + o))
            init.append((torch.rand(o * i, generator=generator, dtype=torch.float32) * 2.0 - 1.0) * bound)
        if self.bias_enabled:
            init.append(torch.zeros(self._bias_offsets[-1] - self._offsets[-1]))
        self.params = nn.Parameter(torch.cat(init))

    @property
    def n_layers(self) -> int:
        return self.n_hidden_layers + 1

    def _views(self, params: Tensor) -> List[Tensor]:
        return [params[self._offsets[l]:self._offsets[l + 1]].view(*self._dims[l]) for l in range(self.n_layers)]

    def _bias_views(self, params: Tensor) -> Optional[List[Tensor]]:
        if not self.bias_enabled:
            return None
        return [params[self._bias_offsets[l]:self._bias_offsets[l + 1]] for l in range(self.n_layers)]

    def _bias_ptr(self, params: Tensor) -> Optional[int]:
        return params.data_ptr() + 4 * self._offsets[-1] if self.bias_enabled else None

    @property
    def _desc(self) -> "B.MLPDesc":
        """struct nfa_mlp_desc of this network (built once; not part of the module's state)."""
        d = self.__dict__.get("_desc_cache")
        if d is None:
            d = self.__dict__["_desc_cache"] = B.MLPDesc(*self._shape, int(self.bias_enabled), self.skip_mask)
        return d

    @property
    def _plain(self) -> bool:
        """No bias and no skip: the network of the ``nfa_mlp_*`` entries, which such a module keeps calling (the
        ``nfa_mlp_net_*`` entries with ``bias = 0, skip_mask = 0`` are the same passes)."""
        return not self.bias_enabled and self.skip_mask == 0 and self._act is None

    @property
    def _act(self) -> Optional["B.MLPAct"]:
        """struct nfa_mlp_act of this network, or None for the default pair (ReLU, None), whose module calls the entries
        without activations."""
        if self._act_names[:2] == DEFAULT_ACT[:2]:
            return None
        a = self.__dict__.get("_act_cache")
        if a is None:
            a = self.__dict__["_act_cache"] = B.MLPAct(B.ACT_CODES[self.activation], B.ACT_CODES[self.output_activation], self.activation_beta)
        return a

    def _weight_gradient(self, elem, x, hidden, dz, dz_out, N, partials, g_p, zero_bias: bool) -> None:
        """dW (and db) on ``(x, hidden)``, or the second order's on ``(v, tangent)``, whose bias segment is zero."""
        if self._plain:
            B.call("nfa_mlp_bwd_weights", elem, B.ptr(x), B.ELEM_CODES[x.dtype], B.ptr(hidden), B.ptr(dz), B.ptr(dz_out), N,
                   *self._shape, B.ptr(partials), partials.numel(), B.ptr(g_p), B.stream())
        else:
            B.call(self._entry("bwd_weights"), elem, self._desc, B.ptr(x), B.ELEM_CODES[x.dtype], B.ptr(hidden), B.ptr(dz),
                   B.ptr(dz_out), N, B.ptr(partials), partials.numel(), B.ptr(g_p), int(zero_bias), B.stream())

    def weight(self, l: int) -> Tensor:
        """The view ``[out_l, in_l]`` of matrix ``l`` in ``params``."""
        return self._views(self.params)[l]

    def bias(self, l: int) -> Tensor:
        """The view ``[out_l]`` of bias ``l`` in ``params`` (a module with ``bias=True``)."""
        if not self.bias_enabled:
            raise ValueError(f"{self._NAME}: this module has no biases (bias=False)")
        return self._bias_views(self.params)[l]

    def linear_weights(self) -> List[Tensor]:
        """Copies of the matrices, for ``nn.Linear.weight``."""
        return [w.detach().clone() for w in self._views(self.params)]

    def linear_biases(self) -> List[Tensor]:
        """Copies of the biases, for ``nn.Linear(bias=True).bias``."""
        return [b.detach().clone() for b in (self._bias_views(self.params) or [])]

    @torch.no_grad()
    def load_linear_weights(self, weights: Sequence[Tensor], biases: Optional[Sequence[Tensor]] = None) -> None:
        if len(weights) != self.n_layers:
            raise ValueError(f"{self._NAME}: {len(weights)} matrices for {self.n_layers} layers")
        if biases is not None and not self.bias_enabled:
            raise ValueError(f"{self._NAME}: biases given to a module without biases (bias=False)")
        if biases is not None and len(biases) != self.n_layers:
            raise ValueError(f"{self._NAME}: {len(biases)} biases for {self.n_layers} layers")
        for l, (w, v) in enumerate(zip(weights, self._views(self.params))):
            if tuple(w.shape) != tuple(v.shape):
                raise ValueError(f"{self._NAME}: matrix {l} is {tuple(w.shape)}, expected {tuple(v.shape)}")
        for l, (b, v) in enumerate(zip(biases or [], self._bias_views(self.params) or [])):
            if tuple(b.shape) != tuple(v.shape):
                raise ValueError(f"{self._NAME}: bias {l} is {tuple(b.shape)}, expected {tuple(v.shape)}")
        for w, v in zip(weights, self._views(self.params)):
            v.copy_(w)
        for b, v in zip(biases or [], self._bias_views(self.params) or []):
            v.copy_(b)

    def load_reference_state_dict(self, sd: dict) -> None:
        """Takes the state dict of the reference's ``MLP`` (ref: examples/radiance_fields/mlp.py): ``hidden_layers.{i}.weight``,
        ``output_layer.weight`` and, for a module with biases, the ``.bias`` keys beside them.  Any other key, a missing key and
        a wrong shape raise ``ValueError``."""
        names = [f"hidden_layers.{i}" for i in range(self.n_hidden_layers)] + ["output_layer"]
        want = {n + ".weight" for n in names} | ({n + ".bias" for n in names} if self.bias_enabled else set())
        if set(sd) != want:
            raise ValueError(f"{self._NAME}: load_reference_state_dict: missing keys {sorted(want - set(sd))}, unexpected keys "
                             f"{sorted(set(sd) - want)}")
        self.load_linear_weights([sd[n + ".weight"] for n in names], [sd[n + ".bias"] for n in names] if self.bias_enabled else None)

    def _images(self, params: Tensor):
        """The packed images of the current masters: one small launch per change of ``params``."""
        key = (params.data_ptr(), params._version, params.device)
        if self._packed is None or self._packed[0] != key:
            fwd = torch.empty(self._image_elems[0], dtype=self.dtype, device=params.device)
            bwd = torch.empty(self._image_elems[1], dtype=self.dtype, device=params.device)
            with torch.cuda.device(params.device):
                if self._plain:
                    B.call("nfa_mlp_pack_weights", B.ELEM_CODES[self.dtype], B.ptr(params), *self._shape, B.ptr(fwd), fwd.numel(),
                           B.ptr(bwd), bwd.numel(), B.stream())
                else:
                    B.call(self._entry("pack_weights"), B.ELEM_CODES[self.dtype], self._desc, B.ptr(params), B.ptr(fwd), fwd.numel(),
                           B.ptr(bwd), bwd.numel(), B.stream())
            self._packed = (key, fwd, bwd)
        return self._packed[1], self._packed[2]

    def forward(self, x: Tensor) -> Tensor:
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise ValueError(f"{self._NAME}: x must be [N, {self.n_input_dims}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, self.dtype):
            raise TypeError(f"{self._NAME}: x is {x.dtype}: torch.float32 or the network's {self.dtype}")
        with torch.autocast(x.device.type, enabled=False):
            return _MLPFn.apply(x.contiguous(), self.params.float().contiguous(), self)

    def extra_repr(self) -> str:
        return (f"{self.n_input_dims} -> {' -> '.join([str(self.n_neurons)] * self.n_hidden_layers)} -> {self.n_output_dims}, "
                f"dtype={self.dtype}, out_dtype={self.out_dtype}" + (", second_order=True" if self.second_order else "")
                + (", bias=True" if self.bias_enabled else "") + (f", skip_layer={self.skip_layer}" if self.skip_layer is not None else "")
                + (f", activation={self.activation}, output_activation={self.output_activation}"
                   + (f", activation_beta={self.activation_beta:g}" if "Softplus" in self._act_names[:2] else "") if self._act is not None else ""))


_TCNN_KEYS = ("otype", "activation", "output_activation", "n_neurons", "n_hidden_layers")


def mlp_from_tcnn_config(n_input_dims: int, n_output_dims: int, config: dict, dtype: torch.dtype = torch.float16,
                         out_dtype: Optional[torch.dtype] = None, generator: Optional[torch.Generator] = None,
                         second_order: bool = False, activations: bool = False, activation_beta: float = 10.0) -> FusedMLP:
    """A :class:`FusedMLP` from a tiny-cuda-nn network config: ``{"otype": "FullyFusedMLP", "activation": "ReLU",
    "output_activation": "None", "n_neurons": 64 | 128, "n_hidden_layers": 1..4}``.  Anything else raises ``ValueError``
    with the offending key in the message (defaults are tcnn's: 128 neurons, 5 hidden layers, so give both).  With
    ``activations=True`` the keys ``activation`` and ``output_activation`` take tiny-cuda-nn's names ``None``, ``ReLU``,
    ``LeakyReLU``, ``Sigmoid``, ``Tanh``, ``Softplus`` (``activation_beta``: tcnn's constant 10), ``Exponential``; ``Sine`` and
    ``Squareplus`` raise."""
    for k in config:
        if k not in _TCNN_KEYS:
            raise ValueError(f"mlp_from_tcnn_config: key '{k}' is not supported (supported: {', '.join(_TCNN_KEYS)})")
    for k, want, default in (("otype", "FullyFusedMLP", "FullyFusedMLP"), ("activation", "ReLU", "ReLU"),
                             ("output_activation", "None", "None")):
        if activations and k != "otype":
            check_activation("mlp_from_tcnn_config", f"'{k}':", config.get(k, default))
        elif config.get(k, default) != want:
            raise ValueError(f"mlp_from_tcnn_config: '{k}': {config.get(k)!r} is not supported, only {want!r}")
    n_neurons, n_hidden = config.get("n_neurons", 128), config.get("n_hidden_layers", 5)
    if n_neurons not in WIDTHS:
        raise ValueError(f"mlp_from_tcnn_config: 'n_neurons': {n_neurons!r} is not supported, one of {WIDTHS}")
    if not (isinstance(n_hidden, int) and 1 <= n_hidden <= MAX_HIDDEN_LAYERS):
        raise ValueError(f"mlp_from_tcnn_config: 'n_hidden_layers': {n_hidden!r} is not supported, 1 to {MAX_HIDDEN_LAYERS}")
    act = dict(activation=config.get("activation", "ReLU"), output_activation=config.get("output_activation", "None"),
               activation_beta=activation_beta) if activations else {}
    return FusedMLP(n_input_dims, n_output_dims, n_neurons, n_hidden, dtype=dtype, out_dtype=out_dtype, generator=generator,
                    second_order=second_order, **act)


def reference_mlp(input_dim: int, output_dim: int, net_depth: int = 4, net_width: int = 64, skip_layer: Optional[int] = 4,
                  bias_enabled: bool = True, dtype: torch.dtype = torch.float16, out_dtype: Optional[torch.dtype] = None,
                  generator: Optional[torch.Generator] = None, second_order: bool = False, output_enabled: bool = True,
                  hidden_activation: str = "ReLU", output_activation: str = "None") -> FusedMLP:
    """A :class:`FusedMLP` from the argument names of the reference's ``MLP`` (ref: examples/radiance_fields/mlp.py:14-29):
    ``net_depth`` is ``n_hidden_layers``, ``net_width`` is ``n_neurons``.  What the kernels do not hold raises ``ValueError``
    naming the argument: ``net_depth`` 0 or above 4, ``net_width`` other than 64 or 128, ``output_enabled=False``, a hidden
    activation other than ReLU, an output activation (those live in :func:`nerfacc_amd.rendering_from_raw`).  The defaults of
    depth and width are NOT the reference's (8 x 256, which this class does not hold: that network is :class:`StreamedMLP` /
    :class:`NerfMLP`): give both."""
    if not (isinstance(net_depth, int) and 1 <= net_depth <= MAX_HIDDEN_LAYERS):
        raise ValueError(f"reference_mlp: 'net_depth': {net_depth!r} is not supported, 1 to {MAX_HIDDEN_LAYERS}")
    if net_width not in WIDTHS:
        raise ValueError(f"reference_mlp: 'net_width': {net_width!r} is not supported, one of {WIDTHS}")
    if not output_enabled:
        raise ValueError("reference_mlp: 'output_enabled': False is not supported (the network ends in its output layer)")
    if hidden_activation != "ReLU":
        raise ValueError(f"reference_mlp: 'hidden_activation': {hidden_activation!r} is not supported, only 'ReLU'")
    if output_activation not in ("None", None):
        raise ValueError(f"reference_mlp: 'output_activation': {output_activation!r} is not supported, only 'None'")
    return FusedMLP(input_dim, output_dim, net_width, net_depth, dtype=dtype, out_dtype=out_dtype, generator=generator,
                    second_order=second_order, bias=bias_enabled, skip_layer=skip_layer)


# ---------------------------------------------------------------- streamed weights (csrc/mlp_stream.hip)

STREAM_WIDTHS = (128, 256)
STREAM_MAX_HIDDEN_LAYERS = 8
STREAM_MAX_INPUT_DIMS = 320
STREAM_MAX_OUTPUT_DIMS = 288
# include/nerfacc_hip.h: NFA_MLP_STREAM_POINTS, NFA_MLP_STREAM_GROUPS, NFA_MLP_STREAM_WGRAD_MIN_SLICE, NFA_MLP_STREAM_WGRAD_MAX_SLICES
STREAM_POINTS = 128              # points a workgroup carries through one pass of the image
STREAM_GROUPS = 256              # workgroups of a fused pass at most: the persistent grid
STREAM_WGRAD_MIN_SLICE = 256
STREAM_WGRAD_MAX_SLICES = 16
STREAM_SLOTS = 2                 # csrc/mlp_stream.hip: ST_SLOTS
STREAM_TABLE_BYTES = 160 * 8     # the piece table (ST_MAX_PIECES entries)


def stream_wgrad_slices(n_points: int) -> int:
    """Slices the streamed weight gradient cuts ``n_points`` into (include/nerfacc_hip.h: nfa_mlp_stream_bwd_weights):
    ``clamp(ceil(n_points / 256), 1, 16)`` slices of a length rounded up to 64 points, those that are not empty."""
    s = min(max(_cdiv(n_points, STREAM_WGRAD_MIN_SLICE), 1), STREAM_WGRAD_MAX_SLICES)
    slice_len = _cdiv(_cdiv(n_points, s), 64) * 64
    return _cdiv(n_points, slice_len)


def stream_piece_bytes(n_in: int, n_out: int, width: int, n_hidden: int, skip_mask: int = 0) -> int:
    """Bytes of the largest piece (one row tile of one layer: 32 rows x all its k-steps, 1 KiB each) of either image."""
    dims = layer_dims(n_in, n_out, width, n_hidden, skip_mask)
    fwd = [_cdiv(width, 16) + _cdiv(n_in, 16) if (skip_mask >> l) & 1 else _cdiv(i, 16) for l, (o, i) in enumerate(dims)]
    bwd = [_cdiv(o, 16) for o, i in dims]
    return max(fwd + bwd) * 1024


def stream_bias_bytes(n_out: int, width: int, n_hidden: int, bias: int) -> int:
    """Bytes of the float32 biases as the streamed forward pass holds them in LDS (the output layer padded to whole row tiles)."""
    return (n_hidden * width + _cdiv(n_out, 32) * 32) * 4 if bias else 0


def stream_lds_bytes(n_in: int, n_out: int, width: int, n_hidden: int, bias: int, skip_mask: int = 0) -> int:
    """LDS of a streamed fused pass at most: the ring, the store staging, the piece table and the forward's biases."""
    return (STREAM_SLOTS * stream_piece_bytes(n_in, n_out, width, n_hidden, skip_mask) + STAGE_BYTES + STREAM_TABLE_BYTES
            + stream_bias_bytes(n_out, width, n_hidden, bias))


def stream_limits_error(n_in: int, n_out: int, width: int, n_hidden: int, bias: int, skip_mask: int) -> Optional[str]:
    """What csrc/mlp_stream.hip's check_stream_shape refuses, in its order; None for a network the streamed passes hold."""
    if width not in STREAM_WIDTHS:
        return f"width {width}: 128 or 256 neurons are supported"
    if not 1 <= n_hidden <= STREAM_MAX_HIDDEN_LAYERS:
        return f"n_hidden {n_hidden}: 1 to {STREAM_MAX_HIDDEN_LAYERS} hidden layers are supported"
    if not 1 <= n_in <= STREAM_MAX_INPUT_DIMS:
        return f"n_in {n_in}: 1 to {STREAM_MAX_INPUT_DIMS} input features are supported"
    if not 1 <= n_out <= STREAM_MAX_OUTPUT_DIMS:
        return f"n_out {n_out}: 1 to {STREAM_MAX_OUTPUT_DIMS} outputs are supported"
    if bias not in (0, 1):
        return f"bias {bias}: 0 or 1"
    if skip_mask & ~((2 << n_hidden) - 4):
        return (f"skip_mask 0x{skip_mask:x}: only bits 2 to n_hidden ({n_hidden}) may be set: layer 0 takes x itself and layer 1 "
                "follows it")
    piece = stream_piece_bytes(n_in, n_out, width, n_hidden, skip_mask)
    lds = stream_lds_bytes(n_in, n_out, width, n_hidden, bias, skip_mask)
    if lds > LDS_BUDGET:
        return (f"the ring does not fit the LDS: {STREAM_SLOTS} slots of the largest piece ({piece} B) with {STAGE_BYTES} B of store "
                f"staging, {STREAM_TABLE_BYTES} B of piece table and {stream_bias_bytes(n_out, width, n_hidden, bias)} B of biases are "
                f"{lds} B, against {LDS_BUDGET} B per compute unit (n_in {n_in}, "
                f"n_out {n_out}, width {width}, n_hidden {n_hidden}, bias {bias}, skip_mask 0x{skip_mask:x})")
    return None


def refuse_activations(who: str, activation, output_activation, activation_beta) -> None:
    """The streamed kernels hold ReLU hidden layers and no output activation only."""
    if (activation, output_activation if output_activation is not None else "None", activation_beta) != DEFAULT_ACT:
        raise ValueError(f"{who}: activation {activation!r}, output_activation {output_activation!r}, activation_beta {activation_beta!r}: "
                         "the streamed network holds only 'ReLU', 'None' and 10.0 (other activations: FusedMLP, up to 128 neurons)")


class StreamedMLP(FusedMLP):
    """:class:`FusedMLP` for the networks it refuses: 128 or 256 neurons, 1..8 hidden layers, ``n_input_dims`` 1..320,
    ``n_output_dims`` 1..288, biases and the reference's skip rule (``skip_layer``; no limit on ``n_input_dims + n_neurons``).
    NeRF's trunk is ``StreamedMLP(63, 257, 256, 8, skip_layer=4)``.

    The contract is :class:`FusedMLP`'s, word for word: one flat float32 ``params`` (all matrices, then all biases), the same
    accessors and loaders, Xavier per matrix with its true fan-in and zero biases, float32 or ``dtype`` ``x``, ``dtype`` or
    float32 ``y``, ``dL/dx`` in ``x``'s dtype, ``dL/dparams`` float32 without atomics (the same bits on every run),
    ``torch.autocast`` changes nothing, the packed images are rebuilt when ``params`` changes, ``N = 0`` works, CPU tensors
    take the torch restatement.  Arithmetic and rounding points are the same too; a 128-wide network that both classes hold
    gives the same bits for ``y`` and ``dL/dx``.

    What differs is the kernels (csrc/mlp_stream.hip): the packed weights stay in global memory and pass through the LDS one
    32-row tile of one layer at a time, through a ring of two slots, while a workgroup's 128 points wait in registers; the
    weight gradient runs on a grid (point slice, layer, 128 x 128 tile of the matrix) with at most 16 slices
    (:func:`stream_wgrad_slices`).  There is no second order: differentiating the gradients again raises
    ``NotImplementedError`` (NeRF has no Eikonal term).
    """

    _NAME = "StreamedMLP"
    _slices = staticmethod(stream_wgrad_slices)

    def __init__(self, n_input_dims: int, n_output_dims: int, n_neurons: int = 256, n_hidden_layers: int = 8,
                 dtype: torch.dtype = torch.float16, out_dtype: Optional[torch.dtype] = None,
                 generator: Optional[torch.Generator] = None, bias: bool = True, skip_layer: Optional[int] = 4,
                 activation: str = "ReLU", output_activation: str = "None", activation_beta: float = 10.0):
        nn.Module.__init__(self)
        refuse_activations("StreamedMLP", activation, output_activation, activation_beta)
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"StreamedMLP: dtype {dtype}: torch.float16 or torch.bfloat16")
        if out_dtype not in (None, dtype, torch.float32):
            raise ValueError(f"StreamedMLP: out_dtype {out_dtype}: None, dtype ({dtype}) or torch.float32")
        if skip_layer is not None and not (isinstance(skip_layer, int) and skip_layer >= 1):
            raise ValueError(f"StreamedMLP: skip_layer {skip_layer!r}: None or a positive integer")
        for name, v in (("n_input_dims", n_input_dims), ("n_output_dims", n_output_dims), ("n_neurons", n_neurons),
                        ("n_hidden_layers", n_hidden_layers)):
            if not isinstance(v, int):
                raise ValueError(f"StreamedMLP: {name} {v!r}: an integer")
        skip_mask = skip_mask_of(skip_layer, n_hidden_layers) if 1 <= n_hidden_layers <= STREAM_MAX_HIDDEN_LAYERS else 0
        err = stream_limits_error(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, int(bool(bias)), skip_mask)
        if err:
            raise ValueError("StreamedMLP: " + err)
        self._setup(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, dtype, out_dtype, generator, False, bias, skip_layer,
                    skip_mask, image_elems(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, skip_mask))

    def _entry(self, name: str) -> str:
        return "nfa_mlp_stream_" + name

    @property
    def _plain(self) -> bool:
        return False   # the streamed entries all take the descriptor


class NerfMLP(nn.Module):
    """The reference's ``NerfMLP`` (ref: examples/radiance_fields/mlp.py:114-165), the network of its vanilla NeRF and T-NeRF
    fields, as two :class:`StreamedMLP`: ``forward(x, condition=None) -> (raw_rgb, raw_sigma)`` and ``query_density(x)``.

    ``trunk``: the reference's ``base`` (``net_depth`` x ``net_width``, biases, the input appended after every hidden layer
    ``i > 0`` with ``i % skip_layer == 0``) with ONE merged output matrix in the place of the linear layers that read its
    output.  With a condition (``condition_dim > 0``) rows ``0 .. net_width-1`` are ``bottleneck_layer`` and row
    ``net_width`` is ``sigma_layer``; without one rows 0..2 are the colour layer and row 3 is ``sigma_layer``.  These are
    linear maps of the same vector, so merging them is exact; if the base ends in ``cat([H, x])``, the merged layer is a cat
    output layer.  Each block of rows is initialised with its own Xavier fan, as the reference's separate layers are.
    ``head`` (with a condition): ``StreamedMLP(net_width + condition_dim, 3, net_width_condition, net_depth_condition)``
    without a skip, applied to ``cat([bottleneck, condition])``.

    A ``condition`` of one row per ray is broadcast over ``x``'s middle dimensions as the reference does.  Outputs are
    ``dtype``.  What stays torch, on purpose: the split of the trunk's output, the cat with the condition, and their
    backward; and ``query_density`` runs the whole merged output layer (about an eighth more work than sigma alone needs).
    :meth:`load_reference_state_dict` takes the reference module's state dict.
    """

    def __init__(self, input_dim: int, condition_dim: int, net_depth: int = 8, net_width: int = 256, skip_layer: Optional[int] = 4,
                 net_depth_condition: int = 1, net_width_condition: int = 128, dtype: torch.dtype = torch.float16,
                 generator: Optional[torch.Generator] = None, activation: str = "ReLU", output_activation: str = "None",
                 activation_beta: float = 10.0):
        super().__init__()
        refuse_activations("NerfMLP", activation, output_activation, activation_beta)
        if not (isinstance(condition_dim, int) and condition_dim >= 0):
            raise ValueError(f"NerfMLP: condition_dim {condition_dim!r}: a non-negative integer")
        if generator is None:
            generator = torch.Generator().manual_seed(1337)
        self.input_dim, self.condition_dim, self.net_width = input_dim, condition_dim, net_width
        n_out = net_width + 1 if condition_dim > 0 else 4
        self.trunk = StreamedMLP(input_dim, n_out, net_width, net_depth, dtype=dtype, generator=generator, bias=True,
                                 skip_layer=skip_layer)
        with torch.no_grad():   # the merged output matrix: each block of rows with the fan of the layer it is
            w = self.trunk.weight(net_depth)
            fan_in, r0 = w.shape[1], 0
            for rows in ((net_width, 1) if condition_dim > 0 else (3, 1)):
                bound = math.sqrt(6.0 / (fan_in + rows))
                w[r0:r0 + rows] = (torch.rand(rows, fan_in, generator=generator, dtype=torch.float32) * 2.0 - 1.0) * bound
                r0 += rows
        self.head = None
        if condition_dim > 0:
            self.head = StreamedMLP(net_width + condition_dim, 3, net_width_condition, net_depth_condition, dtype=dtype,
                                    generator=generator, bias=True, skip_layer=None)

    def _trunk(self, x: Tensor) -> Tensor:
        if x.shape[-1] != self.input_dim:
            raise ValueError(f"NerfMLP: x must be [..., {self.input_dim}], got {tuple(x.shape)}")
        return self.trunk(x.reshape(-1, self.input_dim))

    def query_density(self, x: Tensor) -> Tensor:
        row = self.net_width if self.head is not None else 3
        return self._trunk(x)[:, row:row + 1].reshape(*x.shape[:-1], 1)

    def forward(self, x: Tensor, condition: Optional[Tensor] = None):
        if (condition is None) != (self.head is None):
            raise ValueError(f"NerfMLP: condition_dim is {self.condition_dim}: a condition " +
                             ("is required" if condition is None else "cannot be taken"))
        lead = x.shape[:-1]
        y = self._trunk(x)
        if self.head is None:
            return y[:, :3].reshape(*lead, 3), y[:, 3:4].reshape(*lead, 1)
        W = self.net_width
        if condition.shape[:-1] != lead:   # one row per ray, broadcast over the samples (ref: mlp.py:157-161)
            num_rays, n_dim = condition.shape
            condition = condition.view([num_rays] + [1] * (x.dim() - condition.dim()) + [n_dim]).expand(list(lead) + [n_dim])
        if condition.shape[-1] != self.condition_dim:
            raise ValueError(f"NerfMLP: condition must be [..., {self.condition_dim}], got {tuple(condition.shape)}")
        h = torch.cat([y[:, :W], condition.reshape(-1, self.condition_dim).to(y.device)], dim=-1)
        if h.dtype not in (torch.float32, self.head.dtype):
            h = h.float()
        return self.head(h).reshape(*lead, 3), y[:, W:W + 1].reshape(*lead, 1)

    def reference_keys(self) -> List[str]:
        """The keys of the reference module's state dict for this configuration."""
        names = [f"base.hidden_layers.{i}" for i in range(self.trunk.n_hidden_layers)] + ["sigma_layer.output_layer"]
        if self.head is not None:
            names += ["bottleneck_layer.output_layer"] + [f"rgb_layer.hidden_layers.{i}" for i in range(self.head.n_hidden_layers)]
        names += ["rgb_layer.output_layer"]
        return [n + s for n in names for s in (".weight", ".bias")]

    def load_reference_state_dict(self, sd: dict) -> None:
        """Takes the state dict of the reference's ``NerfMLP``: ``base.hidden_layers.{i}.*``, ``sigma_layer.output_layer.*``,
        ``bottleneck_layer.output_layer.*``, ``rgb_layer.hidden_layers.{i}.*``, ``rgb_layer.output_layer.*`` (``.weight`` and
        ``.bias`` each).  Any other key, a missing key and a wrong shape raise ``ValueError``."""
        want = set(self.reference_keys())
        if set(sd) != want:
            raise ValueError(f"NerfMLP: load_reference_state_dict: missing keys {sorted(want - set(sd))}, unexpected keys "
                             f"{sorted(set(sd) - want)}")
        D = self.trunk.n_hidden_layers
        first = "bottleneck_layer.output_layer" if self.head is not None else "rgb_layer.output_layer"
        for suffix, dim in ((".weight", 2), (".bias", 1)):
            for k in (first + suffix, "sigma_layer.output_layer" + suffix):
                if sd[k].dim() != dim or (dim == 2 and sd[k].shape[1] != self.trunk._dims[D][1]):
                    raise ValueError(f"NerfMLP: load_reference_state_dict: '{k}' is {tuple(sd[k].shape)}")
        merged = lambda s: torch.cat([sd[first + s], sd["sigma_layer.output_layer" + s]], dim=0)
        self.trunk.load_linear_weights([sd[f"base.hidden_layers.{i}.weight"] for i in range(D)] + [merged(".weight")],
                                       [sd[f"base.hidden_layers.{i}.bias"] for i in range(D)] + [merged(".bias")])
        if self.head is not None:
            self.head.load_reference_state_dict({k[len("rgb_layer."):]: v for k, v in sd.items() if k.startswith("rgb_layer.")})

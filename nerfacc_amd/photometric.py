"""The photometric loss: target pixels, loss, its gradient and the MSE (native kernels: csrc/photo.hip).

The target side of a training step, which each of the reference's loaders and trainers runs as torch
(``examples/datasets/nerf_synthetic.py:153,195``, ``nerf_360_v2.py:327``, ``examples/train_ngp_nerf_occ.py:198-208``)::

    rgba   = images[image_id, y, x] / 255.0
    pixels = rgba[:, :3] * alpha + color_bkgd * (1 - alpha)
    loss   = F.smooth_l1_loss(rgb, pixels);  grad_scaler.scale(loss).backward()
    mse    = F.mse_loss(rgb, pixels);        psnr = -10 log10(mse)

about a dozen gather, elementwise and reduction launches.  Here the forward is two launches (the pass over the rays and the
one-wave end of its reduction) and the backward one; the gradient that arrives at the loss -- the loss scale of
``DeviceGradScaler.scale`` -- is read on the device, so scaling costs no launch.  Nothing is read back, nothing is allocated
outside torch: the path captures into a graph (DESIGN.md "Photometric loss").

Not part of ``nerfacc_amd.__all__`` (that list mirrors the reference's exactly); import the module.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Union

import numpy as np
import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B

__all__ = ["target_pixels", "photometric_loss", "psnr", "PhotometricOutput", "KINDS", "reduction_chunk"]

PhotometricOutput = namedtuple("PhotometricOutput", ("loss", "mse", "pixels", "per_ray"))

# include/nerfacc_hip.h: NFA_PHOTO_*
KINDS = {"l1": 0, "l2": 1, "smooth_l1": 2, "huber": 3, "relative_l2": 4, "charbonnier": 5}
_INDEX_CODES = {torch.int32: 1, torch.int64: 2}


_CHUNK = 0


def reduction_chunk() -> int:
    """Rays per partial sum of the forward's reduction."""
    global _CHUNK
    if not _CHUNK:
        _CHUNK = int(B.load().nfa_photometric_chunk())
    return _CHUNK


def _call(dev, name: str, *args) -> None:
    """``B.call`` on ``dev``'s current stream.  The step this belongs to is bound by the host: the device guard is entered only
    when ``dev`` is not the current device already."""
    if B._CUR_DEVICE is not None and B._CUR_DEVICE() == dev.index:
        B.call(name, *args, B.stream())
    else:
        with torch.cuda.device(dev):
            B.call(name, *args, B.stream())


def psnr(mse: Tensor) -> Tensor:
    """``-10 log10(mse)`` as a torch op on the device scalar (no read)."""
    return -10.0 * torch.log10(mse)


# ------------------------------------------------------------------------------------------------ the formulas in torch
def _sign0(d: Tensor) -> Tensor:
    one = torch.ones((), dtype=d.dtype, device=d.device)
    return torch.where(d > 0, one, torch.where(d < 0, -one, d))


def _term_torch(kind: int, param: float, d: Tensor, rgb: Tensor, grad: bool) -> Tensor:
    """csrc/photo.hip's ``loss_term``: the per-element term (``grad``: its derivative in d), operation by operation."""
    P = torch.tensor(param, dtype=d.dtype, device=d.device)
    ad = d.abs()
    if kind == KINDS["l1"]:
        return _sign0(d) if grad else ad
    if kind == KINDS["l2"]:
        return 2.0 * d if grad else d * d
    if kind == KINDS["smooth_l1"]:
        return torch.where(ad < P, d / P, _sign0(d)) if grad else torch.where(ad < P, ((0.5 * d) * d) / P, ad - 0.5 * P)
    if kind == KINDS["huber"]:
        return torch.where(ad <= P, d, P * _sign0(d)) if grad else torch.where(ad <= P, (0.5 * d) * d, P * (ad - 0.5 * P))
    if kind == KINDS["relative_l2"]:
        den = rgb * rgb + 0.01
        return (2.0 * d) / den if grad else (d * d) / den
    # the correctly rounded root, as sqrtf is on the device: torch's vectorised float32 sqrt on the CPU is not (about 0.6 % of
    # arguments come out one ulp off); through float64 it is (53 >= 2 * 24 + 2 bits)
    r = torch.sqrt((d * d + P * P).double()).to(d.dtype)
    return d / r if grad else r


def _target_torch(images, ids, x, y, pixels_in, bkgd, n: int, ct: torch.dtype) -> Tensor:
    """The target of every ray, (n, 3) of dtype ``ct``, with the kernel's clamps and operation order."""
    if images is not None:
        n_images, H, W, C = images.shape
        if x is None:
            flat = images.reshape(-1, C)
            src = flat[torch.arange(n, device=images.device).clamp(max=flat.shape[0] - 1)]
        else:
            i = 0 if ids is None else ids.long().clamp(0, n_images - 1)
            src = images[i, y.long().clamp(0, H - 1), x.long().clamp(0, W - 1)]
        # a true division on every device: by a Python scalar, torch's device kernel multiplies by the reciprocal instead, which
        # gives other bits for 126 of the 256 bytes
        p = src.to(ct) / torch.full((), 255.0, dtype=ct, device=src.device) if images.dtype == torch.uint8 else src.to(ct)
    else:
        p = pixels_in.to(ct)
    if p.shape[-1] == 3 or bkgd is None:
        return p[:, :3].contiguous()
    alpha = p[:, 3:4]
    return p[:, :3] * alpha + bkgd.to(ct) * (1.0 - alpha)


class _PhotometricFn(torch.autograd.Function):
    """``nfa_photometric_fwd`` / ``_bwd`` on flattened inputs, or (``native`` false) the same formulas in torch."""

    @staticmethod
    def forward(ctx, rgb, images, ids, x, y, pixels_in, bkgd, weights, kind, param, want_per_ray, native):
        ctx.set_materialize_grads(False)
        n = rgb.shape[0]
        rgb = rgb.detach()
        if native:
            dev = B.require_device(rgb, images, ids, x, y, pixels_in, bkgd, weights)
            pixels = torch.empty((n, 3), dtype=torch.float32, device=dev)
            per_ray = torch.empty(n, dtype=torch.float32, device=dev) if want_per_ray else None
            if n:
                loss, mse = torch.empty((), dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev)
                _launch_fwd(dev, rgb, images, ids, x, y, pixels_in, bkgd, weights, kind, param, pixels, loss, mse, per_ray)
            else:
                loss, mse = (torch.full((), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
        else:
            ct = torch.float64 if rgb.dtype == torch.float64 else torch.float32
            pixels = _target_torch(images, ids, x, y, pixels_in, bkgd, n, ct)
            r = rgb.to(ct)
            d = r - pixels
            t = _term_torch(kind, param, d, r, grad=False)
            w = None if weights is None else weights.to(ct)
            wt = t if w is None else w[:, None] * t
            loss = (wt.double().sum() / (3 * n)).to(ct) if n else torch.full((), float("nan"), dtype=ct, device=rgb.device)
            mse = ((d * d).double().sum() / (3 * n)).to(ct) if n else torch.full((), float("nan"), dtype=ct, device=rgb.device)
            per_ray = None
            if want_per_ray:
                s = (t[:, 0] + t[:, 1]) + t[:, 2]
                per_ray = (s if w is None else w * s) / 3.0
        ctx.save_for_backward(rgb, pixels, weights)
        ctx.kind, ctx.param, ctx.native = kind, param, native
        ctx.mark_non_differentiable(mse, pixels, *(() if per_ray is None else (per_ray,)))
        return loss, mse, pixels, per_ray

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_mse, g_pixels, g_per_ray):
        none = (None,) * 12
        if g_loss is None or not ctx.needs_input_grad[0]:
            return none
        rgb, pixels, weights = ctx.saved_tensors
        n = rgb.shape[0]
        if ctx.native:
            g = g_loss.to(torch.float32).contiguous()
            g_rgb = torch.empty_like(rgb)
            if n:
                _check_rows(n, rgb=(rgb, 3), pixels=(pixels, 3), weights=(weights, 1), g_rgb=(g_rgb, 3))
                _call(rgb.device, "nfa_photometric_bwd", B.ptr(rgb), B.ELEM_CODES[rgb.dtype], B.ptr(pixels), B.ptr(weights), B.ptr(g), n,
                      ctx.kind, ctx.param, B.ptr(g_rgb))
            return (g_rgb,) + none[1:]
        ct = pixels.dtype
        r = rgb.to(ct)
        dterm = _term_torch(ctx.kind, ctx.param, r - pixels, r, grad=True)
        # inv as the native entry forms it: float32(1) / float32(3 n) (float64 inputs: in float64)
        inv = 1.0 / (3 * n) if ct == torch.float64 else float(np.float32(1.0) / np.float32(3 * n)) if n else 0.0
        g = g_loss.to(ct)
        coef = (g * inv).expand(n) if weights is None else (g * weights.to(ct)) * inv
        return ((coef[:, None] * dterm).to(rgb.dtype),) + none[1:]


def _check_rows(n: int, **arrays) -> None:
    """Every array the kernels index by ray holds exactly n rows of its width: the entries trust these sizes."""
    for name, (t, width) in arrays.items():
        if t is not None and (t.numel() != n * width or not t.is_contiguous()):
            raise RuntimeError(f"nerfacc_amd.photometric: {name} has {t.numel()} elements, the launch needs {n} x {width} contiguous")


def _launch_fwd(dev, rgb, images, ids, x, y, pixels_in, bkgd, weights, kind, param, pixels, loss, mse, per_ray) -> None:
    n = pixels.shape[0]
    shared_bkgd = bkgd is not None and bkgd.shape == (3,)
    _check_rows(n, rgb=(rgb, 3), image_ids=(ids, 1), x=(x, 1), y=(y, 1), pixels_in=(pixels_in, 0 if pixels_in is None else pixels_in.shape[-1]),
                color_bkgd=(None if shared_bkgd else bkgd, 3), weights=(weights, 1), pixels=(pixels, 3), per_ray=(per_ray, 1))
    if images is not None:
        n_images, H, W, C = images.shape
        index_code = _INDEX_CODES[x.dtype] if x is not None else 2
    else:
        n_images, H, W, C, index_code = 0, 0, 0, pixels_in.shape[1], 2
    partials = None
    if rgb is not None:
        chunk = reduction_chunk()
        partials = torch.empty(2 * ((n + chunk - 1) // chunk), dtype=torch.float64, device=dev)
    _call(dev, "nfa_photometric_fwd", B.ptr(rgb), B.ELEM_CODES[rgb.dtype] if rgb is not None else 0, n, B.ptr(images), n_images, H, W,
          B.ptr(ids), B.ptr(x), B.ptr(y), index_code, B.ptr(pixels_in), C, B.ptr(bkgd),
          0 if bkgd is None or shared_bkgd else 3, B.ptr(weights), kind, param, B.ptr(pixels), B.ptr(partials),
          0 if partials is None else partials.numel() // 2, B.ptr(loss), B.ptr(mse), B.ptr(per_ray))


# ------------------------------------------------------------------------------------------------ arguments
def _broadcasts(shape, *shapes) -> bool:
    """Whether every one of ``shapes`` broadcasts to exactly ``shape``."""
    return all(s == shape or (len(s) <= len(shape) and all(a in (1, b) for a, b in zip(reversed(s), reversed(shape)))) for s in shapes)


def _flat(t: Tensor, shape, dtype=None, row=()) -> Tensor:
    """``t`` broadcast to ``shape + row`` as a contiguous ``(n,) + row`` tensor of ``dtype``; as it is where it already is one
    (the usual case, and this code is on a host-bound path)."""
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.shape != shape + row:
        t = t.expand(shape + row)
    if len(shape) != 1:
        t = t.reshape((-1,) + row)
    return t if t.is_contiguous() else t.contiguous()


def _source(lead, pixels, images, image_ids, x, y, color_bkgd):
    """The checked, flattened source: ``(shape, n, images, ids, x, y, pixels_in, bkgd)``.  ``lead`` is the leading shape the
    rays must have (``rgb``'s), or None: the source decides."""
    if (pixels is None) == (images is None):
        raise ValueError("exactly one of pixels and images must be given")
    ids = xs = ys = pixels_in = None
    if pixels is not None:
        if image_ids is not None or x is not None or y is not None:
            raise ValueError("image_ids, x and y go with images, not with pixels")
        if pixels.dim() < 1 or pixels.shape[-1] not in (3, 4) or not pixels.is_floating_point():
            raise ValueError(f"pixels must be floating point (..., 3) or (..., 4), got {pixels.dtype} {tuple(pixels.shape)}")
        shape = tuple(pixels.shape[:-1]) if lead is None else tuple(lead)
        if not _broadcasts(shape, pixels.shape[:-1]):
            raise ValueError(f"pixels {tuple(pixels.shape)} do not broadcast to rays of shape {shape}")
        n_channels = pixels.shape[-1]
        pixels_in = _flat(pixels, shape, None, (n_channels,))
    else:
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if images.dim() != 4 or images.shape[-1] not in (3, 4) or 0 in images.shape:
            raise ValueError(f"images must be (n_images, H, W, 3|4) or (H, W, 3|4), got {tuple(images.shape)}")
        if not (images.dtype == torch.uint8 or images.is_floating_point()):
            raise ValueError(f"images must be uint8 (divided by 255) or floating point (taken as they are), got {images.dtype}")
        n_images, H, W, n_channels = images.shape
        if (x is None) != (y is None):
            raise ValueError("x and y must be given together")
        for t in (image_ids, x, y):
            if isinstance(t, Tensor) and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool):
                raise ValueError("image_ids, x and y must be integer tensors")
        if image_ids is None:
            if n_images > 1:
                raise ValueError(f"image_ids may be None only with one image (there are {n_images})")
        elif not isinstance(image_ids, Tensor):
            image_id = int(image_ids)
            if not 0 <= image_id < n_images:
                raise ValueError(f"image_ids {image_id} is outside the {n_images} images")
            images, n_images, image_ids = images[image_id:image_id + 1], 1, None
        if x is None:
            if image_ids is not None:
                raise ValueError("a tensor of image_ids needs x and y")
            shape = (H, W) if lead is None else tuple(lead)     # every pixel of the image in row-major order
            if math.prod(shape) != H * W:
                raise ValueError(f"rays of shape {shape} against a whole image of {H} x {W} pixels")
        else:
            idx = [t for t in (image_ids, x, y) if t is not None]
            try:
                shape = tuple(torch.broadcast_shapes(*(t.shape for t in idx))) if lead is None else tuple(lead)
            except RuntimeError as e:
                raise ValueError(f"image_ids, x and y do not broadcast against each other: {e}") from None
            if not _broadcasts(shape, *(t.shape for t in idx)):
                raise ValueError(f"image_ids, x and y do not broadcast to rays of shape {shape}")
            dt = idx[0].dtype if all(t.dtype == idx[0].dtype for t in idx) and idx[0].dtype in _INDEX_CODES else torch.int64
            ids, xs, ys = (None if t is None else _flat(t, shape, dt) for t in (image_ids, x, y))
        if not images.is_contiguous():
            images = images.contiguous()
    n = math.prod(shape)
    bkgd = None
    if color_bkgd is not None and n_channels == 4:
        if color_bkgd.shape[-1:] != (3,) or not _broadcasts(shape, color_bkgd.shape[:-1]):
            raise ValueError(f"color_bkgd must be (3,) or broadcast to {shape + (3,)}, got {tuple(color_bkgd.shape)}")
        # one colour for every ray stays a (3,) tensor: its shape is what tells the launch that the row is shared
        bkgd = color_bkgd.reshape(3).contiguous() if color_bkgd.numel() == 3 else _flat(color_bkgd, shape, None, (3,))
    return shape, n, images, ids, xs, ys, pixels_in, bkgd


def _native_source(dev, images, ids, x, y, pixels_in, bkgd, weights) -> bool:
    if dev.type != "cuda" or any(t is not None and t.device != dev for t in (images, ids, x, y, pixels_in, bkgd, weights)):
        return False
    if images is not None and (images.dtype != torch.uint8 or (images.shape[-1] == 4 and images.data_ptr() % 4)):
        return False
    return all(t is None or t.dtype == torch.float32 for t in (pixels_in, bkgd, weights))


def target_pixels(images: Tensor, image_ids: Union[Tensor, int, None] = None, x: Optional[Tensor] = None,
                  y: Optional[Tensor] = None, color_bkgd: Optional[Tensor] = None) -> Tensor:
    """The target pixels of rays: ``images[image_ids, y, x] / 255`` blended with ``color_bkgd`` (see ``photometric_loss``),
    ``(..., 3)`` float32.  With an int ``image_ids`` (or a single image) and no ``x`` / ``y``: every pixel of that image,
    ``(H, W, 3)`` -- the loaders' evaluation branch."""
    shape, n, images, ids, xs, ys, pixels_in, bkgd = _source(None, None, images, image_ids, x, y, color_bkgd)
    dev = images.device
    if bkgd is not None and bkgd.is_floating_point() and bkgd.device == dev:
        bkgd = bkgd.to(torch.float32)
    if _native_source(dev, images, ids, xs, ys, pixels_in, bkgd, None):
        pixels = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n:
            _launch_fwd(dev, None, images, ids, xs, ys, pixels_in, bkgd, None, 0, 0.0, pixels, None, None, None)
    else:
        pixels = _target_torch(images, ids, xs, ys, pixels_in, bkgd, n, torch.float64 if images.dtype == torch.float64 else torch.float32)
    return pixels.view(*shape, 3)


def photometric_loss(
    rgb: Tensor,
    *,
    pixels: Optional[Tensor] = None,
    images: Optional[Tensor] = None,
    image_ids: Union[Tensor, int, None] = None,
    x: Optional[Tensor] = None,
    y: Optional[Tensor] = None,
    color_bkgd: Optional[Tensor] = None,
    kind: str = "smooth_l1",
    beta: float = 1.0,
    weights: Optional[Tensor] = None,
    per_ray: bool = False,
) -> PhotometricOutput:
    """The loss of rendered colours ``rgb`` ``(..., 3)`` against their target pixels, with the MSE from the same pass.

    The target comes from exactly one of

    * ``images``: a stack ``(n_images, H, W, C)`` (or one image ``(H, W, C)``), C = 3 or 4, uint8 (a channel is
      ``byte / 255``, a true division) read at ``(image_ids, y, x)``: integer tensors that broadcast to the rays' shape,
      clamped into the stack.  ``image_ids`` may be a Python int, and with it (or a single image) ``x = y = None`` means every
      pixel of that image in row-major order;
    * ``pixels``: ready ``(..., 3)`` pixels or ``(..., 4)`` rgba.

    With four channels and ``color_bkgd`` (``(3,)`` or ``(..., 3)``) the target is ``p * alpha + color_bkgd * (1 - alpha)``;
    without a background it is the colour channels as they are.  With ``d = rgb - target`` the per-element term is, by
    ``kind`` (``beta`` carries the parameter):

    ==================  ==========================================================  ================================
    ``"l1"``            ``|d|``
    ``"l2"``            ``d * d``
    ``"smooth_l1"``     ``0.5 * d * d / beta`` if ``|d| < beta`` else ``|d| - 0.5 * beta``  (``beta = 0``: ``"l1"``)
    ``"huber"``         ``0.5 * d * d`` if ``|d| <= beta`` else ``beta * (|d| - 0.5 * beta)``
    ``"relative_l2"``   ``d * d / (rgb * rgb + 0.01)``, the denominator a constant for the gradient (instant-ngp)
    ``"charbonnier"``   ``sqrt(d * d + beta * beta)``
    ==================  ==========================================================  ================================

    ``weights`` ``(...)`` multiplies the three terms of a ray; the normaliser stays ``3 N``.

    Returns ``PhotometricOutput(loss, mse, pixels, per_ray)``: ``loss = sum w term / (3 N)`` and ``mse = sum d * d / (3 N)``
    (unweighted; ``psnr(mse)``) as 0-dim tensors, ``pixels (..., 3)`` the target, and with ``per_ray=True`` the error map
    ``w * (t_0 + t_1 + t_2) / 3`` of shape ``(...)`` (else None).  Only ``loss`` is differentiable, and only towards ``rgb``;
    ``mse``, ``pixels`` and ``per_ray`` carry no gradient.

    A CUDA ``rgb`` in float32, fp16 or bf16 with uint8 ``images`` or float32 ``pixels`` runs on libnerfacc_hip.so: two
    launches forward, one backward, float32 arithmetic with every operation rounded on its own, the sums in float64 in a
    fixed order (no atomics: the same bits every run) and rounded to float32 once; ``rgb.grad`` has ``rgb``'s dtype.  The
    gradient arriving at ``loss`` is read on the device, so ``DeviceGradScaler.scale(loss).backward()`` adds no launch, and
    nothing is read back: the path captures into a graph.  Everything else (CPU tensors, float64, floating-point image
    stacks) runs the same formulas in the same order in torch; on CPU float32 tensors the results are those of the native
    path.
    """
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    if rgb.dim() < 1 or rgb.shape[-1] != 3 or not rgb.is_floating_point():
        raise ValueError(f"rgb must be floating point (..., 3), got {rgb.dtype} {tuple(rgb.shape)}")
    param = float(beta)
    if not param >= 0.0:
        raise ValueError(f"beta must be >= 0, got {beta}")
    code = KINDS[kind]
    if kind == "smooth_l1" and param == 0.0:
        code = KINDS["l1"]
    lead = tuple(rgb.shape[:-1])
    shape, n, images, ids, xs, ys, pixels_in, bkgd = _source(lead, pixels, images, image_ids, x, y, color_bkgd)
    if weights is not None:
        if not weights.is_floating_point() or not _broadcasts(shape, weights.shape):
            raise ValueError(f"weights must be floating point and broadcast to {shape}, got {weights.dtype} {tuple(weights.shape)}")
        weights = _flat(weights, shape)
    dev = rgb.device
    native = rgb.dtype in B.ELEM_CODES
    if native and dev.type == "cuda":   # float64 backgrounds and weights next to a float32 rgb: rounded, as rgb's type says
        bkgd = bkgd.to(torch.float32) if bkgd is not None and bkgd.device == dev else bkgd
        weights = weights.to(torch.float32) if weights is not None and weights.device == dev else weights
    native = native and _native_source(dev, images, ids, xs, ys, pixels_in, bkgd, weights)
    loss, mse, target, ray = _PhotometricFn.apply(_flat(rgb, shape, None, (3,)), images, ids, xs, ys, pixels_in, bkgd, weights,
                                                  code, param, bool(per_ray), native)
    if len(shape) != 1:
        target, ray = target.view(*shape, 3), None if ray is None else ray.view(shape)
    return PhotometricOutput(loss, mse, target, ray)

"""OpenCV lens undistortion (ref: nerfacc/cameras.py; native kernels: csrc/camera.hip).

``opencv_lens_undistortion`` / ``opencv_lens_undistortion_fisheye`` run on libnerfacc_hip.so; like the reference's
they are not differentiable.  The three underscore functions are plain torch (they run on any device): the forward
distortion models and a Newton undistortion in torch, which the reference's users take as the forward model and the
reference implementation respectively.

Not part of ``nerfacc_amd.__all__`` (the reference does not export them from its package either); import the module.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _backend as B

__all__ = [
    "opencv_lens_undistortion",
    "opencv_lens_undistortion_fisheye",
    "_opencv_lens_distortion",
    "_opencv_lens_distortion_fisheye",
    "_opencv_lens_undistortion",
]

_OPENCV_COUNTS = (0, 1, 2, 4, 8)


def _pad8(params: Tensor) -> Tensor:
    """{k1}, {k1,k2}, {k1,k2,p1,p2} -> {k1,k2,p1,p2,k3,k4,k5,k6} with zeros."""
    n = params.shape[-1]
    return params if n == 8 else F.pad(params, (0, 8 - n), "constant", 0.0)


def _launch(name: str, uv: Tensor, params: Tensor, eps: float, iters: int) -> Tensor:
    """uv [..., 2] and params [..., P] (P = 8 or 4 here; 5 / 8 / 12 from cuda_compat) on one ROCm device.  A single
    parameter set goes to the kernel once (stride 0); parameters shaped like the batch go per point; any other broadcast
    is expanded here."""
    B.require_device(uv, params)
    if uv.dtype != torch.float32 or params.dtype != torch.float32:
        raise RuntimeError(f"{name}: uv and params must be float32 (got {uv.dtype} and {params.dtype})")
    if uv.shape[-1] != 2:
        raise RuntimeError(f"{name}: uv must have shape [..., 2], got {tuple(uv.shape)}")
    batch, n_params = uv.shape[:-1], params.shape[-1]
    if params.dim() - 1 > len(batch) or torch.broadcast_shapes(params.shape[:-1], batch) != batch:
        raise RuntimeError(f"{name}: params {tuple(params.shape)} do not broadcast to the points {tuple(batch)}")
    n = uv.numel() // 2
    with torch.no_grad():
        uv = uv.detach().reshape(n, 2).contiguous()
        if uv.data_ptr() % 8:   # a view at an odd float offset: the kernel reads (u, v) as one 8-byte load
            uv = uv.clone()
        params = params.detach()
        if all(s == 1 for s in params.shape[:-1]):
            params, stride = params.reshape(n_params).contiguous(), 0
        else:
            params, stride = params.expand(*batch, n_params).reshape(n, n_params).contiguous(), n_params
        out = torch.empty((n, 2), dtype=torch.float32, device=uv.device)
        with torch.cuda.device(uv.device):
            B.call(name, B.ptr(uv), B.ptr(params), n, n_params, stride, float(eps), int(iters), B.ptr(out), B.stream())
    return out.reshape(*batch, 2)


def opencv_lens_undistortion(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """Undistort points of the OpenCV pinhole model (ref: cameras.py:13-47).

    Args:
        uv: (..., 2) distorted normalized image coordinates, float32 on a ROCm device (any strides).
        params: (..., N) or (N,) distortion parameters broadcastable to uv's batch, N in {0, 1, 2, 4, 8}:
            {k1}, {k1, k2}, {k1, k2, p1, p2} or {k1, k2, p1, p2, k3, k4, k5, k6}.  N = 0 returns ``uv`` itself.
        eps: Newton stops when |det J| < eps or both steps are below eps.
        iters: at most this many Newton steps (0 returns a copy of uv).

    Returns:
        (..., 2) undistorted coordinates (not differentiable).
    """
    if uv.shape[-1] != 2 or params.shape[-1] not in _OPENCV_COUNTS:
        raise ValueError(f"uv must be [..., 2] and params [..., N] with N in {_OPENCV_COUNTS}; "
                         f"got {tuple(uv.shape)} and {tuple(params.shape)}")
    if params.shape[-1] == 0:
        return uv
    return _launch("nfa_opencv_lens_undistortion", uv, _pad8(params), eps, iters)


def opencv_lens_undistortion_fisheye(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """Undistort points of the OpenCV fisheye model {k1, k2, k3, k4} (ref: cameras.py:50-72).

    Points that do not converge within ``iters`` steps, or whose angle flips sign, and points with |uv| <= eps are
    returned unchanged (DESIGN.md "Lens undistortion").

    Args:
        uv: (..., 2) distorted normalized image coordinates, float32 on a ROCm device.
        params: (..., 4) or (4,) parameters broadcastable to uv's batch.

    Returns:
        (..., 2) undistorted coordinates (not differentiable).
    """
    if uv.shape[-1] != 2 or params.shape[-1] != 4:
        raise ValueError(f"uv must be [..., 2] and params [..., 4]; got {tuple(uv.shape)} and {tuple(params.shape)}")
    return _launch("nfa_opencv_lens_undistortion_fisheye", uv, params, eps, iters)


def _opencv_lens_distortion(uv: Tensor, params: Tensor) -> Tensor:
    """Forward OpenCV distortion with params {k1, k2, p1, p2, k3, k4, k5, k6} (..., 8) (ref: cameras.py:75-92)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = params.unbind(-1)
    x, y = uv.unbind(-1)
    r = x * x + y * y
    d = (1 + r * (k1 + r * (k2 + r * k3))) / (1 + r * (k4 + r * (k5 + r * k6)))
    xy2 = 2 * x * y
    xd = x * d + p1 * xy2 + p2 * (r + 2 * x * x)
    yd = y * d + p2 * xy2 + p1 * (r + 2 * y * y)
    return torch.stack([xd, yd], dim=-1)


def _opencv_lens_distortion_fisheye(uv: Tensor, params: Tensor, eps: float = 1e-10) -> Tensor:
    """Forward OpenCV fisheye distortion with params {k1, k2, k3, k4} (..., 4) (ref: cameras.py:95-122):
    theta = atan(|uv|), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), uv * theta_d / |uv|."""
    if params.shape[-1] != 4:
        raise ValueError(f"fisheye params must be [..., 4], got {tuple(params.shape)}")
    k1, k2, k3, k4 = params.unbind(-1)
    x, y = uv.unbind(-1)
    rho = torch.sqrt(x * x + y * y)
    theta = torch.atan(rho)
    t2 = theta * theta
    theta_d = theta * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    return uv * (theta_d / rho.clamp(min=eps)).unsqueeze(-1)


def _newton_terms(x: Tensor, y: Tensor, xd: Tensor, yd: Tensor, params: Tensor
                  ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Residual (ex, ey) of the distortion at (x, y) against (xd, yd) and the symmetric Jacobian (jxx, jxy, jyy)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = params.unbind(-1)
    r = x * x + y * y
    num = 1 + r * (k1 + r * (k2 + r * k3))
    den = 1 + r * (k4 + r * (k5 + r * k6))
    d = num / den
    xy2 = 2 * x * y
    ex = d * x + p1 * xy2 + p2 * (r + 2 * x * x) - xd
    ey = d * y + p2 * xy2 + p1 * (r + 2 * y * y) - yd
    num_r = k1 + r * (2 * k2 + r * (3 * k3))
    den_r = k4 + r * (2 * k5 + r * (3 * k6))
    d_r = (num_r * den - num * den_r) / (den * den)
    jxx = d + 2 * x * x * d_r + 2 * p1 * y + 6 * p2 * x
    jxy = xy2 * d_r + 2 * p1 * x + 2 * p2 * y
    jyy = d + 2 * y * y * d_r + 2 * p2 * x + 6 * p1 * y
    return ex, ey, jxx, jxy, jyy


def _opencv_lens_undistortion(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """opencv_lens_undistortion in plain torch (ref: cameras.py:169-205): exactly ``iters`` Newton steps from the
    distorted point; a step is skipped where |det J| <= eps."""
    if uv.shape[-1] != 2 or params.shape[-1] not in _OPENCV_COUNTS:
        raise ValueError(f"uv must be [..., 2] and params [..., N] with N in {_OPENCV_COUNTS}; "
                         f"got {tuple(uv.shape)} and {tuple(params.shape)}")
    if params.shape[-1] == 0:
        return uv
    params = _pad8(params)
    xd, yd = uv.unbind(-1)
    x, y = xd, yd
    for _ in range(iters):
        ex, ey, jxx, jxy, jyy = _newton_terms(x, y, xd, yd, params)
        det = jxx * jyy - jxy * jxy
        ok = det.abs() > eps
        safe = torch.where(ok, det, torch.ones_like(det))
        x = x + torch.where(ok, (jxy * ey - jyy * ex) / safe, torch.zeros_like(x))
        y = y + torch.where(ok, (jxy * ex - jxx * ey) / safe, torch.zeros_like(y))
    return torch.stack([x, y], dim=-1)

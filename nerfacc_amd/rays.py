"""Rays from pixels and cameras (native kernels: csrc/rays.hip, the lens solvers of csrc/camera.h).

``generate_rays`` is the "generate rays" block both of the reference's loaders run every step
(``examples/datasets/nerf_synthetic.py:194-227``, ``examples/datasets/nerf_360_v2.py:326-359``): about a dozen gather and
elementwise torch launches with ``(n_rays, 3, 4)`` and ``(n_rays, 3)`` temporaries, and -- for a distorted camera -- the
``nerfacc.cameras`` call in its middle.  Here it is one pass, with the undistortion inside it.  Its backward carries the
gradients ``samples.sample_positions`` delivers at ``rays_o`` / ``rays_d`` on to the cameras (pose optimisation, the
reference's ``docs/source/examples/camera/barf.rst``): per-camera sums made by a fixed-shape two-level reduction, no float
atomics, the same bits every run (DESIGN.md "Rays from cameras").

Not part of ``nerfacc_amd.__all__`` (that list mirrors the reference's exactly); import the module.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _backend as B
from .cameras import _newton_terms, _opencv_lens_undistortion, _pad8

__all__ = ["generate_rays", "Rays", "mark_sorted", "reduction_chunk"]

Rays = namedtuple("Rays", ("origins", "viewdirs"))   # the loaders' field names

_PIXEL_DTYPES = {torch.float32: 0, torch.int32: 1, torch.int64: 2}
_PINHOLE_COUNTS = (1, 2, 4, 8)
_SORTED = "_nfa_camera_ids_sorted"
_TERMS = 16   # floats of a partial row: 12 of the pose, then fx, fy, cx, cy


def mark_sorted(camera_ids: Tensor) -> Tensor:
    """Declare ``camera_ids`` (flattened) ascending, e.g. rays gathered image by image: the backward of ``generate_rays``
    then takes the rays as they come and skips its sort.  The mark holds until the tensor is written to.  Ids that are not
    sorted after all give wrong gradients (never an access outside the arrays)."""
    setattr(camera_ids, _SORTED, camera_ids._version)
    return camera_ids


def reduction_chunk() -> int:
    """Rays per chunk of the backward's reduction: the constant its summation order depends on."""
    return int(B.load().nfa_generate_rays_chunk())


class _GenerateRaysFn(torch.autograd.Function):
    """``nfa_generate_rays_fwd`` / ``_bwd``.  Nothing per ray is saved beyond the inputs."""

    @staticmethod
    def forward(ctx, K, c2w, x, y, ids, dist, shape, fisheye, opengl, pixel_center, normalize, eps, iters, ids_sorted):
        ctx.set_materialize_grads(False)
        dev = B.require_device(K, c2w, x, y, ids, dist)
        n = x.numel()
        Kc, Pc = K.detach().reshape(-1, 9).contiguous(), c2w.detach().reshape(-1, c2w.shape[-2] * 4).contiguous()
        Dc = None if dist is None else dist.detach().reshape(-1, dist.shape[-1]).contiguous()
        n_cameras = max(Kc.shape[0], Pc.shape[0], 1 if Dc is None else Dc.shape[0])
        tables = (B.ptr(Kc), 9 if Kc.shape[0] > 1 else 0, B.ptr(Pc), Pc.shape[1] if Pc.shape[0] > 1 else 0,
                  B.ptr(Dc), 0 if Dc is None else Dc.shape[1], 0 if Dc is None or Dc.shape[0] == 1 else Dc.shape[1],
                  int(fisheye), int(opengl), float(pixel_center), int(normalize), float(eps), int(iters))
        origins = torch.empty((n, 3), dtype=torch.float32, device=dev)
        viewdirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n:
            with torch.cuda.device(dev):
                B.call("nfa_generate_rays_fwd", B.ptr(x), B.ptr(y), _PIXEL_DTYPES[x.dtype], B.ptr(ids), n, n_cameras, *tables,
                       B.ptr(origins), B.ptr(viewdirs), B.stream())
        ctx.save_for_backward(x, y, ids, Kc, Pc, Dc)
        ctx.tables, ctx.n_cameras, ctx.ids_sorted, ctx.fisheye = tables, n_cameras, ids_sorted, fisheye
        ctx.k_shape, ctx.pose_shape = K.shape, c2w.shape
        return origins.view(*shape, 3), viewdirs.view(*shape, 3)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_origins, g_viewdirs):
        need_K, need_pose = ctx.needs_input_grad[:2]
        none = (None,) * 14
        if (g_origins is None and g_viewdirs is None) or not (need_K or need_pose):
            return none
        x, y, ids, Kc, Pc, Dc = ctx.saved_tensors
        dev, n, C = Kc.device, x.numel(), ctx.n_cameras
        if n == 0:
            return (torch.zeros(ctx.k_shape, device=dev) if need_K else None,
                    torch.zeros(ctx.pose_shape, device=dev) if need_pose else None) + none[2:]
        g_origins = None if g_origins is None else g_origins.to(torch.float32).reshape(n, 3).contiguous()
        g_viewdirs = None if g_viewdirs is None else g_viewdirs.to(torch.float32).reshape(n, 3).contiguous()
        # rays in camera order: as they come (one camera, or ids marked sorted), else by a stable sort on the device
        order = None
        if ids is not None and not ctx.ids_sorted:
            ids, order = torch.sort(ids, stable=True)
        pose_floats = Pc.shape[1]
        n_rows = (n + reduction_chunk() - 1) // reduction_chunk() + C - 1
        partials = torch.empty((n_rows, _TERMS), dtype=torch.float32, device=dev)
        g_pose = torch.empty((C, pose_floats), dtype=torch.float32, device=dev) if need_pose else None
        g_K = torch.empty((C, 9), dtype=torch.float32, device=dev) if need_K else None
        Kp, ks, Pp, ps, Dp, nd, ds, *opts = ctx.tables
        with torch.cuda.device(dev):
            B.call("nfa_generate_rays_bwd", B.ptr(x), B.ptr(y), _PIXEL_DTYPES[x.dtype], B.ptr(ids), B.ptr(order), n, C,
                   B.ptr(Kc), ks, B.ptr(Pc), ps, B.ptr(Dc), nd, ds, *opts, B.ptr(g_origins), B.ptr(g_viewdirs), B.ptr(partials),
                   n_rows, pose_floats, B.ptr(g_pose), B.ptr(g_K), B.stream())
        # a table shared by several cameras: its gradient is the sum of theirs (a deterministic torch reduction)
        if g_pose is not None:
            g_pose = (g_pose if Pc.shape[0] == C else g_pose.sum(0)).view(ctx.pose_shape)
        if g_K is not None:
            g_K = (g_K if Kc.shape[0] == C else g_K.sum(0)).view(ctx.k_shape)
        return (g_K, g_pose) + none[2:]


def _undistort_fisheye_torch(uv: Tensor, params: Tensor, eps: float, iters: int) -> Tensor:
    """csrc/camera.h's fisheye solve as torch expressions: Newton on theta in float64, at most ``iters`` steps, a point that
    does not converge (or sits within eps of the centre) returned unchanged.  Not differentiable."""
    with torch.no_grad():
        xd, yd = uv.unbind(-1)
        theta_d = torch.sqrt(xd * xd + yd * yd).clamp(max=math.pi / 2)
        td = theta_d.double()
        k1, k2, k3, k4 = params.double().unbind(-1)
        theta, done = td.clone(), torch.zeros_like(td, dtype=torch.bool)
        for _ in range(iters):
            t2 = theta * theta
            g = theta * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
            g_t = 1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * (9 * k4))))
            step = g / g_t
            theta = torch.where(done, theta, theta - step)
            done = done | (step.abs() < eps)
        ok = done & (theta >= 0) & (theta_d > eps)
        scale = torch.where(ok, torch.tan(theta.to(uv.dtype)) / torch.where(ok, theta_d, torch.ones_like(theta_d)),
                            torch.ones_like(theta_d))
        return uv.detach() * scale.unsqueeze(-1)


def _undistort_pinhole_torch(u: Tensor, v: Tensor, params: Tensor, eps: float, iters: int):
    """The Newton solve of ``cameras._opencv_lens_undistortion`` with the gradient the native backward uses: through the
    inverse of the distortion Jacobian at the solution, zero where |det J| < eps.  The parameters get none."""
    uvd = torch.stack([u, v], dim=-1)
    params = params.detach()
    with torch.no_grad():
        sol = _opencv_lens_undistortion(uvd, params, eps, iters)
    su, sv = sol.unbind(-1)
    if not (torch.is_grad_enabled() and uvd.requires_grad):
        return su, sv
    with torch.no_grad():
        _, _, jxx, jxy, jyy = _newton_terms(su, sv, u, v, params)
        det = jxx * jyy - jxy * jxy
        ok = ~(det.abs() < eps)
        inv = torch.where(ok, 1 / torch.where(ok, det, torch.ones_like(det)), torch.zeros_like(det))
    du, dv = u - u.detach(), v - v.detach()   # zero, carrying the gradient
    return su + inv * (jyy * du - jxy * dv), sv + inv * (jxx * dv - jxy * du)


def _generate_rays_torch(x, y, K, c2w, ids, dist, fisheye, opengl, pixel_center, normalize, eps, iters):
    """The same formulas as torch expressions (CPU tensors, other dtypes); autograd differentiates them."""
    dt = c2w.dtype
    pick = (lambda t: t[ids] if t.shape[0] > 1 else t[0]) if ids is not None else (lambda t: t[0])
    Kr, Pr = pick(K.reshape(-1, 3, 3)), pick(c2w.reshape(-1, c2w.shape[-2], 4))
    u = (x.to(dt) - Kr[..., 0, 2] + pixel_center) / Kr[..., 0, 0]
    v = (y.to(dt) - Kr[..., 1, 2] + pixel_center) / Kr[..., 1, 1]
    if dist is not None:
        params = pick(dist.reshape(-1, dist.shape[-1])).to(dt)
        if fisheye:
            u, v = _undistort_fisheye_torch(torch.stack([u, v], dim=-1), params, eps, iters).unbind(-1)
        else:
            u, v = _undistort_pinhole_torch(u, v, params, eps, iters)
    s = -1.0 if opengl else 1.0
    c = (u, s * v, torch.full_like(u, s))
    d = torch.stack([Pr[..., i, 0] * c[0] + Pr[..., i, 1] * c[1] + Pr[..., i, 2] * c[2] for i in range(3)], dim=-1)
    if normalize:
        d = d / torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).unsqueeze(-1)
    origins = torch.broadcast_to(Pr[..., :3, 3], d.shape).contiguous()
    return origins, d


def generate_rays(
    x: Tensor,
    y: Tensor,
    K: Tensor,
    camtoworlds: Tensor,
    camera_ids: Optional[Tensor] = None,
    *,
    distortion: Optional[Tensor] = None,
    fisheye: bool = False,
    opengl: bool = False,
    pixel_center: float = 0.5,
    normalize: bool = True,
    eps: float = 1e-6,
    iters: int = 10,
) -> Rays:
    """Rays through pixels ``(x, y)`` of cameras ``(K, camtoworlds)``.

        u = (x - cx + pixel_center) / fx,  v = (y - cy + pixel_center) / fy
        (u, v) <- undistort(u, v)                                  with ``distortion``
        c = (u, s v, s),  s = -1 if opengl else 1
        d_i = sum_j R_ij c_j (left to right);  viewdirs = d / |d| if normalize else d;  origins = the translation

    Args:
        x, y: pixel coordinates of any common shape ``(...)``: int32, int64 or float32 (not differentiable).
        K: ``(3, 3)`` or ``(C, 3, 3)`` intrinsics.
        camtoworlds: ``(3|4, 4)`` or ``(C, 3|4, 4)`` camera-to-world matrices.
        camera_ids: ``(...)`` integer indices into ``C``, in any order; may be ``None`` only with one camera (and is ignored
            then).  ``mark_sorted(camera_ids)`` spares the backward its sort.
        distortion: ``None``, or ``(P,)`` / ``(C, P)``: OpenCV pinhole parameters, ``P`` in {1, 2, 4, 8} in the order of
            ``cameras.opencv_lens_undistortion``, or with ``fisheye=True`` the four of
            ``cameras.opencv_lens_undistortion_fisheye``.
        eps, iters: as in ``cameras``.

    Returns:
        ``Rays(origins, viewdirs)``, each ``(..., 3)``.

    Differentiable w.r.t. ``camtoworlds`` (the bottom row of a 4x4 gets zero) and ``K`` (fx, fy, cx, cy; through the pinhole
    lens by the inverse of the distortion Jacobian at the solution, zero for a ray where |det J| < eps; ``fisheye=True``
    with ``K.requires_grad`` raises ``ValueError``); ``distortion`` gets no gradient, like the reference's undistortion.
    CUDA float32 cameras run on libnerfacc_hip.so, and the undistorted (u, v) have the bits of ``cameras``' functions; the
    gradients are per-camera sums in a fixed order, the same bits every run.  Neither direction reads from the device.
    Anything else (CPU, float64) runs the same formulas in torch.
    """
    if K.shape[-2:] != (3, 3) or K.dim() not in (2, 3):
        raise ValueError(f"K must be (3, 3) or (C, 3, 3), got {tuple(K.shape)}")
    if camtoworlds.dim() not in (2, 3) or camtoworlds.shape[-1] != 4 or camtoworlds.shape[-2] not in (3, 4):
        raise ValueError(f"camtoworlds must be (3|4, 4) or (C, 3|4, 4), got {tuple(camtoworlds.shape)}")
    if distortion is None and fisheye:
        raise ValueError("fisheye=True needs distortion parameters")
    if distortion is not None:
        counts = (4,) if fisheye else _PINHOLE_COUNTS
        if distortion.dim() not in (1, 2) or distortion.shape[-1] not in counts:
            raise ValueError(f"distortion must be (P,) or (C, P) with P in {counts}, got {tuple(distortion.shape)}")
    if fisheye and torch.is_grad_enabled() and K.requires_grad:
        raise ValueError("generate_rays: K is not differentiable through the fisheye lens")
    leading = [t.shape[0] for t, d in ((K, 3), (camtoworlds, 3), (distortion, 2)) if t is not None and t.dim() == d]
    n_cameras = max(leading, default=1)
    if any(c not in (1, n_cameras) for c in leading):
        raise ValueError(f"K, camtoworlds and distortion disagree on the number of cameras: {leading}")
    if camera_ids is None and n_cameras > 1:
        raise ValueError(f"camera_ids may be None only with one camera (there are {n_cameras})")
    if x.is_floating_point() != y.is_floating_point() or (camera_ids is not None and camera_ids.is_floating_point()):
        raise ValueError("x and y must both be integer or both floating point, camera_ids integer")
    ids = camera_ids if n_cameras > 1 else None
    shape = torch.broadcast_shapes(x.shape, y.shape, *(() if ids is None else (ids.shape,)))
    if distortion is not None and not fisheye:
        distortion = _pad8(distortion)
    cams = [t for t in (K, camtoworlds, distortion) if t is not None]
    native = all(t.is_cuda and t.dtype == torch.float32 and t.device == K.device for t in cams) and \
        all(t is None or (t.device == K.device and not t.dtype == torch.float64) for t in (x, y, ids))
    if not native:
        bx, by = x.expand(shape), y.expand(shape)
        return Rays(*_generate_rays_torch(bx, by, K, camtoworlds, None if ids is None else ids.expand(shape).long(), distortion,
                                          fisheye, opengl, pixel_center, normalize, eps, iters))
    if x.dtype != y.dtype or x.dtype not in _PIXEL_DTYPES:
        x, y = x.to(torch.float32), y.to(torch.float32)
    xf, yf = x.expand(shape).reshape(-1).contiguous(), y.expand(shape).reshape(-1).contiguous()
    ids_sorted = False
    if ids is not None:
        ids_sorted = ids.shape == shape and getattr(ids, _SORTED, None) == ids._version
        ids = ids.expand(shape).reshape(-1).to(torch.int64).contiguous()
    out = _GenerateRaysFn.apply(K, camtoworlds, xf, yf, ids, distortion, shape, bool(fisheye), bool(opengl), pixel_center,
                                bool(normalize), eps, iters, ids_sorted)
    return Rays(*out)

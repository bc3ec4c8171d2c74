"""A float64 restatement of nerfacc_amd.rays.generate_rays and of the per-ray terms of its backward, written from the
formulas (not from the package's code), shared by tests/test_rays_cpu.py and tests/test_rays_gpu.py.

    u = (x - cx + pixel_center) / fx,  v = (y - cy + pixel_center) / fy;  (u, v) <- undistort(u, v) with a lens
    c = (u, s v, s), s = -1 (OpenGL) or 1;  d_i = sum_j R_ij c_j;  viewdirs = d / |d| or d;  origins = t
"""
import torch

EPS = 2.0 ** -24   # unit roundoff of float32


def per_ray(t, ids, tail):
    """The rows of a per-camera table ``t`` (shared: no leading dim) for each ray, in float64."""
    t = t.double()
    if t.dim() == tail:
        return t
    return t[ids] if t.shape[0] > 1 else t[0]


def rays_f64(x, y, K, c2w, ids, *, uv=None, opengl=False, pixel_center=0.5, normalize=True):
    """dict(ud, vd, u, v, c, R, t, d, viewdirs, origins) in float64 from the given inputs; ``uv`` (..., 2) replaces the
    undistorted point (the caller's solver)."""
    Kr, Pr = per_ray(K, ids, 2), per_ray(c2w, ids, 2)
    ud = (x.double() - Kr[..., 0, 2] + pixel_center) / Kr[..., 0, 0]
    vd = (y.double() - Kr[..., 1, 2] + pixel_center) / Kr[..., 1, 1]
    u, v = (ud, vd) if uv is None else (uv[..., 0].double(), uv[..., 1].double())
    s = -1.0 if opengl else 1.0
    c = torch.stack([u, s * v, torch.full_like(u, s)], dim=-1)
    R, t = Pr[..., :3, :3], Pr[..., :3, 3]
    d = (R * c[..., None, :]).sum(-1)
    w = d / d.norm(dim=-1, keepdim=True) if normalize else d
    return dict(ud=ud, vd=vd, u=u, v=v, c=c, R=R, t=t, d=d, viewdirs=w, origins=t.expand(d.shape), s=s, fx=Kr[..., 0, 0], fy=Kr[..., 1, 1])


def ray_terms_f64(f, g_origins, g_viewdirs, *, normalize=True, jac=None, eps=1e-6):
    """(n, 16) float64: each ray's share of its camera's gradient, {dR_i0, dR_i1, dR_i2, dt_i} for i = 0, 1, 2, then dfx, dfy,
    dcx, dcy.  ``f`` is rays_f64's dict of flat rays; ``jac`` = (jxx, jxy, jyy) of the pinhole distortion at (u, v): the K
    terms then pass through its inverse, and are zero where |det| < eps."""
    go, gw = g_origins.double(), g_viewdirs.double()
    gd = gw
    if normalize:
        nrm = f["d"].norm(dim=-1, keepdim=True)
        w = f["d"] / nrm
        gd = (gw - w * (w * gw).sum(-1, keepdim=True)) / nrm
    pose = torch.cat([gd[:, :, None] * f["c"][:, None, :], go[:, :, None]], dim=-1).reshape(-1, 12)
    gc = (f["R"] * gd[..., :, None]).sum(-2)   # R^T g_d
    gu, gv = gc[..., 0], f["s"] * gc[..., 1]
    if jac is not None:
        jxx, jxy, jyy = (j.double() for j in jac)
        det = jxx * jyy - jxy * jxy
        ok = ~(det.abs() < eps)
        safe = torch.where(ok, det, torch.ones_like(det))
        gu, gv = torch.where(ok, (jyy * gu - jxy * gv) / safe, 0.0), torch.where(ok, (jxx * gv - jxy * gu) / safe, 0.0)
    k = torch.stack([-gu * f["ud"] / f["fx"], -gv * f["vd"] / f["fy"], -gu / f["fx"], -gv / f["fy"]], dim=-1)
    return torch.cat([pose, k], dim=-1)


def camera_sums(terms, ids, n_cameras):
    """(sum, sum of absolute values) of the per-ray terms by camera, (C, 16) float64 each."""
    rows = torch.zeros(terms.shape[0], dtype=torch.int64, device=terms.device) if ids is None else ids
    z = torch.zeros(n_cameras, terms.shape[1], dtype=terms.dtype, device=terms.device)
    return z.index_add(0, rows, terms), z.index_add(0, rows, terms.abs())


def split_grads(rows, pose_rows=3):
    """(C, 16) -> (grad camtoworlds (C, pose_rows, 4), grad K (C, 3, 3)) in the layout autograd gives."""
    C = rows.shape[0]
    gp = torch.zeros(C, pose_rows, 4, dtype=rows.dtype, device=rows.device)
    gp[:, :3] = rows[:, :12].view(C, 3, 4)
    gk = torch.zeros(C, 3, 3, dtype=rows.dtype, device=rows.device)
    gk[:, 0, 0], gk[:, 1, 1], gk[:, 0, 2], gk[:, 1, 2] = rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15]
    return gp, gk


def random_cameras(n_cameras, seed, pose_rows=3, distortion=None):
    """K (C, 3, 3), camtoworlds (C, pose_rows, 4) with proper rotations, and distortion parameters (C, P) or None
    (``distortion``: P for the pinhole model, "fisheye" for its four)."""
    g = torch.Generator().manual_seed(seed)
    K = torch.zeros(n_cameras, 3, 3)
    K[:, 0, 0] = 500 + 100 * torch.rand(n_cameras, generator=g)
    K[:, 1, 1] = 500 + 100 * torch.rand(n_cameras, generator=g)
    K[:, 0, 2] = 400 + 10 * torch.rand(n_cameras, generator=g)
    K[:, 1, 2] = 300 + 10 * torch.rand(n_cameras, generator=g)
    K[:, 2, 2] = 1
    q, _ = torch.linalg.qr(torch.randn(n_cameras, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.linalg.det(q))[:, None, None]
    pose = torch.zeros(n_cameras, pose_rows, 4)
    pose[:, :3, :3] = q.float()
    pose[:, :3, 3] = torch.randn(n_cameras, 3, generator=g) * 3
    if pose_rows == 4:
        pose[:, 3, 3] = 1
    dist = None
    if distortion == "fisheye":
        dist = (torch.rand(n_cameras, 4, generator=g) - 0.5) * torch.tensor([0.1, 0.02, 0.004, 0.001])
    elif distortion:
        scale = torch.tensor([0.1, 0.02, 0.002, 0.002, 0.004, 0.01, 0.004, 0.001])[:distortion]
        dist = (torch.rand(n_cameras, distortion, generator=g) - 0.5) * scale
    return K, pose, dist


def random_pixels(n, n_cameras, seed, dtype=torch.float32, skip=()):
    """x, y over an 800 x 600 image and camera ids that leave the cameras in ``skip`` without a ray."""
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand(n, generator=g) * 800, torch.rand(n, generator=g) * 600
    if dtype != torch.float32:
        x, y = x.to(dtype), y.to(dtype)
    ids = torch.randint(0, n_cameras, (n,), generator=g)
    for c in skip:
        ids[ids == c] = (c + 1) % n_cameras
    return x, y, ids

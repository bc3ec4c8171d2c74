"""GPU: the native lens undistortion (csrc/camera.hip) against the reference's torch functions (tests/golden/cameras.npz),
the reference's own test_camera.py, wrapper behaviour, the `_C` layouts 5 / 8 / 12 against a float64 restatement, and the
fisheye behaviour DESIGN.md defines where the reference does not."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _cam():
    from nerfacc_amd import cameras
    return cameras


def _max_err(a, b):
    return float((a.double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _disc_points(rng, n, radius=0.8):
    rho = radius * np.sqrt(rng.uniform(0.0, 1.0, n))
    phi = rng.uniform(0.0, 2 * np.pi, n)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi)], -1).astype(np.float32)


def _opencv8(rng, shape):
    # {k1, k2, p1, p2, k3, k4, k5, k6}: the fixture's regime (scripts/gen_camera_golden.py)
    p = rng.uniform(-0.02, 0.02, shape + (8,))
    p[..., 0] = rng.uniform(-0.1, 0.1, shape)
    p[..., 2:4] = rng.uniform(-0.01, 0.01, shape + (2,))
    return p.astype(np.float32)


# ----------------------------------------------------------------------------- float64 restatement of the _C layouts
def _np_newton(uv, k1, k2, k3, k4, k5, k6, p1, p2, eps, iters):
    xd, yd = uv[..., 0], uv[..., 1]
    x, y = xd.copy(), yd.copy()
    active = np.ones(x.shape, bool)
    for _ in range(iters):
        r = x * x + y * y
        num, den = 1 + r * (k1 + r * (k2 + r * k3)), 1 + r * (k4 + r * (k5 + r * k6))
        d = num / den
        ex = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd
        ey = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd
        d_r = ((k1 + r * (2 * k2 + 3 * k3 * r)) * den - num * (k4 + r * (2 * k5 + 3 * k6 * r))) / (den * den)
        jxx = d + 2 * x * x * d_r + 2 * p1 * y + 6 * p2 * x
        jxy = 2 * x * y * d_r + 2 * p1 * x + 2 * p2 * y
        jyy = d + 2 * y * y * d_r + 2 * p2 * x + 6 * p1 * y
        det = jxx * jyy - jxy * jxy
        active &= np.abs(det) >= eps
        safe = np.where(active, det, 1.0)
        dx = np.where(active, (jxy * ey - jyy * ex) / safe, 0.0)
        dy = np.where(active, (jxy * ex - jxx * ey) / safe, 0.0)
        x, y = x + dx, y + dy
        active &= ~((np.abs(dx) < eps) & (np.abs(dy) < eps))
    return np.stack([x, y], -1)


def _np_compat(uv, params, eps, iters):
    uv, q = uv.astype(np.float64), params.astype(np.float64)
    z = np.zeros(uv.shape[:-1])
    if q.shape[-1] == 5:
        return _np_newton(uv, q[..., 0], q[..., 1], q[..., 4], z, z, z, q[..., 2], q[..., 3], eps, iters)
    if q.shape[-1] == 8:
        return _np_newton(uv, q[..., 0], q[..., 1], q[..., 4], q[..., 5], q[..., 6], q[..., 7], q[..., 2], q[..., 3],
                          eps, iters)
    k1, k2, k3, k4, k5, k6, p1, p2, s1, s2, s3, s4 = np.moveaxis(q, -1, 0)
    xd, yd = uv[..., 0], uv[..., 1]
    x, y = xd.copy(), yd.copy()
    bad = np.zeros(x.shape, bool)
    for _ in range(iters):
        r = x * x + y * y
        inv_d = (1 + r * (k4 + r * (k5 + r * k6))) / (1 + r * (k1 + r * (k2 + r * k3)))
        bad |= inv_d < 0
        x_new = (xd - (2 * p1 * x * y + p2 * (r + 2 * x * x) + s1 * r + s2 * r * r)) * inv_d
        y_new = (yd - (2 * p2 * x * y + p1 * (r + 2 * y * y) + s3 * r + s4 * r * r)) * inv_d
        x, y = np.where(bad, x, x_new), np.where(bad, y, y_new)
    out = np.stack([x, y], -1)
    out[bad] = uv[bad]
    return out


def _np_fisheye_theta(theta_d, k, eps, iters):
    theta = theta_d
    for _ in range(iters):
        t2 = theta * theta
        step = (theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - theta_d) / (
            1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3]))))
        theta -= step
        if abs(step) < eps:
            return theta
    return None


# ----------------------------------------------------------------------------- the reference's tests/test_camera.py
@torch.no_grad()
def test_reference_test_camera_restated(dev):
    cam = _cam()
    torch.manual_seed(42)
    x = torch.rand((3, 1000, 2), device=dev)
    params = torch.rand((8,), device=dev) * 0.01
    und = cam.opencv_lens_undistortion(x, params, 1e-5, 10)
    assert _max_err(und, cam._opencv_lens_undistortion(x, params, 1e-5, 10)) <= 1e-5
    assert _max_err(cam._opencv_lens_distortion(und, params), x) <= 1e-5
    params = torch.rand((4,), device=dev) * 0.01
    und = cam.opencv_lens_undistortion_fisheye(x, params, 1e-5, 10)
    assert _max_err(cam._opencv_lens_distortion_fisheye(und, params), x) <= 1e-5


# ----------------------------------------------------------------------------- against the reference's fixture
@torch.no_grad()
def test_native_matches_reference_fixture(dev):
    cam = _cam()
    g = load_golden("cameras")
    eps, iters = float(g["eps"]), int(g["iters"])
    for i in range(int(g["n_cases"])):
        uv, p, fe = (torch.from_numpy(g[f"c{i}_{k}"]).to(dev) for k in ("uv", "params", "fe_params"))
        und = cam.opencv_lens_undistortion(uv, p, eps, iters)
        assert und.shape == uv.shape and und.dtype == torch.float32
        assert _max_err(und, g[f"c{i}_undist"]) <= 1e-5, i
        assert _max_err(cam._opencv_lens_distortion(und, F.pad(p, (0, 8 - p.shape[-1]))), uv) <= 1e-5, i
        und = cam.opencv_lens_undistortion_fisheye(uv, fe, eps, iters)
        assert _max_err(cam._opencv_lens_distortion_fisheye(und, fe), uv) <= 1e-5, i


# ----------------------------------------------------------------------------- wrapper behaviour
@torch.no_grad()
def test_parameter_counts(dev):
    cam = _cam()
    rng = np.random.default_rng(3)
    uv = torch.from_numpy(_disc_points(rng, 4000)).to(dev).reshape(40, 100, 2)
    assert cam.opencv_lens_undistortion(uv, torch.zeros(0, device=dev)) is uv
    full = torch.from_numpy(_opencv8(rng, ())).to(dev)
    for n in (1, 2, 4, 8):
        got = cam.opencv_lens_undistortion(uv, full[:n])
        assert _max_err(got, cam._opencv_lens_undistortion(uv, full[:n])) <= 1e-5, n
        # zero-padding to 8 is what the count means
        assert torch.equal(got, cam.opencv_lens_undistortion(uv, F.pad(full[:n], (0, 8 - n)))), n


@torch.no_grad()
def test_shared_per_point_and_per_camera_parameters_agree(dev):
    cam = _cam()
    rng = np.random.default_rng(4)
    C, P = 5, 777
    uv = torch.from_numpy(_disc_points(rng, C * P)).to(dev).reshape(C, P, 2)
    p = torch.from_numpy(_opencv8(rng, ())).to(dev)
    shared = cam.opencv_lens_undistortion(uv, p)
    assert torch.equal(shared, cam.opencv_lens_undistortion(uv, p.expand(C, P, 8).contiguous()))
    assert torch.equal(shared, cam.opencv_lens_undistortion(uv, p.expand(C, 1, 8)))
    assert torch.equal(shared, cam.opencv_lens_undistortion(uv, p.reshape(1, 1, 8)))
    # different parameters per camera: each camera as if undistorted on its own
    pc = torch.from_numpy(_opencv8(rng, (C, 1))).to(dev)
    per_cam = cam.opencv_lens_undistortion(uv, pc)
    for c in range(C):
        assert torch.equal(per_cam[c], cam.opencv_lens_undistortion(uv[c], pc[c, 0])), c
    fe = torch.rand(4, device=dev) * 0.05
    shared = cam.opencv_lens_undistortion_fisheye(uv, fe)
    assert torch.equal(shared, cam.opencv_lens_undistortion_fisheye(uv, fe.expand(C, P, 4).contiguous()))
    assert torch.equal(shared, cam.opencv_lens_undistortion_fisheye(uv, fe.expand(C, 1, 4)))
    with pytest.raises(RuntimeError):
        cam.opencv_lens_undistortion(uv, torch.zeros(3, P, 8, device=dev))   # does not broadcast


@torch.no_grad()
def test_strided_inputs_empty_batches_and_zero_iterations(dev):
    cam = _cam()
    rng = np.random.default_rng(5)
    base = torch.from_numpy(_disc_points(rng, 2 * 300)).to(dev).reshape(300, 2, 2)
    uv = base.transpose(0, 1)   # (2, 300, 2), not contiguous
    odd = torch.from_numpy(_disc_points(rng, 301)).to(dev).reshape(-1)[1:-1].reshape(300, 2)   # 4-byte offset view
    assert not uv.is_contiguous() and odd.data_ptr() % 8 == 4
    p = torch.from_numpy(_opencv8(rng, ())).to(dev)
    assert torch.equal(cam.opencv_lens_undistortion(uv, p), cam.opencv_lens_undistortion(uv.contiguous(), p))
    assert torch.equal(cam.opencv_lens_undistortion(odd, p), cam.opencv_lens_undistortion(odd.clone(), p))
    fe = torch.rand(4, device=dev) * 0.05
    assert torch.equal(cam.opencv_lens_undistortion_fisheye(uv, fe), cam.opencv_lens_undistortion_fisheye(uv.contiguous(), fe))
    empty = torch.zeros(0, 2, device=dev)
    assert cam.opencv_lens_undistortion(empty, p).shape == (0, 2)
    assert cam.opencv_lens_undistortion_fisheye(torch.zeros(3, 0, 2, device=dev), fe).shape == (3, 0, 2)
    same = cam.opencv_lens_undistortion(uv, p, iters=0)
    assert torch.equal(same, uv) and same.data_ptr() != uv.data_ptr()
    assert torch.equal(cam.opencv_lens_undistortion_fisheye(uv, fe, iters=0), uv)   # never converges: input
    with pytest.raises(RuntimeError):
        cam.opencv_lens_undistortion(uv.double(), p)
    with pytest.raises(RuntimeError, match="iters"):
        cam.opencv_lens_undistortion(uv, p, iters=-1)
    g = uv.clone().requires_grad_(True)
    assert not cam.opencv_lens_undistortion(g, p).requires_grad


@torch.no_grad()
def test_runs_on_the_current_stream(dev):
    cam = _cam()
    rng = np.random.default_rng(6)
    host = torch.from_numpy(_disc_points(rng, 1 << 16))
    p = torch.from_numpy(_opencv8(rng, ())).to(dev)
    expect = cam.opencv_lens_undistortion(host.to(dev), p)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        uv = host.to(dev, non_blocking=True) * 1.0   # produced on s: only s orders it before the kernel
        out = cam.opencv_lens_undistortion(uv, p)
        out_fe = cam.opencv_lens_undistortion_fisheye(uv, p[:4] * 0.5)
    s.synchronize()
    assert torch.equal(out, expect)
    assert torch.equal(out_fe, cam.opencv_lens_undistortion_fisheye(host.to(dev), p[:4] * 0.5))


# ----------------------------------------------------------------------------- at full size
@torch.no_grad()
def test_full_size_against_cpu_reference(dev):
    cam = _cam()
    rng = np.random.default_rng(7)
    n = 1 << 20
    uv = torch.from_numpy(_disc_points(rng, n))
    shared = torch.from_numpy(_opencv8(rng, ()))
    per_point = torch.from_numpy(_opencv8(rng, (n,)))
    for p in (shared, per_point):
        got = cam.opencv_lens_undistortion(uv.to(dev), p.to(dev))
        assert _max_err(got, cam._opencv_lens_undistortion(uv, p)) <= 1e-5
    fe = torch.from_numpy(rng.uniform(-0.05, 0.05, (n, 4)).astype(np.float32))
    und = cam.opencv_lens_undistortion_fisheye(uv.to(dev), fe.to(dev))
    assert torch.isfinite(und).all()
    assert _max_err(cam._opencv_lens_distortion_fisheye(und.cpu(), fe), uv) <= 1e-5


# ----------------------------------------------------------------------------- the _C layouts
@torch.no_grad()
def test_compat_layouts_against_float64_restatement(dev):
    import nerfacc_amd.cuda_compat as _C
    rng = np.random.default_rng(8)
    n = 20000
    uv = _disc_points(rng, n).reshape(4, n // 4, 2)
    p8 = _opencv8(rng, (4, n // 4))
    p5 = p8[..., :5].copy()
    p12 = np.concatenate([p8[..., [0, 1, 4, 5, 6, 7]], p8[..., 2:4],
                          rng.uniform(-0.01, 0.01, (4, n // 4, 4)).astype(np.float32)], -1)
    # a quarter of the thin-prism points with |uv| > 0.2 get a negative inverse radial factor at the first step
    # (1 - 40 r < 0 for r > 0.025): returned unchanged
    neg = (rng.random((4, n // 4)) < 0.25) & (np.linalg.norm(uv, axis=-1) > 0.2)
    p12[..., 3] = np.where(neg, -40.0, p12[..., 3])
    for params in (p5, p8, p12):
        got = _C.opencv_lens_undistortion(torch.from_numpy(uv).to(dev), torch.from_numpy(params).to(dev), 1e-6, 10)
        expect = _np_compat(uv, params, 1e-6, 10)
        assert got.shape == uv.shape
        assert _max_err(got, expect) <= 1e-5, params.shape[-1]
    got = got.cpu().numpy()
    assert neg.sum() > 1000 and (got[neg] == uv[neg]).all()
    fe = rng.uniform(-0.05, 0.05, (4, n // 4, 4)).astype(np.float32)
    und = _C.opencv_lens_undistortion_fisheye(torch.from_numpy(uv).to(dev), torch.from_numpy(fe).to(dev), 1e-6, 10)
    assert _max_err(_cam()._opencv_lens_distortion_fisheye(und.cpu(), torch.from_numpy(fe)), uv) <= 1e-5
    t = torch.from_numpy(uv).to(dev)
    with pytest.raises(RuntimeError):
        _C.opencv_lens_undistortion(t, torch.from_numpy(p8[0]).to(dev), 1e-6, 10)          # ranks differ
    with pytest.raises(RuntimeError):
        _C.opencv_lens_undistortion(t, torch.zeros(4, n // 4, 6, device=dev), 1e-6, 10)   # 6 parameters
    with pytest.raises(RuntimeError):
        _C.opencv_lens_undistortion(t, torch.zeros(4, 1, 8, device=dev), 1e-6, 10)        # not broadcast
    with pytest.raises(RuntimeError):
        _C.opencv_lens_undistortion_fisheye(t, torch.zeros(4, n // 4, 5, device=dev), 1e-6, 10)


# ----------------------------------------------------------------------------- fisheye: defined behaviour
@torch.no_grad()
def test_fisheye_defined_behaviour(dev):
    cam = _cam()
    eps = 1e-6
    k = [0.05, 0.01, 0.0, 0.0]
    uv = torch.tensor([[0.0, 0.0], [3e-8, -4e-8], [3.0, 0.0], [0.0, -10.0], [0.3, 0.4]], device=dev)
    out = cam.opencv_lens_undistortion_fisheye(uv, torch.tensor(k, device=dev), eps, 10).cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out[0], torch.zeros(2))        # centre
    assert torch.equal(out[1], uv[1].cpu())           # |uv| <= eps: scale 1
    theta = _np_fisheye_theta(math.pi / 2, k, eps, 10)   # |uv| > pi/2 clamps theta_d to pi/2
    scale = math.tan(theta) / (math.pi / 2)
    assert abs(out[2, 0].item() - 3.0 * scale) <= 1e-4 * 3.0 * scale and out[2, 1].item() == 0.0
    assert abs(out[3, 1].item() + 10.0 * scale) <= 1e-4 * 10.0 * scale and out[3, 0].item() == 0.0
    theta = _np_fisheye_theta(0.5, k, eps, 10)
    assert abs(out[4, 0].item() - 0.3 * math.tan(theta) / 0.5) <= 1e-6
    # does not converge in one step with a strongly negative k1: the input comes back, finite
    rng = np.random.default_rng(9)
    pts = torch.from_numpy(_disc_points(rng, 4096, radius=1.5)).to(dev)
    strong = torch.tensor([-0.5, 0.0, 0.0, 0.0], device=dev)
    out = cam.opencv_lens_undistortion_fisheye(pts, strong, eps, 1)
    moved = pts.norm(dim=-1) > 0.05   # where one step cannot land within eps
    assert torch.isfinite(out).all() and moved.sum() > 4000
    assert torch.equal(out[moved], pts[moved])
    # theta flips sign: Newton from theta_d overshoots past 0 for a strongly negative k1 at large angles
    flip = cam.opencv_lens_undistortion_fisheye(torch.tensor([[1.5, 0.0]], device=dev),
                                                torch.tensor([-0.6, 0.0, 0.0, 0.0], device=dev), eps, 50)
    assert _np_fisheye_theta(1.5, [-0.6, 0.0, 0.0, 0.0], eps, 50) < 0
    assert torch.equal(flip.cpu(), torch.tensor([[1.5, 0.0]]))

"""CPU: nerfacc_amd.rays.generate_rays on its torch path -- against the float64 restatement of tests/rays_reference.py under
the bounds derived from the count of float32 roundings, gradients (gradcheck in float64, the pinhole lens against autograd
through cameras._opencv_lens_undistortion), argument errors, empty input -- and the C ABI of the native entry points."""
import ctypes as C

import pytest
import torch

from rays_reference import EPS, camera_sums, random_cameras, random_pixels, ray_terms_f64, rays_f64, split_grads


def check_forward(out, x, y, K, pose, ids, *, opengl, normalize, uv=None, pixel_center=0.5):
    """At most 6 float32 roundings reach a component of d (3 in u, 2 products and 2 sums of which one operand is exact),
    at most 12 with the norm and the divide: |d - d64| <= 8 * 2^-24 * |c|, |w - w64| <= 16 * 2^-24."""
    f = rays_f64(x, y, K, pose, ids, uv=uv, opengl=opengl, pixel_center=pixel_center, normalize=normalize)
    assert out.origins.shape == out.viewdirs.shape == f["d"].shape
    assert torch.equal(out.origins.double(), f["origins"])
    err = (out.viewdirs.double() - f["viewdirs"]).abs()
    bound = 16 * EPS * torch.ones_like(err) if normalize else 8 * EPS * f["c"].norm(dim=-1, keepdim=True).expand_as(err)
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("opengl", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shared_K", [False, True])
@pytest.mark.parametrize("pose_rows", [3, 4])
def test_torch_path_matches_the_restatement(opengl, normalize, shared_K, pose_rows):
    from nerfacc_amd.rays import Rays, generate_rays
    K, pose, _ = random_cameras(5, seed=1, pose_rows=pose_rows)
    K = K[0] if shared_K else K
    x, y, ids = random_pixels(6 * 7, 5, seed=2, dtype=torch.int64 if opengl else torch.float32)
    x, y, ids = x.view(6, 7), y.view(6, 7), ids.view(6, 7)
    out = generate_rays(x, y, K, pose, ids, opengl=opengl, normalize=normalize)
    assert isinstance(out, Rays) and out.viewdirs.dtype == torch.float32 and out.viewdirs.shape == (6, 7, 3)
    check_forward(out, x, y, K, pose, ids, opengl=opengl, normalize=normalize)
    # one camera, no ids; x and y broadcast against each other; int32 pixels
    xs, ys = torch.arange(9, dtype=torch.int32)[None, :], torch.arange(4, dtype=torch.int32)[:, None]
    out = generate_rays(xs, ys, K if shared_K else K[1], pose[1], opengl=opengl, normalize=normalize, pixel_center=0.0)
    assert out.viewdirs.shape == (4, 9, 3)
    check_forward(out, xs.expand(4, 9), ys.expand(4, 9), K if shared_K else K[1], pose[1], None, opengl=opengl, normalize=normalize,
                  pixel_center=0.0)


def test_loader_expression_agrees():
    """The loaders' own expression on the same float32 inputs differs from the torch path only in the last bits."""
    from nerfacc_amd.rays import generate_rays
    import torch.nn.functional as F
    K, pose, _ = random_cameras(4, seed=3, pose_rows=4)
    x, y, ids = random_pixels(50, 4, seed=4, dtype=torch.int64)
    c2w = pose[ids]
    camera_dirs = F.pad(torch.stack([(x - K[0, 0, 2] + 0.5) / K[0, 0, 0], (y - K[0, 1, 2] + 0.5) / K[0, 1, 1] * -1.0], dim=-1),
                        (0, 1), value=-1.0)
    directions = (camera_dirs[:, None, :] * c2w[:, :3, :3]).sum(dim=-1)
    viewdirs = directions / torch.linalg.norm(directions, dim=-1, keepdims=True)
    out = generate_rays(x, y, K[0], pose, ids, opengl=True)
    assert torch.equal(out.origins, c2w[:, :3, -1]) and float((out.viewdirs - viewdirs).abs().max()) <= 4 * EPS


@pytest.mark.parametrize("lens", [None, 4, 8])
def test_gradcheck_poses_and_intrinsics(lens):
    from nerfacc_amd.rays import generate_rays
    K, pose, dist = random_cameras(3, seed=5, pose_rows=4, distortion=lens)
    x, y, ids = random_pixels(12, 3, seed=6)
    K, pose = K.double().requires_grad_(True), pose.double().requires_grad_(True)
    dist = None if dist is None else dist.double() * 3
    fn = lambda K_, P_: tuple(generate_rays(x, y, K_, P_, ids, distortion=dist, opengl=True, iters=30, eps=1e-12))
    assert torch.autograd.gradcheck(fn, (K, pose), eps=1e-6, atol=1e-6, rtol=1e-6)
    # a shared K, an unnormalised direction, a 3x4 pose
    K1, P3 = K[1].detach().requires_grad_(True), pose[:, :3].detach().requires_grad_(True)
    fn = lambda K_, P_: tuple(generate_rays(x, y, K_, P_, ids, distortion=dist, normalize=False, iters=30, eps=1e-12))
    assert torch.autograd.gradcheck(fn, (K1, P3), eps=1e-6, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("n_params", [1, 2, 4, 8])
def test_pinhole_gradient_is_autograd_through_the_newton_loop(n_params):
    """The gradient through J^-1 at the solution equals autograd through every Newton step once the loop has converged;
    the gradients also equal the restatement's per-ray terms summed by camera; the bottom row of a 4x4 gets zero."""
    from nerfacc_amd.cameras import _newton_terms, _opencv_lens_undistortion, _pad8
    from nerfacc_amd.rays import generate_rays
    K, pose, dist = random_cameras(3, seed=7, pose_rows=4, distortion=n_params)
    x, y, ids = random_pixels(40, 3, seed=8)
    dist = dist.double() * 3
    g = torch.Generator().manual_seed(9)
    go, gw = torch.randn(40, 3, generator=g, dtype=torch.float64), torch.randn(40, 3, generator=g, dtype=torch.float64)

    def through_the_loop(K_, P_):
        Kr, Pr = K_[ids], P_[ids]
        uv = torch.stack([(x - Kr[:, 0, 2] + 0.5) / Kr[:, 0, 0], (y - Kr[:, 1, 2] + 0.5) / Kr[:, 1, 1]], dim=-1)
        uv = _opencv_lens_undistortion(uv, dist[ids], eps=1e-12, iters=30)
        c = torch.stack([uv[:, 0], uv[:, 1], torch.ones_like(uv[:, 0])], dim=-1)
        d = (Pr[:, :3, :3] * c[:, None, :]).sum(-1)
        return Pr[:, :3, 3], d / d.norm(dim=-1, keepdim=True), uv

    grads = []
    for fn in (lambda K_, P_: tuple(generate_rays(x, y, K_, P_, ids, distortion=dist, iters=30, eps=1e-12)), through_the_loop):
        K_, P_ = K.double().requires_grad_(True), pose.double().requires_grad_(True)
        out = fn(K_, P_)
        grads.append(torch.autograd.grad((out[0] * go).sum() + (out[1] * gw).sum(), (K_, P_)))
    for a, b in zip(*grads):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-9 * float(b.abs().max()))
    assert not bool(grads[0][1][:, 3].any())
    uv = through_the_loop(K.double(), pose.double())[2]
    f = rays_f64(x, y, K, pose, ids, uv=uv)
    jac = _newton_terms(uv[:, 0], uv[:, 1], f["ud"], f["vd"], _pad8(dist)[ids])[2:]
    want_pose, want_K = split_grads(camera_sums(ray_terms_f64(f, go, gw, jac=jac, eps=1e-12), ids, 3)[0], pose_rows=4)
    assert torch.allclose(grads[0][0], want_K, rtol=1e-9, atol=1e-9 * float(want_K.abs().max()))
    assert torch.allclose(grads[0][1], want_pose, rtol=1e-9, atol=1e-9 * float(want_pose.abs().max()))


def test_fisheye_torch_path_inverts_the_distortion():
    from nerfacc_amd.cameras import _opencv_lens_distortion_fisheye
    from nerfacc_amd.rays import generate_rays
    K, pose, dist = random_cameras(3, seed=10, distortion="fisheye")
    x, y, ids = random_pixels(30, 3, seed=11)
    pose = pose.requires_grad_(True)
    eye = torch.eye(3, 4)
    out = generate_rays(x, y, K, eye, ids, distortion=dist, fisheye=True, normalize=False)
    back = _opencv_lens_distortion_fisheye(out.viewdirs[:, :2], dist[ids])
    want = torch.stack([(x - K[ids, 0, 2] + 0.5) / K[ids, 0, 0], (y - K[ids, 1, 2] + 0.5) / K[ids, 1, 1]], dim=-1)
    assert float((back - want).abs().max()) < 1e-5 and bool((out.viewdirs[:, 2] == 1).all())
    generate_rays(x, y, K, pose, ids, distortion=dist, fisheye=True).viewdirs.sum().backward()   # poses stay differentiable
    assert pose.grad is not None and bool(pose.grad.any())


def test_value_errors():
    from nerfacc_amd.rays import generate_rays
    K, pose, _ = random_cameras(3, seed=12)
    x, y, ids = random_pixels(10, 3, seed=13)
    d8, d4 = torch.zeros(3, 8), torch.zeros(4)
    for args, kw in (((x, y, K, pose), {}),                                        # several cameras, no ids
                     ((x, y, K[:2], pose, ids), {}),                               # 2 intrinsics, 3 poses
                     ((x, y, K[0, :2], pose, ids), {}),
                     ((x, y, K, pose[:, :, :3], ids), {}),
                     ((x, y, K, pose[:, :2], ids), {}),
                     ((x, y, K, pose, ids), dict(distortion=torch.zeros(3))),       # P = 3
                     ((x, y, K, pose, ids), dict(distortion=torch.zeros(3, 5))),
                     ((x, y, K, pose, ids), dict(distortion=torch.zeros(2, 8))),    # 2 lenses, 3 cameras
                     ((x, y, K, pose, ids), dict(distortion=d8, fisheye=True)),     # the fisheye lens takes 4
                     ((x, y, K, pose, ids), dict(fisheye=True)),
                     ((x, y.long(), K, pose, ids), {}),
                     ((x, y, K, pose, ids.float()), {}),
                     ((x, y, K.clone().requires_grad_(True), pose, ids), dict(distortion=d4, fisheye=True))):
        with pytest.raises(ValueError):
            generate_rays(*args, **kw)
    with torch.no_grad():   # nothing is differentiated: allowed
        generate_rays(x, y, K.clone().requires_grad_(True), pose, ids, distortion=d4, fisheye=True)


def test_empty_input_and_module_layout():
    import nerfacc_amd
    from nerfacc_amd import rays
    assert len(nerfacc_amd.__all__) == 22 and "generate_rays" not in nerfacc_amd.__all__
    assert rays.Rays._fields == ("origins", "viewdirs")
    K, pose, _ = random_cameras(2, seed=14)
    e = torch.empty(0, 5)
    out = rays.generate_rays(e, e, K, pose, torch.empty(0, 5, dtype=torch.int64))
    assert out.origins.shape == (0, 5, 3) and out.viewdirs.shape == (0, 5, 3)


# ------------------------------------------------------------------------------------------------ C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_FWD = "x y pixel_dtype camera_ids n_rays n_cameras K k_stride camtoworlds pose_stride distortion n_dist dist_stride fisheye " \
       "opengl pixel_center normalize eps iters origins viewdirs stream"
_BWD = "x y pixel_dtype camera_ids order n_rays n_cameras K k_stride camtoworlds pose_stride distortion n_dist dist_stride " \
       "fisheye opengl pixel_center normalize eps iters g_origins g_viewdirs partials n_partial_rows pose_floats " \
       "grad_camtoworlds grad_K stream"
_DEFAULTS = dict(pixel_dtype=0, n_rays=600, n_cameras=5, k_stride=9, pose_stride=12, distortion=None, n_dist=0, dist_stride=0,
                 fisheye=0, opengl=0, pixel_center=0.5, normalize=1, eps=1e-6, iters=10, order=None, n_partial_rows=7,
                 pose_floats=12, stream=None)
_NULLS = dict(x=None, y=None, camera_ids=None, K=None, camtoworlds=None, origins=None, viewdirs=None, order=None, g_origins=None,
              g_viewdirs=None, partials=None, grad_camtoworlds=None, grad_K=None)
_STRIDES = "strides must be 0 (one shared row) or the row length: K 9, camtoworlds 12 or 16, distortion n_dist"
_NDIST = "n_dist must be 0 (no lens) or 8 {k1,k2,p1,p2,k3,k4,k5,k6}, with fisheye 4 {k1,k2,k3,k4} (got %d)"


def _common(name):
    return [
        (dict(n_rays=-1), f"{name}: negative size"),
        (dict(n_cameras=-1), f"{name}: negative size"),
        (dict(n_cameras=(1 << 31) - 1), f"{name}: too many cameras"),
        (dict(pixel_dtype=3), f"{name}: pixel_dtype must be 0 (float32), 1 (int32) or 2 (int64)"),
        (dict(pixel_dtype=-1), f"{name}: pixel_dtype must be 0 (float32), 1 (int32) or 2 (int64)"),
        *[(dict(n_dist=p, distortion=P), f"{name}: " + _NDIST % p) for p in (1, 2, 4, 5, 12)],
        *[(dict(n_dist=p, distortion=P, fisheye=1), f"{name}: " + _NDIST % p) for p in (0, 8)],
        (dict(iters=-1), f"{name}: iters must be >= 0 (got -1)"),
        (dict(k_stride=3), f"{name}: {_STRIDES}"),
        (dict(pose_stride=9), f"{name}: {_STRIDES}"),
        (dict(dist_stride=8), f"{name}: {_STRIDES}"),
        (dict(n_dist=8, distortion=P, dist_stride=4), f"{name}: {_STRIDES}"),
        (dict(_NULLS, n_rays=0), None),
        (dict(n_cameras=0), f"{name}: rays without a camera"),
        *[({k: None}, f"{name}: null pointer") for k in "x y K camtoworlds".split()],
        (dict(n_dist=8), f"{name}: null pointer"),
        (dict(distortion=P), f"{name}: null pointer"),
        (dict(camera_ids=None), f"{name}: camera_ids may be NULL only with one camera"),
        (dict(x=P + 2), f"{name}: x, y and camera_ids must be aligned to their element size"),
        (dict(y=P + 4, pixel_dtype=2), f"{name}: x, y and camera_ids must be aligned to their element size"),
        (dict(camera_ids=P + 4), f"{name}: x, y and camera_ids must be aligned to their element size"),
    ]


_CASES = [
    ("nfa_generate_rays_fwd", _FWD, _common("generate_rays_fwd") + [
        (dict(origins=None), "generate_rays_fwd: null pointer"),
        (dict(viewdirs=None), "generate_rays_fwd: null pointer"),
        (dict(viewdirs=P + 2), "generate_rays_fwd: origins and viewdirs must be 4-byte aligned"),
    ]),
    ("nfa_generate_rays_bwd", _BWD, _common("generate_rays_bwd") + [
        (dict(pose_floats=9), "generate_rays_bwd: pose_floats must be 12 or 16 (got 9)"),
        (dict(n_dist=4, distortion=P, fisheye=1), "generate_rays_bwd: no gradient towards K through the fisheye lens"),
        (dict(g_origins=None, g_viewdirs=None), "generate_rays_bwd: null pointer"),
        (dict(partials=None), "generate_rays_bwd: null pointer"),
        (dict(grad_camtoworlds=None, grad_K=None), "generate_rays_bwd: null pointer"),
        (dict(n_partial_rows=6),
         "generate_rays_bwd: partials must hold ceil(n_rays / chunk) + n_cameras - 1 = 7 rows (got 6)"),
    ]),
]


def test_abi_symbols_and_argument_errors():
    """The entry points are exported, bound, and reject bad arguments with a fixed text before anything reaches the GPU."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert lib.nfa_version() == B.ABI_VERSION == 403
    assert lib.nfa_generate_rays_chunk() == 256 and "nfa_generate_rays_chunk" in B.EXPORTED_SYMBOLS
    for fn, names, cases in _CASES:
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        assert len(B._SIGS[fn]) == len(names.split())
        for kw, msg in cases:
            args = [kw[a] if a in kw else _DEFAULTS[a] if a in _DEFAULTS else P for a in names.split()]
            lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
            rc = getattr(lib, fn)(*args)
            if msg is None:
                assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
            else:
                assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())

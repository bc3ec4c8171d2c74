"""GPU: nerfacc_amd.rays.generate_rays on the native ops nfa_generate_rays_{fwd,bwd} -- the fused undistortion bit for bit
against nerfacc_amd.cameras, the directions against the float64 restatement under the rounding-count bounds, the
per-camera gradients exactly on integer data (run and chunk boundaries, shuffled ids), within the summation bound on random
data, determinism, the chain through sampling() and sample_positions, dispatch, host reads and graph capture."""
import pytest
import torch

from rays_reference import EPS, camera_sums, random_cameras, random_pixels, ray_terms_f64, rays_f64, split_grads

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 4099]
CAMERAS = [1, 3, 300]


def to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def skipped(n_cameras):
    return (1,) if n_cameras == 3 else ()   # with 3 cameras, camera 1 owns no ray; of 300, many own none at the small sizes


def strided(t):
    """The same values seen through a stride of 2 elements."""
    buf = torch.empty(t.numel() * 2, dtype=t.dtype, device=t.device)
    buf[::2] = t
    return buf[::2]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n_cameras", CAMERAS)
@pytest.mark.parametrize("lens", ["pinhole", "fisheye"])
def test_fused_undistortion_is_the_camera_ops_bit_for_bit(dev, n_cameras, lens):
    """K = I, pixel_center 0, R = I, no normalisation: (u, v) is the pixel itself, d = (u', v', 1) exactly."""
    from nerfacc_amd import cameras
    from nerfacc_amd.rays import generate_rays
    _, pose, dist = random_cameras(n_cameras, seed=20, distortion="fisheye" if lens == "fisheye" else 8)
    pose[:, :3, :3] = torch.eye(3)
    K = torch.eye(3)
    undistort = cameras.opencv_lens_undistortion_fisheye if lens == "fisheye" else cameras.opencv_lens_undistortion
    K, pose, dist = to(dev, K, pose, dist * 3)
    for n in SIZES:
        x, y, ids = to(dev, *random_pixels(n, n_cameras, seed=21 + n, skip=skipped(n_cameras)))
        x, y = strided(x / 800 - 0.5), y / 600 - 0.5
        assert n < 2 or not x.is_contiguous()
        if n_cameras == 1:
            out = generate_rays(x, y, K, pose[0], distortion=dist[0], fisheye=lens == "fisheye", pixel_center=0.0, normalize=False)
            want = undistort(torch.stack([x, y], dim=-1), dist[0])
        else:
            out = generate_rays(x, y, K, pose, ids, distortion=dist, fisheye=lens == "fisheye", pixel_center=0.0, normalize=False)
            want = undistort(torch.stack([x, y], dim=-1), dist[ids])
        assert out.viewdirs.shape == (n, 3) and torch.equal(out.viewdirs[:, :2], want)
        assert bool((out.viewdirs[:, 2] == 1).all())
        assert torch.equal(out.origins, pose[ids if n_cameras > 1 else torch.zeros_like(ids), :3, 3])
        if n > 1 and n_cameras == 3:   # the lens did something
            assert not torch.equal(want, torch.stack([x, y], dim=-1))


@pytest.mark.parametrize("n_cameras", CAMERAS)
@pytest.mark.parametrize("lens", [None, "pinhole", "fisheye"])
@pytest.mark.parametrize("opengl,normalize,pixels,pose_rows", [(False, True, torch.float32, 3), (True, False, torch.int64, 4),
                                                               (True, True, torch.int32, 3), (False, False, torch.float32, 4)])
def test_directions_within_the_rounding_bounds(dev, n_cameras, lens, opengl, normalize, pixels, pose_rows):
    """Against float64 from the same float32 inputs (with a lens: from the native undistortion's own (u, v), so that the
    solver's tolerance, which tests/test_cameras_gpu.py owns, stays out): at most 6 roundings reach a component of d, 12
    with the norm and the divide: |d - d64| <= 8 * 2^-24 * |c|, |w - w64| <= 16 * 2^-24.  origins: bit-identical."""
    from nerfacc_amd import cameras
    from nerfacc_amd.rays import generate_rays
    K, pose, dist = random_cameras(n_cameras, seed=30, pose_rows=pose_rows, distortion={None: None, "pinhole": 4, "fisheye": "fisheye"}[lens])
    K, pose, dist = to(dev, K, pose, dist)
    shared_K = n_cameras == 3 and lens is None
    for n in SIZES:
        x, y, ids = to(dev, *random_pixels(n, n_cameras, seed=31 + n, dtype=pixels, skip=skipped(n_cameras)))
        one = n_cameras == 1
        Kc, Pc, Dc = (K[0] if shared_K or one else K), (pose[0] if one else pose), (None if dist is None else dist[0] if one else dist)
        out = generate_rays(strided(x), y, Kc, Pc, None if one else ids, distortion=Dc, fisheye=lens == "fisheye", opengl=opengl,
                            normalize=normalize)
        uv = None
        if lens is not None:   # (x - cx + 0.5) / fx in float32 is the kernel's own sequence of correctly rounded operations
            Kr = Kc if Kc.dim() == 2 else Kc[ids]
            uvd = torch.stack([(x.float() - Kr[..., 0, 2] + 0.5) / Kr[..., 0, 0], (y.float() - Kr[..., 1, 2] + 0.5) / Kr[..., 1, 1]], dim=-1)
            fn = cameras.opencv_lens_undistortion_fisheye if lens == "fisheye" else cameras.opencv_lens_undistortion
            uv = fn(uvd, Dc if one else Dc[ids])
        f = rays_f64(x, y, Kc, Pc, ids, uv=uv, opengl=opengl, normalize=normalize)
        assert out.viewdirs.shape == (n, 3) and torch.equal(out.origins.double(), f["origins"])
        err = (out.viewdirs.double() - f["viewdirs"]).abs()
        bound = 16 * EPS * torch.ones_like(err) if normalize else 8 * EPS * f["c"].norm(dim=-1, keepdim=True).expand_as(err)
        assert bool((err <= bound).all()), (n, float((err / bound).max()))


def test_leading_shape_and_out_of_range_ids(dev):
    from nerfacc_amd.rays import generate_rays
    K, pose, _ = to(dev, *random_cameras(3, seed=40))
    x, y, ids = to(dev, *random_pixels(35, 3, seed=41, dtype=torch.int64))
    flat = generate_rays(x, y, K, pose, ids)
    out = generate_rays(x.view(5, 7), y.view(5, 7), K, pose, ids.view(5, 7))
    assert out.origins.shape == (5, 7, 3) and torch.equal(out.viewdirs.view(35, 3), flat.viewdirs)
    bad = ids.clone()
    bad[3], bad[20] = -1, 3
    out = generate_rays(x, y, K, pose, bad)
    nan = torch.isnan(out.viewdirs).all(-1) & torch.isnan(out.origins).all(-1)
    assert nan.nonzero().flatten().tolist() == [3, 20]


# ------------------------------------------------------------------------------------------------ backward: exact data
def integer_case(n, ids, n_cameras, seed, opengl):
    """Inputs whose every per-ray term and partial sum is an integer below 2^24 (CPU tensors) and the int64 gradients:
    signed permutation rotations, fx = fy = 1, integer cx, cy, pixels and incoming gradients, no normalisation."""
    g = torch.Generator().manual_seed(seed)
    K = torch.zeros(n_cameras, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = K[:, 2, 2] = 1
    K[:, 0, 2], K[:, 1, 2] = torch.randint(0, 8, (n_cameras,), generator=g), torch.randint(0, 8, (n_cameras,), generator=g)
    R = torch.zeros(n_cameras, 3, 3, dtype=torch.int64)
    for c in range(n_cameras):
        R[c, torch.arange(3), torch.randperm(3, generator=g)] = torch.randint(0, 2, (3,), generator=g) * 2 - 1
    pose = torch.cat([R.float(), torch.randint(-4, 5, (n_cameras, 3, 1), generator=g).float()], dim=-1)
    x, y = torch.randint(0, 32, (n,), generator=g), torch.randint(0, 32, (n,), generator=g)
    go, gw = torch.randint(-3, 4, (n, 3), generator=g), torch.randint(-3, 4, (n, 3), generator=g)
    s = -1 if opengl else 1
    Ki = K.long()[ids]
    u, v = x - Ki[:, 0, 2], y - Ki[:, 1, 2]                        # pixel_center 0, fx = fy = 1
    c = torch.stack([u, s * v, torch.full_like(u, s)], dim=-1)
    Rr = R[ids]
    pose_terms = torch.cat([gw[:, :, None] * c[:, None, :], go[:, :, None]], dim=-1).reshape(n, 12)
    gc = (Rr * gw[:, :, None]).sum(1)
    gu, gv = gc[:, 0], s * gc[:, 1]
    terms = torch.cat([pose_terms, torch.stack([-gu * u, -gv * v, -gu, -gv], dim=-1)], dim=-1)
    want = torch.zeros(n_cameras, 16, dtype=torch.int64).index_add(0, ids, terms)
    assert int(torch.zeros(n_cameras, 16, dtype=torch.int64).index_add(0, ids, terms.abs()).max()) < 2 ** 24
    return dict(x=x, y=y, ids=ids, K=K, pose=pose, go=go.float(), gw=gw.float(), opengl=opengl), want


def native_grads(dev, c, ids, mark=False, one_camera=False):
    """(grad K, grad camtoworlds) of sum(origins * go) + sum(viewdirs * gw) for the case's rays taken with ``ids``."""
    from nerfacc_amd.rays import generate_rays, mark_sorted
    K, pose = (c[k].to(dev).requires_grad_(True) for k in ("K", "pose"))
    x, y, go, gw = to(dev, c["x"], c["y"], c["go"], c["gw"])
    ids = ids.to(dev)
    if mark:
        mark_sorted(ids)
    out = generate_rays(x, y, K[0] if one_camera else K, pose[0] if one_camera else pose, None if one_camera else ids,
                        opengl=c["opengl"], pixel_center=0.0, normalize=False)
    return torch.autograd.grad((out.origins * go).sum() + (out.viewdirs * gw).sum(), (K, pose))


def assert_exact(got, want, n_cameras):
    gk, gp = got
    want_pose, want_K = split_grads(want)
    assert gk.shape == (n_cameras, 3, 3) and gp.shape == (n_cameras, 3, 4)
    assert torch.equal(gk.cpu().long(), want_K) and torch.equal(gk.cpu(), want_K.float())
    assert torch.equal(gp.cpu().long(), want_pose) and torch.equal(gp.cpu(), want_pose.float())


def exact_id_sets():
    """name -> (n, sorted ids, n_cameras): one camera with every ray; 300 cameras (some empty) over 4099 rays; and around
    the chunk size, camera 0 ending exactly on the first chunk's boundary, camera 1 empty."""
    from nerfacc_amd.rays import reduction_chunk
    ch = reduction_chunk()
    g = torch.Generator().manual_seed(50)
    sets = {"one": (4099, torch.zeros(4099, dtype=torch.int64), 1)}
    ids = torch.randint(0, 300, (4099,), generator=g)
    ids[ids % 7 == 3] += 1
    sets["many"] = (4099, ids.sort().values, 300)
    for n in (ch - 1, ch, ch + 1, 2 * ch + 1):
        ids = torch.zeros(n, dtype=torch.int64)
        ids[ch:] = 2 + torch.randint(0, 3, (max(n - ch, 0),), generator=g).sort().values
        sets[f"chunk{n - ch:+d}" if n <= ch + 1 else "two_chunks+1"] = (n, ids, 5)
    return sets


@pytest.mark.parametrize("name", ["one", "many", "chunk-1", "chunk+0", "chunk+1", "two_chunks+1"])
@pytest.mark.parametrize("opengl", [False, True])
def test_gradients_are_exact_on_integer_data(dev, name, opengl):
    n, ids, n_cameras = exact_id_sets()[name]
    c, want = integer_case(n, ids, n_cameras, seed=51, opengl=opengl)
    assert name != "many" or int((want.abs().sum(1) == 0).sum()) > 10   # cameras without rays
    assert_exact(native_grads(dev, c, ids, one_camera=name == "one"), want, n_cameras)   # sorted ids, not marked: through the sort
    marked = native_grads(dev, c, ids, mark=True, one_camera=name == "one")
    assert_exact(marked, want, n_cameras)
    # the same rays shuffled: the stable sort brings them into camera order, and the bits are those of the sorted run
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(52))
    cs = dict(c, **{k: c[k][perm] for k in ("x", "y", "go", "gw")})
    shuffled = native_grads(dev, cs, ids[perm], one_camera=name == "one")
    assert torch.equal(shuffled[0], marked[0]) and torch.equal(shuffled[1], marked[1])


# ------------------------------------------------------------------------------------------------ backward: random data
def random_case(dev, n_cameras, per_camera, seed, lens, pose_rows=3):
    K, pose, dist = random_cameras(n_cameras, seed=seed, pose_rows=pose_rows, distortion=lens)
    g = torch.Generator().manual_seed(seed + 1)
    n = n_cameras * per_camera
    x, y, _ = random_pixels(n, n_cameras, seed=seed + 2)
    ids = torch.arange(n_cameras).repeat_interleave(per_camera)
    ids[ids == 2] = 3   # camera 2 owns no ray, camera 3 twice as many: at most 64 per camera with per_camera = 32
    go, gw = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    return dict(zip("K pose dist x y ids go gw".split(), to(dev, K, pose, None if dist is None else dist * 3, x, y, ids, go, gw)))


def run_random(c, ids_order=None, **kw):
    from nerfacc_amd.rays import generate_rays
    K, pose = c["K"].detach().clone().requires_grad_(True), c["pose"].detach().clone().requires_grad_(True)
    sel = slice(None) if ids_order is None else ids_order
    out = generate_rays(c["x"][sel], c["y"][sel], K, pose, c["ids"][sel], distortion=c["dist"], **kw)
    return torch.autograd.grad((out.origins * c["go"][sel]).sum() + (out.viewdirs * c["gw"][sel]).sum(), (K, pose))


@pytest.mark.parametrize("opengl,normalize,lens,pose_rows", [(False, True, None, 3), (True, False, None, 4), (True, True, 8, 4),
                                                             (False, False, 4, 3), (False, True, 2, 3)])
def test_gradients_on_random_data(dev, opengl, normalize, lens, pose_rows):
    """|got - ref| <= (n_cam + 16) * 2^-24 * sum |term| per entry, the sums in float64 over at most n_cam = 64 rays of a
    camera: the first-order worst case of any summation order plus the roundings of a term.  The reference takes the native
    undistortion's own (u, v) and the float64 Jacobian there."""
    from nerfacc_amd import cameras
    c = random_case(dev, 40, 32, seed=60, lens=lens, pose_rows=pose_rows)
    gk, gp = run_random(c, opengl=opengl, normalize=normalize)
    uv = jac = None
    if lens:
        Kr = c["K"][c["ids"]]
        uvd = torch.stack([(c["x"] - Kr[:, 0, 2] + 0.5) / Kr[:, 0, 0], (c["y"] - Kr[:, 1, 2] + 0.5) / Kr[:, 1, 1]], dim=-1)
        params = cameras._pad8(c["dist"])[c["ids"]]
        uv = cameras.opencv_lens_undistortion(uvd, params)
        jac = cameras._newton_terms(uv[:, 0].double(), uv[:, 1].double(), uvd[:, 0].double(), uvd[:, 1].double(), params.double())[2:]
    f = rays_f64(c["x"], c["y"], c["K"], c["pose"], c["ids"], uv=uv, opengl=opengl, normalize=normalize)
    ref, ref_abs = camera_sums(ray_terms_f64(f, c["go"], c["gw"], normalize=normalize, jac=jac), c["ids"], 40)
    n_cam = int(torch.bincount(c["ids"]).max())
    assert n_cam == 64
    (want_pose, want_K), (abs_pose, abs_K) = split_grads(ref, pose_rows), split_grads(ref_abs, pose_rows)
    for got, want, scale, what in ((gp, want_pose, abs_pose, "camtoworlds"), (gk, want_K, abs_K, "K")):
        err, bound = (got.double() - want).abs(), (n_cam + 16) * EPS * scale
        print(what, "max |got - ref| / bound:", float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), (what, float((err / bound.clamp(min=1e-300)).max()))
        assert bool((got[scale == 0] == 0).all())   # the empty camera, the bottom row, the entries of K that are constants
    assert not bool(gp[2].any()) and not bool(gk[2].any()) and bool(gk[3, 0, 0] != 0)


def test_backward_is_deterministic(dev):
    c = random_case(dev, 40, 32, seed=70, lens=8)
    perm = torch.randperm(c["ids"].numel(), generator=torch.Generator().manual_seed(71)).to(dev)
    for order in (None, perm):
        a, b = run_random(c, order), run_random(c, order)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    from nerfacc_amd.rays import generate_rays
    big = random_case(dev, 1, 4099, seed=72, lens=None)
    runs = []
    for _ in range(2):
        K, pose = big["K"][0].clone().requires_grad_(True), big["pose"][0].clone().requires_grad_(True)
        out = generate_rays(big["x"], big["y"], K, pose)
        runs.append(torch.autograd.grad((out.origins * big["go"]).sum() + (out.viewdirs * big["gw"]).sum(), (K, pose)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][0].shape == (3, 3)


def test_shared_intrinsics_sum_over_cameras(dev):
    """One K for every camera: its gradient is the sum of the per-camera ones."""
    from nerfacc_amd.rays import generate_rays
    c = random_case(dev, 40, 32, seed=80, lens=None)
    per = run_random(dict(c, K=c["K"][:1].expand(40, 3, 3).contiguous()))
    K, pose = c["K"][0].clone().requires_grad_(True), c["pose"].clone().requires_grad_(True)
    out = generate_rays(c["x"], c["y"], K, pose, c["ids"])
    gk, gp = torch.autograd.grad((out.origins * c["go"]).sum() + (out.viewdirs * c["gw"]).sum(), (K, pose))
    assert gk.shape == (3, 3) and torch.equal(gp, per[1]) and torch.equal(gk, per[0].view(40, 9).sum(0).view(3, 3))


# ------------------------------------------------------------------------------------------------ with the rest of the library
def test_chain_through_sampling_and_sample_positions(dev):
    """generate_rays -> OccGridEstimator.sampling -> sample_positions -> a scalar loss; the gradient at camtoworlds against
    the float64 torch composition on the same samples.  Two float32 stages of sums: S <= 64 samples of a ray (the segmented
    engine), then the n_cam rays of a camera; with the per-term roundings the first-order bound per entry is
    (S + 16 + n_cam + 16) * 2^-24 * sum |elementary term|, the terms taken through the normalisation with absolute values.
    A second run gives the same bits."""
    import nerfacc_amd as na
    from nerfacc_amd.rays import generate_rays
    from nerfacc_amd.samples import sample_positions
    n_cameras, n = 3, 257
    K, pose, _ = random_cameras(n_cameras, seed=90)
    pose[:, :3, 3] = pose[:, :3, 3] / 10 - 2.5 * pose[:, :3, 2]   # about 2.5 in front of the box, looking at it
    K, pose = to(dev, K, pose)
    x, y, ids = to(dev, *random_pixels(n, n_cameras, seed=91))
    est = na.OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=16).to(dev)
    est.binaries = torch.ones_like(est.binaries)
    est.occs = torch.ones_like(est.occs)
    runs = []
    for _ in range(2):
        P = pose.clone().requires_grad_(True)
        rays = generate_rays(x, y, K, P, ids)
        ri, ts, te = est.sampling(rays.origins.detach(), rays.viewdirs.detach(), render_step_size=0.08)
        gx = torch.randn(ts.numel(), 3, generator=torch.Generator().manual_seed(92)).to(dev)
        pos = sample_positions(rays.origins, rays.viewdirs, ts, te, ri).positions
        runs.append(torch.autograd.grad((pos * gx).sum(), P)[0])
    assert torch.equal(runs[0], runs[1]) and ri.numel() > 4 * n
    S = int(torch.bincount(ri, minlength=n).max())
    n_cam = int(torch.bincount(ids).max())
    assert S <= 64
    # float64 composition on the same samples
    P64 = pose.double().requires_grad_(True)
    f = rays_f64(x, y, K, P64, ids)
    tm = ((ts.double() + te.double()) / 2)[:, None]
    want = torch.autograd.grad(((f["origins"][ri] + f["viewdirs"][ri] * tm) * gx.double()).sum(), P64)[0]
    # sum |term|: |g_origins| and |g_viewdirs| per ray from absolute sample terms, then through |dw/dd| with absolute values
    z = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    A_o, A_w = z.index_add(0, ri, gx.double().abs()), z.index_add(0, ri, (gx.double() * tm).abs())
    f = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in f.items()}
    nrm = f["d"].norm(dim=-1, keepdim=True)
    w = (f["d"] / nrm).abs()
    G_d = (A_w + w * (w * A_w).sum(-1, keepdim=True)) / nrm
    terms_abs = torch.cat([G_d[:, :, None] * f["c"].abs()[:, None, :], A_o[:, :, None]], dim=-1).reshape(n, 12)
    scale = torch.zeros(n_cameras, 12, dtype=torch.float64, device=dev).index_add(0, ids, terms_abs).view(n_cameras, 3, 4)
    err, bound = (runs[0].double() - want).abs(), (S + 16 + n_cam + 16) * EPS * scale
    print("chain: max |got - ref| / bound:", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


def test_native_path_taken_without_host_reads(dev, monkeypatch):
    """Both directions go to the native entry points -- shuffled ids through the device sort -- and nothing in them waits
    for the device (torch's synchronisation check set to raise)."""
    from nerfacc_amd import _backend as B
    c = random_case(dev, 40, 32, seed=100, lens=8)
    perm = torch.randperm(c["ids"].numel(), generator=torch.Generator().manual_seed(101)).to(dev)
    run_random(c, perm)   # (libraries loaded, allocator warm)
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run_random(c, perm)
        run_random(c)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [name for name, _ in calls] == ["nfa_generate_rays_fwd", "nfa_generate_rays_bwd"] * 2
    assert calls[1][1][4] is not None and calls[1][1][3] is not None   # sorted on the device: an order and sorted ids


def test_forward_and_backward_capture_into_a_graph(dev):
    """One camera, and ids marked sorted: forward + backward capture (nerfacc_amd.CapturedStep) and every replay gives the
    eager step's bits.  In a child process, as the other capture tests: a capture that fails takes its process down."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from nerfacc_amd.graphs import CapturedStep
from nerfacc_amd.rays import generate_rays, mark_sorted
import test_rays_gpu as T
dev = torch.device("cuda:0")
c = T.random_case(dev, 40, 32, seed=110, lens=8)
mark_sorted(c["ids"])
def leaves():
    return [c[k].detach().clone().requires_grad_(True) for k in ("K", "pose")]
def step(xs):
    K, pose = xs
    a = generate_rays(c["x"], c["y"], K, pose, c["ids"], distortion=c["dist"])
    b = generate_rays(c["x"], c["y"], K[0], pose[0], opengl=True)
    loss = (a.origins * c["go"]).sum() + (a.viewdirs * c["gw"]).sum() + (b.viewdirs * c["gw"]).sum()
    return (a.viewdirs.detach(), b.viewdirs.detach(), *torch.autograd.grad(loss, xs))
# (leaves first used inside the capture: see tests/test_samples_gpu.py)
xs = leaves()
graph = CapturedStep(lambda: step(xs), warmup=2)
eager = step(leaves())
ok = True
for _ in range(2):
    got = graph()
    torch.cuda.synchronize()
    ok = ok and len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, eager))
print("OK captured", ok, graph.replays)
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK captured True 2" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-500:])

"""GPU: nerfacc_amd.photometric on the native entries nfa_photometric_{fwd,bwd} -- the targets bit for bit against the CPU
path, loss and MSE bit for bit against the numpy reference on exact data and within one float32 ulp on random data, the
gradient bit for bit for every kind and element type, determinism, input forms, dispatch without host reads, byte offsets
beyond 4 GiB, and a captured training step."""
import functools

import numpy as np
import pytest
import torch

import photometric_reference as R

pytestmark = pytest.mark.gpu

STACK = (3, 5, 7)


@functools.lru_cache(maxsize=None)
def sizes():
    from nerfacc_amd.photometric import reduction_chunk
    c = reduction_chunk()
    # around a wave, around a chunk, several chunks with a tail, and more partials (65) than the finish kernel has lanes
    return (1, 63, 65, c - 1, c, c + 1, 3 * c + 7, 64 * c + 5)


def T(a, dev="cpu"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def case(n, C=4, seed=0):
    """Inputs of n rays (numpy) and the numpy reference's targets for a shared background."""
    stack = R.random_stack(100 + seed, STACK + (C,))
    ids, y, x = R.random_indices(101 + seed + n, n)
    r = np.random.default_rng(102 + seed + n)
    c = dict(stack=stack, ids=ids, x=x, y=y, rgb=r.random((n, 3), dtype=np.float32) * 1.5 - 0.25, bkgd=r.random(3, dtype=np.float32),
             bkgd_n=r.random((n, 3), dtype=np.float32), w=r.random(n, dtype=np.float32) * 2)
    c["pixels"] = R.target(stack, ids, x, y, bkgd=c["bkgd"])
    return c


def ulps(a, b):
    """Distance of two positive float32 values in units of the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ------------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bkgd", ["none", "shared", "per_ray"])
def test_pixels_are_the_cpu_path_bit_for_bit(dev, C, index_dtype, bkgd):
    from nerfacc_amd.photometric import photometric_loss, target_pixels
    for n in (0,) + sizes():
        c = case(n, C)
        b = {"none": None, "shared": c["bkgd"], "per_ray": c["bkgd_n"]}[bkgd]
        idx = [T(c[k]).to(index_dtype) for k in ("ids", "x", "y")]
        want = target_pixels(T(c["stack"]), *idx, T(b))
        got = target_pixels(T(c["stack"], dev), *(t.to(dev) for t in idx), T(b, dev))
        assert got.is_cuda and got.shape == (n, 3) and torch.equal(R.bits(got), R.bits(want)), n
        if C == 4 and bkgd == "shared":
            assert torch.equal(R.bits(want), R.bits(T(c["pixels"])))
        # the same targets through the loss entry, and from ready float pixels / rgba
        out = photometric_loss(T(c["rgb"], dev), images=T(c["stack"], dev), image_ids=idx[0].to(dev), x=idx[1].to(dev), y=idx[2].to(dev),
                               color_bkgd=T(b, dev))
        assert torch.equal(R.bits(out.pixels), R.bits(want)), n
        rgba = (T(c["stack"])[idx[0].long(), idx[2].long(), idx[1].long()] / 255.0).to(dev)
        out = photometric_loss(T(c["rgb"], dev), pixels=rgba, color_bkgd=T(b, dev))
        assert torch.equal(R.bits(out.pixels), R.bits(want)), n
    # the whole image of an int id, in row-major order
    c = case(35, C)
    b = {"none": None, "shared": c["bkgd"], "per_ray": c["bkgd_n"].reshape(5, 7, 3)}[bkgd]
    got = target_pixels(T(c["stack"], dev), 2, color_bkgd=T(b, dev))
    assert got.shape == (5, 7, 3) and torch.equal(R.bits(got), R.bits(target_pixels(T(c["stack"]), 2, color_bkgd=T(b))))


# ------------------------------------------------------------------------------------------------ loss and mse
def test_loss_and_mse_are_exact_on_exact_data(dev):
    """rgb and targets multiples of 2^-6 in [0, 1], beta = 1: every term and every sum is exact in any order, so loss and
    mse are the numpy reference's bits at every size; N = 0 gives NaN and launches nothing."""
    from nerfacc_amd.photometric import photometric_loss
    for n in sizes():
        rgb, pix = R.exact_case(200 + n, n)
        want_loss, want_mse, want_ray = R.forward(rgb, pix, "smooth_l1", 1.0)
        for dt in (torch.float32, torch.float16, torch.bfloat16):   # multiples of 2^-6 below 1 need 6 bits: exact in all three
            out = photometric_loss(T(rgb, dev).to(dt), pixels=T(pix, dev), per_ray=True)
            assert out.loss.dtype == torch.float32 and out.loss.shape == ()
            assert out.loss.item() == want_loss and out.mse.item() == want_mse, (n, dt, out.loss.item(), want_loss)
            assert torch.equal(R.bits(out.per_ray), R.bits(T(want_ray))) and torch.equal(R.bits(out.pixels), R.bits(T(pix)))
    empty = photometric_loss(torch.zeros(0, 3, device=dev, requires_grad=True), pixels=torch.zeros(0, 3, device=dev), per_ray=True)
    assert torch.isnan(empty.loss) and torch.isnan(empty.mse) and empty.pixels.shape == (0, 3) and empty.per_ray.shape == (0,)
    empty.loss.backward()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_and_mse_within_one_ulp_on_random_data(dev, kind, weighted):
    """The float32 terms are the reference's; the float64 sums differ from numpy's in order only (relative 2^-53 per
    addition), so after the one rounding to float32 the results differ by at most one ulp.  per_ray: bit for bit."""
    from nerfacc_amd.photometric import photometric_loss
    for n in sizes():
        c = case(n)
        w = c["w"] if weighted else None
        out = photometric_loss(T(c["rgb"], dev), images=T(c["stack"], dev), image_ids=T(c["ids"], dev), x=T(c["x"], dev),
                               y=T(c["y"], dev), color_bkgd=T(c["bkgd"], dev), kind=kind, beta=R.PARAMS[kind], weights=T(w, dev),
                               per_ray=True)
        loss, mse, per_ray = R.forward(c["rgb"], c["pixels"], kind, R.PARAMS[kind], w)
        print(f"{kind} n={n}: loss {out.loss.item()!r} ref {loss!r} ({ulps(out.loss.item(), loss)} ulp), "
              f"mse {ulps(out.mse.item(), mse)} ulp")
        assert ulps(out.loss.item(), loss) <= 1 and ulps(out.mse.item(), mse) <= 1
        assert torch.equal(R.bits(out.per_ray), R.bits(T(per_ray)))


# ------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_is_the_reference_bit_for_bit(dev, kind, dtype, weighted):
    """dL/drgb with a device scalar of 1024 arriving at the loss, as DeviceGradScaler.scale produces."""
    from nerfacc_amd.photometric import photometric_loss
    scale = torch.tensor(1024.0, device=dev)
    for n in sizes():
        c = case(n)
        w = c["w"] if weighted else None
        rgb = T(c["rgb"]).to(dtype)
        r32 = rgb.float().numpy()
        leaf = rgb.to(dev).requires_grad_(True)
        out = photometric_loss(leaf, pixels=T(c["pixels"], dev), kind=kind, beta=R.PARAMS[kind], weights=T(w, dev))
        (out.loss * scale).backward()
        want = R.rounded(R.backward(r32, c["pixels"], kind, R.PARAMS[kind], 1024.0, w), dtype)
        assert leaf.grad.dtype == dtype and leaf.grad.shape == (n, 3)
        assert torch.equal(R.bits(leaf.grad), R.bits(want)), (n, int((R.bits(leaf.grad) != R.bits(want)).sum()))
        assert ulps(out.loss.item(), R.forward(r32, c["pixels"], kind, R.PARAMS[kind], w)[0]) <= 1
        assert not out.mse.requires_grad and not out.pixels.requires_grad


def test_two_runs_give_the_same_bits(dev):
    from nerfacc_amd.photometric import photometric_loss
    c = case(sizes()[-1])
    args = {k: T(c[k], dev) for k in ("stack", "ids", "x", "y", "bkgd_n", "w", "rgb")}
    runs = []
    for _ in range(2):
        leaf = args["rgb"].clone().requires_grad_(True)
        out = photometric_loss(leaf, images=args["stack"], image_ids=args["ids"], x=args["x"], y=args["y"], color_bkgd=args["bkgd_n"],
                               weights=args["w"], kind="charbonnier", beta=1e-3, per_ray=True)
        out.loss.backward()
        runs.append((out.loss, out.mse, out.pixels, out.per_ray, leaf.grad))
    assert all(torch.equal(R.bits(a), R.bits(b)) for a, b in zip(*runs))


def test_non_contiguous_and_broadcast_inputs(dev):
    from nerfacc_amd.photometric import photometric_loss
    c = case(35)
    stack, bkgd = T(c["stack"], dev), T(c["bkgd"], dev)
    yy, xx = torch.meshgrid(torch.arange(5, device=dev), torch.arange(7, device=dev), indexing="ij")
    rgb = T(c["rgb"], dev)
    flat = photometric_loss(rgb, images=stack, image_ids=torch.ones(35, dtype=torch.int64, device=dev), x=xx.reshape(-1), y=yy.reshape(-1),
                            color_bkgd=bkgd, weights=torch.full((35,), 0.5, device=dev), per_ray=True)
    wide = torch.zeros(5, 7, 6, device=dev)
    wide[..., ::2] = rgb.view(5, 7, 3)
    leaf = wide.requires_grad_(True)
    # a strided rgb of shape (5, 7, 3), ids as a 0-dim tensor, x along a row, y down a column, an expanded weight, a (7, 3) background
    out = photometric_loss(leaf[..., ::2], images=stack, image_ids=torch.tensor(1, device=dev), x=torch.arange(7, device=dev),
                           y=torch.arange(5, device=dev)[:, None], color_bkgd=bkgd.expand(7, 3), weights=torch.tensor(0.5, device=dev),
                           per_ray=True)
    assert out.pixels.shape == (5, 7, 3) and out.per_ray.shape == (5, 7)
    for a, b in zip(out, flat):
        assert torch.equal(R.bits(a.reshape(-1)), R.bits(b.reshape(-1)))
    out.loss.backward()
    assert leaf.grad.shape == (5, 7, 6) and bool((leaf.grad[..., ::2] != 0).any()) and not bool(leaf.grad[..., 1::2].any())
    # an int id and no x, y; an rgb whose base is not 16-byte aligned (the element-by-element form): the same bits
    whole = photometric_loss(rgb.view(5, 7, 3), images=stack, image_ids=1, color_bkgd=bkgd, weights=torch.tensor(0.5, device=dev))
    assert torch.equal(whole.loss, flat.loss) and torch.equal(whole.pixels.view(35, 3), flat.pixels)
    # float64 rgb takes the torch restatement on the device: the CPU path's bits (a true division by 255 there too)
    f64 = photometric_loss(rgb.double(), images=stack, image_ids=1, color_bkgd=bkgd)
    cpu = photometric_loss(rgb.double().cpu(), images=stack.cpu(), image_ids=1, color_bkgd=bkgd.cpu())
    assert f64.loss.dtype == torch.float64 and f64.loss.is_cuda and torch.equal(f64.pixels.cpu(), cpu.pixels)
    shifted = torch.zeros(36 * 3 + 1, device=dev)[1:].view(36, 3)
    shifted[:35] = rgb
    assert shifted.data_ptr() % 16 != 0
    off = photometric_loss(shifted[:35], pixels=flat.pixels, weights=torch.full((35,), 0.5, device=dev))
    assert torch.equal(off.loss, flat.loss) and torch.equal(off.mse, flat.mse)


def test_native_entries_are_called_without_host_reads(dev, monkeypatch):
    from nerfacc_amd import _backend as B
    from nerfacc_amd.photometric import photometric_loss, psnr, target_pixels
    c = case(sizes()[4])
    args = {k: T(c[k], dev) for k in ("stack", "ids", "x", "y", "bkgd", "w", "rgb")}
    scale = torch.tensor(1024.0, device=dev)

    def run(dtype):
        leaf = args["rgb"].detach().to(dtype).clone().requires_grad_(True)
        out = photometric_loss(leaf, images=args["stack"], image_ids=args["ids"], x=args["x"], y=args["y"], color_bkgd=args["bkgd"],
                               weights=args["w"], per_ray=True)
        (out.loss * scale).backward()
        return psnr(out.mse)

    run(torch.float32), run(torch.float16)   # (library loaded, allocator warm)
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run(torch.float32)
        run(torch.float16)
        target_pixels(args["stack"], args["ids"], args["x"], args["y"], args["bkgd"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == ["nfa_photometric_fwd", "nfa_photometric_bwd"] * 2 + ["nfa_photometric_fwd"]


# ------------------------------------------------------------------------------------------------ beyond 4 GiB
def test_byte_offsets_beyond_4_gib(dev):
    """A (1, 1, W, 4) stack of 2^32 + 256 bytes: pixels on both sides of the 4 GiB line.  A 32-bit byte offset would send
    pixel 2^30 + k back to pixel k, which holds other values."""
    from nerfacc_amd.photometric import target_pixels
    W = (1 << 30) + 64
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 6 * 10 ** 9:
        pytest.skip(f"needs about 4.3 GB of device memory, {free / 1e9:.1f} GB are free")
    stack = torch.empty((1, 1, W, 4), dtype=torch.uint8, device=dev)
    assert stack.numel() > 1 << 32
    where = [0, 1, 63, (1 << 30) - 2, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 30) + 63]
    values = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (8, 4), dtype=np.uint8))
    values[:, 3] = 255 - values[:, 0]
    for k, v in zip(where, values):
        stack[0, 0, k] = v.to(dev)
    bkgd = torch.tensor([0.25, 0.5, 0.75])
    p = values.float() / 255.0                                     # (on the CPU: a true division)
    want = p[:, :3] * p[:, 3:] + bkgd * (1.0 - p[:, 3:])
    at, zero = torch.tensor(where, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    for dt in (torch.int64, torch.int32):
        got = target_pixels(stack, zero.to(dt), at.to(dt), zero.to(dt), bkgd.to(dev))
        assert torch.equal(R.bits(got), R.bits(want)), dt
    assert len({tuple(v) for v in values.tolist()}) == 8


# ------------------------------------------------------------------------------------------------ a captured step
def _training_run(dev, captured):
    """Three warm-up steps, then three more on new pixels: render, loss, scaled backward, FusedAdam; the parameters' bits."""
    from nerfacc_amd import CapturedStep
    from nerfacc_amd.optim import DeviceGradScaler, FusedAdam
    from nerfacc_amd.photometric import photometric_loss
    from nerfacc_amd.rawrender import rendering_from_raw
    n_rays, per_ray = 300, 6
    g = torch.Generator().manual_seed(11)
    raw_rgb = torch.nn.Parameter(torch.randn(n_rays * per_ray, 3, generator=g).to(dev))
    raw_sig = torch.nn.Parameter(torch.randn(n_rays * per_ray, generator=g).to(dev))
    ri = torch.arange(n_rays, device=dev).repeat_interleave(per_ray)
    ts = (torch.arange(per_ray, device=dev).float() * 0.1).repeat(n_rays)
    te = ts + 0.1
    c = case(n_rays)
    stack, bkgd = T(c["stack"], dev), T(c["bkgd"], dev)
    batches = [[T(v, dev) for v in R.random_indices(300 + k, n_rays)] for k in range(4)]
    ids, y, x = (t.clone() for t in batches[0])
    scaler = DeviceGradScaler(2.0 ** 10, growth_interval=2)
    opt = FusedAdam([raw_rgb, raw_sig], lr=1e-2, eps=1e-15, zero_grad=True, scaler=scaler)

    def fn():
        rgb = rendering_from_raw(ts, te, raw_rgb, raw_sig, ri, n_rays)[0]
        out = photometric_loss(rgb, images=stack, image_ids=ids, x=x, y=y, color_bkgd=bkgd)
        scaler.scale(out.loss).backward()
        opt.step()
        return out.loss, out.mse

    if captured:
        step = CapturedStep(fn, warmup=3)
    else:
        for _ in range(3):
            fn()
        step = fn
    for b in batches[1:]:
        for dst, src in zip((ids, y, x), b):
            dst.copy_(src)
        loss, mse = step()
    torch.cuda.synchronize()
    return [R.bits(t).clone() for t in (raw_rgb, raw_sig, loss, mse)] + [scaler.get_scale()]


def test_captured_training_step_equals_eager(dev):
    eager = _training_run(dev, captured=False)
    graph = _training_run(dev, captured=True)
    assert eager[-1] == graph[-1] and eager[-1] != 2.0 ** 10        # the scale grew on the device in both
    for a, b in zip(eager[:-1], graph[:-1]):
        assert torch.equal(a, b)
    assert np.isfinite(eager[0].view(torch.float32).numpy()).all()

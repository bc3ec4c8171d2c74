"""CPU: nerfacc_amd.photometric's torch path -- the restatement of csrc/photo.hip's contract -- against the numpy reference
(bit for bit), against the reference project's lines (the gather, the division by 255, the blend: bit for bit; smooth_l1_loss
and mse_loss and their autograd gradients in float64: within the rounding budget), every kind against a float64 autograd
restatement of its formula, and the argument handling."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import photometric_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd import photometric as P
from nerfacc_amd.photometric import photometric_loss, psnr, target_pixels

# at most three rounded float32 operations per term plus the final rounding, non-negative terms: about 4 * 2^-23 < 1e-6
REL = 1e-6


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def case(seed, n, C=4):
    stack = R.random_stack(seed, (3, 5, 7, C))
    ids, y, x = R.random_indices(seed + 1, n)
    r = np.random.default_rng(seed + 2)
    return dict(stack=stack, ids=ids, x=x, y=y, rgb=r.random((n, 3), dtype=np.float32), bkgd=r.random(3, dtype=np.float32),
                bkgd_n=r.random((n, 3), dtype=np.float32), w=(r.random(n, dtype=np.float32) * 2).astype(np.float32))


def test_entries_are_declared_and_bound():
    assert {"nfa_photometric_fwd", "nfa_photometric_bwd", "nfa_photometric_chunk"} <= set(B.EXPORTED_SYMBOLS)
    assert P.reduction_chunk() > 0 and P.reduction_chunk() % 4 == 0
    import nerfacc_amd
    assert "photometric_loss" not in nerfacc_amd.__all__


# ------------------------------------------------------------------------------------------------ the target
def test_all_256_bytes_are_the_ieee_quotient():
    v = np.arange(256, dtype=np.uint8)
    for C in (3, 4):
        stack = np.repeat(v.reshape(1, 16, 16, 1), C, axis=-1)
        got = target_pixels(T(stack), 0)
        want = v.astype(np.float32) / np.float32(255.0)
        assert got.shape == (16, 16, 3) and got.dtype == torch.float32
        assert all(np.array_equal(got[..., k].numpy().reshape(-1).view(np.int32), want.view(np.int32)) for k in range(3))
    # float64 division rounded to float32 is the same quotient; a product with the reciprocal is not
    assert np.array_equal((v.astype(np.float64) / 255.0).astype(np.float32), want)
    n_differ = int((v.astype(np.float32) * (np.float32(1.0) / np.float32(255.0)) != want).sum())
    print("bytes for which v * (1 / 255) differs from v / 255:", n_differ)
    assert n_differ == 126


@pytest.mark.parametrize("per_ray_bkgd", [False, True])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_blend_is_the_loaders_expression_bit_for_bit(per_ray_bkgd, dtype):
    c = case(10, 257)
    stack, ids, x, y = T(c["stack"]), T(c["ids"].astype(dtype)), T(c["x"].astype(dtype)), T(c["y"].astype(dtype))
    bkgd = T(c["bkgd_n"] if per_ray_bkgd else c["bkgd"])
    rgba = stack[ids.long(), y.long(), x.long()] / 255.0                     # nerf_synthetic.py:195
    pixels, alpha = torch.split(rgba, [3, 1], dim=-1)
    want = pixels * alpha + bkgd * (1.0 - alpha)                           # nerf_synthetic.py:153
    got = target_pixels(stack, ids, x, y, bkgd)
    assert got.dtype == torch.float32 and torch.equal(R.bits(got), R.bits(want))
    assert torch.equal(R.bits(got), R.bits(T(R.target(c["stack"], c["ids"], c["x"], c["y"], bkgd=bkgd.numpy()))))
    # no background: the colour channels as they are, alpha ignored; three channels: nerf_360_v2.py:327
    assert torch.equal(target_pixels(stack, ids, x, y), pixels)
    rgb_only = stack[..., :3].contiguous()
    assert torch.equal(target_pixels(rgb_only, ids, x, y, bkgd), rgb_only[ids.long(), y.long(), x.long()] / 255.0)
    # the same through photometric_loss, and ready rgba pixels
    out = photometric_loss(T(c["rgb"]), images=stack, image_ids=ids, x=x, y=y, color_bkgd=bkgd)
    assert torch.equal(R.bits(out.pixels), R.bits(want))
    out = photometric_loss(T(c["rgb"]), pixels=rgba, color_bkgd=bkgd)
    assert torch.equal(R.bits(out.pixels), R.bits(want))


def test_clamping_whole_image_and_broadcasting():
    c = case(20, 64)
    stack = T(c["stack"])
    # out-of-range indices are clamped into the stack
    ids, x, y = T(c["ids"]).clone(), T(c["x"]).clone(), T(c["y"]).clone()
    ids[0], ids[1], x[2], x[3], y[4], y[5] = -1, 3, -5, 7, -1, 5 + 10 ** 10
    got = target_pixels(stack, ids, x, y)
    assert torch.equal(got, stack[ids.clamp(0, 2), y.clamp(0, 4), x.clamp(0, 6)][:, :3] / 255.0)
    # an int image id without x, y: the whole image in row-major order
    bkgd = T(c["bkgd"])
    whole = target_pixels(stack, 1, color_bkgd=bkgd)
    yy, xx = torch.meshgrid(torch.arange(5), torch.arange(7), indexing="ij")
    assert whole.shape == (5, 7, 3) and torch.equal(whole, target_pixels(stack, torch.ones_like(xx), xx, yy, bkgd))
    assert torch.equal(target_pixels(stack[2]), target_pixels(stack, 2))
    rgb = torch.rand(5, 7, 3, generator=torch.Generator().manual_seed(1))
    out = photometric_loss(rgb, images=stack, image_ids=1, color_bkgd=bkgd, per_ray=True)
    assert out.pixels.shape == (5, 7, 3) and torch.equal(out.pixels, whole) and out.per_ray.shape == (5, 7)
    assert torch.equal(out.loss, photometric_loss(rgb.view(35, 3), pixels=whole.view(35, 3)).loss)
    # an int id with x, y; index tensors that broadcast against each other
    assert torch.equal(target_pixels(stack, 1, xx, yy, bkgd), whole)
    assert torch.equal(target_pixels(stack, torch.tensor(1), torch.arange(7), torch.arange(5)[:, None], bkgd), whole)
    assert torch.equal(target_pixels(stack, torch.tensor(1, dtype=torch.int32), torch.arange(7), torch.arange(5)[:, None], bkgd), whole)
    out2 = photometric_loss(rgb, images=stack, image_ids=1, x=torch.arange(7), y=torch.arange(5)[:, None], color_bkgd=bkgd,
                            weights=torch.full((7,), 2.0))
    assert torch.equal(out2.pixels, whole) and torch.equal(out2.loss, 2 * out.loss)
    # a per-ray background that broadcasts
    assert torch.equal(target_pixels(stack, 1, color_bkgd=bkgd.expand(7, 3)), whole)


def test_value_errors():
    c = case(30, 16)
    stack, ids, x, y, rgb = T(c["stack"]), T(c["ids"]), T(c["x"]), T(c["y"]), T(c["rgb"])
    pix = target_pixels(stack, ids, x, y)
    bad = [
        dict(kind="l3", pixels=pix),
        dict(),                                                   # neither source
        dict(pixels=pix, images=stack, image_ids=ids, x=x, y=y),  # both
        dict(pixels=pix, x=x, y=y),
        dict(pixels=pix[:, :2]),
        dict(pixels=pix[:5]),
        dict(images=stack, image_ids=ids, x=x.float(), y=y),
        dict(images=stack, image_ids=ids.double(), x=x, y=y),
        dict(images=stack, image_ids=ids, x=x),
        dict(images=stack, x=x, y=y),                             # three images, no ids
        dict(images=stack, image_ids=3, x=x, y=y),
        dict(images=stack, image_ids=ids),
        dict(images=stack, image_ids=0),                          # 16 rays against a whole image of 35
        dict(images=stack[..., :2], image_ids=ids, x=x, y=y),
        dict(images=stack.to(torch.int16), image_ids=ids, x=x, y=y),
        dict(images=stack, image_ids=ids[:5], x=x, y=y),
        dict(images=stack, image_ids=ids, x=x, y=y, color_bkgd=torch.zeros(4)),
        dict(images=stack, image_ids=ids, x=x, y=y, color_bkgd=torch.zeros(5, 3)),
        dict(pixels=pix, weights=torch.ones(5)),
        dict(pixels=pix, weights=torch.ones(16, dtype=torch.int64)),
        dict(pixels=pix, beta=-1.0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            photometric_loss(rgb, **kw)
    with pytest.raises(ValueError):
        photometric_loss(rgb[:, :2], pixels=pix)
    with pytest.raises(ValueError):
        photometric_loss(rgb.long(), pixels=pix)
    with pytest.raises(ValueError):
        target_pixels(stack, ids, x.float(), y.float())


# ------------------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_torch_path_is_the_numpy_reference_bit_for_bit(kind, weighted):
    c = case(40, 1031)
    param = R.PARAMS[kind]
    w = c["w"] if weighted else None
    rgb = T(c["rgb"]).requires_grad_(True)
    out = photometric_loss(rgb, images=T(c["stack"]), image_ids=T(c["ids"]), x=T(c["x"]), y=T(c["y"]), color_bkgd=T(c["bkgd"]),
                           kind=kind, beta=param, weights=T(w), per_ray=True)
    pixels = R.target(c["stack"], c["ids"], c["x"], c["y"], bkgd=c["bkgd"])
    loss, mse, per_ray = R.forward(c["rgb"], pixels, kind, param, w)
    assert out.loss.shape == () and out.loss.dtype == torch.float32 and out.mse.shape == ()
    assert torch.equal(R.bits(out.pixels), R.bits(T(pixels)))
    assert out.loss.item() == loss and out.mse.item() == mse and torch.equal(R.bits(out.per_ray), R.bits(T(per_ray)))
    assert out.loss.requires_grad and not out.mse.requires_grad and not out.pixels.requires_grad and not out.per_ray.requires_grad
    (out.loss * 1024.0).backward()
    assert torch.equal(R.bits(rgb.grad), R.bits(T(R.backward(c["rgb"], pixels, kind, param, 1024.0, w))))
    # half-precision rgb: computed in float32 from the widened values, the gradient rounded once
    for dt in (torch.float16, torch.bfloat16):
        rh = T(c["rgb"]).to(dt).requires_grad_(True)
        oh = photometric_loss(rh, pixels=T(pixels), kind=kind, beta=param, weights=T(w))
        r32 = rh.detach().float().numpy()
        assert oh.loss.dtype == torch.float32 and oh.loss.item() == R.forward(r32, pixels, kind, param, w)[0]
        (oh.loss * 1024.0).backward()
        assert rh.grad.dtype == dt and torch.equal(R.bits(rh.grad), R.bits(R.rounded(R.backward(r32, pixels, kind, param, 1024.0, w), dt)))


def _f64_term(kind, p, d, rgb):
    ad = d.abs()
    if kind == "l1":
        return ad
    if kind == "l2":
        return d * d
    if kind == "smooth_l1":
        return torch.where(ad < p, 0.5 * d * d / p, ad - 0.5 * p)
    if kind == "huber":
        return torch.where(ad <= p, 0.5 * d * d, p * (ad - 0.5 * p))
    if kind == "relative_l2":
        return d * d / (rgb.detach() * rgb.detach() + float(np.float32(0.01)))
    return torch.sqrt(d * d + p * p)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_every_kind_against_float64_autograd(kind, weighted):
    """loss and rgb.grad against the formula written in float64 on the same float32 inputs and differentiated by autograd.
    Per element at most 4 rounded float32 operations reach a term (5 with a weight), each relative 2^-24: REL = 1e-6 covers
    the sum of non-negative terms; a gradient element passes through at most 6.  The relative_l2 denominator's constant is
    the float32 0.01 in both."""
    c = case(50, 777)
    param = float(np.float32(R.PARAMS[kind]))
    w = T(c["w"]) if weighted else None
    pixels = target_pixels(T(c["stack"]), T(c["ids"]), T(c["x"]), T(c["y"]), T(c["bkgd_n"]))
    rgb = T(c["rgb"]).requires_grad_(True)
    out = photometric_loss(rgb, pixels=pixels, kind=kind, beta=param, weights=w)
    out.loss.backward()
    r64 = T(c["rgb"]).double().requires_grad_(True)
    t = _f64_term(kind, param, r64 - pixels.double(), r64)
    want = ((t if w is None else w.double()[:, None] * t).sum() / t.numel())
    want.backward()
    assert abs(out.loss.item() - want.item()) <= REL * abs(want.item()), (out.loss.item(), want.item())
    err, ref = (rgb.grad.double() - r64.grad).abs(), r64.grad.abs()
    assert bool((err <= REL * ref).all()), float((err / ref.clamp(min=1e-300)).max())
    assert bool((rgb.grad != 0).any())


def test_smooth_l1_and_mse_against_the_trainers_lines():
    """F.smooth_l1_loss / F.mse_loss in float64 on the same float32 inputs, values and autograd gradients, within REL."""
    c = case(60, 1500)
    pixels = target_pixels(T(c["stack"]), T(c["ids"]), T(c["x"]), T(c["y"]), T(c["bkgd"]))
    spread = T(c["rgb"]) * 4 - 1.5                                   # |d| on both sides of beta = 1
    for kind, fn in (("smooth_l1", TF.smooth_l1_loss), ("l2", TF.mse_loss)):
        rgb = spread.clone().requires_grad_(True)
        out = photometric_loss(rgb, pixels=pixels, kind=kind)
        out.loss.backward()
        r64 = spread.double().requires_grad_(True)
        want = fn(r64, pixels.double())
        want.backward()
        assert abs(out.loss.item() - want.item()) <= REL * want.item()
        assert bool(((rgb.grad.double() - r64.grad).abs() <= REL * r64.grad.abs()).all())
        want_mse = TF.mse_loss(spread.double(), pixels.double()).item()
        assert abs(out.mse.item() - want_mse) <= REL * want_mse
        assert abs(psnr(out.mse).item() - (-10.0 * np.log10(want_mse))) <= 1e-5
    assert bool(((spread - pixels).abs() > 1).any()) and bool(((spread - pixels).abs() < 1).any())
    # beta = 0 is l1 (torch's rule)
    a, b = photometric_loss(spread, pixels=pixels, kind="smooth_l1", beta=0.0), photometric_loss(spread, pixels=pixels, kind="l1")
    assert torch.equal(a.loss, b.loss) and abs(a.loss.item() - TF.l1_loss(spread.double(), pixels.double()).item()) <= REL * a.loss.item()


def test_float64_empty_and_non_contiguous_inputs():
    c = case(70, 33)
    pixels = target_pixels(T(c["stack"]), T(c["ids"]), T(c["x"]), T(c["y"]), T(c["bkgd"]))
    rgb = T(c["rgb"])
    out64 = photometric_loss(rgb.double(), pixels=pixels.double())
    assert out64.loss.dtype == torch.float64 and abs(out64.loss.item() - TF.smooth_l1_loss(rgb.double(), pixels.double()).item()) < 1e-15
    wide = torch.zeros(33, 6)
    wide[:, ::2] = rgb
    assert torch.equal(photometric_loss(wide[:, ::2], pixels=pixels).loss, photometric_loss(rgb, pixels=pixels).loss)
    empty = photometric_loss(torch.zeros(0, 3, requires_grad=True), pixels=torch.zeros(0, 3), per_ray=True)
    assert torch.isnan(empty.loss) and torch.isnan(empty.mse) and empty.pixels.shape == (0, 3) and empty.per_ray.shape == (0,)
    empty.loss.backward()
    assert target_pixels(T(c["stack"]), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                         torch.zeros(0, dtype=torch.int64)).shape == (0, 3)
    # a floating-point stack is taken as it is
    fstack = T(c["stack"]).float() / 255.0
    assert torch.equal(target_pixels(fstack, T(c["ids"]), T(c["x"]), T(c["y"]), T(c["bkgd"])), pixels)


def test_launch_arguments(monkeypatch):
    """What the wrapper hands to nfa_photometric_fwd, with the call itself recorded instead of made: the ray count, the index
    type, the channel count and above all the background's stride -- 0 for one shared colour in any shape it may come in,
    3 only for an array that holds a row per ray -- and that an array of another size never reaches the entry."""
    calls = []
    monkeypatch.setattr(P, "_call", lambda dev, name, *a: calls.append((name, a)))
    monkeypatch.setattr(P, "_native_source", lambda *a: True)
    c = case(80, 35)
    stack, ids, x, y = T(c["stack"]), T(c["ids"]), T(c["x"]), T(c["y"])
    shared, per_ray = T(c["bkgd"]), T(c["bkgd_n"])
    forms = [(None, 0), (shared, 0), (shared.view(1, 3), 0), (shared.expand(35, 3), 3), (per_ray, 3), (per_ray.view(5, 7, 3), 3)]
    for bkgd, stride in forms:
        for dt, code in ((torch.int32, 1), (torch.int64, 2), (torch.int16, 2)):
            del calls[:]
            shape = (5, 7) if bkgd is not None and bkgd.dim() == 3 else (35,)
            target_pixels(stack, ids.to(dt).view(shape), x.to(dt).view(shape), y.to(dt).view(shape), bkgd)
            (name, a), = calls
            assert name == "nfa_photometric_fwd" and a[0] is None and a[2] == 35 and tuple(a[4:7]) == (3, 5, 7)
            assert a[10] == code and a[12] == 4 and a[14] == stride and (a[13] is None) == (bkgd is None), (stride, a[13:15])
    # whole image of an int id: one image, no index arrays
    del calls[:]
    target_pixels(stack, 2, color_bkgd=shared)
    a = calls[0][1]
    assert a[2] == 35 and a[4] == 1 and a[7] is None and a[8] is None and a[9] is None and a[14] == 0
    assert a[3] == stack[2:3].data_ptr()
    # ready pixels
    del calls[:]
    P._launch_fwd(torch.device("cpu"), None, None, None, None, None, torch.zeros(35, 4), shared, None, 0, 0.0,
                  torch.zeros(35, 3), None, None, None)
    assert calls[0][1][11] is not None and calls[0][1][12] == 4 and calls[0][1][14] == 0
    for bad in (dict(bkgd=torch.zeros(34, 3)), dict(bkgd=torch.zeros(1, 3)), dict(weights=torch.zeros(34)), dict(per_ray=torch.zeros(36)),
                dict(pixels_in=torch.zeros(34, 4)), dict(pixels_in=torch.zeros(35, 8)[:, ::2])):
        kw = dict(pixels_in=torch.zeros(35, 4), bkgd=shared, weights=None, per_ray=None)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            P._launch_fwd(torch.device("cpu"), torch.zeros(35, 3), None, None, None, None, kw["pixels_in"], kw["bkgd"], kw["weights"], 2, 1.0,
                          torch.zeros(35, 3), torch.zeros(()), torch.zeros(()), kw["per_ray"])

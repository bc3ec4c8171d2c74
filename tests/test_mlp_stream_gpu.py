"""GPU: the streamed-weight fused MLP (csrc/mlp_stream.hip).  Bit for bit on the integer-valued cases of
tests/mlp_stream_reference.py through StreamedMLP and through the four nfa_mlp_stream_* entries (every H_l and dZ_l too), every
output between guard rows; a 128-wide network against the resident kernels' bits; Xavier weights within the derived bound at
the trunk and at the colour head; the same bits on every run; NerfMLP against the reference's own class (the golden fixture)."""
import pytest
import torch

import mlp_bias_skip_reference as S
import mlp_reference as R
import mlp_stream_reference as Q
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, StreamedMLP, image_elems, stream_wgrad_slices
from test_mlp_stream_cpu import grads, make_stream, nerf_golden_check

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DEV = "cuda"
GUARD = 3          # guard rows on either side of every output buffer
SENTINEL = -7.0


def guarded(rows, cols, dtype):
    whole = torch.full((rows + 2 * GUARD, cols), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows]


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def run_abi(shape, skip_mask, dtype, ws, bs, x, g, out_f32, hidden_in=None, prefix="nfa_mlp_stream_", slices=stream_wgrad_slices):
    """The four entries called directly; the backward runs on ``hidden_in`` where given (float64 values of ``dtype`` numbers:
    one mask on both sides), else on what the forward wrote.  Returns CPU float64 tensors: y, hidden, dz (dZ_0 .. dZ_L), dx, dp
    (flat: matrices, then biases)."""
    n_in, n_out, width, n_hidden = shape
    N, elem = x.shape[0], B.ELEM_CODES[dtype]
    desc = B.MLPDesc(*shape, int(bs is not None), skip_mask)
    params = S.flat_params(ws, bs).to(DEV)
    P, n_w = params.numel(), sum(w.numel() for w in ws)
    fe, be = image_elems(*shape, skip_mask)
    fwd_w, fwd = guarded(fe // 512, 512, dtype)
    bwd_w, bwd = guarded(be // 512, 512, dtype)
    B.call(prefix + "pack_weights", elem, desc, B.ptr(params), B.ptr(fwd), fe, B.ptr(bwd), be, B.stream())
    xd, gd = x.to(DEV), g.to(DEV)
    bias_ptr = params.data_ptr() + 4 * n_w if bs is not None else None
    end = torch.float32 if out_f32 else dtype
    y_w, y = guarded(N, n_out, end)
    hid_w, hid = guarded(n_hidden * N, width, dtype)
    B.call(prefix + "fwd", elem, desc, B.ptr(xd), B.ELEM_CODES[xd.dtype], B.ptr(fwd), bias_ptr, N, B.ptr(y), B.ELEM_CODES[end],
           B.ptr(hid), 1, B.stream())
    hidden_used = hid if hidden_in is None else torch.cat(list(hidden_in)).to(dtype).to(DEV).contiguous()
    dz_w, dz = guarded(n_hidden * N, width, dtype)
    dzo_w, dzo = guarded(N, n_out, dtype)
    dx_w, dx = guarded(N, n_in, xd.dtype)
    g_is_half = gd.dtype == dtype
    B.call(prefix + "bwd_data", elem, desc, B.ptr(gd), B.ELEM_CODES[gd.dtype], B.ptr(hidden_used), B.ptr(bwd), N, B.ptr(dz),
           None if g_is_half else B.ptr(dzo), B.ptr(dx), B.ELEM_CODES[xd.dtype], B.stream())
    dz_out = gd if g_is_half else dzo
    part_w, part = guarded(slices(N) * P, 1, torch.float32)
    gp_w, gp = guarded(P, 1, torch.float32)
    B.call(prefix + "bwd_weights", elem, desc, B.ptr(xd), B.ELEM_CODES[xd.dtype], B.ptr(hidden_used), B.ptr(dz), B.ptr(dz_out), N,
           B.ptr(part), part.numel(), B.ptr(gp), 0, B.stream())
    torch.cuda.synchronize()
    for name, whole in [("fwd image", fwd_w), ("bwd image", bwd_w), ("y", y_w), ("hidden", hid_w), ("dz", dz_w), ("dz_out", dzo_w),
                        ("dx", dx_w), ("partials", part_w), ("grad_params", gp_w)]:
        assert guards_intact(whole), f"{name}: guard rows overwritten"
    if g_is_half:
        assert bool((dzo == SENTINEL).all()), "dz_out written although it was not passed"
    c = lambda t: t.cpu().double()
    rows = lambda t: [c(t[l * N:(l + 1) * N]) for l in range(n_hidden)]
    return dict(y=c(y), hidden=rows(hid), dz=rows(dz) + [c(gd) if g_is_half else c(dzo)], dx=c(dx), dp=c(gp).view(-1),
                fwd=fwd.cpu(), bwd=bwd.cpu())


def check_exact(case, dtype, through_module=True):
    shape, skip_mask, ws, bs, x, g, f, b = Q.exact_case(case, dtype)
    n_hidden, out_f32 = shape[3], case[5][4]
    want_p = S.flat_params(b["dw"], b["db"] if bs is not None else None)
    tag = f"{Q.case_id(case)} {dtype}"
    a = run_abi(shape, skip_mask, dtype, ws, bs, x, g, out_f32)
    assert torch.equal(a["y"], f["y"]), f"abi y: {tag}"
    for l in range(n_hidden):
        assert torch.equal(a["hidden"][l], f["hidden"][l]), f"hidden {l}: {tag}"
    for l in range(n_hidden, -1, -1):
        assert torch.equal(a["dz"][l], b["dz"][l]), f"dZ_{l}: {tag}"
    assert torch.equal(a["dx"], b["dx"]), f"abi dL/dx: {tag}"
    assert torch.equal(a["dp"], want_p), f"abi dW, db: {tag}"
    if through_module:
        y, g_x, g_p = grads(make_stream(shape, dtype, ws, bs, case[3], out_f32, device=DEV), x, g)
        assert y.dtype == (torch.float32 if out_f32 else dtype) and g_x.dtype == x.dtype and g_p.dtype == torch.float32
        assert torch.equal(y.cpu().double(), f["y"]), f"y: {tag}"
        assert torch.equal(g_x.cpu().double(), b["dx"]), f"dL/dx: {tag}"
        assert torch.equal(g_p.cpu().double(), want_p), f"dL/dparams: {tag}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", Q.TRUNK_CASES, ids=Q.case_id)
def test_trunk_exact_gpu(case, dtype):
    """63 -> 8 x 256 -> 257, the input appended after hidden layer 4: NeRF's trunk with its merged output layer."""
    check_exact(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", Q.CASES[len(Q.TRUNK_CASES):], ids=Q.case_id)
def test_exact(case, dtype):
    check_exact(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_partial_tile_after_a_full_sweep(dtype):
    """256 wide, 2 hidden layers: 256 workgroups x 128 points are one sweep of the persistent grid; then two full tiles and a
    tile of 7 points, in a workgroup whose last wave has nothing, and 16 weight-gradient slices."""
    assert Q.SWEEP_CASE[5][0] == Q.GROUPS * Q.T + 71 and stream_wgrad_slices(Q.SWEEP_CASE[5][0]) == 16
    check_exact(Q.SWEEP_CASE, dtype, through_module=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_128_wide_network_gives_the_resident_kernels_bits(dtype):
    """What both designs hold: the images byte for byte, y, every H_l and dZ_l and dL/dx bit for bit.  (dL/dparams sums other
    slices in another order: it is compared against the bound elsewhere.)"""
    from nerfacc_amd.mlp import wgrad_slices
    shape, skip_layer = (36, 3, 128, 3), 2
    skip_mask = S.skip_mask_of(skip_layer, 3)
    gen = torch.Generator().manual_seed(5)
    ws = [(torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 for o, i in S.layer_dims(*shape, skip_mask)]
    bs = [torch.rand(w.shape[0], generator=gen) - 0.5 for w in ws]
    x, g = torch.randn(300, 36, generator=gen), torch.randn(300, 3, generator=gen)
    new = run_abi(shape, skip_mask, dtype, ws, bs, x, g, False)
    old = run_abi(shape, skip_mask, dtype, ws, bs, x, g, False, prefix="nfa_mlp_net_", slices=wgrad_slices)
    for k in ("fwd", "bwd", "y", "dx"):
        assert torch.equal(new[k], old[k]), k
    for l in range(3):
        assert torch.equal(new["hidden"][l], old["hidden"][l]) and torch.equal(new["dz"][l], old["dz"][l]), l
    resident = FusedMLP(*shape, dtype=dtype, bias=True, skip_layer=skip_layer)
    resident.load_linear_weights(ws, bs)
    y_old, gx_old, _ = grads(resident.to(DEV), x, g)
    y_new, gx_new, _ = grads(make_stream(shape, dtype, ws, bs, skip_layer, False, device=DEV), x, g)
    assert torch.equal(y_old, y_new) and torch.equal(gx_old, gx_new)


# ---------------------------------------------------------------- random data, the derived bound

TRUNK = (63, 257, 256, 8, 4)       # n_in, n_out, width, n_hidden, skip_layer; biases
COLOUR_HEAD = (283, 3, 128, 1, None)
RANDOM_NETS = {"trunk": TRUNK, "colour_head": COLOUR_HEAD}


def random_case(net, dtype, f32_ends, N=300):
    *shape, skip_layer = RANDOM_NETS[net]
    skip_mask = S.skip_mask_of(skip_layer, shape[3])
    gen = torch.Generator().manual_seed(7)
    ws = [(torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 for o, i in S.layer_dims(*shape, skip_mask)]
    bs = [torch.rand(w.shape[0], generator=gen) - 0.5 for w in ws]
    end = torch.float32 if f32_ends else dtype
    x, g = (torch.randn(N, n, generator=gen).to(end) for n in (shape[0], shape[1]))
    return tuple(shape), skip_layer, skip_mask, ws, bs, x, g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", list(RANDOM_NETS))
@pytest.mark.parametrize("f32_ends", [False, True])
def test_random_within_the_bound(net, dtype, f32_ends):
    shape, skip_layer, skip_mask, ws, bs, x, g = random_case(net, dtype, f32_ends)
    n_hidden = shape[3]
    f = S.forward(x, ws, bs, skip_mask, dtype, f32_ends)
    b = S.backward(x, ws, f["hidden"], g, skip_mask, dtype)
    with torch.no_grad():
        y = make_stream(shape, dtype, ws, bs, skip_layer, f32_ends, device=DEV)(x.to(DEV))
    ratios = {"y": S.worst_ratio(y.cpu(), f["y"], f["e_y"])}
    # the backward on the REFERENCE's hidden activations: one mask on both sides
    a = run_abi(shape, skip_mask, dtype, ws, bs, x, g, f32_ends, hidden_in=f["hidden"])
    n_w = sum(w.numel() for w in ws)
    ratios["dx"] = S.worst_ratio(a["dx"], b["dx"], b["e_dx"])
    for l in range(n_hidden + 1):
        ratios[f"dz{l}"] = S.worst_ratio(a["dz"][l], b["dz"][l], b["e_dz"][l])
    ratios["dw"] = S.worst_ratio(a["dp"][:n_w], S.flat_params(b["dw"]), S.flat_params(b["e_dw"]))
    ratios["db"] = S.worst_ratio(a["dp"][n_w:], S.flat_params(b["db"]), S.flat_params(b["e_db"]))
    print(f"mlp stream error/bound ratios {net} {dtype} f32_ends={f32_ends}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert torch.equal(a["dz"][n_hidden], R.rnd(g.double(), dtype)), "dZ_L is g rounded: no error allowed"
    assert bool(a["dp"][n_w:].any()) and bool(a["dx"].any())
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", list(RANDOM_NETS))
def test_bitwise_reproducible(net, dtype):
    shape, skip_layer, skip_mask, ws, bs, x, g = random_case(net, dtype, False)
    m = make_stream(shape, dtype, ws, bs, skip_layer, False, device=DEV)
    first = grads(m, x, g)
    second = grads(m, x, g)
    grads(m, x[:131], g[:131])   # another N in between: other slices, other partials
    with torch.autocast("cuda", dtype=torch.bfloat16 if dtype == torch.float16 else torch.float16):
        third = grads(m, x, g)
    for other in (second, third):
        for a, b_ in zip(first, other):
            assert a.dtype == b_.dtype and torch.equal(a, b_)
    assert bool(first[2].any())


def test_empty_batch_and_second_order_refusal():
    m = StreamedMLP(63, 257).to(DEV)
    x = torch.zeros(0, 63, device=DEV, requires_grad=True)
    y = m(x)
    assert y.shape == (0, 257)
    y.sum().backward()
    assert x.grad.shape == (0, 63) and not bool(m.params.grad.any())
    x = torch.randn(5, 63, device=DEV, requires_grad=True)
    (g_x,) = torch.autograd.grad(m(x).float().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="StreamedMLP"):
        g_x.sum().backward()


# ---------------------------------------------------------------- the reference's own NerfMLP class

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("condition", [True, False])
@pytest.mark.parametrize("kind", ["exact", "xavier"])
def test_nerf_mlp_golden_gpu(kind, condition, dtype):
    ratios = nerf_golden_check(kind, condition, dtype, DEV)
    if ratios:
        print(f"NerfMLP golden {kind} condition={condition} {dtype} error/bound ratios: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))

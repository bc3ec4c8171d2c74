"""GPU: the fused MLP of csrc/mlp.hip.  Bit for bit on integer-valued data (tests/mlp_reference.py: signed permutations and
thinned dense matrices, every intermediate an integer the half type represents, so that any summation order gives the same
bits) through the module and through the C ABI (saved hidden activations and every dZ_l too), every output buffer between
guard rows; within the derived bound on Xavier weights and normal inputs at the NGP shapes; and the same bits on every run."""
import pytest
import torch

import mlp_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, image_elems, wgrad_slices

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DEV = "cuda"
GUARD = 3          # guard rows on either side of every output buffer
SENTINEL = -7.0

# (N, n_in, n_out, x float32?, y and g float32?): the tile edges 31 / 32 / 33 and 127 / 128 / 129 (a workgroup's four waves
# hold 128 points), rows that are not 16-byte aligned (1, 31, 63 wide: the element-wise load path), 1 / 3 / 16 / 32 outputs,
# and 300 points: two split-K slices of 192, the second short (108) and ending inside a 64-point chunk.
CONFIGS = [
    (1, 1, 1, True, False),
    (31, 16, 3, False, False),
    (32, 31, 16, True, True),
    (33, 32, 32, False, True),
    (127, 63, 3, False, False),
    (128, 32, 16, False, False),
    (129, 16, 1, True, True),
    (300, 32, 16, True, False),
]
WIDE_INPUT = (40, 150, 32, False, False)   # with 128 neurons: 10 k-steps of the first layer, 5 row tiles of dL/dx
assert wgrad_slices(300) == 2 and wgrad_slices(129) == 1


def configs(width, n_hidden):
    return CONFIGS + ([WIDE_INPUT] if width == 128 and n_hidden <= 2 else [])


def guarded(rows, cols, dtype):
    """(whole buffer, the view a kernel writes): GUARD sentinel rows before and after."""
    whole = torch.full((rows + 2 * GUARD, cols), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows]


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def run_abi(shape, dtype, ws, x, g, out_f32, hidden_in=None):
    """The four entries called directly; returns y, hidden, dz (list, dZ_0 .. dZ_L), dx, dw (flat) as CPU float64 tensors."""
    n_in, n_out, width, n_hidden = shape
    N, elem = x.shape[0], B.ELEM_CODES[dtype]
    params = R.flat(ws).to(DEV)
    P = params.numel()
    fe, be = image_elems(*shape)
    fwd_w, fwd = guarded(fe // 512, 512, dtype)
    bwd_w, bwd = guarded(be // 512, 512, dtype)
    B.call("nfa_mlp_pack_weights", elem, B.ptr(params), *shape, B.ptr(fwd), fe, B.ptr(bwd), be, B.stream())
    xd, gd = x.to(DEV), g.to(DEV)
    y_w, y = guarded(N, n_out, torch.float32 if out_f32 else dtype)
    hid_w, hid = guarded(n_hidden * N, width, dtype)
    B.call("nfa_mlp_fwd", elem, B.ptr(xd), B.ELEM_CODES[xd.dtype], B.ptr(fwd), N, *shape, B.ptr(y), B.ELEM_CODES[y.dtype], B.ptr(hid),
           1, B.stream())
    hidden_used = hid if hidden_in is None else torch.cat(hidden_in).to(dtype).to(DEV)
    dz_w, dz = guarded(n_hidden * N, width, dtype)
    dzo_w, dzo = guarded(N, n_out, dtype)
    dx_w, dx = guarded(N, n_in, xd.dtype)
    g_is_half = gd.dtype == dtype
    B.call("nfa_mlp_bwd_data", elem, B.ptr(gd), B.ELEM_CODES[gd.dtype], B.ptr(hidden_used), B.ptr(bwd), N, *shape, B.ptr(dz),
           None if g_is_half else B.ptr(dzo), B.ptr(dx), B.ELEM_CODES[xd.dtype], B.stream())
    part_w, part = guarded(wgrad_slices(N) * P, 1, torch.float32)
    gp_w, gp = guarded(P, 1, torch.float32)
    B.call("nfa_mlp_bwd_weights", elem, B.ptr(xd), B.ELEM_CODES[xd.dtype], B.ptr(hidden_used), B.ptr(dz), B.ptr(gd if g_is_half else dzo),
           N, *shape, B.ptr(part), part.numel(), B.ptr(gp), B.stream())
    torch.cuda.synchronize()
    for name, whole in [("fwd image", fwd_w), ("bwd image", bwd_w), ("y", y_w), ("hidden", hid_w), ("dz", dz_w), ("dz_out", dzo_w),
                        ("dx", dx_w), ("partials", part_w), ("grad_params", gp_w)]:
        assert guards_intact(whole), f"{name}: guard rows overwritten"
    if g_is_half:
        assert bool((dzo == SENTINEL).all()), "dz_out written although it was not passed"
    c = lambda t: t.cpu().double()
    dzs = [c(dz[l * N:(l + 1) * N]) for l in range(n_hidden)] + [c(gd) if g_is_half else c(dzo)]
    return dict(y=c(y), hidden=[c(hid[l * N:(l + 1) * N]) for l in range(n_hidden)], dz=dzs, dx=c(dx), dw=c(gp).view(-1))


def run_module(m, x, g):
    x = x.to(DEV).requires_grad_(True)
    m.params.grad = None
    y = m(x)
    y.backward(g.to(DEV).to(y.dtype))
    return y.detach(), x.grad, m.params.grad.clone()


def make(shape, dtype, ws, out_f32):
    m = FusedMLP(*shape, dtype=dtype, out_dtype=torch.float32 if out_f32 else None)
    m.load_linear_weights(ws)
    return m.to(DEV)


def check_exact(family, dtype, width, n_hidden, cfg):
    N, n_in, n_out, x_f32, out_f32 = cfg
    shape = (n_in, n_out, width, n_hidden)
    ws = R.exact_weights(family, *shape)
    x, g = R.exact_inputs(N, n_in, n_out, torch.float32 if x_f32 else dtype, torch.float32 if out_f32 else dtype)
    f = R.forward(x, ws, dtype, out_f32, exact=True)
    b = R.backward(x, ws, f["hidden"], g, dtype, exact=True)
    tag = f"{family} {dtype} W={width} hidden={n_hidden} cfg={cfg}"
    # through the module
    y, g_x, g_p = run_module(make(shape, dtype, ws, out_f32), x, g)
    assert y.dtype == (torch.float32 if out_f32 else dtype) and g_x.dtype == x.dtype and g_p.dtype == torch.float32
    assert torch.equal(y.cpu().double(), f["y"]), f"y: {tag}"
    assert torch.equal(g_x.cpu().double(), b["dx"]), f"dL/dx: {tag}"
    assert torch.equal(g_p.cpu().double(), R.flat(b["dw"])), f"dL/dparams: {tag}"
    # through the C ABI: the intermediates too
    a = run_abi(shape, dtype, ws, x, g, out_f32)
    assert torch.equal(a["y"], f["y"]), f"abi y: {tag}"
    for l in range(n_hidden):
        assert torch.equal(a["hidden"][l], f["hidden"][l]), f"hidden {l}: {tag}"
    for l in range(n_hidden + 1):
        assert torch.equal(a["dz"][l], b["dz"][l]), f"dZ_{l}: {tag}"
    assert torch.equal(a["dx"], b["dx"]), f"abi dL/dx: {tag}"
    assert torch.equal(a["dw"], R.flat(b["dw"])), f"abi dW: {tag}"


@pytest.mark.parametrize("family", ["perm", "dense"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("n_hidden", [1, 2, 4])
def test_exact(family, dtype, width, n_hidden):
    for cfg in configs(width, n_hidden):
        check_exact(family, dtype, width, n_hidden, cfg)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_partial_tile_after_full_sweeps(dtype):
    """128 wide with 4 hidden layers: 112 KiB of weights, one workgroup per compute unit, 256 x 4 waves x 32 points a sweep.
    Two full sweeps, five full tiles and a tile of 7 points."""
    N = 2 * 256 * 4 * 32 + 5 * 32 + 7
    check_exact("perm", dtype, 128, 4, (N, 32, 16, False, False))


# ---------------------------------------------------------------- random data, the derived bound

RATIOS = {}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.NGP_SHAPES)
@pytest.mark.parametrize("f32_ends", [False, True])
def test_random_within_the_bound(dtype, shape, f32_ends):
    n_in, n_out, width, n_hidden = shape
    N = 1000
    ws = R.xavier_weights(*shape, seed=7)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N, n_in, generator=gen).to(torch.float32 if f32_ends else dtype)
    g = torch.randn(N, n_out, generator=gen).to(torch.float32 if f32_ends else dtype)
    f = R.forward(x, ws, dtype, f32_ends)
    # forward through the module
    with torch.no_grad():
        y = make(shape, dtype, ws, f32_ends)(x.to(DEV))
    ratios = {"y": R.worst_ratio(y.cpu(), f["y"], f["e_y"])}
    # backward entries on the REFERENCE's hidden activations (the same ReLU mask on both sides)
    b = R.backward(x, ws, f["hidden"], g, dtype)
    a = run_abi(shape, dtype, ws, x, g, f32_ends, hidden_in=f["hidden"])
    ratios["dx"] = R.worst_ratio(a["dx"], b["dx"], b["e_dx"])
    for l in range(n_hidden + 1):
        ratios[f"dz{l}"] = R.worst_ratio(a["dz"][l], b["dz"][l], b["e_dz"][l])
    ratios["dw"] = R.worst_ratio(a["dw"], R.flat(b["dw"]), R.flat(b["e_dw"]))
    print(f"mlp error/bound ratios {dtype} {shape} f32_ends={f32_ends}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert torch.equal(a["dz"][n_hidden], R.rnd(g.double(), dtype)), "dZ_L is g rounded: no error allowed"
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.NGP_SHAPES)
def test_bitwise_reproducible(dtype, shape):
    n_in, n_out, width, n_hidden = shape
    ws = R.xavier_weights(*shape, seed=13)
    gen = torch.Generator().manual_seed(17)
    x, g = torch.randn(1000, n_in, generator=gen), torch.randn(1000, n_out, generator=gen)
    m = make(shape, dtype, ws, False)
    first = run_module(m, x, g)
    second = run_module(m, x, g)
    with torch.autocast("cuda", dtype=dtype):
        third = run_module(m, x, g)
    run_module(m, x[:333], g[:333])   # another N in between: other slices, other scratch
    fourth = run_module(m, x, g)
    for other in (second, third, fourth):
        for a, b_ in zip(first, other):
            assert a.dtype == b_.dtype and torch.equal(a, b_)
    assert first[0].dtype == dtype and first[1].dtype == torch.float32


def test_matches_autocast_sequential_and_edge_cases():
    from torch import nn
    m = FusedMLP(32, 3, 64, 2, dtype=torch.float16).to(DEV)
    seq = nn.Sequential(nn.Linear(32, 64, bias=False), nn.ReLU(), nn.Linear(64, 64, bias=False), nn.ReLU(), nn.Linear(64, 3, bias=False)).to(DEV)
    with torch.no_grad():
        for l, w in zip([s for s in seq if isinstance(s, nn.Linear)], m.linear_weights()):
            l.weight.copy_(w)
    x = torch.randn(515, 32, device=DEV)
    with torch.autocast("cuda", dtype=torch.float16):
        want = seq(x)
    assert torch.allclose(m(x).float(), want.float(), atol=2e-2, rtol=2e-2)
    # N = 0: empty tensors, no launch
    x0 = torch.zeros(0, 32, device=DEV, requires_grad=True)
    y0 = m(x0)
    y0.sum().backward()
    assert y0.shape == (0, 3) and x0.grad.shape == (0, 32) and not bool(m.params.grad.any())
    # the masters change: the images are packed again
    y1 = m(x)
    with torch.no_grad():
        m.params.mul_(2.0)
    assert torch.allclose(m(x).float(), 8.0 * y1.float(), atol=1e-2, rtol=1e-2)
    # second order is refused by name
    xr = x[:8].clone().requires_grad_(True)
    (g_x,) = torch.autograd.grad(m(xr).float().sum(), xr, create_graph=True)
    with pytest.raises(NotImplementedError, match="second order"):
        g_x.sum().backward()

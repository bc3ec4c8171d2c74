"""GPU: the fused MLP's second order (csrc/mlp.hip: nfa_mlp_tangent, and nfa_mlp_bwd_weights on the tangent activations).  Bit
for bit on the integer-valued data of tests/mlp_reference.py through the module (real double backward) and through the C ABI
(every T_l too), every output buffer between guard rows; within the derived bound of tests/mlp_grad2_reference.py on Xavier
weights and normal inputs, fed the reference's own hidden activations and dZ; the same bits on every run; and an Eikonal step
through a Smoothstep hash grid with no torch pass in the field."""
import pytest
import torch

import mlp_grad2_reference as G
import mlp_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.encodings import HashGridEncoding
from nerfacc_amd.mlp import FusedMLP, image_elems, mlp_from_tcnn_config, wgrad_slices

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


def stacked(mats, dtype):
    return torch.cat(list(mats)).to(dtype).to(DEV).contiguous()


def run_abi(shape, dtype, ws, v, hidden, dz, u_f32):
    """nfa_mlp_tangent and nfa_mlp_bwd_weights called directly on the given hidden activations ([H_l]) and dZ ([dZ_0 .. dZ_L]),
    float64 values of ``dtype`` numbers.  Returns u, t (list, T_0 .. T_{L-1}) and dw (flat) as CPU float64 tensors."""
    n_in, n_out, width, n_hidden = shape
    N, elem = v.shape[0], B.ELEM_CODES[dtype]
    params = R.flat(ws).to(DEV)
    P = params.numel()
    fe, be = image_elems(*shape)
    fwd = torch.empty(fe, dtype=dtype, device=DEV)
    bwd = torch.empty(be, dtype=dtype, device=DEV)
    B.call("nfa_mlp_pack_weights", elem, B.ptr(params), *shape, B.ptr(fwd), fe, B.ptr(bwd), be, B.stream())
    vd, hid, dzd, dzo = v.to(DEV), stacked(hidden, dtype), stacked(dz[:-1], dtype), dz[-1].to(dtype).to(DEV).contiguous()
    u_dtype = torch.float32 if u_f32 else dtype
    tan_w, tan = guarded(n_hidden * N, width, dtype)
    u_w, u = guarded(N, n_out, u_dtype)
    B.call("nfa_mlp_tangent", elem, B.ptr(vd), B.ELEM_CODES[vd.dtype], B.ptr(hid), B.ptr(fwd), N, *shape, B.ptr(tan), B.ptr(u),
           B.ELEM_CODES[u_dtype], B.stream())
    # once more without the tangent buffer: the same u, and nothing else written
    idle_w, idle = guarded(n_hidden * N, width, dtype)
    u2_w, u2 = guarded(N, n_out, u_dtype)
    B.call("nfa_mlp_tangent", elem, B.ptr(vd), B.ELEM_CODES[vd.dtype], B.ptr(hid), B.ptr(fwd), N, *shape, None, B.ptr(u2),
           B.ELEM_CODES[u_dtype], B.stream())
    part_w, part = guarded(wgrad_slices(N) * P, 1, torch.float32)
    gp_w, gp = guarded(P, 1, torch.float32)
    B.call("nfa_mlp_bwd_weights", elem, B.ptr(vd), B.ELEM_CODES[vd.dtype], B.ptr(tan), B.ptr(dzd), B.ptr(dzo), N, *shape, B.ptr(part),
           part.numel(), B.ptr(gp), B.stream())
    torch.cuda.synchronize()
    for name, whole in [("tangent", tan_w), ("u", u_w), ("u (no tangent)", u2_w), ("partials", part_w), ("grad_params", gp_w)]:
        assert guards_intact(whole), f"{name}: guard rows overwritten"
    assert bool((idle_w == SENTINEL).all()), "a tangent buffer that was not passed was written"
    as_bits = torch.int32 if u_f32 else torch.int16   # the bits: u may hold NaN (tests/test_mlp_edges_gpu.py)
    assert torch.equal(u.view(as_bits), u2.view(as_bits)), "u depends on whether the tangent is stored"
    c = lambda t: t.cpu().double()
    return dict(u=c(u), t=[c(tan[l * N:(l + 1) * N]) for l in range(n_hidden)], dw=c(gp).view(-1))


def make(shape, dtype, ws, out_f32, second_order=True):
    m = FusedMLP(*shape, dtype=dtype, out_dtype=torch.float32 if out_f32 else None, second_order=second_order)
    m.load_linear_weights(ws)
    return m.to(DEV)


def second_order(m, x, g, v):
    """(u, ds/dparams, ds/dx or None) of s = <v, dL/dx> through autograd on the device."""
    x = x.to(DEV).requires_grad_(True)
    y = m(x)
    g = g.to(DEV).to(y.dtype).requires_grad_(True)
    (g_x,) = torch.autograd.grad(y, x, g, create_graph=True)
    assert g_x.dtype == x.dtype
    g_p, u, s_x = torch.autograd.grad((g_x * v.to(DEV)).sum(), [m.params, g, x], allow_unused=True)
    return u, g_p, s_x


def check_exact(family, dtype, width, n_hidden, cfg, v_mod=3):
    shape, ws, x, g, v, f, b, s = G.exact_case(family, dtype, width, n_hidden, cfg, v_mod)
    tag = f"{family} {dtype} W={width} hidden={n_hidden} cfg={cfg} v mod {v_mod}"
    # through the module: a real double backward
    u, g_p, s_x = second_order(make(shape, dtype, ws, cfg[4]), x, g, v)
    assert u.dtype == g.dtype and g_p.dtype == torch.float32 and g_p.shape == (sum(w.numel() for w in ws),)
    assert torch.equal(u.cpu().double(), s["u"]), f"u: {tag}"
    assert torch.equal(g_p.cpu().double(), R.flat(s["dw"])), f"ds/dparams: {tag}"
    assert s_x is None or not bool(s_x.any()), f"ds/dx: {tag}"
    # through the C ABI: the intermediates too
    a = run_abi(shape, dtype, ws, v, f["hidden"], b["dz"], cfg[4])
    assert torch.equal(a["u"], s["u"]), f"abi u: {tag}"
    for l in range(n_hidden):
        assert torch.equal(a["t"][l], s["t"][l + 1]), f"T_{l}: {tag}"
    assert torch.equal(a["dw"], R.flat(s["dw"])), f"abi ds/dW: {tag}"


@pytest.mark.parametrize("family", ["perm", "dense"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("n_hidden", [1, 2, 4])
def test_exact(family, dtype, width, n_hidden):
    for cfg, v_mod in G.configs(family, width, n_hidden):
        check_exact(family, dtype, width, n_hidden, cfg, v_mod)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_partial_tile_after_full_sweeps(dtype):
    """128 wide with 4 hidden layers: one workgroup per compute unit, 256 x 4 waves x 32 points a sweep.  Two full sweeps, five
    full tiles and a tile of 7 points."""
    N = 2 * 256 * 4 * 32 + 5 * 32 + 7
    check_exact("perm", dtype, 128, 4, (N, 32, 16, False, False))


# ---------------------------------------------------------------- random data, the derived bound

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.NGP_SHAPES)
@pytest.mark.parametrize("f32_ends", [False, True])
def test_random_within_the_bound(dtype, shape, f32_ends):
    n_in, n_out, width, n_hidden = shape
    N = 1000
    ws = R.xavier_weights(*shape, seed=7)
    gen = torch.Generator().manual_seed(11)
    end = torch.float32 if f32_ends else dtype
    x = torch.randn(N, n_in, generator=gen).to(end)
    g = torch.randn(N, n_out, generator=gen).to(end)
    v = torch.randn(N, n_in, generator=gen).to(end)
    f = R.forward(x, ws, dtype, f32_ends)
    b = R.backward(x, ws, f["hidden"], g, dtype)
    s = G.second_order(v, ws, f["hidden"], b["dz"], dtype, f32_ends)
    # the entries on the REFERENCE's hidden activations and dZ: one mask and one dZ on both sides
    a = run_abi(shape, dtype, ws, v, f["hidden"], b["dz"], f32_ends)
    ratios = {"u": R.worst_ratio(a["u"], s["u"], s["e_u"])}
    for l in range(n_hidden):
        ratios[f"t{l}"] = R.worst_ratio(a["t"][l], s["t"][l + 1], s["e_t"][l + 1])
    ratios["dw"] = R.worst_ratio(a["dw"], R.flat(s["dw"]), R.flat(s["e_dw"]))
    print(f"mlp second order error/bound ratios {dtype} {shape} f32_ends={f32_ends}: " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)


# ---------------------------------------------------------------- behaviour

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.NGP_SHAPES)
def test_bitwise_reproducible(dtype, shape):
    n_in, n_out, width, n_hidden = shape
    ws = R.xavier_weights(*shape, seed=13)
    gen = torch.Generator().manual_seed(17)
    x, g, v = torch.randn(1000, n_in, generator=gen), torch.randn(1000, n_out, generator=gen), torch.randn(1000, n_in, generator=gen)
    m = make(shape, dtype, ws, False)
    first = second_order(m, x, g, v)
    second = second_order(m, x, g, v)
    with torch.autocast("cuda", dtype=dtype):
        third = second_order(m, x, g, v)
    second_order(m, x[:333], g[:333], v[:333])   # another N in between: other slices, other scratch
    fourth = second_order(m, x, g, v)
    for other in (second, third, fourth):
        for a, c in zip(first[:2], other[:2]):
            assert a.dtype == c.dtype and torch.equal(a, c)
    assert first[0].dtype == dtype and first[1].dtype == torch.float32 and bool(first[0].any()) and bool(first[1].any())


def test_plain_backward_unaffected_launches_and_edge_cases(monkeypatch):
    shape = (32, 3, 64, 2)
    ws = R.xavier_weights(*shape, seed=13)
    gen = torch.Generator().manual_seed(17)
    x, g = torch.randn(1000, 32, generator=gen).to(DEV), torch.randn(1000, 3, generator=gen).to(DEV).half()
    v = torch.randn(1000, 32, generator=gen).to(DEV)
    # y.backward() without create_graph: the same bits and the same peak memory as a default module
    outs, peaks = [], []
    for so in (False, True):
        m = make(shape, torch.float16, ws, False, second_order=so)
        for _ in range(2):   # the first step packs the images
            xr = x.clone().requires_grad_(True)
            m.params.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = m(xr)
            y.backward(g)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base   # what the step itself adds at its peak
        outs.append((y.detach(), xr.grad, m.params.grad))
        peaks.append(peak)
    for a, c in zip(*outs):
        assert a.dtype == c.dtype and torch.equal(a, c)
    assert peaks[0] == peaks[1], peaks
    # the default still refuses
    xr = x[:8].clone().requires_grad_(True)
    (g_x,) = torch.autograd.grad(make(shape, torch.float16, ws, False, second_order=False)(xr).float().sum(), xr, create_graph=True)
    with pytest.raises(NotImplementedError, match="second order"):
        g_x.sum().backward()
    # the launches of the second pass, and no device read
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    xr = x.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    (g_x,) = torch.autograd.grad(m(xr), xr, gr, create_graph=True)
    del calls[:]
    torch.cuda.set_sync_debug_mode("error")
    try:
        s_p, s_g = torch.autograd.grad(g_x, [m.params, gr], v)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == ["nfa_mlp_tangent", "nfa_mlp_bwd_weights"], calls
    assert s_g.dtype == torch.float16 and s_g.shape == (1000, 3) and s_p.shape == m.params.shape
    # a cotangent for dL/dparams, and a third order
    (g_p,) = torch.autograd.grad(m(xr).float().sum(), m.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="dL/dparams"):
        g_p.sum().backward()
    (g_x,) = torch.autograd.grad(m(xr), xr, gr, create_graph=True)
    (u,) = torch.autograd.grad(g_x, gr, v, create_graph=True)
    with pytest.raises(RuntimeError):
        u.sum().backward()
    # N = 0: empty / zero gradients, no launch
    x0 = torch.zeros(0, 32, device=DEV, requires_grad=True)
    g0 = torch.zeros(0, 3, dtype=torch.float16, device=DEV, requires_grad=True)
    (g_x0,) = torch.autograd.grad(m(x0), x0, g0, create_graph=True)
    del calls[:]
    s_p, s_g = torch.autograd.grad(g_x0.sum(), [m.params, g0])
    assert calls == [] and s_g.shape == (0, 3) and s_g.dtype == torch.float16 and not bool(s_p.any())
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    assert mlp_from_tcnn_config(8, 1, cfg, second_order=True).second_order and not mlp_from_tcnn_config(8, 1, cfg).second_order


# ---------------------------------------------------------------- end to end: an Eikonal step with no torch pass in the field

def test_eikonal_step_through_a_smoothstep_hash_grid():
    torch.manual_seed(0)
    enc = HashGridEncoding(3, 4, 2, 14, 16, 1.5, out_dtype=torch.float16, interpolation="Smoothstep").to(DEV)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    mlp = FusedMLP(8, 1, 64, 2, second_order=True).to(DEV)
    x = torch.rand(300, 3, device=DEV, requires_grad=True)
    seen = {}
    e = enc(x)
    # g_e = dL/de of the first backward; the hook on IT sees what the hash grid's second order hands back.  (The hook on e
    # fires in the second backward too, with no gradient: ds/de is None.)
    def on_g_e(g_e):
        if g_e is not None and g_e.requires_grad:
            g_e.register_hook(lambda gg_e: seen.__setitem__("gg_e", gg_e.detach().clone()))

    e.register_hook(on_g_e)
    sdf = mlp(e)
    sdf.register_hook(lambda g_: seen.__setitem__("g", g_.detach().clone()))
    (n,) = torch.autograd.grad(sdf.float().sum(), x, create_graph=True)
    ((n.norm(dim=-1) - 1.0) ** 2).mean().backward()
    assert set(seen) == {"g", "gg_e"} and seen["g"].shape == (300, 1) and seen["gg_e"].shape == (300, 8)
    for grad in (enc.params.grad, mlp.params.grad):
        assert bool(torch.isfinite(grad).all()) and bool(grad.any())
    # the Eikonal loss reaches the network's parameters through the second order alone; the module on its own, on the
    # captured tensors, must return the same bits (every pass is deterministic)
    alone = FusedMLP(8, 1, 64, 2, second_order=True).to(DEV)
    alone.load_state_dict(mlp.state_dict())
    ed = e.detach().clone().requires_grad_(True)
    (g_e,) = torch.autograd.grad(alone(ed), ed, seen["g"], create_graph=True)
    (want,) = torch.autograd.grad(g_e, alone.params, seen["gg_e"])
    assert torch.equal(mlp.params.grad, want)

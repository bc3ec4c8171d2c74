"""GPU: the fused MLP with biases and skip connections (csrc/mlp.hip behind nfa_mlp_desc).  Bit for bit on the integer-valued
families of tests/mlp_bias_skip_reference.py through the module and through the five nfa_mlp_net_* entries (hidden, every
dZ_l and every T_l too), every output buffer between guard rows; the golden fixture made from the reference's own MLP class;
random data within the derived bound at the T-NeRF warp shape and the SDF head; the same bits on every run; a bias segment of
the second-order gradient that is exactly zero; the old entries against the new ones; and one Eikonal step end to end."""
import pytest
import torch

import mlp_bias_skip_reference as S
import mlp_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, image_elems, wgrad_slices
from test_mlp_bias_skip_cpu import (GOLDEN_NETS, first_and_second_order, golden, golden_bound, golden_grads, golden_module, make,
                                    v_mod_of)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DEV = "cuda"
GUARD = 3          # guard rows on either side of every output buffer
SENTINEL = -7.0
assert wgrad_slices(300) == 2 and wgrad_slices(129) == 1


def guarded(rows, cols, dtype):
    whole = torch.full((rows + 2 * GUARD, cols), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows]


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def stacked(mats, dtype):
    return torch.cat(list(mats)).to(dtype).to(DEV).contiguous()


def run_abi(shape, skip_mask, dtype, ws, bs, x, g, v, out_f32, hidden_in=None, dz_in=None):
    """The five entries called directly.  The backward runs on ``hidden_in`` and the second order on ``hidden_in`` and
    ``dz_in`` where given (float64 values of ``dtype`` numbers: one mask and one dZ on both sides), else on what the passes
    before them wrote.  Returns CPU float64 tensors: y, hidden, dz (dZ_0 .. dZ_L), dx, dp (flat: matrices, then biases), u, t
    (T_0 .. T_{L-1}), sp (flat second-order gradient)."""
    n_in, n_out, width, n_hidden = shape
    N, elem = x.shape[0], B.ELEM_CODES[dtype]
    desc = B.MLPDesc(*shape, int(bs is not None), skip_mask)
    params = S.flat_params(ws, bs).to(DEV)
    P, n_w = params.numel(), sum(w.numel() for w in ws)
    fe, be = image_elems(*shape, skip_mask)
    fwd_w, fwd = guarded(fe // 512, 512, dtype)
    bwd_w, bwd = guarded(be // 512, 512, dtype)
    B.call("nfa_mlp_net_pack_weights", elem, desc, B.ptr(params), B.ptr(fwd), fe, B.ptr(bwd), be, B.stream())
    xd, gd, vd = x.to(DEV), g.to(DEV), v.to(DEV)
    bias_ptr = params.data_ptr() + 4 * n_w if bs is not None else None
    end = torch.float32 if out_f32 else dtype
    y_w, y = guarded(N, n_out, end)
    hid_w, hid = guarded(n_hidden * N, width, dtype)
    B.call("nfa_mlp_net_fwd", elem, desc, B.ptr(xd), B.ELEM_CODES[xd.dtype], B.ptr(fwd), bias_ptr, N, B.ptr(y), B.ELEM_CODES[end],
           B.ptr(hid), 1, B.stream())
    hidden_used = hid if hidden_in is None else stacked(hidden_in, dtype)
    dz_w, dz = guarded(n_hidden * N, width, dtype)
    dzo_w, dzo = guarded(N, n_out, dtype)
    dx_w, dx = guarded(N, n_in, xd.dtype)
    g_is_half = gd.dtype == dtype
    B.call("nfa_mlp_net_bwd_data", elem, desc, B.ptr(gd), B.ELEM_CODES[gd.dtype], B.ptr(hidden_used), B.ptr(bwd), N, B.ptr(dz),
           None if g_is_half else B.ptr(dzo), B.ptr(dx), B.ELEM_CODES[xd.dtype], B.stream())
    dz_out = gd if g_is_half else dzo
    part_w, part = guarded(wgrad_slices(N) * P, 1, torch.float32)
    gp_w, gp = guarded(P, 1, torch.float32)
    B.call("nfa_mlp_net_bwd_weights", elem, desc, B.ptr(xd), B.ELEM_CODES[xd.dtype], B.ptr(hidden_used), B.ptr(dz), B.ptr(dz_out), N,
           B.ptr(part), part.numel(), B.ptr(gp), 0, B.stream())
    # the second order
    dz_used, dzo_used = (dz, dz_out) if dz_in is None else (stacked(dz_in[:-1], dtype), dz_in[-1].to(dtype).to(DEV).contiguous())
    tan_w, tan = guarded(n_hidden * N, width, dtype)
    u_w, u = guarded(N, n_out, end)
    B.call("nfa_mlp_net_tangent", elem, desc, B.ptr(vd), B.ELEM_CODES[vd.dtype], B.ptr(hidden_used), B.ptr(fwd), N, B.ptr(tan), B.ptr(u),
           B.ELEM_CODES[end], B.stream())
    part2_w, part2 = guarded(wgrad_slices(N) * P, 1, torch.float32)
    sp_w, sp = guarded(P, 1, torch.float32)
    B.call("nfa_mlp_net_bwd_weights", elem, desc, B.ptr(vd), B.ELEM_CODES[vd.dtype], B.ptr(tan), B.ptr(dz_used), B.ptr(dzo_used), N,
           B.ptr(part2), part2.numel(), B.ptr(sp), 1, B.stream())
    torch.cuda.synchronize()
    for name, whole in [("fwd image", fwd_w), ("bwd image", bwd_w), ("y", y_w), ("hidden", hid_w), ("dz", dz_w), ("dz_out", dzo_w),
                        ("dx", dx_w), ("partials", part_w), ("grad_params", gp_w), ("tangent", tan_w), ("u", u_w),
                        ("partials (second order)", part2_w), ("second-order grad_params", sp_w)]:
        assert guards_intact(whole), f"{name}: guard rows overwritten"
    if g_is_half:
        assert bool((dzo == SENTINEL).all()), "dz_out written although it was not passed"
    c = lambda t: t.cpu().double()
    rows = lambda t: [c(t[l * N:(l + 1) * N]) for l in range(n_hidden)]
    return dict(y=c(y), hidden=rows(hid), dz=rows(dz) + [c(gd) if g_is_half else c(dzo)], dx=c(dx), dp=c(gp).view(-1), u=c(u), t=rows(tan),
                sp=c(sp).view(-1))


def check_exact(case, dtype):
    family, width, n_hidden, skip_layer, bias, cfg = case
    shape, skip_mask, ws, bs, x, g, v, f, b, s = S.exact_case(family, dtype, width, n_hidden, cfg, bias, skip_layer, v_mod_of(case))
    n_bias = sum(w.shape[0] for w in ws) if bias else 0
    want_p = S.flat_params(b["dw"], b["db"] if bias else None)
    want_sp = torch.cat([S.flat_params(s["dw"]), torch.zeros(n_bias, dtype=torch.float64)])
    tag = f"{case} {dtype}"
    # through the module: a real backward and double backward
    y, g_x, g_p, u, s_p, s_x = first_and_second_order(make(shape, dtype, ws, bs, skip_layer, cfg[4], device=DEV), x, g, v)
    assert y.dtype == (torch.float32 if cfg[4] else dtype) and g_x.dtype == x.dtype and g_p.dtype == s_p.dtype == torch.float32
    assert torch.equal(y.cpu().double(), f["y"]), f"y: {tag}"
    assert torch.equal(g_x.cpu().double(), b["dx"]), f"dL/dx: {tag}"
    assert torch.equal(g_p.cpu().double(), want_p), f"dL/dparams: {tag}"
    assert torch.equal(u.cpu().double(), s["u"]), f"u: {tag}"
    assert torch.equal(s_p.cpu().double(), want_sp), f"ds/dparams: {tag}"
    assert s_x is None or not bool(s_x.any()), f"ds/dx: {tag}"
    # through the C ABI: the intermediates too
    a = run_abi(shape, skip_mask, dtype, ws, bs, x, g, v, cfg[4])
    assert torch.equal(a["y"], f["y"]), f"abi y: {tag}"
    for l in range(n_hidden):
        assert torch.equal(a["hidden"][l], f["hidden"][l]), f"hidden {l}: {tag}"
        assert torch.equal(a["t"][l], s["t"][l + 1]), f"T_{l}: {tag}"
    for l in range(n_hidden + 1):
        assert torch.equal(a["dz"][l], b["dz"][l]), f"dZ_{l}: {tag}"
    assert torch.equal(a["dx"], b["dx"]), f"abi dL/dx: {tag}"
    assert torch.equal(a["dp"], want_p), f"abi dW, db: {tag}"
    assert torch.equal(a["u"], s["u"]), f"abi u: {tag}"
    assert torch.equal(a["sp"], want_sp), f"abi ds/dW, ds/db: {tag}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: f"{c[0]}-W{c[1]}-L{c[2]}-skip{c[3]}-bias{int(c[4])}-N{c[5][0]}-in{c[5][1]}-out{c[5][2]}")
def test_exact(case, dtype):
    check_exact(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_partial_tile_after_full_sweeps(dtype):
    """128 wide, 4 hidden layers, layer 3 takes [H, x], biases: 128 KiB of forward and 132 KiB of backward image, one workgroup
    per compute unit, 256 x 4 waves x 32 points a sweep.  Two full sweeps, five full tiles and a tile of 7 points."""
    N = 2 * 256 * 4 * 32 + 5 * 32 + 7
    assert [e * 2 // 1024 for e in image_elems(36, 3, 128, 4, 8)] == [128, 132]
    check_exact(("perm", 128, 4, 2, True, (N, 36, 3, False, False)), dtype)


# ---------------------------------------------------------------- the golden fixture on the device

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", GOLDEN_NETS)
def test_golden_exact(net, dtype):
    meta, sd, d = golden(net + "_exact")
    y, g_x, g_p, want_p = golden_grads(golden_module(meta, sd, dtype, True, DEV), d, torch.float32)
    assert torch.equal(y.double(), d["y"]) and torch.equal(g_x.double(), d["dx"]) and torch.equal(g_p.double(), want_p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", GOLDEN_NETS)
def test_golden_xavier_within_the_bound(net, dtype):
    meta, sd, d = golden(net + "_xavier")
    m = golden_module(meta, sd, dtype, True, DEV)
    e_y, e_dx, e_p = golden_bound(meta, sd, d, dtype, m.n_hidden_layers, m.skip_mask)
    y, g_x, g_p, want_p = golden_grads(m, d, torch.float32)
    ratios = dict(y=S.worst_ratio(y, d["y"], e_y), dx=S.worst_ratio(g_x, d["dx"], e_dx), dparams=S.worst_ratio(g_p, want_p, e_p))
    print(f"golden {net} {dtype} error/bound ratios: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


# ---------------------------------------------------------------- random data, the derived bound

WARP = (36, 3, 64, 4, 2)       # T-NeRF's warp network: n_in, n_out, width, n_hidden, skip_layer; biases
SDF_HEAD = (32, 1, 64, 2, None)
RANDOM_NETS = {"warp": WARP, "sdf_head": SDF_HEAD}


def random_case(net, dtype, f32_ends, N=1000):
    *shape, skip_layer = RANDOM_NETS[net]
    skip_mask = S.skip_mask_of(skip_layer, shape[3])
    gen = torch.Generator().manual_seed(7)
    ws = [(torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 for o, i in S.layer_dims(*shape, skip_mask)]
    bs = [torch.rand(w.shape[0], generator=gen) - 0.5 for w in ws]
    end = torch.float32 if f32_ends else dtype
    x, g, v = (torch.randn(N, n, generator=gen).to(end) for n in (shape[0], shape[1], shape[0]))
    return tuple(shape), skip_layer, skip_mask, ws, bs, x, g, v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", list(RANDOM_NETS))
@pytest.mark.parametrize("f32_ends", [False, True])
def test_random_within_the_bound(net, dtype, f32_ends):
    shape, skip_layer, skip_mask, ws, bs, x, g, v = random_case(net, dtype, f32_ends)
    n_hidden = shape[3]
    f = S.forward(x, ws, bs, skip_mask, dtype, f32_ends)
    b = S.backward(x, ws, f["hidden"], g, skip_mask, dtype)
    s = S.second_order(v, ws, f["hidden"], b["dz"], skip_mask, dtype, f32_ends)
    with torch.no_grad():
        y = make(shape, dtype, ws, bs, skip_layer, f32_ends, device=DEV)(x.to(DEV))
    ratios = {"y": S.worst_ratio(y.cpu(), f["y"], f["e_y"])}
    # the backward and the second order on the REFERENCE's hidden activations and dZ: one mask and one dZ on both sides
    a = run_abi(shape, skip_mask, dtype, ws, bs, x, g, v, f32_ends, hidden_in=f["hidden"], dz_in=b["dz"])
    n_w = sum(w.numel() for w in ws)
    ratios["dx"] = S.worst_ratio(a["dx"], b["dx"], b["e_dx"])
    for l in range(n_hidden + 1):
        ratios[f"dz{l}"] = S.worst_ratio(a["dz"][l], b["dz"][l], b["e_dz"][l])
    ratios["dw"] = S.worst_ratio(a["dp"][:n_w], S.flat_params(b["dw"]), S.flat_params(b["e_dw"]))
    ratios["db"] = S.worst_ratio(a["dp"][n_w:], S.flat_params(b["db"]), S.flat_params(b["e_db"]))
    ratios["u"] = S.worst_ratio(a["u"], s["u"], s["e_u"])
    for l in range(n_hidden):
        ratios[f"t{l}"] = S.worst_ratio(a["t"][l], s["t"][l + 1], s["e_t"][l + 1])
    ratios["sw"] = S.worst_ratio(a["sp"][:n_w], S.flat_params(s["dw"]), S.flat_params(s["e_dw"]))
    print(f"mlp bias/skip error/bound ratios {net} {dtype} f32_ends={f32_ends}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert torch.equal(a["dz"][n_hidden], R.rnd(g.double(), dtype)), "dZ_L is g rounded: no error allowed"
    assert not bool(a["sp"][n_w:].any()), "the bias segment of the second-order gradient must be exactly zero"
    assert bool(a["dp"][n_w:].any()) and bool(a["sp"][:n_w].any())
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", list(RANDOM_NETS))
def test_bitwise_reproducible_and_zero_bias_segment(net, dtype):
    shape, skip_layer, skip_mask, ws, bs, x, g, v = random_case(net, dtype, False)
    m = make(shape, dtype, ws, bs, skip_layer, False, device=DEV)
    first = first_and_second_order(m, x, g, v)
    second = first_and_second_order(m, x, g, v)
    first_and_second_order(m, x[:333], g[:333], v[:333])   # another N in between: other slices, other scratch
    third = first_and_second_order(m, x, g, v)
    for other in (second, third):
        for a, b_ in zip(first[:5], other[:5]):
            assert a.dtype == b_.dtype and torch.equal(a, b_)
    n_w = m._offsets[-1]
    g_p, s_p = first[2], first[4]
    assert bool(g_p[n_w:].any()) and bool(s_p[:n_w].any()) and not bool(s_p[n_w:].any())
    assert first[5] is None or not bool(first[5].any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_old_entries_and_default_module_match_the_new_entries(dtype):
    """bias = 0, skip_mask = 0 through nfa_mlp_net_*: the bits of nfa_mlp_* and of a default FusedMLP."""
    import test_mlp_grad2_gpu as OLD2
    import test_mlp_gpu as OLD
    shape = (32, 3, 64, 2)
    ws = R.xavier_weights(*shape, seed=13)
    gen = torch.Generator().manual_seed(17)
    x, g, v = torch.randn(300, 32, generator=gen), torch.randn(300, 3, generator=gen).to(dtype), torch.randn(300, 32, generator=gen)
    new = run_abi(shape, 0, dtype, ws, None, x, g, v, False)
    old = OLD.run_abi(shape, dtype, ws, x, g, False)
    for k_new, k_old in [("y", "y"), ("dx", "dx"), ("dp", "dw")]:
        assert torch.equal(new[k_new], old[k_old]), k_new
    for l in range(2):
        assert torch.equal(new["hidden"][l], old["hidden"][l]) and torch.equal(new["dz"][l], old["dz"][l])
    old2 = OLD2.run_abi(shape, dtype, ws, v, new["hidden"], new["dz"], False)
    assert torch.equal(new["u"], old2["u"]) and torch.equal(new["sp"], old2["dw"])
    for l in range(2):
        assert torch.equal(new["t"][l], old2["t"][l])
    m = FusedMLP(*shape, dtype=dtype, second_order=True)
    m.load_linear_weights(ws)
    y, g_x, g_p, u, s_p, _ = first_and_second_order(m.to(DEV), x, g, v)
    assert torch.equal(y.cpu().double(), new["y"]) and torch.equal(g_x.cpu().double(), new["dx"]) and torch.equal(g_p.cpu().double(), new["dp"])
    assert torch.equal(u.cpu().double(), new["u"]) and torch.equal(s_p.cpu().double(), new["sp"])


def test_eikonal_step_from_a_sphere_like_start():
    """Smoothstep hash grid (fp16 out) -> FusedMLP(8 -> 64 -> 64 -> 1, bias, second order) with the output bias at -0.5: one
    step on the Eikonal term plus an SDF term gives finite, non-zero gradients for the table, the matrices and the biases.
    (The Eikonal term alone reaches the matrices through the second order and the biases not at all: ds/db is zero.)"""
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(0)
    enc = HashGridEncoding(3, 4, 2, 14, 16, 1.5, out_dtype=torch.float16, interpolation="Smoothstep").to(DEV)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    mlp = FusedMLP(8, 1, 64, 2, bias=True, second_order=True).to(DEV)
    with torch.no_grad():
        mlp.bias(2).fill_(-0.5)
    x = torch.rand(300, 3, device=DEV).requires_grad_(True)
    sdf = mlp(enc(x))
    (normals,) = torch.autograd.grad(sdf.float().sum(), x, create_graph=True)
    loss = ((normals.norm(dim=-1) - 1.0) ** 2).mean() + sdf.float().abs().mean()
    loss.backward()
    n_w = mlp._offsets[-1]
    for name, t in [("table", enc.params.grad), ("matrices", mlp.params.grad[:n_w]), ("biases", mlp.params.grad[n_w:])]:
        assert bool(torch.isfinite(t).all()) and bool(t.any()), name
    # the Eikonal term alone: the bias segment is exactly zero, the matrices are reached
    mlp.params.grad = None
    (normals,) = torch.autograd.grad(mlp(enc(x)).float().sum(), x, create_graph=True)
    ((normals.norm(dim=-1) - 1.0) ** 2).mean().backward()
    assert bool(mlp.params.grad[:n_w].any()) and not bool(mlp.params.grad[n_w:].any())

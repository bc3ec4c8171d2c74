"""CPU: the fused MLP's second order (FusedMLP(second_order=True)) through real autograd on the torch path: bit for bit the
float64 reference of tests/mlp_grad2_reference.py AND float64 torch.autograd on a plain ReLU nn.Linear stack on the
integer-valued data, within the derived bound on random data, the refusals and edge cases, and nfa_mlp_tangent's argument
checks through the loaded library (nothing reaches a GPU)."""
import pytest
import torch

import mlp_grad2_reference as G
import mlp_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, _tangent_torch, mlp_from_tcnn_config

DTYPES = [torch.float16, torch.bfloat16]


def make(shape, dtype, ws, out_f32, second_order=True):
    m = FusedMLP(*shape, dtype=dtype, out_dtype=torch.float32 if out_f32 else None, second_order=second_order)
    m.load_linear_weights(ws)
    return m


def second_order(m, x, g, v):
    """(u, ds/dparams, ds/dx or None) of s = <v, dL/dx> through autograd, g in y's dtype."""
    x = x.clone().requires_grad_(True)
    y = m(x)
    g = g.to(y.dtype).clone().requires_grad_(True)
    (g_x,) = torch.autograd.grad(y, x, g, create_graph=True)
    assert g_x.dtype == x.dtype
    g_p, u, s_x = torch.autograd.grad((g_x * v).sum(), [m.params, g, x], allow_unused=True)
    return u, g_p, s_x


@pytest.mark.parametrize("family", ["perm", "dense"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("n_hidden", [1, 2, 4])
def test_exact(family, dtype, width, n_hidden):
    for cfg, v_mod in G.configs(family, width, n_hidden):
        shape, ws, x, g, v, f, b, s = G.exact_case(family, dtype, width, n_hidden, cfg, v_mod)
        tag = f"{family} {dtype} W={width} hidden={n_hidden} cfg={cfg} v mod {v_mod}"
        u, g_p, s_x = second_order(make(shape, dtype, ws, cfg[4]), x, g, v)
        assert u.dtype == g.dtype and g_p.dtype == torch.float32 and g_p.shape == (sum(w.numel() for w in ws),)
        assert torch.equal(u.double(), s["u"]), f"u: {tag}"
        assert torch.equal(g_p.double(), R.flat(s["dw"])), f"ds/dparams: {tag}"
        assert s_x is None or not bool(s_x.any()), f"ds/dx: {tag}"
        # float64 autograd of a plain network: nothing rounds on this data, so it needs none of the formulas
        u64, dw64, sx64 = G.autograd_float64(x, ws, g, v)
        assert torch.equal(u.double(), u64), f"u against autograd: {tag}"
        assert torch.equal(g_p.double(), R.flat(dw64)), f"ds/dparams against autograd: {tag}"
        assert sx64 is None or not bool(sx64.any())


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
    # the torch path on the REFERENCE's hidden activations and dZ: one mask and one dZ on both sides
    u, g_p, ts = _tangent_torch(v, ws, [h.float() for h in f["hidden"]], [d.float() for d in b["dz"]], dtype, True)
    u = u if f32_ends else u.to(dtype)
    ratios = {"u": R.worst_ratio(u, s["u"], s["e_u"])}
    assert torch.equal(ts[0].double(), s["t"][0]), "T_{-1} is v rounded: no error allowed"
    for l in range(n_hidden):
        ratios[f"t{l}"] = R.worst_ratio(ts[l + 1], s["t"][l + 1], s["e_t"][l + 1])
    ratios["dw"] = R.worst_ratio(g_p, R.flat(s["dw"]), R.flat(s["e_dw"]))
    print(f"mlp second order error/bound ratios (torch path) {dtype} {shape} f32_ends={f32_ends}: "
          + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)


def test_reproducible_and_plain_backward_unaffected():
    shape = (32, 3, 64, 2)
    ws = R.xavier_weights(*shape, seed=13)
    gen = torch.Generator().manual_seed(17)
    x, g, v = torch.randn(200, 32, generator=gen), torch.randn(200, 3, generator=gen), torch.randn(200, 32, generator=gen)
    m = make(shape, torch.float16, ws, False)
    first = second_order(m, x, g, v)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        second = second_order(m, x, g, v)
    second_order(m, x[:77], g[:77], v[:77])
    third = second_order(m, x, g, v)
    for other in (second, third):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    # y.backward() without create_graph: the same bits as a default module
    outs = []
    for so in (False, True):
        mm = make(shape, torch.float16, ws, False, second_order=so)
        xr = x.clone().requires_grad_(True)
        y = mm(xr)
        y.backward(g.to(y.dtype))
        outs.append((y.detach(), xr.grad, mm.params.grad))
    for a, c in zip(*outs):
        assert a.dtype == c.dtype and torch.equal(a, c)


def test_refusals_and_edge_cases():
    ws = R.xavier_weights(16, 3, 64, 1, seed=3)
    x = torch.randn(8, 16, requires_grad=True)
    # the default still refuses, by name
    m0 = make((16, 3, 64, 1), torch.float16, ws, False, second_order=False)
    assert not m0.second_order and FusedMLP(16, 3).second_order is False
    (g_x,) = torch.autograd.grad(m0(x).float().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="second order"):
        g_x.sum().backward()
    m = make((16, 3, 64, 1), torch.float16, ws, False)
    assert m.second_order and "second_order=True" in m.extra_repr() and "second_order" not in m0.extra_repr()
    # a cotangent for dL/dparams
    y = m(x)
    (g_p,) = torch.autograd.grad(y.float().sum(), m.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="dL/dparams"):
        g_p.sum().backward()
    # a third order
    g = torch.ones(8, 3, dtype=torch.float16, requires_grad=True)
    (g_x,) = torch.autograd.grad(m(x), x, g, create_graph=True)
    (u,) = torch.autograd.grad(g_x.sum(), g, create_graph=True)
    with pytest.raises(RuntimeError):
        u.sum().backward()
    # N = 0: empty / zero gradients
    x0 = torch.zeros(0, 16, requires_grad=True)
    g0 = torch.zeros(0, 3, dtype=torch.float16, requires_grad=True)
    (g_x0,) = torch.autograd.grad(m(x0), x0, g0, create_graph=True)
    s_p, s_g = torch.autograd.grad(g_x0.sum(), [m.params, g0])
    assert g_x0.shape == (0, 16) and s_g.shape == (0, 3) and s_g.dtype == torch.float16
    assert s_p.shape == m.params.shape and not bool(s_p.any())
    # the flag through the tcnn config
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    assert mlp_from_tcnn_config(8, 1, cfg, second_order=True).second_order
    assert not mlp_from_tcnn_config(8, 1, cfg).second_order


def test_eikonal_step_matches_a_torch_network():
    """An SDF head: the Eikonal loss' parameter gradient against float32 autograd through nn.Linear layers with the rounded
    weights; loose, since the module rounds its activations: the exact tests carry the precision."""
    from torch import nn
    shape = (8, 1, 64, 2)
    ws = R.xavier_weights(*shape, seed=5)
    m = make(shape, torch.float16, ws, True)
    x = torch.randn(300, 8, generator=torch.Generator().manual_seed(2))

    def eikonal_grad(net, params):
        xr = x.clone().requires_grad_(True)
        (n,) = torch.autograd.grad(net(xr).float().sum(), xr, create_graph=True)
        return torch.autograd.grad(((n.norm(dim=-1) - 1.0) ** 2).mean(), params)

    (got,) = eikonal_grad(m, [m.params])
    lin = [nn.Linear(w.shape[1], w.shape[0], bias=False) for w in ws]
    with torch.no_grad():
        for l, w in zip(lin, ws):
            l.weight.copy_(w.half().float())
    seq = nn.Sequential(lin[0], nn.ReLU(), lin[1], nn.ReLU(), lin[2])
    want = R.flat(eikonal_grad(seq, [l.weight for l in lin]))
    assert got.shape == want.shape and bool(got.any())
    assert float((got - want).abs().max()) <= 0.02 * float(want.abs().max())


# ---------------------------------------------------------------- nfa_mlp_tangent's checks (nothing reaches a GPU)

P = 0x1000   # a stand-in address that is never dereferenced
F16, BF16, F32 = 1, 2, 0


def _tangent(elem=F16, n=64, n_in=32, n_out=16, width=64, n_hidden=2, v=P, v_elem=F32, hidden=P, img=P, tangent=P, u=P, u_elem=None):
    return B.load().nfa_mlp_tangent(elem, v, v_elem, hidden, img, n, n_in, n_out, width, n_hidden, tangent, u,
                                    elem if u_elem is None else u_elem, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(elem=F32), b"elem 0"), (dict(elem=7), b"elem 7"), (dict(width=96), b"width 96"), (dict(width=256), b"width 256"),
    (dict(n_hidden=0), b"n_hidden 0"), (dict(n_hidden=5), b"n_hidden 5"), (dict(n_in=0), b"n_in 0"), (dict(n_in=257), b"n_in 257"),
    (dict(n_out=0), b"n_out 0"), (dict(n_out=33), b"n_out 33"), (dict(n=-1), b"n_points -1 is negative"),
    (dict(width=128, n_hidden=4, n_in=256), b"do not fit the LDS"),
    (dict(v_elem=BF16), b"v_elem 2"), (dict(v_elem=5), b"v_elem 5"), (dict(u_elem=BF16), b"u_elem 2"), (dict(u_elem=9), b"u_elem 9"),
    (dict(v=None), b"null pointer"), (dict(hidden=None), b"null pointer"), (dict(img=None), b"null pointer"), (dict(u=None), b"null pointer"),
    (dict(img=P + 8), b"misaligned"), (dict(hidden=P + 4), b"misaligned"), (dict(tangent=P + 4), b"misaligned"),
    (dict(v=P + 2), b"misaligned"), (dict(v=P + 1, v_elem=F16), b"misaligned"), (dict(u=P + 1), b"misaligned"),
    (dict(u=P + 2, u_elem=F32), b"misaligned"),
])
def test_tangent_entry_argument_checks(kw, msg):
    lib = B.load()
    assert _tangent(**kw) == -1 and msg in lib.nfa_last_error() and b"nfa_mlp_tangent" in lib.nfa_last_error(), lib.nfa_last_error()


def test_tangent_entry_empty_and_exported():
    # N = 0 returns 0 with every pointer null; the tangent buffer itself is optional (checked on the GPU)
    assert _tangent(n=0, v=None, hidden=None, img=None, tangent=None, u=None) == 0
    assert "nfa_mlp_tangent" in B.EXPORTED_SYMBOLS and B.load().nfa_version() == 403

"""CPU: the fused MLP's activations (FusedMLP(activation=, output_activation=, activation_beta=)).  The torch restatements of
nerfacc_amd/mlp.py against the float64 reference of tests/mlp_act_reference.py within its derived bound, for every activation
as hidden and as output activation, both half types, with biases and a skip; the unrounded float64 form of the restatements
against torch.autograd with create_graph=True (the mathematics: dx, dW, db, u, ds/dx, ds/dW, ds/db); the module's autograd
wiring against the restatements; and what the constructors and mlp_from_tcnn_config accept and refuse."""
import pytest
import torch

import mlp_act_reference as A
import mlp_bias_skip_reference as S
from nerfacc_amd import mlp as M
from nerfacc_amd.mlp import FusedMLP, NerfMLP, StreamedMLP, mlp_from_tcnn_config, reference_mlp

DTYPES = [torch.float16, torch.bfloat16]
CURVED = [("Sigmoid", 10.0), ("Tanh", 10.0), ("Softplus", 10.0), ("Softplus", 100.0), ("Exponential", 10.0)]
# every activation once as hidden and once as output activation: (hidden, output, beta)
ACTS = ([(n, "None", b) for n, b in CURVED] + [("ReLU", n, b) for n, b in CURVED]
        + [("LeakyReLU", "None", 10.0), ("None", "LeakyReLU", 10.0), ("ReLU", "ReLU", 10.0), ("Softplus", "Sigmoid", 100.0)])
NET = (12, 3, 64, 3, 2)   # n_in, n_out, width, n_hidden, skip_layer: layer 3, the output layer, takes [H, x]; biases
N = 70
act_id = lambda a: f"{a[0]}-{a[1]}-b{a[2]:g}"


def make(shape, dtype, ws, bs, skip_layer, act, out_f32=False, second_order=True, device="cpu"):
    m = FusedMLP(*shape, dtype=dtype, out_dtype=torch.float32 if out_f32 else None, second_order=second_order, bias=bs is not None,
                 skip_layer=skip_layer, activation=act[0], output_activation=act[1], activation_beta=act[2])
    m.load_linear_weights(ws, bs)
    return m.to(device)


def case(act, dtype, f32_ends=False):
    *shape, skip_layer = NET
    scale = 0.25 if "Exponential" in act[:2] else 1.0
    skip_mask, ws, bs, x, g, v = A.random_net(tuple(shape), skip_layer, N=N, dtype=dtype, f32_ends=f32_ends, scale=scale)
    return tuple(shape), skip_layer, skip_mask, ws, bs, x, g, v


def first_and_second_order(m, x, g, v):
    """(y, dL/dx, dL/dparams, u, ds/dparams, ds/dx) through the module's autograd."""
    xr = x.to(m.params.device).clone().requires_grad_(True)
    gr = g.to(m.params.device).clone().requires_grad_(True)
    y = m(xr)
    g_x, g_p = torch.autograd.grad(y, [xr, m.params], gr, create_graph=True)
    u, s_p, s_x = torch.autograd.grad(g_x, [gr, m.params, xr], v.to(g_x.device).to(g_x.dtype), allow_unused=True)
    return y.detach(), g_x.detach(), g_p.detach(), u, s_p, s_x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ACTS, ids=act_id)
def test_restatements_within_the_bound(act, dtype):
    shape, skip_layer, skip_mask, ws, bs, x, g, v = case(act, dtype)
    f = A.forward(x, ws, bs, skip_mask, dtype, act)
    y, hidden = M._forward_torch(x, ws, dtype, False, bs, skip_mask, act)
    ratios = {"y": A.worst_ratio(y, f["y"], f["e_y"])}
    for l, h in enumerate(hidden):
        ratios[f"h{l}"] = A.worst_ratio(h, f["hidden"][l], f["e_hidden"][l])
    # everything behind the forward on the REFERENCE's stored values: one derivative factor, one dZ, one R on both sides
    hid32, y32 = [h.float() for h in f["hidden"]], f["y"].float()
    b = A.backward(x, ws, f["hidden"], f["y"], g, skip_mask, dtype, act)
    g_x, g_p, dzs = M._backward_torch(x, ws, hid32, g, dtype, True, True, True, skip_mask, act, y32)
    n_w = sum(w.numel() for w in ws)
    ratios["dx"] = A.worst_ratio(g_x, b["dx"], b["e_dx"])
    for l, d in enumerate(dzs):
        ratios[f"dz{l}"] = A.worst_ratio(d, b["dz"][l], b["e_dz"][l])
    ratios["dw"] = A.worst_ratio(g_p[:n_w], S.flat_params(b["dw"]), S.flat_params(b["e_dw"]))
    ratios["db"] = A.worst_ratio(g_p[n_w:], S.flat_params(b["db"]), S.flat_params(b["e_db"]))
    t = A.tangent(v, ws, f["hidden"], f["y"], b["dz"], skip_mask, dtype, act, out_f32=True)
    u, s_p, ts, rs = M._tangent_terms(v, ws, hid32, [d.float() for d in b["dz"]], dtype, True, True, skip_mask, act, y32)
    ratios["u"] = A.worst_ratio(u, t["u"], t["e_u"])
    for l in range(len(hidden)):
        ratios[f"t{l}"] = A.worst_ratio(ts[l + 1], t["t"][l + 1], t["e_t"][l + 1])
    for l in range(len(ws)):
        ratios[f"r{l}"] = A.worst_ratio(rs[l], t["r"][l], t["e_r"][l])
    sw, e_sw = A.tangent_weight_grad(b["dz"], t, skip_mask)
    ratios["sw"] = A.worst_ratio(s_p[:n_w], S.flat_params(sw), S.flat_params(e_sw))
    assert not bool(s_p[n_w:].any())
    c = A.backward(x, ws, f["hidden"], None, t["r"][-1], skip_mask, dtype, act, inject=t["r"][:-1])
    s_x, c_p, es = M._curvature_torch(x, ws, hid32, [r.float() for r in t["r"]], dtype, True, True, True, skip_mask, act)
    ratios["sx"] = A.worst_ratio(s_x, c["dx"], c["e_dx"])
    for l, e in enumerate(es):
        ratios[f"e{l}"] = A.worst_ratio(e, c["dz"][l], c["e_dz"][l])
    ratios["cw"] = A.worst_ratio(c_p[:n_w], S.flat_params(c["dw"]), S.flat_params(c["e_dw"]))
    ratios["cb"] = A.worst_ratio(c_p[n_w:], S.flat_params(c["db"]), S.flat_params(c["e_db"]))
    print(f"mlp act cpu error/bound ratios {act} {dtype}: " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    curved = act[0] in A.CURVED or act[1] in A.CURVED
    assert bool(u.any()) and bool(g_x.any()) and bool(torch.cat([r.reshape(-1) for r in rs]).any()) == curved
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)


@pytest.mark.parametrize("bias,skip_layer", [(True, 2), (False, None)])
@pytest.mark.parametrize("act", ACTS, ids=act_id)
def test_float64_form_against_autograd(act, bias, skip_layer):
    """The restatements with dtype=torch.float64 round nothing: the mathematics of all four passes against torch.autograd."""
    shape = NET[:4]
    skip_mask, ws, bs, x, g, v = A.random_net(shape, skip_layer, N=40, scale=0.25 if "Exponential" in act[:2] else 1.0)
    bs = bs if bias else None
    ws, x, g, v = [w.double() for w in ws], x.double(), g.double(), v.double()
    bs = [b_.double() for b_ in bs] if bias else None
    want = A.autograd_float64(x, ws, bs, skip_mask, act, g, v)
    d = torch.float64
    y, hidden = M._forward_torch(x, ws, d, True, bs, skip_mask, act)
    g_x, g_p, dzs = M._backward_torch(x, ws, hidden, g, d, True, True, bias, skip_mask, act, y)
    u, s_p, ts, rs = M._tangent_terms(v, ws, hidden, dzs, d, True, bias, skip_mask, act, y)
    s_x, c_p, _ = M._curvature_torch(x, ws, hidden, rs, d, True, True, bias, skip_mask, act)
    flat = lambda mats, vecs: S.flat_params(mats, vecs if bias else None)
    for name, got, ref in [("y", y, want["y"]), ("dx", g_x, want["dx"]), ("dW, db", g_p, flat(want["dw"], want["db"])), ("u", u, want["u"]),
                           ("ds/dx", s_x, want["sx"]), ("ds/dW, ds/db", s_p + c_p, flat(want["sw"], want["sb"]))]:
        scale = max(float(ref.abs().max()), 1.0)
        assert float((got - ref).abs().max()) <= 1e-10 * scale, (name, float((got - ref).abs().max()), scale)
    if not (act[0] in A.CURVED or act[1] in A.CURVED):
        assert not bool(s_x.any()) and not bool(c_p.any())
    elif bias:
        assert bool(want["sb"][0].any()) and bool(want["sx"].any())


@pytest.mark.parametrize("act", [("Softplus", "Sigmoid", 100.0), ("Tanh", "None", 10.0), ("LeakyReLU", "Exponential", 10.0),
                                 ("ReLU", "None", 10.0), ("None", "LeakyReLU", 10.0), ("ReLU", "ReLU", 10.0)], ids=act_id)
@pytest.mark.parametrize("f32_ends", [False, True])
def test_module_is_the_restatements(act, f32_ends):
    """The module's autograd on CPU tensors: the bits of the four restatements chained by hand, ds/dx included."""
    dtype = torch.float16
    shape, skip_layer, skip_mask, ws, bs, x, g, v = case(act, dtype, f32_ends)
    m = make(shape, dtype, ws, bs, skip_layer, act, f32_ends)
    y, g_x, g_p, u, s_p, s_x = first_and_second_order(m, x, g, v)
    with torch.no_grad():
        wy, hidden = M._forward_torch(x, ws, dtype, f32_ends, bs, skip_mask, act)
        wx, wp, dzs = M._backward_torch(x, ws, hidden, g, dtype, True, True, True, skip_mask, act, wy)
        wu, wsp, _, rs = M._tangent_terms(v, ws, hidden, dzs, dtype, True, True, skip_mask, act, wy)
        wsx, wcp, _ = M._curvature_torch(x, ws, hidden, rs, dtype, True, True, True, skip_mask, act)
    curved = act[0] in A.CURVED or act[1] in A.CURVED
    assert torch.equal(y, wy) and torch.equal(g_x, wx) and torch.equal(g_p, wp) and torch.equal(u, wu.to(g.dtype))
    assert torch.equal(s_p, wsp + wcp if curved else wsp)
    n_w = m._offsets[-1]
    if curved:
        assert torch.equal(s_x, wsx) and s_x.dtype == x.dtype and bool(s_x.any()) and bool(s_p[n_w:].any())
    else:
        assert s_x is None and not bool(s_p[n_w:].any())
    assert repr(m).count("activation=") == (0 if act[:2] == ("ReLU", "None") else 2)


def test_constructor_and_config_accept_and_refuse():
    for name in A.NAMES:
        m = FusedMLP(8, 2, 64, 1, activation=name, output_activation=name)
        assert (m.activation, m.output_activation, m.activation_beta) == (name, name, 10.0)
        cfg = {"otype": "FullyFusedMLP", "activation": name, "output_activation": name, "n_neurons": 64, "n_hidden_layers": 2}
        c = mlp_from_tcnn_config(8, 2, cfg, activations=True, activation_beta=100.0)
        assert (c.activation, c.output_activation, c.activation_beta) == (name, name, 100.0)
    assert FusedMLP(8, 2, output_activation=None).output_activation == "None"
    for bad in ("Sine", "Squareplus"):
        for kw in ("activation", "output_activation"):
            with pytest.raises(ValueError, match=bad):
                FusedMLP(8, 2, **{kw: bad})
            with pytest.raises(ValueError, match=bad):
                mlp_from_tcnn_config(8, 2, {kw: bad, "n_neurons": 64, "n_hidden_layers": 1}, activations=True)
    with pytest.raises(ValueError, match="'gelu'"):
        FusedMLP(8, 2, activation="gelu")
    for beta in (0.0, -1.0, float("nan"), float("inf"), "10"):
        with pytest.raises(ValueError, match="activation_beta"):
            FusedMLP(8, 2, activation="Softplus", activation_beta=beta)
    for kw in (dict(activation="Softplus"), dict(output_activation="Sigmoid"), dict(activation_beta=100.0)):
        with pytest.raises(ValueError, match="StreamedMLP"):
            StreamedMLP(63, 4, **kw)
        with pytest.raises(ValueError, match="NerfMLP"):
            NerfMLP(63, 0, **kw)
    assert StreamedMLP(63, 4, 128, 2, activation="ReLU", output_activation="None").activation == "ReLU"


def test_default_path_is_unchanged():
    cfg = {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2}
    with pytest.raises(ValueError, match="'activation'"):
        mlp_from_tcnn_config(8, 1, dict(cfg, activation="Sigmoid"))
    with pytest.raises(ValueError, match="'output_activation'"):
        mlp_from_tcnn_config(8, 1, dict(cfg, output_activation="ReLU"))
    with pytest.raises(ValueError, match="hidden_activation"):
        reference_mlp(8, 1, 2, 64, hidden_activation="Softplus")
    with pytest.raises(ValueError, match="output_activation"):
        reference_mlp(8, 1, 2, 64, output_activation="Sigmoid")
    m, d = FusedMLP(8, 1, 64, 2, second_order=True, bias=True), mlp_from_tcnn_config(8, 1, cfg, activations=True)
    assert m._act is None and d._act is None and "activation" not in repr(m) and not m._curved and not m._out_act
    assert repr(FusedMLP(8, 1, 64, 2)) == ("FusedMLP(8 -> 64 -> 64 -> 1, dtype=torch.float16, out_dtype=torch.float16)")
    # the default module's second order: ds/dx is None, ds/db exactly zero
    x, g, v = torch.randn(33, 8), torch.randn(33, 1), torch.randn(33, 8)
    *_, s_p, s_x = first_and_second_order(m, x, g, v)
    assert s_x is None and not bool(s_p[m._offsets[-1]:].any()) and bool(s_p.any())
    # the second order of dL/dparams keeps raising, with activations too
    a = FusedMLP(8, 1, 64, 2, second_order=True, activation="Softplus")
    (g_p,) = torch.autograd.grad(a(x.requires_grad_(True)).float().sum(), a.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="dL/dparams"):
        g_p.sum().backward()

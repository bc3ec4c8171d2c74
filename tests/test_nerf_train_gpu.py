"""The fused NeRF field's training pass (nfa_nerf_train_fwd in nerfacc_amd/csrc/nerf_field.hip, nfa_nerf_train_bwd in
nerfacc_amd/csrc/nerf_train.hip, VanillaNeRFRadianceField(fused_training=True)) against the no-grad launch, the composed chain
and float64 autograd.

Largest (fused error) / (composed chain's error) against float64 seen on the device in test_gradients_against_float64: 1.105
(trunk.w2, 1.8e-3 against 1.6e-3; the bound is 2); DESIGN.md, "Fused NeRF field: training".
"""
import pytest
import torch

import mlp_stream_reference as M
import nerf_field_reference as F
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import TNeRFRadianceField, VanillaNeRFRadianceField
from test_nerf_field_gpu import CAT_OUT, FLAT, REF, make_inputs

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
# (network, N, ray samples?, dtype, weights, roll).  N: 1; 33 (a partial tile and three idle waves); 129 (two passes); 300.
# The rolls are chosen so that on the composed chain every layer receives a gradient, at N = 1 too (one open path per output).
CASES = [
    (REF, 1, False, F16, "perm", (3, 85)), (REF, 33, True, BF16, "perm", (11, 130)), (REF, 129, False, BF16, "xavier", None),
    (REF, 300, True, F16, "xavier", None), (FLAT, 1, True, BF16, "xavier", None), (FLAT, 33, False, F16, "perm", (0, 130)),
    (FLAT, 129, True, F16, "perm", (5, 140)), (FLAT, 300, False, BF16, "perm", (0, 0)), (CAT_OUT, 1, False, BF16, "perm", (0, 84)),
    (CAT_OUT, 33, True, F16, "xavier", None), (CAT_OUT, 129, False, F16, "perm", (3, 85)), (CAT_OUT, 300, True, BF16, "perm", (0, 85)),
]
case_id = lambda c: f"W{c[0][0]}-D{c[0][1]}-N{c[1]}-{'rays' if c[2] else 'points'}-{'fp16' if c[3] == F16 else 'bf16'}-{c[4]}"


def make_field(net, dtype, dev, kind, roll, fused_training):
    f = VanillaNeRFRadianceField(net[1], net[0], net[2], net[3], dtype=dtype, fused_training=fused_training)
    if kind == "perm":
        _, tw, tb, hw, hb = F.perm_weights(net[0], net[1], net[2], net[3], roll)
        f.mlp.trunk.load_linear_weights(tw, tb), f.mlp.head.load_linear_weights(hw, hb)
    else:
        f.mlp.load_reference_state_dict(M.nerf_state_dict("xavier", F.POS_DIMS, F.DIR_DIMS, net[1], net[0], net[2], net[3], 128))
    return f.to(dev)


def stream_forward(mlp, x):
    """(y, hidden) of the composed chain's own streamed forward with its activations saved."""
    N, p = x.shape[0], mlp.params
    y = torch.empty(N, mlp.n_output_dims, dtype=mlp.dtype, device=x.device)
    hidden = torch.empty(mlp.n_hidden_layers, N, mlp.n_neurons, dtype=mlp.dtype, device=x.device)
    B.call("nfa_mlp_stream_fwd", B.ELEM_CODES[mlp.dtype], mlp._desc, B.ptr(x), B.ELEM_CODES[x.dtype], B.ptr(mlp._images(p)[0]), mlp._bias_ptr(p),
           N, B.ptr(y), B.ELEM_CODES[y.dtype], B.ptr(hidden), 1, B.stream())
    return y, hidden


def param_grads(f):
    """Every parameter gradient as named per-layer views, and the gradients cleared."""
    out = {}
    for name, mlp in (("trunk", f.mlp.trunk), ("head", f.mlp.head)):
        g = mlp.params.grad
        for l, (w, b) in enumerate(zip(mlp._views(g), mlp._bias_views(g))):
            out[f"{name}.w{l}"], out[f"{name}.b{l}"] = w.clone(), b.clone()
        mlp.params.grad = None
    return out


def incoming(N, dev):
    gen = torch.Generator().manual_seed(3 + N)
    return torch.randn(N, 3, generator=gen).to(dev), torch.randn(N, generator=gen).to(dev)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_bits_and_saved_buffers(dev, case):
    net, N, rays, dtype, kind, roll = case
    f = make_field(net, dtype, dev, kind, roll, True)
    t, h, W = f.mlp.trunk, f.mlp.head, net[0]
    inp, x, d = make_inputs(N, rays, dev)
    new = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=dev)
    with torch.no_grad():
        enc_x, enc_d = f.posi_encoder(x), f.view_encoder(d)   # what the composed chain stores: computed once
        y, t_hidden = stream_forward(t, enc_x)
        h_in = torch.cat([y[:, :W], enc_d], 1)
        h_hidden = stream_forward(h, h_in)[1]
        for act in (False, True):
            for kw in ({}, dict(rgb_dtype=F32, sigma_dtype=F32)):
                saved = [new(N, 63), new(t.n_hidden_layers, N, W), new(N, W + 27), new(h.n_hidden_layers, N, 128)]
                got, want = f._launch(True, N, act, **inp, **kw, save=saved), f._launch(True, N, act, **inp, **kw)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                assert torch.equal(saved[0], enc_x) and torch.equal(saved[1], t_hidden) and torch.equal(saved[2], h_in)
                if kind == "perm":   # otherwise the head's first layer sums in another order
                    assert torch.equal(saved[3], h_hidden)


@pytest.mark.parametrize("g_f32", [True, False], ids=["g-float32", "g-half"])
@pytest.mark.parametrize("case", [c for c in CASES if c[4] == "perm"], ids=case_id)
def test_gradients_exact_on_the_perm_family(dev, case, g_f32):
    net, N, rays, dtype, kind, roll = case
    on, off = (make_field(net, dtype, dev, kind, roll, ft) for ft in (True, False))
    inp, x, d = make_inputs(N, rays, dev)
    g_rgb, g_sigma = incoming(N, dev)
    rgb, sigma = off.query_raw(x, d)
    ((rgb.float() * g_rgb).sum() + (sigma.float() * g_sigma).sum()).backward()
    want = param_grads(off)
    # the guard: the composed chain's gradients are non-zero in every layer, so that nothing is compared as 0 == 0
    assert [k for k, v in want.items() if not v.abs().max() > 0] == []
    kw = dict(rgb_dtype=F32, sigma_dtype=F32) if g_f32 else {}
    rgb, sigma = on._train(False, N, **inp, **kw)
    ((rgb.float() * g_rgb).sum() + (sigma.float() * g_sigma).sum()).backward()
    got = param_grads(on)
    assert [k for k in want if not torch.equal(got[k], want[k])] == []


def float64_gradients(f, x, d, g_rgb, g_sigma, activated):
    """float64 autograd over a plain restatement of the field from the same master weights."""
    def enc(v, L):
        s = v.double()[:, None, :] * (2.0 ** torch.arange(L, dtype=torch.float64, device=v.device))[None, :, None]
        return torch.cat([v.double(), torch.sin(s).flatten(1), torch.cos(s).flatten(1)], 1)

    def mlp(m, name, x0, leaves):
        hid = x0
        for l, (w, b) in enumerate(zip(m.linear_weights(), m.linear_biases())):
            w, b = w.double().requires_grad_(), b.double().requires_grad_()
            leaves[f"{name}.w{l}"], leaves[f"{name}.b{l}"] = w, b
            z = (torch.cat([hid, x0], 1) if (m.skip_mask >> l) & 1 else hid) @ w.t() + b
            hid = torch.relu(z) if l < m.n_hidden_layers else z
        return hid

    leaves, W = {}, f.mlp.net_width
    y = mlp(f.mlp.trunk, "trunk", enc(x, 10), leaves)
    rgb, sigma = mlp(f.mlp.head, "head", torch.cat([y[:, :W], enc(d, 4)], 1), leaves), y[:, W]
    if activated:
        rgb, sigma = torch.sigmoid(rgb), torch.relu(sigma)
    ((rgb * g_rgb.double()).sum() + (sigma * g_sigma.double()).sum()).backward()
    return {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("activated", [False, True], ids=["raw", "activated"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("net", [REF, FLAT, CAT_OUT], ids=["ref", "flat", "cat_out"])
def test_gradients_against_float64(dev, net, dtype, activated):
    """Xavier weights, biases in +-0.5, N = 300.  Per parameter tensor: max |g - ref| / max |ref|; the fused path's is at most twice
    the composed chain's ("Fused NeRF field: training": the same rounding points, another summation order in the head's
    first layer)."""
    N, rays = 300, (net is FLAT) != activated
    on, off = (make_field(net, dtype, dev, "xavier", None, ft) for ft in (True, False))
    inp, x, d = make_inputs(N, rays, dev)
    g_rgb, g_sigma = incoming(N, dev)
    ref = float64_gradients(off, x, d, g_rgb, g_sigma, activated)
    grads = []
    for f in (on, off):
        if rays:
            rgb, sigma = f.query_on_rays(*inp["rays"], raw=not activated)
        else:
            rgb, sigma = f(x, d) if activated else f.query_raw(x, d)
        ((rgb.float() * g_rgb).sum() + (sigma.float().view(-1) * g_sigma).sum()).backward()
        grads.append(param_grads(f))
    err = lambda g, k: float((g[k].double() - ref[k]).abs().max() / ref[k].abs().max())
    ratios = {k: (err(grads[0], k), err(grads[1], k)) for k in ref}
    worst = max(ratios, key=lambda k: ratios[k][0] / max(ratios[k][1], 1e-300))
    print(f"worst fused / composed error ratio: {worst} {ratios[worst][0]:.3e} / {ratios[worst][1]:.3e} = "
          f"{ratios[worst][0] / max(ratios[worst][1], 1e-300):.3f}; largest fused error {max(v[0] for v in ratios.values()):.3e}")
    assert [(k, v) for k, v in ratios.items() if not v[0] <= 2.0 * v[1]] == []


def test_dispatch(dev, monkeypatch):
    f = VanillaNeRFRadianceField(2, 128, None, 1, fused_training=True).to(dev)
    off = VanillaNeRFRadianceField(2, 128, None, 1).to(dev)
    off.load_state_dict(f.state_dict())
    gen = torch.Generator().manual_seed(5)
    x, d = torch.rand(200, 3, generator=gen).to(dev), torch.randn(200, 3, generator=gen).to(dev)
    names, call = [], B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), call(name, *a))[1])

    def grads(field, xin):
        rgb, sigma = field(xin, d)
        (rgb.float().sum() + sigma.float().sum()).backward()
        return param_grads(field)

    first = grads(f, x)
    assert names.count("nfa_nerf_train_fwd") == 1 and names.count("nfa_nerf_train_bwd") == 1 and "nfa_mlp_stream_fwd" not in names
    again = grads(f, x)
    assert all(torch.equal(first[k], again[k]) for k in first)
    # positions that require grad: the composed chain, its values and a gradient towards x
    del names[:]
    xg = x.clone().requires_grad_()
    rgb, sigma = f(xg, d)
    assert "nfa_nerf_train_fwd" not in names and "nfa_mlp_stream_fwd" in names
    want = off(x, d)
    assert torch.equal(rgb, want[0]) and torch.equal(sigma, want[1])
    (rgb.float().sum() + sigma.float().sum()).backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
    # fused={"full": False} switches the training launches off with the fused full query
    del names[:]
    sw = VanillaNeRFRadianceField(2, 128, None, 1, fused={"full": False}, fused_training=True).to(dev)
    sw(x, d)
    assert "nfa_nerf_train_fwd" not in names and "nfa_mlp_stream_fwd" in names
    # the second order
    rgb, sigma = f(x, d)
    g, = torch.autograd.grad(rgb.float().sum(), f.mlp.head.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="VanillaNeRFRadianceField"):
        g.sum().backward()
    # T-NeRF trains unchanged: its nerf takes the composed chain
    del names[:]
    tn = TNeRFRadianceField().to(dev)
    rgb, sigma = tn(x, torch.rand(200, 1, generator=gen).to(dev), d)
    (rgb.float().sum() + sigma.float().sum()).backward()
    assert "nfa_nerf_train_fwd" not in names and all(p.grad is not None and torch.isfinite(p.grad).all() for p in tn.parameters())
    assert f(x[:0], d[:0])[0].shape == (0, 3)

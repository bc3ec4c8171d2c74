"""The fused T-NeRF field's training pass (nfa_tnerf_train_fwd in nerfacc_amd/csrc/nerf_field.hip, nfa_tnerf_train_bwd in
nerfacc_amd/csrc/nerf_train.hip, TNeRFRadianceField(fused_training=True)) against the no-grad launch, the composed chain and
float64 autograd.

Largest (fused error) / (composed chain's error) against float64 seen on the device in test_gradients_against_float64: 1.446
(head.b2 of the cat-output network, 5.5e-3 against 3.8e-3); over the warp's tensors 1.021 (warp.b1, 1.46e-1 against 1.43e-1), over
the trunk's 1.022; the bound is 2.  DESIGN.md, "Fused T-NeRF field: training".
"""
import pytest
import torch

import mlp_stream_reference as M
import nerf_field_reference as F
import tnerf_field_reference as T
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import TNeRFRadianceField, VanillaNeRFRadianceField
from nerfacc_amd.mlp import reference_mlp
from test_nerf_field_gpu import CAT_OUT, FLAT, REF
from test_nerf_train_gpu import incoming, stream_forward
from test_tnerf_field_gpu import SMALL

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
# (network, N, ray samples?, dtype, weights, the NeRF networks' rolls, delta_1's column, the warp's (net_depth, skip_layer)).  N: 1; 33 (a
# partial tile and three idle waves); 129 (two passes); 300.  Warps: the reference's; one whose OUTPUT layer is the cat layer; one
# hidden layer.  Rolls and columns are chosen so that on the composed chain every layer of all three networks receives a gradient.
CASES = [
    (REF, 1, False, F16, "perm", (0, 0), "pos_sine", (4, 2)), (REF, 33, True, BF16, "perm", (11, 130), "time_sine", (2, 1)),
    (REF, 129, False, BF16, "xavier", None, None, (4, 2)), (REF, 300, True, F16, "perm", (0, 0), "pos_identity", (1, None)),
    (SMALL, 1, True, BF16, "perm", (0, 84), "pos_identity", (4, 2)), (FLAT, 33, False, F16, "perm", (0, 130), "time_identity", (4, 2)),
    (SMALL, 129, True, F16, "perm", (5, 140), "pos_identity", (2, 1)), (FLAT, 300, False, BF16, "xavier", None, None, (4, 2)),
    (CAT_OUT, 1, False, BF16, "perm", (0, 84), "pos_sine", (1, None)), (CAT_OUT, 33, True, F16, "xavier", None, None, (4, 2)),
    (CAT_OUT, 129, False, F16, "perm", (0, 125), "pos_identity", (4, 2)), (CAT_OUT, 300, True, BF16, "perm", (0, 85), "pos_sine", (2, 1)),
]
case_id = lambda c: f"W{c[0][0]}-D{c[0][1]}-N{c[1]}-{'rays' if c[2] else 'points'}-{'fp16' if c[3] == F16 else 'bf16'}-{c[4]}-warp{c[7][0]}"
NETS = (("warp", lambda f: f.warp), ("trunk", lambda f: f.nerf.mlp.trunk), ("head", lambda f: f.nerf.mlp.head))


def make_field(net, dtype, dev, kind, roll, column, warp_shape, fused_training):
    f = TNeRFRadianceField(dtype=dtype, fused_training=fused_training)
    f.warp = reference_mlp(36, 3, warp_shape[0], 64, warp_shape[1], dtype=dtype, out_dtype=F32)
    f.nerf = VanillaNeRFRadianceField(net[1], net[0], net[2], net[3], dtype=dtype)
    if kind == "perm":
        f.warp.load_linear_weights(*T.perm_weights(T.ROLL[column], warp_shape[0], F.S.skip_mask_of(warp_shape[1], warp_shape[0])))
        _, tw, tb, hw, hb = F.perm_weights(net[0], net[1], net[2], net[3], roll)
        f.nerf.mlp.trunk.load_linear_weights(tw, tb), f.nerf.mlp.head.load_linear_weights(hw, hb)
    else:
        f.warp.load_linear_weights(*T.xavier_weights())
        f.nerf.mlp.load_reference_state_dict(M.nerf_state_dict("xavier", F.POS_DIMS, F.DIR_DIMS, net[1], net[0], net[2], net[3], 128))
    return f.to(dev)


def param_grads(f):
    """Every parameter gradient of the three networks as named per-layer views, and the gradients cleared."""
    out = {}
    for name, get in NETS:
        mlp = get(f)
        g = mlp.params.grad
        for l, (w, b) in enumerate(zip(mlp._views(g), mlp._bias_views(g))):
            out[f"{name}.w{l}"], out[f"{name}.b{l}"] = w.clone(), b.clone()
        mlp.params.grad = None
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_bits_and_saved_buffers(dev, case):
    net, N, rays, dtype, kind, roll, column, warp_shape = case
    f = make_field(net, dtype, dev, kind, roll, column, warp_shape, True)
    t, h, w, W = f.nerf.mlp.trunk, f.nerf.mlp.head, f.warp, net[0]
    inp, x, tm, d = T.make_inputs(N, rays, dev)
    new = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=dev)
    with torch.no_grad():
        w_in = torch.cat([f.posi_encoder(x), f.time_encoder(tm)], -1)   # what the composed chain stores: computed once
        w_hidden = torch.empty(w.n_hidden_layers, N, 64, dtype=dtype, device=dev)
        delta = torch.empty(N, 3, device=dev)
        B.call("nfa_mlp_net_fwd", B.ELEM_CODES[dtype], w._desc, B.ptr(w_in), B.ELEM_CODES[dtype], B.ptr(w._images(w.params)[0]), w._bias_ptr(w.params),
               N, B.ptr(delta), 0, B.ptr(w_hidden), 1, B.stream())
        enc_x, enc_d = f.nerf.posi_encoder(x + delta), f.nerf.view_encoder(d)
        y, t_hidden = stream_forward(t, enc_x)
        h_in = torch.cat([y[:, :W], enc_d], 1)
        h_hidden = stream_forward(h, h_in)[1]
        for act in (False, True):
            for kw in ({}, dict(rgb_dtype=F32, sigma_dtype=F32)):
                saved = [new(N, 63), new(t.n_hidden_layers, N, W), new(N, W + 27), new(h.n_hidden_layers, N, 128), new(N, 36), new(w.n_hidden_layers, N, 64)]
                got, want = f._launch("full", N, act, **inp, **kw, save=saved, warped=True), f._launch("full", N, act, **inp, **kw, warped=True)
                assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(got[2], x + delta)
                assert [i for i, (a, b) in enumerate(zip(saved, (enc_x, t_hidden, h_in, None, w_in, w_hidden))) if b is not None and not torch.equal(a, b)] == []
                if kind == "perm":   # otherwise the head's first layer sums in another order
                    assert torch.equal(saved[3], h_hidden)


@pytest.mark.parametrize("g_f32", [True, False], ids=["g-float32", "g-half"])
@pytest.mark.parametrize("case", [c for c in CASES if c[4] == "perm"], ids=case_id)
def test_gradients_exact_on_the_perm_family(dev, case, g_f32):
    net, N, rays, dtype, kind, roll, column, warp_shape = case
    on, off = (make_field(net, dtype, dev, kind, roll, column, warp_shape, ft) for ft in (True, False))
    inp, x, tm, d = T.make_inputs(N, rays, dev)
    g_rgb, g_sigma = incoming(N, dev)
    rgb, sigma = off.query_raw(x, tm, d)
    ((rgb.float() * g_rgb).sum() + (sigma.float() * g_sigma).sum()).backward()
    want = param_grads(off)
    # the guard: the composed chain's gradients are non-zero in every layer, so that nothing is compared as 0 == 0
    assert [k for k, v in want.items() if not v.abs().max() > 0] == []
    kw = dict(rgb_dtype=F32, sigma_dtype=F32) if g_f32 else {}
    rgb, sigma = on._train(False, N, **inp, **kw)
    ((rgb.float() * g_rgb).sum() + (sigma.float() * g_sigma).sum()).backward()
    got = param_grads(on)
    assert [k for k in want if not torch.equal(got[k], want[k])] == []


def float64_gradients(f, x, tm, d, g_rgb, g_sigma, activated):
    """float64 autograd over a plain restatement of the whole field from the same master weights: encoders, warp, add, NeRF."""
    def enc(v, L):
        s = v[:, None, :] * (2.0 ** torch.arange(L, dtype=torch.float64, device=v.device))[None, :, None]
        return torch.cat([v, torch.sin(s).flatten(1), torch.cos(s).flatten(1)], 1)

    def mlp(m, name, x0, leaves):
        hid = x0
        for l, (w, b) in enumerate(zip(m.linear_weights(), m.linear_biases())):
            w, b = w.double().requires_grad_(), b.double().requires_grad_()
            leaves[f"{name}.w{l}"], leaves[f"{name}.b{l}"] = w, b
            z = (torch.cat([hid, x0], 1) if (m.skip_mask >> l) & 1 else hid) @ w.t() + b
            hid = torch.relu(z) if l < m.n_hidden_layers else z
        return hid

    leaves, W = {}, f.nerf.mlp.net_width
    xw = x.double() + mlp(f.warp, "warp", torch.cat([enc(x.double(), 4), enc(tm.double(), 4)], 1), leaves)
    y = mlp(f.nerf.mlp.trunk, "trunk", enc(xw, 10), leaves)
    rgb, sigma = mlp(f.nerf.mlp.head, "head", torch.cat([y[:, :W], enc(d.double(), 4)], 1), leaves), y[:, W]
    if activated:
        rgb, sigma = torch.sigmoid(rgb), torch.relu(sigma)
    ((rgb * g_rgb.double()).sum() + (sigma * g_sigma.double()).sum()).backward()
    return {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("activated", [False, True], ids=["raw", "activated"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("net", [REF, FLAT, CAT_OUT], ids=["ref", "flat", "cat_out"])
def test_gradients_against_float64(dev, net, dtype, activated):
    """Xavier weights, biases in +-0.5, N = 300.  Per parameter tensor: max |g - ref| / max |ref|; the fused path's is at most twice
    the composed chain's (the sibling test's bound and rationale: the same rounding points, another summation order in the head's
    first layer).  Worst ratios seen on the device: warp 1.021 (warp.b1), trunk 1.022 (trunk.b3), head 1.446 (head.b2).  Both paths'
    errors themselves are large for the warp and the trunk's first layers (1e-1 .. 8e-1): the gradient passes the trunk's 2^9 frequency
    as a half-type row."""
    N, rays = 300, (net is FLAT) != activated
    on, off = (make_field(net, dtype, dev, "xavier", None, None, (4, 2), ft) for ft in (True, False))
    inp, x, tm, d = T.make_inputs(N, rays, dev)
    g_rgb, g_sigma = incoming(N, dev)
    ref = float64_gradients(off, x, tm, d, g_rgb, g_sigma, activated)
    grads = []
    for f in (on, off):
        if rays:
            rgb, sigma = f.query_on_rays(*inp["rays"], inp["times"].view(-1, 1), raw=not activated)
        else:
            rgb, sigma = f(x, tm, d) if activated else f.query_raw(x, tm, d)
        ((rgb.float() * g_rgb).sum() + (sigma.float().view(-1) * g_sigma).sum()).backward()
        grads.append(param_grads(f))
    err = lambda g, k: float((g[k].double() - ref[k]).abs().max() / ref[k].abs().max())
    ratios = {k: (err(grads[0], k), err(grads[1], k)) for k in ref}
    for net_name in ("warp", "trunk", "head"):
        ks = [k for k in ratios if k.startswith(net_name)]
        worst = max(ks, key=lambda k: ratios[k][0] / max(ratios[k][1], 1e-300))
        print(f"worst fused / composed error ratio, {net_name}: {worst} {ratios[worst][0]:.3e} / {ratios[worst][1]:.3e} = "
              f"{ratios[worst][0] / max(ratios[worst][1], 1e-300):.3f}; largest fused error {max(ratios[k][0] for k in ks):.3e}")
    assert [(k, v) for k, v in ratios.items() if not v[0] <= 2.0 * v[1]] == []


def test_dispatch(dev, monkeypatch):
    def field(head_depth=1, **kw):
        f = TNeRFRadianceField(**kw)
        f.nerf = VanillaNeRFRadianceField(2, 128, None, head_depth)
        with torch.no_grad():   # the reference's initial deformation of 1e-4 would leave the warp's gradients near zero
            f.warp.weight(4).copy_(T.xavier_weights()[0][4])
        return f.to(dev)

    f, off = field(fused_training=True), field()
    off.load_state_dict(f.state_dict())
    gen = torch.Generator().manual_seed(5)
    x, d, t = torch.rand(200, 3, generator=gen).to(dev), torch.randn(200, 3, generator=gen).to(dev), torch.rand(200, 1, generator=gen).to(dev)
    names, call = [], B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), call(name, *a))[1])

    def grads(fld):
        rgb, sigma = fld(x, t, d)
        (rgb.float().sum() + sigma.float().sum()).backward()
        return param_grads(fld)

    first = grads(f)
    assert names.count("nfa_tnerf_train_fwd") == 1 and names.count("nfa_tnerf_train_bwd") == 1
    assert "nfa_mlp_stream_fwd" not in names and not [n for n in names if n.startswith("nfa_sinenc")]
    again = grads(f)
    assert all(torch.equal(first[k], again[k]) for k in first) and all(v.abs().max() > 0 for v in first.values())
    # every fallback takes the composed chain and gives its values
    frozen, sw = field(fused_training=True), field(fused={"full": False}, fused_training=True)
    frozen.load_state_dict(f.state_dict()), sw.load_state_dict(f.state_dict())
    frozen.warp.params.requires_grad_(False)
    deep, deep_off = field(5, fused_training=True), field(5)   # five hidden layers in the head: outside fused_supported(True)
    deep_off.load_state_dict(deep.state_dict())
    grid = lambda v: v.view(20, 10, -1)
    for fld, ref, args in [(f, off, (x.clone().requires_grad_(), t, d)), (f, off, (x, t.clone().requires_grad_(), d)),
                           (f, off, (grid(x), grid(t), d[:20])), (sw, off, (x, t, d)), (frozen, off, (x, t, d)), (deep, deep_off, (x, t, d))]:
        del names[:]
        got, want = fld(*args), ref(*[a.detach() for a in args])
        assert "nfa_tnerf_train_fwd" not in names and "nfa_mlp_stream_fwd" in names
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    del names[:]
    assert torch.equal(f.query_density(x, t), off.query_density(x, t)) and torch.equal(f.warped_positions(x, t), off.warped_positions(x, t))
    assert not [n for n in names if n.startswith("nfa_tnerf_train")]
    with pytest.raises(ValueError, match="a condition is required"):   # condition=None is the composed chain's to refuse
        f(x, t, None)
    # the second order
    rgb, sigma = f(x, t, d)
    g, = torch.autograd.grad(rgb.float().sum(), f.warp.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="TNeRFRadianceField"):
        g.sum().backward()
    f.zero_grad(set_to_none=True)
    rgb0, sigma0 = f(x[:0], t[:0], d[:0])
    assert rgb0.shape == (0, 3) and sigma0.shape == (0, 1)
    (rgb0.float().sum() + sigma0.float().sum()).backward()
    assert all(float(v.abs().max()) == 0 for v in param_grads(f).values())

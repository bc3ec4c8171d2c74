"""The fused T-NeRF field query (nerfacc_amd/csrc/nerf_field.hip, WARP) against the float64 restatement of tests/tnerf_field_reference.py
and the composed chain of the same module.  Largest error / bound seen on the device: DESIGN.md, "Fused T-NeRF field"."""
import pytest
import torch

import mlp_stream_reference as M
import nerf_field_reference as F
import tnerf_field_reference as T
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import TNeRFRadianceField, VanillaNeRFRadianceField
from nerfacc_amd.mlp import reference_mlp

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
REF, SMALL = (256, 8, 4, 1), (128, 2, None, 1)   # (net_width, net_depth, skip_layer, net_depth_condition) of the NeRF network
# (network, N, ray samples?, delta_1's column, the NeRF networks' rolls, the warp's (net_depth, skip_layer)).  N: 1; 33 (a partial tile,
# three idle waves); 129 (two passes); 300; a full sweep of the grid plus 71: every workgroup makes a second pass on the image it staged.
# The last two: a warp whose OUTPUT layer is the cat layer (2 hidden layers, mask 4), and one with a single hidden layer.
WARP = (4, 2)
EXACT_CASES = [
    (REF, 1, False, "pos_identity", (0, 125), WARP), (REF, 33, True, "pos_sine", (11, 130), WARP), (REF, 129, False, "time_identity", (20, 140), WARP),
    (REF, 300, True, "time_sine", (0, 0), WARP), (SMALL, 1, True, "time_sine", (35, 125), WARP), (SMALL, 33, False, "time_identity", (0, 130), WARP),
    (SMALL, 129, True, "pos_identity", (5, 140), WARP), (SMALL, 300, False, "pos_sine", (0, 0), WARP),
    (SMALL, 256 * 128 + 71, False, "time_sine", (0, 130), WARP), (SMALL, 33, True, "pos_sine", (0, 130), (2, 1)), (SMALL, 129, False, "time_identity", (5, 140), (1, None)),
]


def make_field(net, dtype, dev, warp, nerf_load, warp_shape=WARP):
    f = TNeRFRadianceField(dtype=dtype)
    f.warp = reference_mlp(36, 3, warp_shape[0], 64, warp_shape[1], dtype=dtype, out_dtype=torch.float32)
    f.nerf = VanillaNeRFRadianceField(net[1], net[0], net[2], net[3], dtype=dtype)
    f.warp.load_linear_weights(*warp)
    nerf_load(f.nerf.mlp)
    return f.to(dev)


density_inputs = lambda inp: {k: v for k, v in inp.items() if k != "dirs"}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: f"W{c[0][0]}-N{c[1]}-{'rays' if c[2] else 'points'}-{c[3]}-warp{c[5][0]}")
def test_bit_for_bit_on_the_perm_family(dev, case, dtype):
    net, N, rays, column, roll, warp_shape = case
    wmask = F.S.skip_mask_of(warp_shape[1], warp_shape[0])
    ww, wb = T.perm_weights(T.ROLL[column], warp_shape[0], wmask)
    mask, tw, tb, hw, hb = F.perm_weights(net[0], net[1], net[2], net[3], roll)
    f = make_field(net, dtype, dev, (ww, wb), lambda m: (m.trunk.load_linear_weights(tw, tb), m.head.load_linear_weights(hw, hb)), warp_shape)
    inp, x, t, d = T.make_inputs(N, rays, dev)
    f32 = torch.float32
    with torch.no_grad():
        row = torch.cat([f.posi_encoder(x), f.time_encoder(t)], -1)
        delta = T.warp(row.cpu(), None, ww, wb, dtype, exact=True, mask=wmask)["delta"]
        want_xw = T.warped(x.cpu(), delta, torch.zeros_like(delta))[0]
        comp_xw = x + f.warp(row)
        rgb32, sig32, xw = f._launch("full", N, False, **inp, warped=True, rgb_dtype=f32, sigma_dtype=f32)
        rgbh, sigh, _ = f._launch("full", N, False, **inp)
        _, sigd, xwd = f._launch("density", N, False, **density_inputs(inp), warped=True, sigma_dtype=f32)
        xww = f._launch("warp", N, **density_inputs(inp))[2]
        enc_x, enc_d = f.nerf.posi_encoder(comp_xw), f.nerf.view_encoder(d)
        ref = F.query(enc_x.cpu(), enc_d.cpu(), tw, tb, hw, hb, mask, dtype, exact=True)
        comp_rgb, comp_sig = f.nerf.mlp(enc_x, enc_d)
    assert float(delta.abs().max()) > 0 and f.fused_supported() and torch.equal(comp_xw.cpu(), want_xw)
    assert torch.equal(xw, comp_xw) and torch.equal(xwd, xw) and torch.equal(xww, xw)
    assert torch.equal(sig32.cpu().double(), ref["sigma"]) and torch.equal(sigd, sig32) and torch.equal(rgb32.cpu().double(), ref["rgb"])
    assert torch.equal(sigh, comp_sig.view(-1)) and torch.equal(rgbh, comp_rgb)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rays", [False, True], ids=["points", "rays"])
@pytest.mark.parametrize("net", [REF, SMALL], ids=["ref", "small"])
def test_real_valued_within_the_reference_bound(dev, net, rays, dtype):
    """Xavier weights, biases in +-0.5, N = 300: `warped` and the half-type sigma are the composed chain's bits, the deformation is
    within the warp's own float64 bound (no incoming error), the colour within the HEAD's own bound (tests/test_nerf_field_gpu.py)."""
    N = 300
    ww, wb = T.xavier_weights()
    sd = M.nerf_state_dict("xavier", F.POS_DIMS, F.DIR_DIMS, net[1], net[0], net[2], net[3], 128)
    f = make_field(net, dtype, dev, (ww, wb), lambda m: m.load_reference_state_dict(sd))
    cpu = lambda ts: [v.cpu() for v in ts]
    tr, hd = f.nerf.mlp.trunk, f.nerf.mlp.head
    inp, x, t, d = T.make_inputs(N, rays, dev)
    with torch.no_grad():
        row = torch.cat([f.posi_encoder(x), f.time_encoder(t)], -1)
        w = T.warp(row.cpu(), torch.zeros(N, T.WARP_DIMS, dtype=torch.float64), ww, wb, dtype)
        want_xw, e_xw = T.warped(x.cpu(), w["delta"], w["e_delta"])
        comp_xw = x + f.warp(row)
        rgb32, _, xw = f._launch("full", N, False, **inp, warped=True, rgb_dtype=torch.float32)
        rgbh, sigh, _ = f._launch("full", N, False, **inp)
        sigd = f._launch("density", N, False, **density_inputs(inp))[1]
        enc_x, enc_d = f.nerf.posi_encoder(comp_xw), f.nerf.view_encoder(d)
        comp_rgb, comp_sig = f.nerf.mlp(enc_x, enc_d)
        head = F.head(tr(enc_x)[:, :net[0]].cpu(), enc_d.cpu(), cpu(hd.linear_weights()), cpu(hd.linear_biases()), dtype)
    r_xw, r_head = T.worst_ratio(xw.cpu(), want_xw.double(), e_xw), T.worst_ratio(rgb32.cpu(), head["rgb"], head["e_rgb"])
    print(f"deformation up to {float(w['delta'].abs().max()):.2f}: worst err / bound {r_xw:.2e} (<= {float(e_xw.max()):.1e}); colour / head's bound {r_head:.3f}")
    assert torch.equal(xw, comp_xw) and torch.equal(sigh, comp_sig.view(-1)) and torch.equal(sigd, sigh)
    assert r_xw <= 1.0 and r_head <= 1.0
    assert T.worst_ratio(rgbh.cpu(), *F.rounded(head["rgb"], head["e_rgb"], dtype)) <= 1.0


def test_module_dispatch(dev, monkeypatch):
    """One native call per no-grad query; with grad the composed chain, which trains the warp too; the same bits again; N = 0."""
    f = TNeRFRadianceField()
    f.nerf = VanillaNeRFRadianceField(2, 128, None, 1)
    with torch.no_grad():   # the reference's initial deformation of 1e-4 would leave the warp's gradients near zero
        f.warp.weight(4).copy_(T.xavier_weights()[0][4])
    f = f.to(dev)
    gen = torch.Generator().manual_seed(5)
    x, d, t = torch.rand(200, 3, generator=gen).to(dev), torch.randn(200, 3, generator=gen).to(dev), torch.rand(200, 1, generator=gen).to(dev)
    o, ts, ri = torch.zeros(1, 3, device=dev), torch.rand(200, generator=gen).to(dev), torch.zeros(200, dtype=torch.int64, device=dev)
    with torch.no_grad():
        first = (*f(x, t, d), f.warped_positions(x, t))
        f.query_density(x[:77], t[:77])
        again = (*f(x, t, d), f.warped_positions(x, t))
        names, call = [], B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
        queries = [lambda: f(x, t, d), lambda: f.query_raw(x, t, d), lambda: f.query_density(x, t), lambda: f.query_opacity(x, t[:5], 0.01),
                   lambda: f.density_on_rays(o, d[:1], ts, ts + 0.01, ri, t[:1]), lambda: f.query_on_rays(o, d[:1], ts, ts + 0.01, ri, t[:1]),
                   lambda: f.query_on_rays(o, d[:1], ts, ts + 0.01, ri, t[:1], raw=False), lambda: f.warped_positions(x, t)]
        for q in queries:
            del names[:]
            q()
            assert names in (["nfa_tnerf_field"], ["nfa_tnerf_density"], ["nfa_tnerf_warp"]), names
        rgb0, sigma0 = f(x[:0], t[:0], d[:0])
        assert rgb0.shape == (0, 3) and sigma0.shape == (0, 1) and f.query_density(x[:0], t[:0]).shape == (0, 1)
        assert f.query_on_rays(o, d[:1], ts[:0], ts[:0], ri[:0], t[:1])[0].shape == (0, 3) and f.warped_positions(x[:0], t[:0]).shape == (0, 3)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    del names[:]
    rgb, sigma = f(x, t, d)   # parameters require grad: the composed chain
    assert not [n for n in names if n.startswith("nfa_tnerf")] and "nfa_mlp_net_fwd" in names and "nfa_mlp_stream_fwd" in names
    (rgb.float().sum() + sigma.float().sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in f.parameters())
    tol = 0.02   # as tests/test_nerf_field_gpu.py: the composed chain's outputs are the half type and the head sums in another order
    assert torch.allclose(rgb.detach().float(), first[0].float(), atol=tol) and torch.allclose(sigma.detach().float(), first[1].float(), atol=tol, rtol=tol)

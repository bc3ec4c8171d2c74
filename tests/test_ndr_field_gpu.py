"""The fused NDR T-NeRF field query (nerfacc_amd/csrc/ndr_warp.h, nerf_field.hip WARP == 2) against tests/ndr_field_reference.py's
float64 restatement and the composed chain of the same module.  Largest error / bound seen: DESIGN.md, "Fused NDR field"."""
import pytest
import torch

import mlp_stream_reference as M
import ndr_field_reference as R
import nerf_field_reference as F
import tnerf_field_reference as T
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import NDRTNeRFRadianceField, VanillaNeRFRadianceField

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
REF, SMALL = (256, 8, 4, 1), (128, 2, None, 1)   # (net_width, net_depth, skip_layer, net_depth_condition) of the NeRF network
# (network, N, ray samples?, the NeRF networks' rolls).  N: 1; 33 (a partial tile, three waves with clamped loads that still take
# every barrier); 129 (two passes); 300; a full sweep of the grid plus 71: every workgroup makes a second pass on its ring.
EXACT_CASES = [
    (REF, 1, False, (0, 125)), (REF, 33, True, (11, 130)), (REF, 129, False, (20, 140)), (REF, 300, True, (0, 0)),
    (SMALL, 1, True, (35, 125)), (SMALL, 33, False, (0, 130)), (SMALL, 129, True, (5, 140)), (SMALL, 300, False, (0, 0)),
    (SMALL, 256 * 128 + 71, False, (0, 130)),
]


def make_field(net, dtype, dev, blocks, nerf_load):
    f = NDRTNeRFRadianceField(dtype=dtype)
    f.nerf = VanillaNeRFRadianceField(net[1], net[0], net[2], net[3], dtype=dtype)
    nerf_load(f.nerf.mlp)
    return R.load(f, blocks).to(dev)


density_inputs = lambda inp: {k: v for k, v in inp.items() if k != "dirs"}
encoders = lambda f, dev: (lambda v: f.posi_encoder_1(v.to(dev)), lambda v: f.posi_encoder_2(v.to(dev)))


def launches(f, N, inp, f32=torch.float32):   # all three entries: float32 and half-type outputs, warped from each
    rgb32, sig32, xw = f._launch("full", N, False, **inp, warped=True, rgb_dtype=f32, sigma_dtype=f32)
    rgbh, sigh, _ = f._launch("full", N, False, **inp)
    _, sigd, xwd = f._launch("density", N, False, **density_inputs(inp), warped=True, sigma_dtype=f32)
    xww = f._launch("warp", N, **density_inputs(inp))[2]
    return rgb32, sig32, xw, rgbh, sigh, sigd, xwd, xww


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: f"W{c[0][0]}-N{c[1]}-{'rays' if c[2] else 'points'}")
def test_bit_for_bit_on_the_perm_family(dev, case, dtype):
    net, N, rays, roll = case
    blocks = R.perm_weights()
    mask, tw, tb, hw, hb = F.perm_weights(net[0], net[1], net[2], net[3], roll)
    f = make_field(net, dtype, dev, blocks, lambda m: (m.trunk.load_linear_weights(tw, tb), m.head.load_linear_weights(hw, hb)))
    inp, x, t, d = T.make_inputs(N, rays, dev)
    with torch.no_grad():
        want = R.warp(x.cpu(), f.time_encoder(t).cpu(), blocks, dtype, encoders(f, dev), exact=True)
        f.fused = dict(density=False, full=False)
        comp_xw = f.warp(x, t)
        rgb32, sig32, xw, rgbh, sigh, sigd, xwd, xww = launches(f, N, inp)
        enc_x, enc_d = f.nerf.posi_encoder(xw), f.nerf.view_encoder(d)
        ref = F.query(enc_x.cpu(), enc_d.cpu(), tw, tb, hw, hb, mask, dtype, exact=True)
    assert want["dw"] > 0 and want["tr"] > 0 and want["theta"] == 0 and f.fused_supported()
    assert torch.equal(xw.cpu().double(), want["warped"]) and torch.equal(xw, comp_xw) and torch.equal(xwd, xw) and torch.equal(xww, xw)
    assert torch.equal(sig32.cpu().double(), ref["sigma"]) and torch.equal(sigd, sig32) and torch.equal(rgb32.cpu().double(), ref["rgb"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rays", [False, True], ids=["points", "rays"])
@pytest.mark.parametrize("net", [REF, SMALL], ids=["ref", "small"])
@pytest.mark.parametrize("family", ["xavier", "rot"])
def test_real_valued_within_the_reference_bound(dev, family, net, rays, dtype):
    """N = 300: `warped` is the composed chain's bits and within the warp's own float64 bound, sigma the composed NeRF's bits at the
    launch's own `warped`, the colour within the HEAD's bound.  `xavier` (biases in +-0.5): the bound on `warped` is loose, the bit
    equality is the statement.  `rot`: one-term sums, theta != 0, a bias on every layer; its bound is a few roundings (asserted)."""
    N = 300
    blocks = R.xavier_weights() if family == "xavier" else R.perm_weights(rot=True)
    sd = M.nerf_state_dict("xavier", F.POS_DIMS, F.DIR_DIMS, net[1], net[0], net[2], net[3], 128)
    f = make_field(net, dtype, dev, blocks, lambda m: m.load_reference_state_dict(sd))
    cpu = lambda ts: [v.cpu() for v in ts]
    tr, hd = f.nerf.mlp.trunk, f.nerf.mlp.head
    inp, x, t, d = T.make_inputs(N, rays, dev)
    with torch.no_grad():
        want = R.warp(x.cpu(), f.time_encoder(t).cpu(), blocks, dtype, encoders(f, dev))
        rgb32, _, xw, rgbh, sigh, _, xwd, xww = launches(f, N, inp)
        sigd = f._launch("density", N, False, **density_inputs(inp))[1]
        f.fused = dict(density=False, full=False)
        comp_xw = f.warp(x, t)
        enc_x, enc_d = f.nerf.posi_encoder(xw), f.nerf.view_encoder(d)
        comp_rgb, comp_sig = f.nerf.mlp(enc_x, enc_d)
        head = F.head(tr(enc_x)[:, :net[0]].cpu(), enc_d.cpu(), cpu(hd.linear_weights()), cpu(hd.linear_biases()), dtype)
    r_xw, r_head = R.worst_ratio(xw.cpu(), want["warped"], want["e_warped"]), R.worst_ratio(rgb32.cpu(), head["rgb"], head["e_rgb"])
    print(f"dw up to {want['dw']:.2f}, translation {want['tr']:.2f}, theta {want['theta']:.2f}: warped worst err / bound {r_xw:.2e} "
          f"(<= {float(want['e_warped'].max()):.1e}); colour / head's bound {r_head:.3f}")
    assert want["dw"] > 0.01 and want["tr"] > 0.01 and want["theta"] > 0.01
    sharp = float((want["e_warped"] < 0.1 * (want["warped"] - x.cpu().double()).abs()).double().mean())
    assert family == "xavier" or sharp >= 1 / 3, sharp
    assert torch.equal(xw, comp_xw) and torch.equal(xwd, xw) and torch.equal(xww, xw)
    assert torch.equal(sigh, comp_sig.view(-1)) and torch.equal(sigd, sigh)
    assert r_xw <= 1.0 and r_head <= 1.0
    assert R.worst_ratio(rgbh.cpu(), *F.rounded(head["rgb"], head["e_rgb"], dtype)) <= 1.0


def test_module_dispatch(dev, monkeypatch):
    """One native call per no-grad query; with grad the composed chain, which trains every parameter; the same bits again; N = 0."""
    f = NDRTNeRFRadianceField()
    f.nerf = VanillaNeRFRadianceField(2, 128, None, 1)
    R.load(f, R.xavier_weights())   # the reference's initial outputs of 1e-4 would leave the warp's gradients near zero
    f = f.to(dev)
    gen = torch.Generator().manual_seed(5)
    x, d, t = torch.rand(200, 3, generator=gen).to(dev), torch.randn(200, 3, generator=gen).to(dev), torch.rand(200, 1, generator=gen).to(dev)
    o, ts, ri = torch.zeros(1, 3, device=dev), torch.rand(200, generator=gen).to(dev), torch.zeros(200, dtype=torch.int64, device=dev)
    with torch.no_grad():
        first = (*f(x, t, d), f.warp(x, t))
        names, call = [], B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
        queries = [lambda: f(x, t, d), lambda: f.query_raw(x, t, d), lambda: f.query_density(x, t), lambda: f.query_opacity(x, t[:5], 0.01),
                   lambda: f.density_on_rays(o, d[:1], ts, ts + 0.01, ri, t[:1]), lambda: f.query_on_rays(o, d[:1], ts, ts + 0.01, ri, t[:1]),
                   lambda: f.query_on_rays(o, d[:1], ts, ts + 0.01, ri, t[:1], raw=False), lambda: f.warp(x, t)]
        for q in queries:
            del names[:]
            q()
            assert names in (["nfa_ndr_field"], ["nfa_ndr_density"], ["nfa_ndr_warp"]), names
        rgb0, sigma0 = f(x[:0], t[:0], d[:0])
        assert rgb0.shape == (0, 3) and sigma0.shape == (0, 1) and f.query_density(x[:0], t[:0]).shape == (0, 1)
        assert f.query_on_rays(o, d[:1], ts[:0], ts[:0], ri[:0], t[:1])[0].shape == (0, 3) and f.warp(x[:0], t[:0]).shape == (0, 3)
        assert all(torch.equal(a, b) for a, b in zip(first, (*f(x, t, d), f.warp(x, t))))
    del names[:]
    rgb, sigma = f(x, t, d)   # parameters require grad: the composed chain
    assert not [n for n in names if n.startswith("nfa_ndr") and n != "nfa_ndr_time_features"] and "nfa_ndr_time_features" in names
    (rgb.float().sum() + sigma.float().sum()).backward()
    assert len(list(f.parameters())) == 6 + 12 + 2
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in f.parameters())
    tol = 0.02   # as tests/test_tnerf_field_gpu.py between the two paths
    assert torch.allclose(rgb.detach().float(), first[0].float(), atol=tol) and torch.allclose(sigma.detach().float(), first[1].float(), atol=tol, rtol=tol)

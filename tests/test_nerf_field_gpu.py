"""The fused NeRF field query (nerfacc_amd/csrc/nerf_field.hip) against the float64 restatement of tests/nerf_field_reference.py
and against the composed chain of the same module.

Largest error / bound seen on the device: see DESIGN.md, "Fused NeRF field".
"""
import pytest
import torch

import mlp_stream_reference as M
import nerf_field_reference as F
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import VanillaNeRFRadianceField
from nerfacc_amd.samples import sample_positions

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# (net_width, net_depth, skip_layer, net_depth_condition)
REF, FLAT, CAT_OUT = (256, 8, 4, 1), (256, 2, None, 1), (128, 3, 2, 2)   # the reference's; no skip; a cat OUTPUT layer, head 128 x 2
# (network, N, ray samples?, roll).  N: 1; 33 (a partial tile and three idle waves); 129 (two passes); 300.  The rolls route
# sigma to an identity (REF 11, FLAT 35, CAT_OUT 33), a sine (REF 20, FLAT 0, CAT_OUT 0) and a cosine (REF 0, FLAT 5, CAT_OUT 3)
# column of the position and one colour channel to an identity (125; 84), a sine (130; 85) and a cosine (140; 84, 85) column of
# the direction; the other channels come through the bottleneck from sine and cosine columns of the position.
EXACT_CASES = [
    (REF, 1, False, (0, 125)), (REF, 33, True, (11, 130)), (REF, 129, False, (20, 140)), (REF, 300, True, (0, 0)),
    (FLAT, 1, True, (35, 125)), (FLAT, 33, False, (0, 130)), (FLAT, 129, True, (5, 140)), (FLAT, 300, False, (0, 0)),
    (CAT_OUT, 1, False, (33, 84)), (CAT_OUT, 33, True, (0, 85)), (CAT_OUT, 129, False, (3, 84)), (CAT_OUT, 300, True, (0, 85)),
    # a full sweep of the persistent grid and a last pass of 71 points: a tile of 7 in a workgroup whose last wave has nothing
    (FLAT, 256 * 128 + 71, False, (0, 130)),
]


def make_field(net, dtype, dev, load):
    f = VanillaNeRFRadianceField(net[1], net[0], net[2], net[3], dtype=dtype)
    load(f)
    return f.to(dev)


def make_inputs(N, rays, dev):
    """The launch's inputs and the (positions, directions) they mean.  Ray samples: seven rays with per-ray directions, ray 2
    without a sample; positions in and around the unit box."""
    gen = torch.Generator().manual_seed(7 + N)
    if not rays:
        x = (torch.rand(N, 3, generator=gen) * 3.0 - 1.5).to(dev)
        d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(dev)
        return dict(positions=x, dirs=d), x, d
    o = (torch.rand(7, 3, generator=gen) - 0.5).to(dev)
    d = torch.nn.functional.normalize(torch.randn(7, 3, generator=gen), dim=-1).to(dev)
    ri = torch.sort(torch.tensor([0, 1, 3, 4, 5, 6])[torch.randint(0, 6, (N,), generator=gen)]).values.to(dev)
    ts = (torch.rand(N, generator=gen) * 2.0).to(dev)
    te = ts + 0.01
    s = sample_positions(o, d, ts, te, ri, dirs="raw")
    return dict(rays=(o, d, ts, te, ri)), s.positions, s.dirs


def density_inputs(inp):
    return dict(rays=inp["rays"]) if "rays" in inp else dict(positions=inp["positions"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: f"W{c[0][0]}-D{c[0][1]}-N{c[1]}-{'rays' if c[2] else 'points'}-roll{c[3][0]}.{c[3][1]}")
def test_bit_for_bit_on_the_perm_family(dev, case, dtype):
    net, N, rays, roll = case
    mask, tw, tb, hw, hb = F.perm_weights(net[0], net[1], net[2], net[3], roll)
    f = make_field(net, dtype, dev, lambda f: (f.mlp.trunk.load_linear_weights(tw, tb), f.mlp.head.load_linear_weights(hw, hb)))
    inp, x, d = make_inputs(N, rays, dev)
    f32 = torch.float32
    with torch.no_grad():
        enc_x, enc_d = f.posi_encoder(x), f.view_encoder(d)
        ref = F.query(enc_x.cpu(), enc_d.cpu(), tw, tb, hw, hb, mask, dtype, exact=True)
        rgb32, sig32 = f._launch(True, N, False, **inp, rgb_dtype=f32, sigma_dtype=f32)
        rgbh, sigh = f._launch(True, N, False, **inp)
        _, sigd = f._launch(False, N, False, **density_inputs(inp), sigma_dtype=f32)
        _, relu = f._launch(False, N, True, **density_inputs(inp))
        comp_rgb, comp_sig = f.mlp(enc_x, enc_d)
        act32, acth = f._launch(True, N, True, **inp, rgb_dtype=f32)[0], f._launch(True, N, True, **inp)[0]
    # the activated colour: the sigmoid in float32 of a raw value that is its own rounding, then rounded once
    a_w, a_e = F.activated(ref["rgb"], torch.zeros_like(ref["rgb"]), dtype, True, exact=True)
    assert F.worst_ratio(act32.cpu(), a_w, a_e) <= 1.0 and F.worst_ratio(acth.cpu(), *F.rounded(a_w, a_e, dtype)) <= 1.0
    assert torch.equal(sig32.cpu().double(), ref["sigma"]) and torch.equal(sigd, sig32)
    assert torch.equal(rgb32.cpu().double(), ref["rgb"])
    assert torch.equal(sigh, comp_sig.view(-1)) and torch.equal(rgbh, comp_rgb)
    assert torch.equal(sigh.cpu().double(), ref["sigma"]) and torch.equal(rgbh.cpu().double(), ref["rgb"])
    assert torch.equal(relu, torch.relu(sigh))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rays", [False, True], ids=["points", "rays"])
@pytest.mark.parametrize("net", [REF, FLAT, CAT_OUT], ids=["ref", "flat", "cat_out"])
def test_real_valued_within_the_reference_bound(dev, net, rays, dtype):
    """Xavier weights, biases in +-0.5, N = 300.  Raw and activated outputs, as float32 and as the half type, through both
    entries, against two bounds.  'whole': the restatement of the whole query with the encoded rows' rounding carried in; that
    bound is the worst case of up to 8 + 2 layers and far above the outputs (DESIGN.md has its size), so it says little.  The
    sharp ones: sigma in the half type is the composed chain's bits (the trunk sums in its order), and the colour is within the
    HEAD's own bound ('head': the float64 head on the native trunk's bottleneck, a few ulps of the half type), which a wrong
    head bias, k-step, multi-term sum or sigmoid misses by orders of magnitude."""
    N, f32 = 300, torch.float32
    sd = M.nerf_state_dict("xavier", F.POS_DIMS, F.DIR_DIMS, net[1], net[0], net[2], net[3], 128)
    f = make_field(net, dtype, dev, lambda f: f.mlp.load_reference_state_dict(sd))
    cpu = lambda ts: [t.cpu() for t in ts]
    t, h = f.mlp.trunk, f.mlp.head
    inp, x, d = make_inputs(N, rays, dev)
    with torch.no_grad():
        enc_x, enc_d = f.posi_encoder(x), f.view_encoder(d)
        ref = F.query(enc_x.cpu(), enc_d.cpu(), cpu(t.linear_weights()), cpu(t.linear_biases()), cpu(h.linear_weights()),
                      cpu(h.linear_biases()), t.skip_mask, dtype)
        ref["head_rgb"], ref["e_head_rgb"] = F.head(t(enc_x)[:, :net[0]].cpu(), enc_d.cpu(), cpu(h.linear_weights()), cpu(h.linear_biases()),
                                                    dtype).values()
        want = {}   # (activated, half outputs) -> ((rgb, e_rgb), (sigma, e_sigma), (rgb, e_rgb) of the head alone)
        for act in (False, True):
            for half in (False, True):
                triple = []
                for key, colour in (("rgb", True), ("sigma", False), ("head_rgb", True)):
                    v, e = F.activated(ref[key], ref["e_" + key], dtype, colour) if act else (ref[key], ref["e_" + key])
                    triple.append(F.rounded(v, e, dtype) if half else (v, e))
                want[act, half] = triple
        for (act, half), ((rgb_w, rgb_e), (sig_w, sig_e), (head_w, head_e)) in want.items():
            kw = {} if half else dict(rgb_dtype=f32, sigma_dtype=f32)
            rgb, sigma = f._launch(True, N, act, **inp, **kw)
            dens = f._launch(False, N, act, **density_inputs(inp), **({} if half else dict(sigma_dtype=f32)))[1]
            r_rgb, r_sig = F.worst_ratio(rgb.cpu(), rgb_w, rgb_e), F.worst_ratio(sigma.cpu(), sig_w, sig_e)
            r_head = F.worst_ratio(rgb.cpu(), head_w, head_e)
            print(f"activated {act}, half {half}: worst err / bound whole: rgb {r_rgb:.2e} (bound <= {float(rgb_e.max()):.1e}), sigma {r_sig:.2e} "
                  f"(bound <= {float(sig_e.max()):.1e}); head: rgb {r_head:.3f} (bound <= {float(head_e.max()):.1e})")
            assert r_rgb <= 1.0 and r_sig <= 1.0 and r_head <= 1.0
            assert torch.equal(dens, sigma)
        rgb, sigma = f._launch(True, N, False, **inp)
        comp_rgb, comp_sig = f.mlp(enc_x, enc_d)
        assert torch.equal(sigma, comp_sig.view(-1))
        ulps = (rgb.double() - comp_rgb.double()).abs() / F.ulp(dtype, comp_rgb.double())
        print(f"raw colour against the composed chain: at most {float(ulps.max()):.1f} ulps of the half type, {int((ulps > 0).sum())} of {3 * N} differ")


def test_module_dispatch(dev, monkeypatch):
    """One native call per no-grad query; with grad the composed chain, which trains; bit for bit across runs and after another
    N in between; N = 0."""
    f = VanillaNeRFRadianceField(2, 128, None, 1).to(dev)
    gen = torch.Generator().manual_seed(5)
    x, d = torch.rand(200, 3, generator=gen).to(dev), torch.randn(200, 3, generator=gen).to(dev)
    o, ts, ri = torch.zeros(1, 3, device=dev), torch.rand(200, generator=gen).to(dev), torch.zeros(200, dtype=torch.int64, device=dev)
    with torch.no_grad():
        first = f(x, d)
        f.query_density(x[:77])   # packs nothing new; another N in between
        again = f(x, d)
        names, call = [], B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
        queries = [lambda: f(x, d), lambda: f.query_raw(x, d), lambda: f.query_density(x), lambda: f.query_opacity(x, 0.01),
                   lambda: f.density_on_rays(o, d[:1], ts, ts + 0.01, ri), lambda: f.query_on_rays(o, d[:1], ts, ts + 0.01, ri)]
        for q in queries:
            del names[:]
            q()
            assert names in (["nfa_nerf_field"], ["nfa_nerf_density"]), names
        rgb0, sigma0 = f(x[:0], d[:0])
        assert rgb0.shape == (0, 3) and sigma0.shape == (0, 1) and f.query_density(x[:0]).shape == (0, 1)
        assert f.query_on_rays(o, d[:1], ts[:0], ts[:0], ri[:0])[0].shape == (0, 3)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    del names[:]
    rgb, sigma = f(x, d)   # parameters require grad: the composed chain
    assert "nfa_nerf_field" not in names and "nfa_mlp_stream_fwd" in names
    (rgb.float().sum() + sigma.float().sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in f.parameters())
    tol = 0.02   # the composed chain's outputs are the half type (1 ulp of fp16 at 1 is 2^-10) and the head sums in another order
    assert torch.allclose(rgb.detach().float(), first[0].float(), atol=tol) and torch.allclose(sigma.detach().float(), first[1].float(), atol=tol, rtol=tol)

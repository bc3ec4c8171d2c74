"""GPU: the fused Instant-NGP field query of csrc/ngp_field.hip (nerfacc_amd/fields.py) against the float64 restatement of
tests/ngp_field_reference.py, bit for bit on integer-valued data, against the composed chain of the same module, and its
selector, contraction, activation and ray-sample input form.

The radiance grid is 16 levels from 4 to 64 with ``log2_hashmap_size = 10``, the smallest table HashGridEncoding accepts
(levels up to resolution 10 are dense, the finer ones hashed); the density grid has 5 levels, so its second k-step is zero
columns and its first k-step has one level on lane half 1.
"""
import copy
import functools

import pytest
import torch

import mlp_reference as R
import ngp_field_reference as NR
from nerfacc_amd.fields import NGPDensityField, NGPRadianceField
from nerfacc_amd.samples import sample_positions

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
N_MAX = 257
FIELDS = [("radiance", 15), ("radiance", 7), ("density", 0)]


def make_field(kind, G, dtype, **kw):
    gen = torch.Generator().manual_seed(11 + G)
    if kind == "radiance":
        f = NGPRadianceField(AABB, geo_feat_dim=G, n_levels=16, log2_hashmap_size=10, base_resolution=4, max_resolution=64, dtype=dtype, **kw)
    else:
        f = NGPDensityField(AABB, n_levels=5, log2_hashmap_size=10, base_resolution=4, max_resolution=64, dtype=dtype, **kw)
    with torch.no_grad():
        f.encoding.params.copy_(torch.rand(f.encoding.params.shape, generator=gen) * 2 - 1)
    return f


@functools.lru_cache(maxsize=None)
def case(kind, G, dtype):
    """(field on the GPU, positions, directions, reference of all N_MAX points): computed once, rows are independent."""
    f = make_field(kind, G, dtype)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(N_MAX, 3, generator=gen) * 1.96 - 0.98
    d = torch.nn.functional.normalize(torch.randn(N_MAX, 3, generator=gen), dim=-1)
    ref = NR.query(f, x, d if kind == "radiance" else None)
    return copy.deepcopy(f).to("cuda:0"), x.to("cuda:0"), d.to("cuda:0"), ref


def launch_guarded(f, full, want, N, x, d):
    """The fused launch into rows 1 .. N of buffers of N + 2 rows; the guard rows must stay as they were."""
    width = {"sigma": 1, "density": 1, "rgb": 3, "rgb_act": 3, "feat": f.geo_feat_dim}
    bufs = {k: torch.full((N + 2, width[k]), 7.0, device=x.device, dtype=f.dtype if k == "feat" else torch.float32) for k in want}
    f._launch(full, N, (N,), want, positions=x[:N].contiguous(), dirs=d[:N].contiguous(), outputs={k: b[1:N + 1] for k, b in bufs.items()})
    for k, b in bufs.items():
        assert bool((b[0] == 7).all()) and bool((b[-1] == 7).all()), f"{k}: a guard row was written"
    return {k: b[1:N + 1] for k, b in bufs.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("kind,G", FIELDS)
def test_fused_matches_the_float64_reference(dev, kind, G, N, dtype):
    f, x, d, ref = case(kind, G, dtype)
    full = kind == "radiance"
    with torch.no_grad():
        out = launch_guarded(f, full, ["sigma", "rgb"] if full else ["sigma"], N, x, d)
    r = R.worst_ratio(out["sigma"][:, 0].cpu(), ref["sigma"][:N], ref["e_sigma"][:N])
    print(f"raw sigma: worst err / bound {r:.3f}")
    assert r <= 1.0
    if full:
        r = R.worst_ratio(out["rgb"].cpu(), ref["rgb"][:N], ref["e_rgb"][:N])
        print(f"raw rgb: worst err / bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [15, 7])
@pytest.mark.parametrize("part", ["geo", "sh"])
def test_bit_for_bit_on_integer_valued_data(dev, part, G, dtype):
    """Scales 4 * 2^l - 1 put x = 0.5 + k on a node of EVERY level, so each encoded value is one table entry; tables and
    weights hold small integers.  The head reads one input column per neuron with both signs, then a permutation, then signed
    sums: 'geo' reads the geometry feature alone (integers), 'sh' the harmonics alone, at directions (components in
    {-1, -0.5, 0, 0.5, 1}) whose harmonics take one rounding whatever the association.  A wrong k position reads another column."""
    f = NGPRadianceField([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], geo_feat_dim=G, n_levels=16, log2_hashmap_size=10, base_resolution=4,
                         max_resolution=4 * 2 ** 15, dtype=dtype)
    assert f.encoding.scales == [float(4 * 2 ** l - 1) for l in range(16)]
    o = torch.arange(64)
    w0, w1, w2 = torch.zeros(64, 16 + G), torch.zeros(64, 64), torch.zeros(3, 64)
    w0[o, o % 16 if part == "sh" else 16 + o % G] = 1.0 - 2.0 * ((o // 16) % 2)   # every input column, with both signs
    w1[o, (5 * o + 3) % 64] = 1.0                                                 # a permutation
    w2[o % 3, o] = 1.0 - 2.0 * ((o // 3) % 2)                                     # 21 or 22 terms a row: the float32 sums stay exact
    b0, b1, r = torch.zeros(64, 32), torch.zeros(1 + G, 64), torch.arange(1 + G)
    b0[o, o % 32] = 1.0 - 2.0 * (o // 32)                                         # relu(f) and relu(-f) of every encoded value f
    b1[r, r], b1[r, r + 32], b1[r, r + 16], b1[r, r + 48] = 1.0, -1.0, 2.0, -2.0  # row r of the base output = f_r + 2 f_{r+16}
    with torch.no_grad():
        f.encoding.params.copy_(((torch.arange(f.encoding.params.numel()) * 7 + 3) % 13 - 6).float())
        f.mlp_base.load_linear_weights([b0, b1])
        f.mlp_head.load_linear_weights([w0, w1, w2])
    n = torch.arange(33).view(-1, 1)
    x = 0.5 + ((n * (torch.arange(3).view(1, -1) + 1) + torch.arange(3).view(1, -1)) % 6 - 2).float()
    d = ((n + 2 * torch.arange(3).view(1, -1)) % 5 - 2).float() / 2
    ref = NR.query(f, x, d)
    g = copy.deepcopy(f).to(dev)
    with torch.no_grad():
        rgb, sigma, _ = g.query_raw(x.to(dev), d.to(dev))
    assert float(ref["rgb"].abs().max()) > 0 and float(ref["sigma"].abs().max()) > 0
    assert torch.equal(sigma.double().cpu(), ref["sigma"])
    assert torch.equal(rgb.double().cpu(), ref["rgb"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,G", FIELDS)
def test_fused_against_the_composed_chain(dev, kind, G, dtype):
    f, x, d, ref = case(kind, G, dtype)
    with torch.no_grad():
        if kind == "density":
            fused = f(x)
            f.fused = False
            try:
                assert torch.equal(fused, f(x))
            finally:
                f.fused = True
            return
        rgb, sigma, sel = f.query_raw(x, d)
        dens, feat = f.query_density(x, return_feat=True)
        f.fused = False
        try:
            rgb_c, sigma_c, sel_c = f.query_raw(x, d)
            dens_c, feat_c = f.query_density(x, return_feat=True)
        finally:
            f.fused = True
    assert torch.equal(sigma, sigma_c) and torch.equal(feat, feat_c) and torch.equal(sel, sel_c)
    assert R.worst_ratio(dens.cpu(), dens_c.double().cpu(), 2.0 ** -22 * dens_c.double().abs().cpu()) <= 1.0   # expf against torch.exp
    assert R.worst_ratio(rgb.cpu(), rgb_c.double().cpu(), ref["e_rgb"]) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unbounded", [False, True])
def test_selector_contraction_and_activation(dev, unbounded, dtype):
    f = make_field("radiance", 15, dtype, unbounded=unbounded).to(dev)
    # the largest coordinate whose box coordinate (x + 1) / 2 is still below 1 in float32: x + 1 = the float below 2
    inside, outside = float(torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)) - 1.0), 1.5
    if unbounded:   # radius 0.5, 1 and 10 along a fixed direction: the contraction puts all of them inside
        u = torch.nn.functional.normalize(torch.tensor([[1.0, -2.0, 0.5]]), dim=-1)
        x = torch.cat([0.5 * u, u, 10.0 * u])
        want_sel = [True, True, True]
    else:           # on a face, just inside it, outside; and the same at the lower face
        x = torch.tensor([[1.0, 0.1, 0.2], [inside, 0.1, 0.2], [outside, 0.1, 0.2], [0.3, -1.0, 0.2], [0.3, -inside, 0.2], [0.3, 0.1, -outside]])
        want_sel = [False, True, False, False, True, False]
    x = x.to(dev)
    with torch.no_grad():
        out = f._launch(False, x.shape[0], (x.shape[0],), ["sigma", "density", "selector"], positions=x)
    sel, raw, dens = out["selector"].cpu(), out["sigma"][:, 0].cpu(), out["density"][:, 0].cpu()
    assert sel.tolist() == want_sel
    assert bool((dens[~sel] == 0).all())
    z = raw + (-1.0)   # float32, as the kernel forms it
    want = torch.exp(z.double())
    assert R.worst_ratio(dens[sel], want[sel], ((z.abs().double() + 1) * 2.0 ** -23 * want)[sel]) <= 1.0
    assert bool((dens[sel] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_ray_sample_form_equals_the_position_form(dev, dtype):
    f, _, _, _ = case("radiance", 15, dtype)
    gen = torch.Generator().manual_seed(3)
    o = (torch.rand(3, 3, generator=gen) * 0.4 - 0.2).to(dev)
    d = torch.nn.functional.normalize(torch.randn(3, 3, generator=gen), dim=-1).to(dev)
    ts = (torch.rand(15, generator=gen) * 1.5).to(dev)
    te = ts + 0.05
    ri = torch.arange(3, device=dev).repeat_interleave(5)
    with torch.no_grad():
        sp = sample_positions(o, d, ts, te, ri, dirs="raw")
        a = f.query_on_rays(o, d, ts, te, ri, raw=True)
        b = f.query_raw(sp.positions, sp.dirs)
        dens = f.density_on_rays(o, d, ts, te, ri)
        assert torch.equal(dens, f.query_density(sp.positions)[:, 0])
    for got, want in zip(a, b):
        assert torch.equal(got, want)
    assert bool(a[2].any()) and float(a[0].abs().max()) > 0

"""GPU: the fused training pass of the Instant-NGP fields (``fused_training=True``: csrc/ngp_field.hip, ngp_train_fwd_kernel and
ngp_train_bwd_kernel) against the no-grad launch (forward, bit for bit), the composed chain of the same module and the float64
autograd restatement of tests/ngp_train_reference.py.  Grids as in tests/test_ngp_field_gpu.py."""
import copy

import pytest
import torch

import mlp_reference as R
import ngp_train_reference as TR
from nerfacc_amd.fields import NGPDensityField, NGPRadianceField
from nerfacc_amd.mlp import image_elems
from nerfacc_amd.samples import sample_positions

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
UNIT = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
FIELDS = [("radiance", 15), ("radiance", 7), ("density", 0)]
SMALL = dict(log2_hashmap_size=10, base_resolution=4)


def make_field(kind, G, dtype, **kw):
    """Random table, Xavier networks."""
    gen = torch.Generator().manual_seed(11 + G)
    if kind == "radiance":
        f = NGPRadianceField(AABB, geo_feat_dim=G, n_levels=16, max_resolution=64, dtype=dtype, fused_training=True, **SMALL, **kw)
        f.mlp_head.load_linear_weights(R.xavier_weights(16 + G, 3, 64, 2, seed=3))
    else:
        f = NGPDensityField(AABB, n_levels=5, max_resolution=64, dtype=dtype, fused_training=True, **SMALL, **kw)
    f.mlp_base.load_linear_weights(R.xavier_weights(2 * f.n_levels, 1 + G, 64, 1, seed=5))
    with torch.no_grad():
        f.encoding.params.copy_(torch.rand(f.encoding.params.shape, generator=gen) * 2 - 1)
    return f


def points(N, spread=0.98):
    gen = torch.Generator().manual_seed(5)
    return (torch.rand(N, 3, generator=gen) * 2 - 1) * spread, torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)


def grads(f, fused_training, query, gs):
    """d sum_i <gs[i], query(f)[i]> / d (table, base params, head params) on the fused training pass or the composed chain."""
    f.fused_training = fused_training
    outs = query(f)
    outs = outs if isinstance(outs, tuple) else (outs,)
    params = [f.encoding.params, f.mlp_base.params] + ([f.mlp_head.params] if hasattr(f, "mlp_head") else [])
    return torch.autograd.grad(sum((g * o).sum() for g, o in zip(gs, outs)), params, allow_unused=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("kind,G", FIELDS)
def test_forward_equals_the_no_grad_launch(dev, kind, G, N, dtype):
    f = make_field(kind, G, dtype).to(dev)
    x, d = (t.to(dev) for t in points(N))
    queries = [lambda: f(x)] if kind == "density" else [lambda: f.query_raw(x, d), lambda: f(x, d), lambda: f.query_density(x)]
    for q in queries:
        with torch.no_grad():
            want = q()
        got = q()
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        assert got[0].requires_grad and type(got[0].grad_fn).__name__ == "_NGPTrainFnBackward"
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a, b)
    # what the forward saved for the base network against the composed chain's modules: (table, base, head, inputs.., enc, hidden, out, ..)
    saved = got[0].grad_fn.saved_tensors
    enc, hidden, out = saved[4:7]
    e = f.encoding(f._normalise(x)[0])
    y = f.mlp_base(e)
    assert torch.equal(enc, e) and torch.equal(out, y) and torch.equal(hidden, y.grad_fn.saved_tensors[2])


def exact_field(kind, part, G, dtype, **kw):
    """tests/test_ngp_field_gpu.py's integer construction: scales 4 * 2^l - 1 put x = 0.5 + k on a node of every level; integer
    tables, signed permutation weights.  Returns (CPU field, x, d); only k = 0 is inside the unit box."""
    o, n = torch.arange(64), torch.arange(33).view(-1, 1)
    if kind == "radiance":
        f = NGPRadianceField(UNIT, geo_feat_dim=G, n_levels=16, max_resolution=4 * 2 ** 15, dtype=dtype, **SMALL, **kw)
        w0, w1, w2 = torch.zeros(64, 16 + G), torch.zeros(64, 64), torch.zeros(3, 64)
        w0[o, o % 16 if part == "sh" else 16 + o % G] = 1.0 - 2.0 * ((o // 16) % 2)
        w1[o, (5 * o + 3) % 64] = 1.0
        w2[o % 3, o] = 1.0 - 2.0 * ((o // 3) % 2)
        f.mlp_head.load_linear_weights([w0, w1, w2])
        b0, b1, r = torch.zeros(64, 32), torch.zeros(1 + G, 64), torch.arange(1 + G)
        b0[o, o % 32] = 1.0 - 2.0 * (o // 32)
        b1[r, r], b1[r, r + 32], b1[r, r + 16], b1[r, r + 48] = 1.0, -1.0, 2.0, -2.0
    else:
        f = NGPDensityField(UNIT, n_levels=5, max_resolution=64, dtype=dtype, **SMALL, **kw)
        b0, b1 = torch.zeros(64, 10), torch.ones(1, 64)
        b0[o, o % 10] = 1.0 - 2.0 * (o // 32)
        b1[0, 32:] = 2.0   # raw = sum relu(f) + 2 relu(-f) > 0
    f.mlp_base.load_linear_weights([b0, b1])
    assert f.encoding.scales == [float(4 * 2 ** l - 1) for l in range(f.n_levels)]
    with torch.no_grad():
        f.encoding.params.copy_(((torch.arange(f.encoding.params.numel()) * 7 + 3) % 13 - 6).float())
    x = 0.5 + ((n * (torch.arange(3).view(1, -1) + 1) + torch.arange(3).view(1, -1)) % 6 - 2).float()
    d = ((n + 2 * torch.arange(3).view(1, -1)) % 5 - 2).float() / 2
    return f, x, d


def int_grads(N):
    n = torch.arange(N).view(-1, 1)
    return ((n + torch.arange(3).view(1, -1)) % 3 - 1).float(), ((n[:, 0] * 3) % 5 - 2).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [15, 7])
@pytest.mark.parametrize("part", ["geo", "sh"])
def test_gradients_bit_for_bit_on_integer_valued_data(dev, part, G, dtype):
    """Every product and sum is exact, so the fused pass, the composed chain and float64 autograd agree to the bit (the harmonics'
    columns of the head's dW_0 are float32 sums of inexact products: against the composed chain only, whose pass forms them)."""
    f, x, d = exact_field("radiance", part, G, dtype)
    g_rgb, g_sigma = int_grads(33)
    ref = TR.grads(f, x, d, g_rgb, g_sigma, False)
    g = copy.deepcopy(f).to(dev)
    q = lambda m: m.query_raw(x.to(dev), d.to(dev))[:2]
    got, comp = grads(g, True, q, (g_rgb.to(dev), g_sigma.to(dev))), grads(g, False, q, (g_rgb.to(dev), g_sigma.to(dev)))
    keep = torch.ones(64, 16 + G, dtype=torch.bool)
    keep[:, :16] = False
    keep = torch.cat([keep.reshape(-1), torch.ones(64 * 64 + 3 * 64, dtype=torch.bool)])
    for name, a, b, r, m in zip(("table", "base", "head"), got, comp, ref, (slice(None), slice(None), keep)):
        assert bool(a.any()), name
        assert torch.equal(a, b), name
        assert torch.equal(a.double().cpu()[m], r[m]), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_density_field_bit_for_bit_and_the_selector(dev, dtype):
    """relu(raw) * selector: the derivative is 0 or 1.  The points at k != 0 are outside the box and add exactly nothing; a batch of
    them alone leaves every gradient an exact zero."""
    f, x, _ = exact_field("density", None, 0, dtype, density_activation="relu", density_bias=0.0)
    x = torch.where((torch.arange(33) % 4 != 3).view(-1, 1), torch.full_like(x, 0.5), x)
    g_d = int_grads(33)[1].view(-1, 1)
    ref = TR.grads(f, x, None, None, g_d[:, 0], True)
    g = copy.deepcopy(f).to(dev)
    for inputs, live in ((x, True), (x[3::4], False)):
        assert bool(f._normalise(inputs)[1].any()) == live
        q, gs = (lambda m: m(inputs.to(dev))), (g_d[:inputs.shape[0]].to(dev),)
        got, comp = grads(g, True, q, gs), grads(g, False, q, gs)
        for a, b, r in zip(got, comp, ref):
            assert torch.equal(a, b) and bool(a.any()) == live
            assert not live or torch.equal(a.double().cpu(), r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_activated_mode_is_the_raw_mode_fed_the_derivative(dev, dtype):
    """relu density, no colour gradient: g * act'(raw) * selector is exact, so both modes scatter the same table gradient."""
    f, x, d = exact_field("radiance", "geo", 15, dtype, density_activation="relu", density_bias=0.0, fused_training=True)
    x = torch.where((torch.arange(33) % 4 != 3).view(-1, 1), torch.full_like(x, 0.5), x)
    f, x, d, g_d = f.to(dev), x.to(dev), d.to(dev), int_grads(33)[1].to(dev)
    with torch.no_grad():
        _, raw, sel = f.query_raw(x, d)
    assert bool(sel.any()) and not bool(sel.all())
    act = grads(f, True, lambda m: m(x, d)[1], (g_d.view(-1, 1),))
    fed = grads(f, True, lambda m: m.query_raw(x, d)[1], (g_d * (raw > 0) * sel,))
    assert torch.equal(act[0], fed[0]) and torch.equal(act[1], fed[1]) and bool(act[0].any())
    with pytest.raises(NotImplementedError, match="NGPRadianceField"):
        first = torch.autograd.grad(f(x, d)[1].sum(), f.mlp_base.params, create_graph=True)[0]
        first.sum().backward()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_loop_after_full_sweeps(dev, dtype):
    """Two full sweeps of the backward launch's grid, five full tiles and a tile of 7 points, on the integer case repeated (every
    partial sum stays below 2^24, so the order of the atomics cannot show)."""
    lds = (image_elems(32, 16, 64, 1)[1] + image_elems(31, 3, 64, 2)[1]) * 2 + 4 * 32 * 33 * 4   # both backward images, the staging tiles
    N = 2 * (256 * min(8, 160 * 1024 // lds)) * 4 * 32 + 5 * 32 + 7
    f, x, d = exact_field("radiance", "geo", 15, dtype)
    idx = torch.arange(N) % 33
    f, x, d = f.to(dev), x[idx].to(dev), d[idx].to(dev)
    gs = tuple(t.to(dev) for t in int_grads(N))
    q = lambda m: m.query_raw(x, d)[:2]
    for a, b in zip(grads(f, True, q, gs), grads(f, False, q, gs)):
        assert torch.equal(a, b) and bool(a.any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unbounded", [False, True])
@pytest.mark.parametrize("kind,activated", [("radiance", False), ("radiance", True), ("density", True)])
def test_random_data_within_twice_the_composed_chain(dev, kind, activated, unbounded, dtype):
    """err = max |got - ref| / max |ref| per gradient tensor against float64 autograd; the yardstick is the composed chain's own err
    (the same rounding points, another order of the atomics and of the head's k-steps).
    Measured on an MI355X: fp16 2.4e-4 .. 5.8e-4 on both paths, largest fused / composed 1.09 (head, activated, unbounded); bf16
    1.0e-3 .. 4.1e-3, equal to four digits ("Fused NGP field: training")."""
    f = make_field(kind, 15 if kind == "radiance" else 0, dtype, unbounded=unbounded)
    x, d = points(1000, 1.3)   # inside and outside the box
    gen = torch.Generator().manual_seed(9)
    g_rgb, g_sigma = torch.randn(1000, 3, generator=gen), torch.randn(1000, generator=gen)
    ref = TR.grads(f, x, d if kind == "radiance" else None, g_rgb, g_sigma, activated)
    g, x, d = copy.deepcopy(f).to(dev), x.to(dev), d.to(dev)
    if kind == "density":
        q, gs = (lambda m: m(x)), (g_sigma.view(-1, 1).to(dev),)
    elif activated:
        q, gs = (lambda m: m(x, d)), (g_rgb.to(dev), g_sigma.view(-1, 1).to(dev))
    else:
        q, gs = (lambda m: m.query_raw(x, d)[:2]), (g_rgb.to(dev), g_sigma.to(dev))
    err = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max())
    for name, a, b, r in zip(("table", "base", "head"), grads(g, True, q, gs), grads(g, False, q, gs), ref):
        e_fused, e_comp = err(a, r), err(b, r)
        print(f"{kind} activated={activated} unbounded={unbounded} {dtype} {name}: fused {e_fused:.3e} composed {e_comp:.3e}")
        assert float(r.abs().max()) > 0 and e_fused <= 2 * e_comp


@pytest.mark.parametrize("dtype", DTYPES)
def test_ray_form_equals_the_position_form(dev, dtype):
    """Samples of zero length at t = 0 sit on the origins, the integer case's nodes: the gradients are exact either way."""
    f, x, d = exact_field("radiance", "geo", 15, dtype, fused_training=True, density_activation="relu", density_bias=0.0)
    x = torch.where((torch.arange(33) % 4 != 3).view(-1, 1), torch.full_like(x, 0.5), x)   # (the density needs points inside)
    f, x, d = f.to(dev), x.to(dev), d.to(dev)
    ri = torch.arange(33, device=dev).repeat_interleave(2)
    t = torch.zeros(66, device=dev)
    gs = tuple(g.to(dev) for g in int_grads(66))
    sp = sample_positions(x, d, t, t, ri, dirs="raw")
    assert type(f.query_on_rays(x, d, t, t, ri)[0].grad_fn).__name__ == "_NGPTrainFnBackward"
    on_rays = grads(f, True, lambda m: m.query_on_rays(x, d, t, t, ri)[:2], gs)
    at_points = grads(f, True, lambda m: m.query_raw(sp.positions, sp.dirs)[:2], gs)
    dens = grads(f, True, lambda m: m.density_on_rays(x, d, t, t, ri), gs[1:])
    at_dens = grads(f, True, lambda m: m.query_density(sp.positions)[:, 0], gs[1:])
    for a, b in zip(on_rays + dens[:2], at_points + at_dens[:2]):
        assert torch.equal(a, b) and bool(a.any())

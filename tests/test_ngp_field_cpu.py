"""CPU: nerfacc_amd/fields.py on CPU tensors (the torch path) against tests/ngp_field_reference.py, the fallback rules of the
fused dispatch, and the argument checks of the two fused entries, which are decided before anything reaches a device."""
import ctypes as C

import pytest
import torch

import mlp_reference as R
import ngp_field_reference as NR
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import NGPDensityField, NGPRadianceField

AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
SMALL = dict(log2_hashmap_size=10, base_resolution=4, max_resolution=64)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("unbounded", [False, True])
def test_module_on_cpu_matches_the_reference(dtype, unbounded):
    f = NGPRadianceField(AABB, geo_feat_dim=7, unbounded=unbounded, dtype=dtype, **SMALL)
    gen = torch.Generator().manual_seed(2)
    with torch.no_grad():
        f.encoding.params.copy_(torch.rand(f.encoding.params.shape, generator=gen) * 2 - 1)
    x = torch.rand(40, 3, generator=gen) * 2.4 - 1.2
    d = torch.nn.functional.normalize(torch.randn(40, 3, generator=gen), dim=-1)
    ref = NR.query(f, x, d)
    with torch.no_grad():
        rgb, sigma, sel = f.query_raw(x, d)
        rgb_a, dens = f(x, d)
    assert torch.equal(sel, ref["selector"]) and bool(sel.any()) and bool(sel.all()) == unbounded   # (the contraction puts all inside)
    assert R.worst_ratio(sigma, ref["sigma"], ref["e_sigma"]) <= 1.0
    assert R.worst_ratio(rgb, ref["rgb"], ref["e_rgb"]) <= 1.0
    assert rgb_a.shape == (40, 3) and dens.shape == (40, 1) and bool((dens[~sel] == 0).all()) and bool((dens[sel] > 0).all())
    assert torch.allclose(dens[sel][:, 0], torch.exp(sigma[sel] - 1.0)) and torch.allclose(rgb_a, torch.sigmoid(rgb))
    g = NGPDensityField(AABB, unbounded=unbounded, dtype=dtype, n_levels=5, **SMALL)
    want = NR.query(g, x)
    with torch.no_grad():
        raw, dens = g._base(x)[0][:, 0], g(x)[:, 0]
    assert R.worst_ratio(raw, want["sigma"], want["e_sigma"]) <= 1.0
    assert torch.equal(sel, want["selector"]) and bool((dens[~sel] == 0).all())
    # density = exp(z), z = raw - 1 in float32: the raw value's bound through exp, one rounding of z (|z| 2^-24 relative in the
    # result) and one ulp of the float32 exponential
    z = want["sigma"] - 1.0
    e_dens = torch.exp(z) * (torch.expm1(want["e_sigma"]) + (z.abs() + 2) * 2.0 ** -23)
    assert R.worst_ratio(dens[sel], torch.exp(z)[sel], e_dens[sel]) <= 1.0


@pytest.mark.parametrize("kw,full_only", [
    (dict(num_dim=2), False), (dict(n_levels=20, max_resolution=256), False), (dict(density_activation=lambda r: torch.exp(r - 1)), False),
    (dict(geo_feat_dim=16), False), (dict(use_viewdirs=False), True), (dict(geo_feat_dim=0), True)])
def test_unsupported_configurations_take_the_composed_chain(kw, full_only):
    kw = {**SMALL, **kw}
    D = kw.get("num_dim", 3)
    f = NGPRadianceField(AABB[:D] + AABB[3:3 + D], **kw)
    assert not f.fused_supported(True) and f.fused_supported(False) == full_only
    x = torch.rand(9, D) - 0.5
    dens, feat = f.query_density(x, return_feat=True)
    assert dens.shape == (9, 1) and feat.shape == (9, f.geo_feat_dim) and bool(torch.isfinite(dens).all())
    if f.geo_feat_dim:
        assert f._query_rgb(torch.rand(9, 3), feat).shape == (9, 3)
    assert NGPRadianceField(AABB, **SMALL).fused_supported(True) and NGPDensityField(AABB).fused_supported(False)


P = 0x1000   # a stand-in address that is never dereferenced


def test_fused_entries_report_argument_errors():
    lib = B.load()
    arr = lambda t, v: (t * len(v))(*v)
    scales, res, sizes = arr(C.c_float, [15.0, 31.0]), arr(C.c_int32, [16, 32]), arr(C.c_int32, [1024, 1024])
    vp = lambda a: C.cast(a, C.c_void_p)

    def call(full, elem=1, grid_kw=None, G=3, positions=P, n=4, box=(P, None), contraction=0, act=1, sigma=P, null_grid=False):
        g = dict(params=P, n_params=4096, n_levels=2, n_features=2, log2_hashmap_size=10, interp=0, scales_host=vp(scales),
                 resolutions_host=vp(res), sizes_host=vp(sizes))
        g.update(grid_kw or {})
        grid, inp = B.NGPGrid(**g), B.NGPInput(positions=positions, dirs=P)
        lead = (elem, None if null_grid else C.byref(grid), P) + ((P,) if full else ())
        tail = (G, C.byref(inp), n, *box, contraction, act, -1.0, sigma, 0)
        rc = lib.nfa_ngp_field(*lead, *tail, None, 0, None, None, None, None) if full else lib.nfa_ngp_density(*lead, *tail, None, None, None, None)
        return rc, lib.nfa_last_error().decode()

    for full, nm in ((False, "ngp_density"), (True, "ngp_field")):
        for kw, msg in [
            (dict(elem=0), f"{nm}: elem 0: the networks' type is NFA_ELEM_F16 or NFA_ELEM_BF16"),
            (dict(null_grid=True), f"{nm}: the grid or the input descriptor is null"),
            (dict(grid_kw=dict(n_features=4)), f"{nm}: n_features must be 2 (got 4)"),
            (dict(grid_kw=dict(n_levels=17)), f"{nm}: n_levels must be in 1..16 (got 17)"),
            (dict(grid_kw=dict(interp=2)), f"{nm}: interp must be NFA_INTERP_LINEAR (0) or NFA_INTERP_SMOOTHSTEP (1) (got 2)"),
            (dict(G=16), f"{nm}: geo_feat_dim must be in {1 if full else 0}..15 (got 16)"),
            (dict(grid_kw=dict(log2_hashmap_size=9)), f"{nm}: log2_hashmap_size must be in 10..24 (got 9)"),
            (dict(grid_kw=dict(n_params=5)), f"{nm}: n_params 5 != 2048 entries x 2 features"),
            (dict(contraction=2), f"{nm}: contraction must be 0 (the box) or 1 (the unit sphere) (got 2)"),
            (dict(box=(None, None)), f"{nm}: the aabb is given once, on the host or on the device"),
            (dict(box=(P, P)), f"{nm}: the aabb is given once, on the host or on the device"),
            (dict(act=5), f"{nm}: density_act must be in 0..4 (got 5)"),
            (dict(positions=None), f"{nm}: n_rays 0 out of range"),
            (dict(grid_kw=dict(params=None)), f"{nm}: null pointer (table or image)"),
            (dict(sigma=None), f"{nm}: no output requested"),
            (dict(n=0, sigma=None), None),
        ]:
            rc, err = call(full, **kw)
            assert (rc == 0) if msg is None else (rc == -1 and err == msg), (nm, kw, rc, err)
    rc = lib.nfa_ngp_pack_head(1, P, 0, P, 8192, None)
    assert rc == -1 and lib.nfa_last_error() == b"ngp_pack_head: geo_feat_dim must be in 1..15 (got 0)"
    rc = lib.nfa_ngp_pack_head(1, P, 15, P, 100, None)
    assert rc == -1 and lib.nfa_last_error() == b"ngp_pack_head: the image holds 8192 elements for this shape, got 100"

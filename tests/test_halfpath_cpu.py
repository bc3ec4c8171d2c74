"""CPU: the half-precision field path's Python layer -- ``out_dtype`` of the encodings (validation, the torch path equal to
``float32_output.to(out_dtype)`` bit for bit, ``"autocast"``, backward from a half output, pass-through of
``encoding_from_tcnn_config``) and ``rendering_from_raw``'s unchanged fallback for CPU half inputs."""
import pytest
import torch

from nerfacc_amd.encodings import HashGridEncoding, SphericalHarmonicsEncoding, encoding_from_tcnn_config
from nerfacc_amd.rawrender import rendering_from_raw

HALF = [torch.float16, torch.bfloat16]
GRID = dict(n_levels=5, n_features_per_level=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.7)


def grid_pair(out_dtype):
    """A float32 grid and one with ``out_dtype`` that shares its parameters."""
    torch.manual_seed(0)
    ref = HashGridEncoding(3, **GRID)
    with torch.no_grad():
        ref.params.uniform_(-1, 1)
    enc = HashGridEncoding(3, out_dtype=out_dtype, **GRID)
    enc.params = ref.params
    return ref, enc


def points(n, seed=1):
    x = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 1.5 - 0.25
    x[0] = torch.tensor([1.0, 0.0, 0.5])
    return x


@pytest.mark.parametrize("bad", [torch.float64, torch.int32, "bf16", "half", 16, torch.float8_e4m3fn])
def test_out_dtype_validation(bad):
    with pytest.raises(ValueError):
        HashGridEncoding(3, out_dtype=bad, **GRID)
    with pytest.raises(ValueError):
        SphericalHarmonicsEncoding(3, 4, out_dtype=bad)
    with pytest.raises(ValueError):
        encoding_from_tcnn_config(3, {"otype": "SphericalHarmonics", "degree": 2}, out_dtype=bad)


def test_out_dtype_accepted_values():
    for ok in (None, torch.float16, torch.bfloat16, "autocast"):
        assert HashGridEncoding(3, out_dtype=ok, **GRID).out_dtype == ok
        assert SphericalHarmonicsEncoding(3, 3, out_dtype=ok).out_dtype == ok
    assert HashGridEncoding(3, **GRID).out_dtype is None


@pytest.mark.parametrize("d", HALF)
def test_hashgrid_equals_float32_rounded_once(d):
    ref, enc = grid_pair(d)
    x = points(257)
    y = enc(x)
    assert y.dtype == d and y.shape == (257, 10)
    assert torch.equal(y, ref(x).to(d))
    assert ref(x).dtype == torch.float32                       # the default is untouched
    assert enc(x.view(257, 1, 3)).shape == (257, 1, 10)


@pytest.mark.parametrize("d", HALF)
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_equals_float32_rounded_once(d, degree):
    dirs = torch.rand(101, 3, generator=torch.Generator().manual_seed(degree))
    y = SphericalHarmonicsEncoding(3, degree, out_dtype=d)(dirs)
    assert y.dtype == d and y.shape == (101, degree * degree)
    assert torch.equal(y, SphericalHarmonicsEncoding(3, degree)(dirs).to(d))


def test_autocast_resolves_to_the_active_dtype():
    ref, enc = grid_pair("autocast")
    sh = SphericalHarmonicsEncoding(3, 4, out_dtype="autocast")
    x = points(33)
    assert enc(x).dtype == torch.float32 and sh(x).dtype == torch.float32
    assert torch.equal(enc(x), ref(x))
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y, s, y_ref = enc(x), sh(x), ref(x)
    assert y.dtype == torch.bfloat16 and s.dtype == torch.bfloat16
    assert y_ref.dtype == torch.float32                        # out_dtype=None: float32 under autocast, as ever
    assert torch.equal(y, y_ref.to(torch.bfloat16))
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=False):
        assert enc(x).dtype == torch.float32


@pytest.mark.parametrize("d", HALF)
def test_backward_from_a_half_output(d):
    ref, enc = grid_pair(d)
    x = points(65).requires_grad_(True)
    y = enc(x)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(d)
    y.backward(g)
    assert enc.params.grad.dtype == torch.float32 and x.grad.dtype == torch.float32
    gp, gx = enc.params.grad.clone(), x.grad.clone()
    enc.params.grad = None
    x2 = x.detach().clone().requires_grad_(True)
    ref(x2).backward(g.float())                               # the float32 op fed the widened gradient
    torch.testing.assert_close(gp, ref.params.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gx, x2.grad, rtol=1e-5, atol=1e-5)
    assert float(gp.abs().sum()) > 0

    dirs = torch.rand(17, 3).requires_grad_(True)
    s = SphericalHarmonicsEncoding(3, 4, out_dtype=d)(dirs)
    s.backward(torch.ones_like(s))
    assert dirs.grad.dtype == torch.float32 and bool(torch.isfinite(dirs.grad).all())


def test_tcnn_config_passes_out_dtype_through():
    grid = encoding_from_tcnn_config(3, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2,
                                         "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5},
                                     out_dtype=torch.float16)
    assert isinstance(grid, HashGridEncoding) and grid.out_dtype == torch.float16
    comp = encoding_from_tcnn_config(3, {"otype": "Composite", "nested": [
        {"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 3}]}, out_dtype="autocast")
    assert isinstance(comp, SphericalHarmonicsEncoding) and comp.out_dtype == "autocast"
    assert encoding_from_tcnn_config(3, {"otype": "SphericalHarmonics"}).out_dtype is None
    x = points(9)
    assert grid(x).dtype == torch.float16
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert comp(x).dtype == torch.bfloat16


@pytest.mark.parametrize("d", HALF)
def test_rendering_from_raw_cpu_half_inputs_take_the_fallback(d):
    g = torch.Generator().manual_seed(5)
    counts = torch.tensor([3, 0, 5, 1])
    ri = torch.repeat_interleave(torch.arange(4), counts)
    n = int(counts.sum())
    ts = torch.rand(n, generator=g)
    te = ts + 0.05
    raw_rgb = torch.randn(n, 3, generator=g).to(d).requires_grad_(True)
    raw_sig = torch.randn(n, generator=g).to(d).requires_grad_(True)
    colors, opac, depth, extras = rendering_from_raw(ts, te, raw_rgb, raw_sig, ri, 4, return_activated=True)
    assert colors.shape == (4, 3) and opac.shape == (4, 1) and depth.shape == (4, 1)
    assert colors.dtype == torch.float32 and extras["weights"].dtype == torch.float32   # torch's promotion
    assert extras["sigmas"].dtype == d and extras["rgbs"].dtype == d
    assert all(bool(torch.isfinite(t).all()) for t in (colors, opac, depth))
    (colors.sum() + opac.sum()).backward()
    assert raw_rgb.grad.dtype == d and raw_sig.grad.dtype == d
    assert bool(torch.isfinite(raw_rgb.grad.float()).all()) and float(raw_sig.grad.float().abs().sum()) > 0


def test_unknown_element_type_is_an_argument_error():
    """The `_t` entries reject a code that is not NFA_ELEM_F32 / F16 / BF16 before they look at anything else."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for name in ("nfa_hashgrid_fwd_t", "nfa_hashgrid_bwd_t", "nfa_sh_fwd_t", "nfa_sh_bwd_t", "nfa_render_raw_fwd_t",
                 "nfa_render_raw_bwd_t"):
        fn = getattr(lib, name)
        for code in (3, -1):
            assert fn(code, *[0] * (len(fn.argtypes) - 1)) == -1, name   # NFA_EINVAL
            assert b"elem must be NFA_ELEM_F32" in lib.nfa_last_error(), name
    assert B.ELEM_CODES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2} and B.ABI_VERSION == lib.nfa_version()

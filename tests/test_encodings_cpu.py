"""CPU: nerfacc_amd.encodings -- the hash grid's level table (known answers of ngp.py's two configs), its torch path
against an independent float64 loop-over-corners restatement, gradients (gradcheck), spherical harmonics against the
Instant-NGP constants, encoding_from_tcnn_config on ngp.py's dicts, and the C ABI's argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

M32 = 0xFFFFFFFF


def ngp_per_level_scale(base, max_res, n_levels):
    # examples/radiance_fields/ngp.py
    return np.exp((np.log(max_res) - np.log(base)) / (n_levels - 1)).tolist()


# ----------------------------------------------------------------------------- level table
def test_level_table_radiance_field_config():
    from nerfacc_amd.encodings import HashGridEncoding
    enc = HashGridEncoding(3, n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16,
                           per_level_scale=ngp_per_level_scale(16, 4096, 16))
    assert abs(enc.per_level_scale - 1.4472692) < 1e-7
    assert enc.resolutions == [16, 24, 34, 49, 71, 102, 148, 213, 308, 446, 646, 934, 1352, 1956, 2831, 4096]
    assert enc.sizes == [4096, 13824, 39304, 117656, 357912] + [524288] * 11
    assert enc.offsets == [sum(enc.sizes[:l]) for l in range(16)]
    assert sum(enc.sizes) == 6299960 and enc.params.numel() == 12599920 and enc.params.numel() * 4 == 50399680
    assert enc.n_output_dims == 32
    assert enc.table.hashed == [False] * 5 + [True] * 11
    # scale_l = exp2f(l log2f(s)) * 16 - 1 in float32, res = ceil(scale) + 1
    for l, (s, r) in enumerate(zip(enc.scales, enc.resolutions)):
        assert np.float32(s) == s and math.ceil(s) + 1 == r
    assert enc.scales[0] == 15.0


def test_level_table_density_field_config():
    from nerfacc_amd.encodings import HashGridEncoding
    enc = HashGridEncoding(3, n_levels=5, n_features_per_level=2, log2_hashmap_size=17, base_resolution=16,
                           per_level_scale=ngp_per_level_scale(16, 128, 5))
    assert enc.resolutions == [16, 27, 46, 77, 128]
    assert sum(enc.sizes) == 383264
    assert enc.sizes == [4096, 19688, 97336, 131072, 131072]
    assert enc.params.numel() == 2 * 383264
    p = enc.params.detach()
    assert p.dtype == torch.float32 and float(p.abs().max()) <= 1e-4 and float(p.abs().max()) > 0


# ----------------------------------------------------------------------------- torch path vs a float64 restatement
def restate_hashgrid(x, params, enc):
    """float64 over corners, one point at a time: p in float32 as the spec has it, weights and sums in float64."""
    x = np.asarray(x, np.float32)
    P = np.asarray(params, np.float64).reshape(-1, enc.n_features_per_level)
    F, L = enc.n_features_per_level, enc.n_levels
    T = 1 << enc.log2_hashmap_size
    out = np.zeros((x.shape[0], L * F))
    for n in range(x.shape[0]):
        for l in range(L):
            s, res, size, off = np.float32(enc.scales[l]), enc.resolutions[l], enc.sizes[l], enc.offsets[l]
            hashed = (res ** 3 + 7) // 8 * 8 > T
            p = [np.float32(np.float32(x[n, d]) * s) + np.float32(0.5) for d in range(3)]
            g = [int(math.floor(float(v))) & M32 for v in p]
            f = [float(v) - math.floor(float(v)) for v in p]
            acc = np.zeros(F)
            for c in range(8):
                b = [(c >> d) & 1 for d in range(3)]
                q = [(g[d] + b[d]) & M32 for d in range(3)]
                if hashed:
                    idx = (q[0] ^ ((q[1] * 2654435761) & M32) ^ ((q[2] * 805459861) & M32)) & (size - 1)
                else:
                    idx = ((q[0] + q[1] * res + q[2] * res * res) & M32) % size
                w = 1.0
                for d in range(3):
                    w *= f[d] if b[d] else 1.0 - f[d]
                acc += w * P[off + idx]
            out[n, l * F:(l + 1) * F] = acc
    return out


@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_torch_path_matches_restatement(F):
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(F)
    # levels 0-1 dense, 2-3 hashed (2^10 entries)
    enc = HashGridEncoding(3, n_levels=4, n_features_per_level=F, log2_hashmap_size=10, base_resolution=4,
                           per_level_scale=2.5)
    assert enc.table.hashed == [False, False, True, True]
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    x = torch.rand(64, 3) * 2.0 - 0.5          # [-0.5, 1.5]^3
    x[:4] = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [-0.5, 1.5, 0.25], [0.5, 0.5, 0.5]])
    y = enc(x)
    assert y.shape == (64, 4 * F) and y.dtype == torch.float32
    ref = restate_hashgrid(x.numpy(), enc.params.detach().numpy(), enc)
    np.testing.assert_allclose(y.detach().numpy(), ref, rtol=0, atol=2e-6)


def test_torch_path_leading_dims_and_float64():
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(0)
    enc = HashGridEncoding(3, n_levels=3, n_features_per_level=2, log2_hashmap_size=10, base_resolution=2,
                           per_level_scale=3.0)
    x = torch.rand(2, 5, 3)
    y = enc(x)
    assert y.shape == (2, 5, 6)
    torch.testing.assert_close(y.view(10, 6), enc(x.view(10, 3)), rtol=0, atol=0)
    y64 = enc(x.double())
    assert y64.dtype == torch.float64
    torch.testing.assert_close(y64.float(), y, rtol=1e-5, atol=1e-9)


def test_torch_path_nonfinite_inputs_stay_in_table():
    from nerfacc_amd.encodings import HashGridEncoding
    enc = HashGridEncoding(3, n_levels=2, n_features_per_level=2, log2_hashmap_size=10, base_resolution=4,
                           per_level_scale=4.0)
    x = torch.tensor([[float("nan"), 0.5, 0.5], [float("inf"), -float("inf"), 0.0], [1e30, -1e30, 3e9]])
    y = enc(x)   # no index error: every index is reduced into its level
    assert y.shape == (3, 4)
    assert torch.isfinite(y[2]).all()


def test_gradcheck_params_and_x():
    from nerfacc_amd.encodings import HashGridEncoding, _hashgrid_torch
    torch.manual_seed(1)
    enc = HashGridEncoding(3, n_levels=2, n_features_per_level=1, log2_hashmap_size=10, base_resolution=4,
                           per_level_scale=3.0)
    assert enc.table.hashed == [False, True]
    p = enc.params.detach().double().uniform_(-1, 1).requires_grad_(True)
    x = (torch.rand(6, 3, dtype=torch.float64) * 0.9 + 0.05).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda p_: _hashgrid_torch(x.detach(), p_, enc.table, 1), (p,), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda x_: _hashgrid_torch(x_, p.detach(), enc.table, 1), (x,), eps=1e-7, atol=1e-5)
    # through the module: gradients only for what needs them
    enc.params.requires_grad_(False)
    xx = torch.rand(4, 3, requires_grad=True)
    enc(xx).sum().backward()
    assert xx.grad is not None and enc.params.grad is None


def test_autocast_runs_in_float32():
    from nerfacc_amd.encodings import HashGridEncoding, SphericalHarmonicsEncoding
    enc = HashGridEncoding(3, n_levels=2, n_features_per_level=2, log2_hashmap_size=10, base_resolution=4)
    sh = SphericalHarmonicsEncoding(3, 4)
    x = torch.rand(8, 3)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y = enc(x.bfloat16())
        s = sh(x)
    assert y.dtype == torch.float32 and s.dtype == torch.float32
    torch.testing.assert_close(y, enc(x.bfloat16().float()), rtol=0, atol=0)


# ----------------------------------------------------------------------------- spherical harmonics
def sh_reference(d):
    x, y, z = (2.0 * np.asarray(d, np.float64) - 1.0).T
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
        -1.0925484305920792 * x * z, 0.54627421529603959 * (x * x - y * y),
        0.59004358992664352 * y * (-3 * x * x + y * y), 2.8906114426405538 * x * y * z,
        0.45704579946446572 * y * (1 - 5 * z * z), 0.3731763325901154 * z * (5 * z * z - 3),
        0.45704579946446572 * x * (1 - 5 * z * z), 1.4453057213202769 * z * (x * x - y * y),
        0.59004358992664352 * x * (-x * x + 3 * y * y)], -1)


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_constants(degree):
    from nerfacc_amd.encodings import SphericalHarmonicsEncoding
    sh = SphericalHarmonicsEncoding(3, degree)
    assert sh.n_output_dims == degree * degree
    d = torch.rand(3, 7, 3, dtype=torch.float64)
    out = sh(d)
    assert out.shape == (3, 7, degree * degree)
    np.testing.assert_allclose(out.reshape(-1, degree * degree).numpy(), sh_reference(d.reshape(-1, 3))[:, :degree ** 2],
                               rtol=1e-14, atol=1e-15)
    assert sh(d.float()).dtype == torch.float32


def test_sh_backward_finite_differences():
    from nerfacc_amd.encodings import SphericalHarmonicsEncoding
    sh = SphericalHarmonicsEncoding(3, 4)
    d = torch.rand(9, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(sh, (d,), eps=1e-6, atol=1e-8)


# ----------------------------------------------------------------------------- tcnn configs (ngp.py)
def test_encoding_from_tcnn_config_ngp_dicts():
    from nerfacc_amd.encodings import HashGridEncoding, SphericalHarmonicsEncoding, encoding_from_tcnn_config
    import nerfacc_amd
    dir_cfg = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 4}]}
    e = encoding_from_tcnn_config(3, dir_cfg)
    assert isinstance(e, SphericalHarmonicsEncoding) and e.degree == 4 and e.n_output_dims == 16
    rf = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
          "per_level_scale": ngp_per_level_scale(16, 4096, 16)}
    g = encoding_from_tcnn_config(3, rf)
    assert isinstance(g, HashGridEncoding) and g.n_output_dims == 32 and sum(g.sizes) == 6299960
    df = {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 2, "log2_hashmap_size": 17, "base_resolution": 16,
          "per_level_scale": ngp_per_level_scale(16, 128, 5)}
    g = encoding_from_tcnn_config(3, df)
    assert g.resolutions == [16, 27, 46, 77, 128] and g.n_output_dims == 10
    for name in ("HashGridEncoding", "SphericalHarmonicsEncoding", "encoding_from_tcnn_config", "encodings"):
        assert name not in nerfacc_amd.__all__
    assert len(nerfacc_amd.__all__) == 22


@pytest.mark.parametrize("n_dims,cfg,match", [
    (3, {"otype": "Frequency", "n_frequencies": 4}, "unsupported tcnn encoding 'Frequency'"),
    (3, {"otype": "HashGrid", "interpolation": "Smoothstep"}, "only linear interpolation"),
    (2, {"otype": "HashGrid"}, "only 3 input dimensions"),
    (3, {"otype": "HashGrid", "n_features_per_level": 3}, "n_features_per_level must be 1, 2, 4 or 8"),
    (3, {"otype": "HashGrid", "n_levels": 33}, "n_levels must be in 1..32"),
    (3, {"otype": "HashGrid", "log2_hashmap_size": 25}, "log2_hashmap_size must be in 10..24"),
    (3, {"otype": "SphericalHarmonics", "degree": 5}, "degree must be in 1..4"),
    (3, {"otype": "Composite", "nested": [{"otype": "SphericalHarmonics", "n_dims_to_encode": 2}]}, "all 3 dimensions"),
    (3, {"otype": "Composite", "nested": [{"otype": "SphericalHarmonics"}, {"otype": "Identity"}]}, "exactly one"),
    (3, {"n_levels": 4}, "not a tcnn encoding config"),
])
def test_encoding_from_tcnn_config_errors(n_dims, cfg, match):
    from nerfacc_amd.encodings import encoding_from_tcnn_config
    with pytest.raises(ValueError, match=match):
        encoding_from_tcnn_config(n_dims, cfg)


# ----------------------------------------------------------------------------- C ABI argument checks
P = 0x1000   # a stand-in address that is never dereferenced
# a 2-level table: res 4 (dense, 64 entries) and res 12 (hashed, 2^10 entries), F = 1
_SCALES = (ctypes.c_float * 2)(3.0, 11.0)
_RES = (ctypes.c_int32 * 2)(4, 12)
_SIZES = (ctypes.c_int32 * 2)(64, 1024)
_BAD_SIZES = (ctypes.c_int32 * 2)(64, 1000)
_ARGS = {
    "nfa_hashgrid_fwd": "x params n_points n_levels n_features log2 scales res sizes n_params y stream",
    "nfa_hashgrid_bwd": "x params grad_y n_points n_levels n_features log2 scales res sizes n_params grad_params "
                        "grad_x stream",
    "nfa_sh_fwd": "dirs n_points degree out stream",
    "nfa_sh_bwd": "dirs grad_out n_points degree grad_dirs stream",
}
_SCALARS = {"n_points": 16, "n_levels": 2, "n_features": 1, "log2": 10, "scales": _SCALES, "res": _RES,
            "sizes": _SIZES, "n_params": 1088, "degree": 4}


def _cases():
    cases = []
    for fn in ("nfa_hashgrid_fwd", "nfa_hashgrid_bwd"):
        nm = fn[len("nfa_"):]
        cases += [
            (fn, {"n_points": -1}, f"{nm}: negative size"),
            (fn, {"n_params": -1}, f"{nm}: negative size"),
            (fn, {"n_features": 3}, f"{nm}: n_features must be 1, 2, 4 or 8 (got 3)"),
            (fn, {"n_levels": 0}, f"{nm}: n_levels must be in 1..32 (got 0)"),
            (fn, {"n_levels": 33}, f"{nm}: n_levels must be in 1..32 (got 33)"),
            (fn, {"log2": 9}, f"{nm}: log2_hashmap_size must be in 10..24 (got 9)"),
            (fn, {"n_params": 1 << 31}, f"{nm}: too many parameters (2147483648)"),
            (fn, {"sizes": None}, f"{nm}: null level table"),
            (fn, {"sizes": _BAD_SIZES}, f"{nm}: level 1 size 1000 is not min(roundup8(res^3), 2^10)"),
            (fn, {"n_params": 1089}, f"{nm}: n_params 1089 != 1088 entries x 1 features"),
            (fn, {"x": None}, f"{nm}: null pointer"),
            (fn, {"n_points": 0, "all_null": True}, None),
        ]
    cases += [("nfa_hashgrid_fwd", {a: None}, "hashgrid_fwd: null pointer") for a in ("params", "y")]
    cases += [("nfa_hashgrid_bwd", {"grad_y": None}, "hashgrid_bwd: null pointer"),
              ("nfa_hashgrid_bwd", {"grad_params": None, "grad_x": None}, "hashgrid_bwd: null pointer"),
              ("nfa_hashgrid_bwd", {"params": None}, "hashgrid_bwd: null pointer")]
    for fn in ("nfa_sh_fwd", "nfa_sh_bwd"):
        nm = fn[len("nfa_"):]
        cases += [
            (fn, {"n_points": -1}, f"{nm}: negative size"),
            (fn, {"degree": 0}, f"{nm}: degree must be in 1..4 (got 0)"),
            (fn, {"degree": 5}, f"{nm}: degree must be in 1..4 (got 5)"),
            (fn, {"dirs": None}, f"{nm}: null pointer"),
            (fn, {"n_points": 0, "all_null": True}, None),
        ]
    cases += [("nfa_sh_fwd", {"out": None}, "sh_fwd: null pointer"),
              ("nfa_sh_fwd", {"out": P + 4}, "sh_fwd: out must be 16-byte aligned"),
              ("nfa_sh_bwd", {"grad_out": None}, "sh_bwd: null pointer"),
              ("nfa_sh_bwd", {"grad_dirs": None}, "sh_bwd: null pointer"),
              ("nfa_sh_bwd", {"grad_out": P + 8}, "sh_bwd: grad_out must be 16-byte aligned")]
    return cases


def test_encoding_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn, kw, msg in _cases():
        kw = dict(kw)
        all_null = kw.pop("all_null", False)
        args = [kw[a] if a in kw else _SCALARS[a] if a in _SCALARS else (None if all_null or a == "stream" else P)
                for a in _ARGS[fn].split()]
        assert len(args) == len(B._SIGS[fn])
        lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
        rc = getattr(lib, fn)(*args)
        if msg is None:
            assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
        else:
            assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())

"""CPU: ``HashGridEncoding(interpolation="Smoothstep")`` -- autograd's own checks of the torch path, the float64 restatement
of tests/hashgrid_smoothstep_reference.py against autograd's double backward, the pure second partial that the linear grid
lacks, C^1 at cell faces, the constructor, the `_i` entries' refusal of an unknown interpolation, and the numpy restatement of
the sorted table gradient against its own float64 sums."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hashgrid_smoothstep_reference as R
from conftest import ROOT
from hashgrid2_reference import interior_points, restate_grad2


def small_grid(interpolation="Smoothstep", n_levels=4, F=2):
    """4 levels 3, 15, 63 and 255 cells wide (one dense, three hashed into 2^10 entries)."""
    from nerfacc_amd.encodings import HashGridEncoding
    enc = HashGridEncoding(3, n_levels=n_levels, n_features_per_level=F, log2_hashmap_size=10, base_resolution=4,
                           per_level_scale=4.0, interpolation=interpolation)
    assert enc.scales == [3.0, 15.0, 63.0, 255.0][:n_levels] and enc.table.hashed == [False, True, True, True][:n_levels]
    return enc


# ----------------------------------------------------------------------------- autograd's checks of the torch path
def test_gradcheck_and_gradgradcheck():
    torch.manual_seed(1)
    enc = small_grid().double()
    x = interior_points(5, enc, seed=2).double().requires_grad_(True)
    p = (torch.rand(enc.params.numel(), dtype=torch.float64) * 2 - 1).requires_grad_(True)

    def fn(x_, p_):
        return torch.func.functional_call(enc, {"params": p_}, (x_,))

    assert torch.autograd.gradcheck(lambda x_: fn(x_, p.detach()), (x,), eps=1e-6, atol=1e-5)
    # (6,272 parameters, in which y is linear: random directions instead of one perturbation per parameter)
    assert torch.autograd.gradcheck(lambda p_: fn(x.detach(), p_), (p,), eps=1e-6, atol=1e-5, fast_mode=True)
    assert torch.autograd.gradgradcheck(lambda x_: fn(x_, p.detach()), (x,), eps=1e-6, atol=1e-5)


# ----------------------------------------------------------------------------- the float64 restatement
def exact_case(F=2, n=40):
    """Coordinates that are multiples of 2^-6 on integer scales: p = x * scale + 0.5 and the three smoothstep factors (f has
    6 fractional bits, S at most 19 significant ones) are exact in float32, so the restatement's float32 factors are those
    of the float64 torch path."""
    enc = small_grid(F=F)
    x = interior_points(n, enc, seed=F, lo=-0.25, hi=1.25, grid=64.0)
    for l, s in enumerate(enc.scales):
        assert torch.equal((x * s + 0.5).double(), x.double() * s + 0.5)
        _, S, S1, S2 = R.level_cell(x, enc, l)
        f = (x.double() * s + 0.5) - torch.floor(x.double() * s + 0.5)
        assert torch.equal(S.double(), (f * f) * (3.0 - 2.0 * f)) and torch.equal((1.0 - S).double(), 1.0 - S.double())
        assert torch.equal(S1.double(), (6.0 * f) * (1.0 - f)) and torch.equal(S2.double(), 6.0 - 12.0 * f)
    gen = torch.Generator().manual_seed(10 + F)
    params = torch.rand(enc.params.numel(), dtype=torch.float64, generator=gen) * 2 - 1
    g = torch.randn(n, enc.n_output_dims, dtype=torch.float64, generator=gen)
    v = torch.randn(n, 3, dtype=torch.float64, generator=gen)
    return enc, x, params, g, v


@pytest.mark.parametrize("F", [1, 2, 4])
def test_restatement_matches_autograd_double_backward(F):
    from nerfacc_amd.encodings import _hashgrid_torch
    enc, x, params, g, v = exact_case(F)
    x64 = x.double().requires_grad_(True)
    p64 = params.clone().requires_grad_(True)
    g64 = g.clone().requires_grad_(True)
    y = _hashgrid_torch(x64, p64, enc.table, F, enc.interp)
    (g_x,) = torch.autograd.grad(y, x64, g64, create_graph=True)
    (g_p,) = torch.autograd.grad(y, p64, g64, retain_graph=True)
    x2, g2_p, gg_y = torch.autograd.grad(g_x, (x64, p64, g64), v)

    r = R.restate(x, params, enc, g, v)
    close = lambda got, want: torch.testing.assert_close(got, want.detach(), rtol=1e-10,   # noqa: E731
                                                         atol=1e-10 * float(want.detach().abs().mean()))
    close(r["y"], y)
    close(r["g_x"], g_x)
    close(r["g_params"], g_p)
    close(r["gg_y"], gg_y)
    close(r["g2_params"], g2_p)
    close(r["x2"], x2)
    # the term counts and magnitudes: 24 per gg_y element, 3 per touching corner, 24 L F per x2 element
    L = enc.n_levels
    assert bool((r["gg_y_k"] == 24).all()) and bool((r["x2_k"] == 24 * L * F).all())
    assert float(r["hits"].sum()) == 8 * L * x.shape[0]
    assert torch.equal(r["g2_params_k"].view(-1, F)[:, 0], 3 * r["hits"])
    for name in ("g_params", "gg_y", "g2_params", "x2"):
        assert bool((r[name].abs() <= r[name + "_abs"] * (1 + 1e-12)).all())


@pytest.mark.parametrize("e", [0, 1, 2])
def test_pure_second_partial(e):
    """v along one axis e: the linear grid's x2[:, e] has no term at all, the smoothstep grid's has S''."""
    enc, _, params, g, _ = exact_case()
    x = interior_points(g.shape[0], enc, seed=20 + e, lo=-0.25, hi=1.25)      # (off the 2^-6 lattice: S''(0.5) = 0)
    v = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    v[:, e] = torch.randn(x.shape[0], dtype=torch.float64, generator=torch.Generator().manual_seed(e)) + 3.0
    smooth = R.restate(x, params, enc, g, v)["x2"]
    linear = restate_grad2(x, params, small_grid("Linear"), g, v)["x2"]
    assert bool((smooth[:, e] != 0).all())
    assert bool((linear[:, e] == 0).all())
    others = [d for d in range(3) if d != e]
    assert bool((linear[:, others] != 0).any()) and bool((smooth[:, others] != 0).any())


@pytest.mark.parametrize("d", [0, 1, 2])
def test_c1_at_cell_faces(d):
    enc = small_grid(n_levels=1)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    x = R.face_points(enc, d).requires_grad_(True)
    g = torch.randn(x.shape[0], enc.n_output_dims, generator=torch.Generator().manual_seed(9))
    (g_x,) = torch.autograd.grad(enc(x), x, g)
    assert bool((g_x[:, d] == 0).all())
    assert bool((g_x[:, [k for k in range(3) if k != d]] != 0).any())
    lin = small_grid("Linear", n_levels=1)
    lin.params = enc.params
    (g_lin,) = torch.autograd.grad(lin(x), x, g)
    assert bool((g_lin[:, d] != 0).any())                      # the linear grid has a one-sided slope there


# ----------------------------------------------------------------------------- the constructor
def test_constructor():
    from nerfacc_amd import _backend as B
    from nerfacc_amd.encodings import HashGridEncoding
    kw = dict(n_levels=2, n_features_per_level=2, log2_hashmap_size=10, base_resolution=4)
    lin = HashGridEncoding(3, **kw)
    assert lin.interpolation == "Linear" and lin.interp == 0 and "interpolation" not in lin.extra_repr()
    for name in ("Smoothstep", "smoothstep", "SMOOTHSTEP"):
        enc = HashGridEncoding(3, interpolation=name, **kw)
        assert enc.interpolation == "Smoothstep" and enc.interp == B.INTERP_CODES["Smoothstep"] == 1
        assert "interpolation=Smoothstep" in enc.extra_repr()
    assert HashGridEncoding(3, interpolation="linear", **kw).interpolation == "Linear"
    for bad in ("Nearest", "cubic", "", None, 1):
        with pytest.raises(ValueError, match="interpolation must be"):
            HashGridEncoding(3, interpolation=bad, **kw)
    assert list(enc.state_dict()) == list(lin.state_dict()) == ["params"]
    assert enc.params.shape == lin.params.shape and [p.numel() for p in enc.parameters()] == [lin.params.numel()]
    assert enc.scales == lin.scales and enc.sizes == lin.sizes and enc.offsets == lin.offsets
    torch.manual_seed(3)
    a = HashGridEncoding(3, **kw).params
    torch.manual_seed(3)
    b = HashGridEncoding(3, interpolation="Smoothstep", **kw).params
    assert torch.equal(a, b)                                       # the same initialisation
    # the torch path: another function of the same table
    lin.params = enc.params
    x = torch.rand(50, 3, generator=torch.Generator().manual_seed(4))
    assert enc(x).shape == lin(x).shape and not torch.equal(enc(x), lin(x))


def test_tcnn_config_still_refuses_smoothstep():
    from nerfacc_amd.encodings import encoding_from_tcnn_config
    with pytest.raises(ValueError, match="only linear interpolation"):
        encoding_from_tcnn_config(3, {"otype": "HashGrid", "interpolation": "Smoothstep"})
    assert "interpolation=\"Smoothstep\"" in encoding_from_tcnn_config.__doc__


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced  (tests/test_encodings_cpu.py)
_SCALES = (ctypes.c_float * 2)(3.0, 11.0)
_RES = (ctypes.c_int32 * 2)(4, 12)
_SIZES = (ctypes.c_int32 * 2)(64, 1024)
_TABLE = "n_points n_levels n_features log2 scales res sizes n_params"
_ARGS = {
    "nfa_hashgrid_fwd_i": f"interp elem x params {_TABLE} y stream",
    "nfa_hashgrid_bwd_i": f"interp elem x params grad_y {_TABLE} grad_params grad_x stream",
    "nfa_hashgrid_bwd_bwd_i": f"interp elem x params grad_y grad_grad_x {_TABLE} grad_grad_y grad_params grad_x stream",
    "nfa_hashgrid_bwd_sorted_i": f"interp elem x params grad_y {_TABLE} grad_params grad_x scratch scratch_bytes stream",
    "nfa_hashgrid_bwd_bwd_sorted_i": f"interp elem x params grad_y grad_grad_x {_TABLE} grad_grad_y grad_params grad_x scratch "
                                     "scratch_bytes stream",
}
_SCALARS = {"interp": 1, "elem": 0, "n_points": 16, "n_levels": 2, "n_features": 1, "log2": 10, "scales": _SCALES,
            "res": _RES, "sizes": _SIZES, "n_params": 1088, "scratch_bytes": 1 << 20}


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    all_null = kw.pop("all_null", False)
    args = [kw[a] if a in kw else _SCALARS[a] if a in _SCALARS else (None if all_null or a == "stream" else P)
            for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
    return getattr(lib, fn)(*args), lib.nfa_last_error()


@pytest.mark.parametrize("fn", list(_ARGS))
def test_unknown_interp_is_rejected(fn):
    from nerfacc_amd import _backend as B
    lib = B.load()
    nm = fn[len("nfa_"):-len("_i")]
    for bad in (2, -1, 7):
        rc, err = _call(lib, fn, interp=bad)
        assert rc == -1 and err == f"{nm}: interp must be NFA_INTERP_LINEAR (0) or NFA_INTERP_SMOOTHSTEP (1) (got {bad})".encode()
        rc, err = _call(lib, fn, interp=bad, elem=9, n_points=-1)          # checked before every other argument
        assert rc == -1 and b"interp must be" in err
    for ok in (0, 1):
        # a known interpolation goes on to the other argument checks, and an empty input is accepted with no pointer at all
        rc, err = _call(lib, fn, interp=ok, n_features=3)
        assert rc == -1 and err == f"{nm}: n_features must be 1, 2, 4 or 8 (got 3)".encode()
        rc, err = _call(lib, fn, interp=ok, elem=3)
        assert rc == -1 and b"elem must be" in err
        rc, err = _call(lib, fn, interp=ok, n_points=0, all_null=True)
        assert rc == 0, err


def test_symbols_in_library_and_header():
    from nerfacc_amd import _backend as B
    lib = B.load()
    hdr = open(os.path.join(ROOT, "include", "nerfacc_hip.h")).read()
    assert re.search(r"#define\s+NFA_INTERP_LINEAR\s+0\b", hdr) and re.search(r"#define\s+NFA_INTERP_SMOOTHSTEP\s+1\b", hdr)
    assert B.INTERP_CODES == {"Linear": 0, "Smoothstep": 1}
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for fn, names in _ARGS.items():
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        general = fn[:-2] if "sorted" in fn else fn[:-2] + "_t"       # the most general existing entry, plus the interp
        assert B._SIGS[fn] == [ctypes.c_int32] + B._SIGS[general] and len(B._SIGS[fn]) == len(names.split())
        decl = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)", hdr)
        assert decl is not None and len(decl.group(1).split(",")) == len(names.split())
    assert lib.nfa_version() == B.ABI_VERSION == 403                  # additions only: no existing entry changed


# ----------------------------------------------------------------------------- the numpy restatement of the sorted path
@pytest.mark.parametrize("kind", ["F2_odd_res", "collide", "same_point"])
@pytest.mark.parametrize("order", [1, 2])
def test_sorted_restatement_within_bound_of_float64(kind, order):
    n = 65 if kind == "F2_odd_res" else 4097
    enc = R.make_grid(kind)
    x, g, v = R.make_inputs(kind, n, enc)
    grad, info = R.sorted_table_grad(x.numpy(), enc, g.numpy(), v.numpy() if order == 2 else None)
    F = enc.n_features_per_level
    assert grad.dtype == np.float32 and grad.shape == (enc.params.numel(),)
    assert int(info["cnt"].sum()) == 8 * n * enc.n_levels
    R.check_bound(grad, info, F, 2 if order == 1 else 8)
    # its float64 sums are those of the float64 restatement
    r = R.restate(x, enc.params.detach(), enc, g, v)
    want = r["g_params" if order == 1 else "g2_params"].view(-1, F)[info["entry"]]
    # (at second order its u_d = (c_d ? v_d : -v_d) * S'_d is the rounded float32 product: one rounding per term apart)
    err = np.abs(info["sum64"] - want.numpy())
    assert np.all(err <= (2.0 ** -23 if order == 2 else 1e-12) * info["abs64"]), float(err.max())
    if kind == "same_point":
        assert int(info["cnt"].min()) == 4097                         # every run crosses tile borders
    # and it is not the linear gradient
    import hashgrid_sorted_reference as RL
    lin, _ = RL.sorted_table_grad(x.numpy(), enc, g.numpy(), v.numpy() if order == 2 else None)
    assert not np.array_equal(lin, grad)

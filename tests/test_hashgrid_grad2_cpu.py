"""CPU: the hash grid's second order -- the float64 restatement of tests/hashgrid2_reference.py against autograd's own double
backward of the float64 torch path, gradgradcheck of HashGridEncoding, and the argument checks and symbols of
nfa_hashgrid_bwd_bwd / nfa_hashgrid_bwd_bwd_t."""
import ctypes
import os
import re

import torch

from conftest import ROOT
from hashgrid2_reference import interior_points, restate_grad2


def test_restatement_matches_autograd_double_backward():
    """Levels 3, 15 and 63 cells wide (dense, hashed, hashed) and coordinates that are multiples of 2^-12: x * scale + 0.5 is
    exact in float32, so the float32 cells and fractions of the restatement are those of the float64 torch path."""
    from nerfacc_amd.encodings import HashGridEncoding, _hashgrid_torch
    torch.manual_seed(0)
    for F in (1, 2, 4):
        enc = HashGridEncoding(3, n_levels=3, n_features_per_level=F, log2_hashmap_size=10, base_resolution=4,
                               per_level_scale=4.0)
        assert enc.scales == [3.0, 15.0, 63.0] and enc.table.hashed == [False, True, True]
        x = interior_points(200, enc, seed=F, lo=-0.25, hi=1.25, grid=4096.0)
        for s in enc.scales:
            assert torch.equal((x * s + 0.5).double(), x.double() * s + 0.5)
        params = torch.rand(enc.params.numel(), dtype=torch.float64) * 2 - 1
        g = torch.randn(x.shape[0], enc.n_output_dims, dtype=torch.float64)
        v = torch.randn(x.shape[0], 3, dtype=torch.float64)

        x64 = x.double().requires_grad_(True)
        p64 = params.clone().requires_grad_(True)
        g64 = g.clone().requires_grad_(True)
        y = _hashgrid_torch(x64, p64, enc.table, F)
        (g_x,) = torch.autograd.grad(y, x64, g64, create_graph=True)
        x2, g2_p, gg_y = torch.autograd.grad(g_x, (x64, p64, g64), v)

        r = restate_grad2(x, params, enc, g, v)
        torch.testing.assert_close(r["gg_y"], gg_y, rtol=1e-10, atol=1e-10 * float(gg_y.abs().mean()))
        torch.testing.assert_close(r["g2_params"], g2_p, rtol=1e-10, atol=1e-10 * float(g2_p.abs().max()))
        torch.testing.assert_close(r["x2"], x2, rtol=1e-10, atol=1e-10 * float(x2.abs().mean()))
        # the term counts and magnitudes: 24 per gg_y element, 3 per touching corner, 16 L F per x2 element
        assert bool((r["gg_y_k"] == 24).all()) and bool((r["x2_k"] == 16 * 3 * F).all())
        assert float(r["hits"].sum()) == 8 * 3 * x.shape[0]
        assert torch.equal(r["g2_params_k"].view(-1, F)[:, 0], 3 * r["hits"])
        for name in ("gg_y", "g2_params", "x2"):
            assert bool((r[name].abs() <= r[name + "_abs"] * (1 + 1e-12)).all())


def test_gradgradcheck_hashgrid_encoding():
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(1)
    enc = HashGridEncoding(3, n_levels=2, n_features_per_level=2, log2_hashmap_size=10, base_resolution=4,
                           per_level_scale=3.0).double()
    assert enc.table.hashed == [False, True]
    x = interior_points(6, enc, seed=2).double().requires_grad_(True)
    p = (torch.rand(enc.params.numel(), dtype=torch.float64) * 2 - 1).requires_grad_(True)

    def fn(x_, p_):
        return torch.func.functional_call(enc, {"params": p_}, (x_,))

    assert torch.autograd.gradgradcheck(fn, (x, p), eps=1e-6, atol=1e-5)


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
# a 2-level table: res 4 (dense, 64 entries) and res 12 (hashed, 2^10 entries), F = 1  (tests/test_encodings_cpu.py)
_SCALES = (ctypes.c_float * 2)(3.0, 11.0)
_RES = (ctypes.c_int32 * 2)(4, 12)
_SIZES = (ctypes.c_int32 * 2)(64, 1024)
_BAD_SIZES = (ctypes.c_int32 * 2)(64, 1000)
_NAMES = "x params grad_y grad_grad_x n_points n_levels n_features log2 scales res sizes n_params grad_grad_y grad_params grad_x stream"
_ARGS = {"nfa_hashgrid_bwd_bwd": _NAMES, "nfa_hashgrid_bwd_bwd_t": "elem " + _NAMES}
_SCALARS = {"elem": 0, "n_points": 16, "n_levels": 2, "n_features": 1, "log2": 10, "scales": _SCALES, "res": _RES,
            "sizes": _SIZES, "n_params": 1088}


def _cases():
    cases = []
    nm = "hashgrid_bwd_bwd"
    for fn in _ARGS:
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
            (fn, {"n_points": 0, "all_null": True}, None),
            (fn, {"grad_grad_x": None}, f"{nm}: grad_grad_x is null"),
            (fn, {"grad_grad_y": None, "grad_params": None, "grad_x": None}, f"{nm}: no output requested"),
            (fn, {"x": None}, f"{nm}: null pointer"),
            (fn, {"params": None}, f"{nm}: null pointer"),                             # gg_y and x2 read the corners
            (fn, {"params": None, "grad_params": None}, f"{nm}: null pointer"),
            (fn, {"grad_y": None}, f"{nm}: null pointer"),                             # G2_T and x2 read dL/dy
            (fn, {"grad_y": None, "grad_grad_y": None}, f"{nm}: null pointer"),
        ]
    t = "nfa_hashgrid_bwd_bwd_t"
    cases += [
        (t, {"elem": 3}, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)"),
        (t, {"elem": 1, "grad_y": P + 8}, f"{nm}: half grad_y and grad_grad_y must be 16-byte aligned"),
        (t, {"elem": 2, "grad_grad_y": P + 2}, f"{nm}: half grad_y and grad_grad_y must be 16-byte aligned"),
    ]
    return cases


def test_bwd_bwd_argument_errors():
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


def test_symbols_in_library_and_header():
    from nerfacc_amd import _backend as B
    lib = B.load()
    hdr = open(os.path.join(ROOT, "include", "nerfacc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for fn, n_args in (("nfa_hashgrid_bwd_bwd", 16), ("nfa_hashgrid_bwd_bwd_t", 17)):
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        assert len(B._SIGS[fn]) == n_args == len(_ARGS[fn].split())
        decl = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)", hdr)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
    assert re.search(r"#define\s+NFA_VERSION\s+403\b", hdr) and lib.nfa_version() == 403

"""CPU: the hash grid's reproducible (sorted) table gradient -- the float32 restatement of tests/hashgrid_sorted_reference.py
against the float64 sum within the project's derived bound, the ``deterministic`` keyword on the torch path, the scratch
formula, and the argument checks of nfa_hashgrid_bwd_sorted / nfa_hashgrid_bwd_bwd_sorted (no device needed).

The bound, per table entry that received cnt contributions: (cnt + 2) * 2^-23 * sum|term| at first order, (cnt + 8) * 2^-23 *
sum|term| at second order (tests/test_encodings_gpu.py, tests/test_hashgrid_grad2_gpu.py): each term is a product of at most
three / six float32 roundings and each of the cnt additions adds at most 2^-24 of a running sum that sum|term| bounds; the
bound is twice that worst case and holds for any order of float32 additions."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import hashgrid_sorted_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["F1_L1", "F1_L32", "F8_L7_edge", "F2_odd_res", "density", "collide", "same_point", "top_digit"]


@functools.lru_cache(maxsize=None)
def _grid(kind):
    return R.make_grid(kind)


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_within_bound_of_float64(kind, n):
    enc = _grid(kind)
    x, g, v = R.make_inputs(kind, n, enc)
    F = enc.n_features_per_level
    for second, extra in ((None, 2), (v.numpy(), 8)):
        grad, info = R.sorted_table_grad(x.numpy(), enc, g.numpy(), second)
        assert int(info["cnt"].sum()) == 8 * n * enc.n_levels
        R.check_bound(grad, info, F, extra)
    if kind == "same_point":
        assert info["entry"].size == 8 * enc.n_levels and bool((info["cnt"] == n).all())
    if kind == "collide" and n == 4097:
        assert info["entry"].size == 2048 and int(info["cnt"].max()) > 32     # every entry of both levels, long lists


def test_restatement_first_order_matches_autograd():
    """The float64 sum of the restatement is the table gradient autograd gives for the float64 torch path."""
    from nerfacc_amd.encodings import _hashgrid_torch
    enc = _grid("F2_odd_res")
    x, g, _ = R.make_inputs("F2_odd_res", 65, enc)
    from hashgrid2_reference import interior_points
    x = interior_points(65, enc, seed=3)                   # boundary-free: the float32 and float64 cells coincide
    p64 = enc.params.detach().double().requires_grad_(True)
    y = _hashgrid_torch(x.double(), p64, enc.table, enc.n_features_per_level)
    (want,) = torch.autograd.grad(y, p64, g.double())
    _, info = R.sorted_table_grad(x.numpy(), enc, g.numpy())
    got = np.zeros((enc.table.n_entries, enc.n_features_per_level))
    got[info["entry"]] = info["sum64"]
    np.testing.assert_allclose(got.reshape(-1), want.numpy(), rtol=0, atol=1e-4)   # f differs by 2^-24 p between the float32 and float64 cells


def test_deterministic_flag_changes_nothing_on_the_torch_path():
    outs = []
    for det in (False, True):
        enc = R.make_grid("density", deterministic=det)
        x, g, _ = R.make_inputs("density", 65, enc)
        x = x.requires_grad_(True)
        y = enc(x)
        y.backward(g)
        outs.append((y.detach(), x.grad, enc.params.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_keyword_repr_and_tcnn_config():
    from nerfacc_amd.encodings import HashGridEncoding, encoding_from_tcnn_config
    assert HashGridEncoding(3, 2, 2, 10).deterministic is False
    assert "deterministic" not in repr(HashGridEncoding(3, 2, 2, 10))
    assert "deterministic=True" in repr(HashGridEncoding(3, 2, 2, 10, deterministic=True))
    cfg = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 16}
    assert encoding_from_tcnn_config(3, cfg).deterministic is False
    assert encoding_from_tcnn_config(3, cfg, deterministic=True).deterministic is True
    assert encoding_from_tcnn_config(3, {"otype": "Composite", "nested": [cfg]}, None, True).deterministic is True
    sh = encoding_from_tcnn_config(3, {"otype": "SphericalHarmonics", "degree": 2}, deterministic=True)
    assert not hasattr(sh, "deterministic")


def test_id_limit_raises_without_allocating():
    from nerfacc_amd import encodings as E
    enc = E.HashGridEncoding(3, 2, 2, 10, deterministic=True)
    assert E.SORTED_MAX_POINTS == (1 << 29) - 1
    with pytest.raises(ValueError, match="2\\^29 - 1"):
        E._sorted_scratch(enc, 1 << 29, "meta")
    assert E._sorted_scratch(enc, 65, "meta").numel() == R.scratch_bytes(65, 2)


def test_scratch_bytes():
    from nerfacc_amd import _backend as B
    f = B.load().nfa_hashgrid_sorted_scratch_bytes
    assert f(0, 16, 19) == 0 and f(-1, 16, 19) == 0
    last = 0
    for n in (1, 2, 63, 64, 65, 511, 512, 513, 4097, 1 << 18, (1 << 18) + 1, 1 << 20, 1 << 24, (1 << 29) - 1):
        for L in (1, 5, 16, 32):
            assert f(n, L, 19) == R.scratch_bytes(n, L), (n, L)
            assert f(n, L, 19) == f(n, L, 10)
        assert f(n, 16, 19) >= last                                  # monotone in n_points
        last = f(n, 16, 19)
    # the levels are sorted in groups: the total stays at 2^29 as long as one level fits
    assert f(1 << 20, 16, 19) == f(1 << 20, 32, 19) == 1 << 29 and f(1 << 20, 3, 19) < 1 << 29
    assert f(1 << 24, 16, 19) == f(1 << 24, 1, 19) > 1 << 29        # one level alone is over the budget: one at a time
    assert f(1000, 2, 19) == 2 * f(1000, 1, 19)


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_SCALES = (ctypes.c_float * 2)(3.0, 11.0)
_RES = (ctypes.c_int32 * 2)(4, 12)
_SIZES = (ctypes.c_int32 * 2)(64, 1024)
_BAD_SIZES = (ctypes.c_int32 * 2)(64, 1000)
_B1 = "elem x params grad_y n_points n_levels n_features log2 scales res sizes n_params grad_params grad_x scratch scratch_bytes stream"
_B2 = ("elem x params grad_y grad_grad_x n_points n_levels n_features log2 scales res sizes n_params grad_grad_y grad_params "
       "grad_x scratch scratch_bytes stream")
_ARGS = {"nfa_hashgrid_bwd_sorted": _B1, "nfa_hashgrid_bwd_bwd_sorted": _B2}
_SCALARS = {"elem": 0, "n_points": 16, "n_levels": 2, "n_features": 1, "log2": 10, "scales": _SCALES, "res": _RES,
            "sizes": _SIZES, "n_params": 1088, "scratch_bytes": 1 << 20}


def _cases():
    cases = []
    need = R.scratch_bytes(16, 2)
    for fn, nm in (("nfa_hashgrid_bwd_sorted", "hashgrid_bwd_sorted"), ("nfa_hashgrid_bwd_bwd_sorted", "hashgrid_bwd_bwd_sorted")):
        cases += [
            (fn, {"n_points": -1}, f"{nm}: negative size"),
            (fn, {"n_features": 3}, f"{nm}: n_features must be 1, 2, 4 or 8 (got 3)"),
            (fn, {"n_levels": 33}, f"{nm}: n_levels must be in 1..32 (got 33)"),
            (fn, {"log2": 9}, f"{nm}: log2_hashmap_size must be in 10..24 (got 9)"),
            (fn, {"sizes": _BAD_SIZES}, f"{nm}: level 1 size 1000 is not min(roundup8(res^3), 2^10)"),
            (fn, {"n_params": 1089}, f"{nm}: n_params 1089 != 1088 entries x 1 features"),
            (fn, {"n_points": 0, "all_null": True}, None),
            (fn, {"n_points": 0}, None),                                               # returns before it looks at a pointer
            (fn, {"x": None}, f"{nm}: null pointer"),
            (fn, {"grad_y": None}, f"{nm}: null pointer"),
            (fn, {"params": None}, f"{nm}: null pointer"),
            (fn, {"scratch": None}, f"{nm}: scratch is null (a table gradient needs nfa_hashgrid_sorted_scratch_bytes bytes)"),
            (fn, {"scratch": P + 4}, f"{nm}: scratch must be 16-byte aligned"),
            (fn, {"scratch_bytes": need - 1}, f"{nm}: scratch too small ({need - 1} bytes, {need} needed)"),
            (fn, {"scratch_bytes": 0}, f"{nm}: scratch too small (0 bytes, {need} needed)"),
            (fn, {"n_points": 1 << 29}, f"{nm}: 8 * n_points must be below 2^32 (got n_points {1 << 29})"),
            (fn, {"elem": 3}, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)"),
            (fn, {"elem": -1}, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got -1)"),
        ]
    cases += [
        ("nfa_hashgrid_bwd_sorted", {"elem": 1, "grad_y": P + 8}, "hashgrid_bwd_sorted: a half grad_y must be 16-byte aligned"),
        ("nfa_hashgrid_bwd_sorted", {"elem": 2, "grad_y": P + 2}, "hashgrid_bwd_sorted: a half grad_y must be 16-byte aligned"),
        ("nfa_hashgrid_bwd_bwd_sorted", {"grad_grad_x": None}, "hashgrid_bwd_bwd_sorted: grad_grad_x is null"),
        ("nfa_hashgrid_bwd_bwd_sorted", {"elem": 1, "grad_y": P + 8},
         "hashgrid_bwd_bwd_sorted: half grad_y and grad_grad_y must be 16-byte aligned"),
        ("nfa_hashgrid_bwd_bwd_sorted", {"elem": 2, "grad_grad_y": P + 2},
         "hashgrid_bwd_bwd_sorted: half grad_y and grad_grad_y must be 16-byte aligned"),
        # without grad_params the entries are the existing ones, errors included, and scratch is not looked at
        ("nfa_hashgrid_bwd_sorted", {"grad_params": None, "grad_x": None, "scratch": None}, "hashgrid_bwd: null pointer"),
        ("nfa_hashgrid_bwd_bwd_sorted", {"grad_params": None, "grad_x": None, "grad_grad_y": None, "scratch": None},
         "hashgrid_bwd_bwd: no output requested"),
    ]
    return cases


def test_sorted_argument_errors():
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
    for fn, n_args, ret in (("nfa_hashgrid_sorted_scratch_bytes", 3, "int64_t"), ("nfa_hashgrid_bwd_sorted", 17, "int"),
                            ("nfa_hashgrid_bwd_bwd_sorted", 19, "int")):
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        assert len(B._SIGS[fn]) == n_args
        decl = re.search(r"\b" + ret + r"\s+" + fn + r"\s*\(([^)]*)\)", hdr)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
    assert len(_B1.split()) == 17 and len(_B2.split()) == 19
    assert lib.nfa_version() == B.ABI_VERSION

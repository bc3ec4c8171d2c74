"""CPU: the ``table_gradient`` keyword of the hash grid (its values, ``extra_repr``, the torch path, ``encoding_from_tcnn_config``
and the two NGP fields) and the argument checks of nfa_hashgrid_bwd_merged, which are decided on the host before any launch."""
import ctypes

import pytest
import torch

import hashgrid_sorted_reference as R
from nerfacc_amd.encodings import HashGridEncoding, encoding_from_tcnn_config


def test_keyword():
    from nerfacc_amd.fields import NGPDensityField, NGPRadianceField
    assert HashGridEncoding(3, 2, 2, 10).table_gradient == "atomic" and "table_gradient" not in repr(HashGridEncoding(3, 2, 2, 10))
    assert "table_gradient=merged" in repr(HashGridEncoding(3, 2, 2, 10, table_gradient="Merged"))   # case-insensitive, shown lowered
    for kw, msg in (({"table_gradient": "sorted"}, "must be 'atomic' or 'merged'"), ({"table_gradient": None}, "must be 'atomic' or 'merged'"),
                    ({"table_gradient": "merged", "deterministic": True}, "not reproducible")):
        with pytest.raises(ValueError, match=msg):
            HashGridEncoding(3, 2, 2, 10, **kw)
    cfg = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 16}
    assert encoding_from_tcnn_config(3, {"otype": "Composite", "nested": [cfg]}, table_gradient="merged").table_gradient == "merged"
    for cls in (NGPRadianceField, NGPDensityField):
        kw = dict(aabb=[0.0, 0.0, 0.0, 1.0, 1.0, 1.0], n_levels=2, log2_hashmap_size=10, max_resolution=32)
        field = cls(table_gradient="merged", fused_training=True, **kw)
        assert field.encoding.table_gradient == "merged" and cls(**kw).encoding.table_gradient == "atomic"
        assert not field._use_train(False, torch.zeros(4, 3))       # a query with grad takes the composed chain


def test_torch_path_ignores_the_keyword():
    outs = []
    for tg in ("atomic", "merged"):
        torch.manual_seed(0)
        enc = HashGridEncoding(3, *R.configs()["density"], table_gradient=tg)
        x, g, _ = R.make_inputs("density", 65, enc)
        outs.append(torch.autograd.grad(enc(x.requires_grad_(True)), (x, enc.params), g))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


P, _I32 = 0x1000, ctypes.c_int32 * 2   # P: a stand-in address that is never dereferenced
_NAMES = "n_dims interp elem x grad_y n_points n_levels n_features log2 scales res sizes n_params grad_params stream".split()
_OK = {"n_dims": 3, "interp": 0, "elem": 0, "n_points": 16, "n_levels": 2, "n_features": 1, "log2": 10,
       "scales": (ctypes.c_float * 2)(3.0, 11.0), "res": _I32(4, 12), "sizes": _I32(64, 1024), "n_params": 1088}
CASES = [
    ({"x": None}, "null pointer"), ({"grad_y": None}, "null pointer"), ({"grad_params": None}, "null pointer"),
    ({"n_dims": 5}, "n_dims must be 2, 3 or 4 (got 5)"), ({"n_points": -1}, "negative size"),
    ({"interp": 2}, "interp must be NFA_INTERP_LINEAR (0) or NFA_INTERP_SMOOTHSTEP (1) (got 2)"),
    ({"elem": 3}, "elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)"),
    ({"elem": 1, "grad_y": P + 8}, "a half grad_y must be 16-byte aligned"), ({"elem": 2, "grad_y": P + 2}, "a half grad_y must be 16-byte aligned"),
    ({"n_dims": 2, "x": P + 8, "sizes": _I32(16, 144), "n_params": 160}, "x must be 16-byte aligned at n_dims 2"),
    ({"sizes": _I32(64, 1000)}, "level 1 size 1000 is not min(roundup8(res^3), 2^10)"), ({"n_params": 1089}, "n_params 1089 != 1088 entries x 1 features"),
    ({"n_points": 0}, None), ({"n_points": 0, "x": None, "grad_y": None, "grad_params": None}, None),
]


@pytest.mark.parametrize("kw,msg", CASES, ids=[str(i) for i in range(len(CASES))])
def test_argument_errors(kw, msg):
    from nerfacc_amd import _backend as B
    lib = B.load()
    args = [kw[a] if a in kw else _OK[a] if a in _OK else (None if a == "stream" else P) for a in _NAMES]
    assert len(args) == len(B._SIGS["nfa_hashgrid_bwd_merged"])
    lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
    rc = lib.nfa_hashgrid_bwd_merged(*args)
    assert (rc == 0) if msg is None else (rc == -1 and lib.nfa_last_error().decode() == "hashgrid_bwd_merged: " + msg), (rc, lib.nfa_last_error())

"""CPU: the plane regularisers of nerfacc_amd.losses -- the torch path of ``plane_terms`` and the float32 restatement of the
native gradient against the float64 slicing form of tests/planereg_reference.py, ``plane_regularization``'s weighting, the C
entries' argument checks (stand-in pointers, no device) and the pins the addition must not move."""
import ctypes

import pytest
import torch

import planereg_reference as R


def _enc(res, ms, F, params=None):
    from nerfacc_amd.encodings import PlaneGridEncoding
    enc = PlaneGridEncoding(len(res), res, ms, n_features=F)
    with torch.no_grad():
        enc.params.copy_(R.make_params(res, ms, F) if params is None else params)
    return enc


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


SHAPES = [(res, ms, F) for _, res, ms in R.CASES for F in R.FEATURES]


# ----------------------------------------------------------------------------- the torch path against the reference
@pytest.mark.parametrize("res,ms,F", SHAPES)
def test_torch_path_values_and_gradient(res, ms, F):
    from nerfacc_amd.losses import plane_terms
    p, g, ref, ref_gp = R.case(res, ms, F)
    enc = _enc(res, ms, F, p)
    got = plane_terms(enc)
    assert got.shape == (len(ms), len(enc.planes), 4) and got.dtype == torch.float32 and got.device == enc.params.device
    torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=0.0)
    for k, (a, b) in enumerate(enc.planes):          # a spatial plane has no smoothness and no L1 term: exactly 0
        if b != 3:
            assert (got[:, k, 2:] == 0).all()
        else:
            assert (got[:, k, 3] > 0).all()
    (gp,) = torch.autograd.grad(got, enc.params, g)
    torch.testing.assert_close(gp.double(), ref_gp, **_tol(ref_gp))


def test_two_time_nodes_have_no_smoothness():
    from nerfacc_amd.losses import plane_terms
    res, ms, F = (5, 4, 3, 2), (1, 2), 4
    enc = _enc(res, ms, F)
    terms = plane_terms(enc)
    assert (terms[:, :, 2] == 0).all()
    (gp,) = torch.autograd.grad(terms[:, :, 2].sum() + terms.sum(), enc.params)
    assert torch.isfinite(gp).all()
    (gs,) = torch.autograd.grad(plane_terms(enc)[:, :, 2].sum(), enc.params, allow_unused=True)
    assert gs is None or (gs == 0).all()


def test_other_dtypes_take_the_torch_path():
    from nerfacc_amd.losses import plane_terms
    res, ms, F = (5, 4, 3, 4), (1, 2), 4
    p, _, ref, _ = R.case(res, ms, F)
    enc = _enc(res, ms, F, p).double()
    got = plane_terms(enc)
    assert got.dtype == torch.float32
    torch.testing.assert_close(got.double(), ref, rtol=1e-6, atol=0.0)


def test_torch_path_differentiates_twice():
    from nerfacc_amd.losses import plane_terms
    enc = _enc((5, 4, 3, 4), (1,), 4)
    (gp,) = torch.autograd.grad(plane_terms(enc).sum(), enc.params, create_graph=True)
    (ggp,) = torch.autograd.grad((gp * gp).sum(), enc.params)
    assert torch.isfinite(ggp).all() and ggp.abs().sum() > 0


# ----------------------------------------------------------------------------- plane_regularization
def test_regularization_is_the_weighted_sum():
    from nerfacc_amd.losses import plane_regularization, plane_terms
    res, ms, F = (5, 4, 3, 5), (1, 2), 4
    enc = _enc(res, ms, F)
    t = plane_terms(enc).detach().double()
    time = torch.tensor([b == 3 for _, b in enc.planes])
    tv_s, tv_t = (t[:, ~time, 0] + t[:, ~time, 1]).sum(), (t[:, time, 0] + t[:, time, 1]).sum()
    sm, l1 = t[:, time, 2].sum(), t[:, time, 3].sum()
    got = plane_regularization(enc, tv=0.3, tv_time=0.7, time_smoothness=0.11, l1_time=0.05)
    assert got.shape == () and got.dtype == torch.float32
    torch.testing.assert_close(got.double(), 0.3 * tv_s + 0.7 * tv_t + 0.11 * sm + 0.05 * l1, rtol=1e-5, atol=0.0)
    # tv_time=None means tv
    torch.testing.assert_close(plane_regularization(enc, tv=0.3).double(), 0.3 * (tv_s + tv_t), rtol=1e-5, atol=0.0)
    assert torch.equal(plane_regularization(enc, tv=0.3), plane_regularization(enc, tv=0.3, tv_time=0.3))
    # K-Planes' PlaneTV(w): the spatial planes twice, 2 (tv_h + tv_w) per plane
    w = 0.01
    per_plane = 2.0 * (t[:, :, 0] + t[:, :, 1])
    plane_tv = w * (2.0 * per_plane[:, ~time].sum() + per_plane[:, time].sum())
    torch.testing.assert_close(plane_regularization(enc, tv=4 * w, tv_time=2 * w).double(), plane_tv, rtol=1e-5, atol=0.0)
    # differentiable, and the default is nothing at all
    plane_regularization(enc, tv=1.0, time_smoothness=1.0, l1_time=1.0).backward()
    assert torch.isfinite(enc.params.grad).all() and enc.params.grad.abs().sum() > 0
    assert float(plane_regularization(enc).detach()) == 0.0


def test_regularization_weights_are_built_once():
    from nerfacc_amd import losses
    enc = _enc((5, 4, 3, 5), (1, 2), 4)
    losses.plane_regularization(enc, tv=0.25, l1_time=0.5)
    n = len(losses._REG_WEIGHTS)
    w = losses._reg_weights(enc, 0.25, 0.25, 0.0, 0.5)
    losses.plane_regularization(enc, tv=0.25, l1_time=0.5)
    assert len(losses._REG_WEIGHTS) == n and losses._reg_weights(enc, 0.25, 0.25, 0.0, 0.5) is w
    assert w.shape == (2, 6, 4) and w[0, 0].tolist() == [0.25, 0.25, 0.0, 0.0] and w[1, 5].tolist() == [0.25, 0.25, 0.0, 0.5]


def test_smoothness_needs_three_time_nodes():
    from nerfacc_amd.losses import plane_regularization
    enc = _enc((5, 4, 3, 2), (1, 2), 4)
    with pytest.raises(ValueError, match="time_smoothness needs at least 3 nodes"):
        plane_regularization(enc, tv=1.0, time_smoothness=0.1)
    assert torch.isfinite(plane_regularization(enc, tv=1.0, l1_time=1.0))
    tri = _enc((6, 5, 4), (1,), 4)                     # no time axis: the time weights are ignored
    assert torch.equal(plane_regularization(tri, tv=1.0, time_smoothness=0.1, l1_time=3.0), plane_regularization(tri, tv=1.0))


# ----------------------------------------------------------------------------- the float32 restatement of the native gradient
@pytest.mark.parametrize("res,ms,F", SHAPES)
def test_gradient_restatement_against_float64_autograd(res, ms, F):
    from nerfacc_amd.losses import _plane_terms_grad_torch
    p, g, _, ref_gp = R.case(res, ms, F)
    enc = _enc(res, ms, F, p)
    got = _plane_terms_grad_torch(p, g, enc.table)
    assert got.dtype == torch.float32 and got.shape == p.shape
    torch.testing.assert_close(got.double(), ref_gp, **_tol(ref_gp))
    # p == 1 exactly: the L1 term contributes nothing there
    only_l1 = torch.zeros_like(g)
    only_l1[:, :, 3] = 1.0
    got = _plane_terms_grad_torch(p, only_l1, enc.table)
    assert (got[p == 1.0] == 0).all() and (p == 1.0).any()


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_planereg_partials": "n_dims n_scales n_features res",
    "nfa_planereg_fwd": "n_dims params n_scales n_features res partials n_partials terms stream",
    "nfa_planereg_bwd": "n_dims params n_scales n_features res grad_terms grad_params stream",
}


def _res(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    base = {"n_dims": 3, "n_scales": 2, "n_features": 4, "res": _res(5, 7, 4, 10, 14, 8), "n_partials": 0, "stream": None}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


def test_c_abi_argument_errors():
    """Every check in its documented order with its text.  No case reaches a launch: a call that passes every other check
    ends at n_partials (0 here), the last one; nfa_planereg_bwd has no such check, so each of its cases carries a fault."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert lib.nfa_version() == 403 and B.ABI_VERSION == 403
    assert [len(B._SIGS[fn]) for fn in _ARGS] == [4, 9, 8]
    assert B._RESTYPES["nfa_planereg_partials"] == ctypes.c_int64
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        for bad in (2, 5):
            assert _call(lib, fn, n_dims=bad) == (-1, f"{nm}: n_dims must be 3 or 4 (got {bad})")
        for bad in (2, 12, 64):
            assert _call(lib, fn, n_features=bad) == (-1, f"{nm}: n_features must be 4, 8, 16 or 32 (got {bad})")
        for bad in (0, 9):
            assert _call(lib, fn, n_scales=bad) == (-1, f"{nm}: n_scales must be in 1..8 (got {bad})")
        assert _call(lib, fn, res=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 7, 4, 10, 1, 8)) == (-1, f"{nm}: scale 1 axis 1 resolution 1 is below 2")
        big = _res(1 << 13, 1 << 13, 1 << 13, 2, 2, 2)
        assert _call(lib, fn, n_features=32, res=big) == (-1, f"{nm}: too many parameters (at most 2^31 - 1 floats)")
        # the order is fixed: the first failing check speaks
        assert _call(lib, fn, n_dims=5, n_features=5, n_scales=0, res=None)[1] == f"{nm}: n_dims must be 3 or 4 (got 5)"
        assert _call(lib, fn, n_features=5, n_scales=0, res=None)[1].startswith(f"{nm}: n_features must be")
        assert _call(lib, fn, n_scales=0, res=None, params=None)[1].startswith(f"{nm}: n_scales must be")
        assert _call(lib, fn, res=None, params=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 7, 4, 10, 1, 8), params=None)[1].endswith("is below 2")
    for fn, ptrs in (("nfa_planereg_fwd", "params partials terms"), ("nfa_planereg_bwd", "params grad_terms grad_params")):
        nm = fn[len("nfa_"):]
        for name in ptrs.split():
            assert _call(lib, fn, **{name: None}) == (-1, f"{nm}: null pointer")
            if name != "params":                        # a null pointer speaks before the alignment
                assert _call(lib, fn, **{name: None, "params": P + 4}) == (-1, f"{nm}: null pointer")
    assert _call(lib, "nfa_planereg_fwd", params=P + 4) == (-1, "planereg_fwd: params, partials and terms must be 16-byte aligned")
    assert _call(lib, "nfa_planereg_fwd", terms=P + 8, n_partials=-1)[1] == "planereg_fwd: params, partials and terms must be 16-byte aligned"
    assert _call(lib, "nfa_planereg_bwd", params=P + 4) == (-1, "planereg_bwd: params and grad_params must be 16-byte aligned")
    assert _call(lib, "nfa_planereg_bwd", grad_params=P + 12) == (-1, "planereg_bwd: params and grad_params must be 16-byte aligned")
    need = lib.nfa_planereg_partials(3, 2, 4, _res(5, 7, 4, 10, 14, 8))
    assert need == 6                                    # 3 planes per scale of at most 16 rows by 256 quads: one tile each
    assert _call(lib, "nfa_planereg_fwd", n_partials=need - 1) == (-1, f"planereg_fwd: n_partials is below nfa_planereg_partials ({need - 1} < {need})")


def test_partial_rows_follow_the_shape():
    """nfa_planereg_partials: ceil(H / 16) * ceil(W F / 1024) tiles per plane, summed; -1 for a refused shape."""
    from nerfacc_amd import _backend as B
    lib = B.load()

    def tiles(D, res, ms, F):
        import itertools
        return sum(-(-r[b] // 16) * -(-r[a] * F // 1024) for r in R.scale_resolutions(res, ms) for a, b in itertools.combinations(range(D), 2))

    for D, res, ms, F in [(4, (70, 33, 9, 11), (1, 2), 8), (4, (64, 64, 64, 150), (1, 2, 4, 8), 32), (3, (6, 5, 4), (1, 2), 4)]:
        flat = [v for r in R.scale_resolutions(res, ms) for v in r]
        assert lib.nfa_planereg_partials(D, len(ms), F, _res(*flat)) == tiles(D, res, ms, F)
    assert lib.nfa_planereg_partials(5, 1, 4, _res(4, 4, 4, 4, 4)) == -1
    assert lib.nfa_last_error() == b"planereg_partials: n_dims must be 3 or 4 (got 5)"


# ----------------------------------------------------------------------------- pins
def test_pins():
    import nerfacc_amd
    from nerfacc_amd import losses
    assert len(nerfacc_amd.__all__) == 22
    for name in ("plane_terms", "plane_regularization"):
        assert name in losses.__all__ and name not in nerfacc_amd.__all__
    assert "distortion" in losses.__all__

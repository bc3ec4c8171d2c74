"""CPU: the voxel-grid regularisers of nerfacc_amd.losses -- the torch path of ``voxel_terms`` and the float32 restatement of
the native gradient against the float64 form of tests/voxreg_reference.py, exact results on integer-valued tables,
``voxel_regularization``'s weighting, ``voxel_tv_add_grad_`` on CPU tensors, the wrappers' errors and the C entries' argument
checks (stand-in pointers, no device)."""
import ctypes

import pytest
import torch

import voxreg_reference as R

SHAPES = [(res, C) for res in R.RESOLUTIONS for C in R.FEATURES]


def _enc(res, C, params=None, **kw):
    from nerfacc_amd.encodings import VoxelGridEncoding
    enc = VoxelGridEncoding(res, n_features=C, **kw)
    with torch.no_grad():
        enc.params.copy_(R.make_params(res, C) if params is None else params)
    return enc


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _int_params(res, C, seed=0):
    """Small integers in -3..3: every difference, penalty and sum below is exact in float32 (far below 2^24)."""
    return torch.randint(-3, 4, (R.n_params(res, C),), generator=torch.Generator().manual_seed(seed)).float()


# ----------------------------------------------------------------------------- the torch path against the reference
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("res,C", SHAPES)
def test_torch_path_values_and_gradient_in_float64(res, C, kind, reduction):
    from nerfacc_amd.losses import _voxel_terms_torch
    p, g, ref, ref_gp = R.case(res, C, kind, 0, reduction)
    pr = p.double().requires_grad_(True)
    got = _voxel_terms_torch(pr, res, C, kind, reduction)
    assert got.shape == (4,) and got.dtype == torch.float64
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0.0)
    (gp,) = torch.autograd.grad(got, pr, g.double())
    torch.testing.assert_close(gp, ref_gp, rtol=1e-12, atol=1e-12 * float(ref_gp.abs().mean()))


def test_the_cases_exercise_the_edges():
    """Differences of exactly 0, +1 and -1 and parameters that are exactly 0 are in every case's table."""
    for res, C in SHAPES:
        p = R.make_params(res, C)
        g = p.view(res[2], res[1], res[0], C)
        assert (p == 0.0).any()
        assert ((g[1:] - g[:-1]) == 0.0).any() and ((g[:, 1:] - g[:, :-1]) == 1.0).any() and ((g[:, :, 1:] - g[:, :, :-1]) == -1.0).any()
    d = R.view(R.make_params((9, 17, 33), 4), (9, 17, 33), 4)
    d = torch.diff(d, dim=2).abs()
    assert (d > 1.0).any() and (d < 1.0).any()                        # huber's two branches


def test_voxel_terms_on_cpu_tensors():
    """float32 and float64 parameters both give float32 terms on the parameters' device, differentiable by autograd; the
    strides play no part."""
    from nerfacc_amd.losses import voxel_terms
    res, C = (5, 4, 7), 12
    for kind in R.KINDS:
        p, g, ref, ref_gp = R.case(res, C, kind)
        enc = _enc(res, C, p, strides=(1, 2))
        got = voxel_terms(enc, kind)
        assert got.shape == (4,) and got.dtype == torch.float32 and got.device == enc.params.device
        torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=0.0)
        (gp,) = torch.autograd.grad(got, enc.params, g)
        torch.testing.assert_close(gp.double(), ref_gp, **_tol(ref_gp))
        got64 = voxel_terms(enc.double(), kind)
        assert got64.dtype == torch.float32
        torch.testing.assert_close(got64.double(), ref, rtol=1e-6, atol=0.0)


def test_torch_path_differentiates_twice():
    from nerfacc_amd.losses import voxel_terms
    enc = _enc((5, 4, 7), 4)
    (gp,) = torch.autograd.grad(voxel_terms(enc).sum(), enc.params, create_graph=True)
    (ggp,) = torch.autograd.grad((gp * gp).sum(), enc.params)
    assert torch.isfinite(ggp).all() and ggp.abs().sum() > 0


# ----------------------------------------------------------------------------- the float32 restatement of the native gradient
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("res,C", SHAPES)
def test_gradient_restatement_against_float64_autograd(res, C, kind):
    """Measured worst error over these 36 cases: 5.4e-4 of the tolerance (l2 on (9, 17, 33) with C = 12)."""
    from nerfacc_amd.losses import _voxel_terms_grad_torch
    p, g, _, ref_gp = R.case(res, C, kind)
    got = _voxel_terms_grad_torch(p, g, res, C, kind, "mean")
    assert got.dtype == torch.float32 and got.shape == p.shape
    err = (got.double() - ref_gp).abs() / (1e-4 * ref_gp.abs() + 1e-3 * ref_gp.abs().mean())
    print("worst error over the tolerance", float(err.max()))
    torch.testing.assert_close(got.double(), ref_gp, **_tol(ref_gp))
    # a parameter that is exactly 0: the L1 term contributes nothing there
    got = _voxel_terms_grad_torch(p, torch.tensor([0.0, 0.0, 0.0, 1.0]), res, C, kind, "sum")
    assert torch.equal(got, torch.sign(p))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("res,C", [((5, 4, 7), 1), ((5, 4, 7), 2), ((9, 17, 33), 12)])
def test_integer_valued_tables_are_exact(res, C, kind):
    """Every sum stays far below 2^24, so the float32 torch path and the restatement give the float64 reference exactly."""
    from nerfacc_amd.losses import _voxel_terms_grad_torch, _voxel_terms_torch
    p = _int_params(res, C)
    pr = p.double().requires_grad_(True)
    ref = R.terms_reference(pr, res, C, kind, "sum")
    assert float(ref.detach().max()) < 2 ** 24
    got = _voxel_terms_torch(p, res, C, kind, "sum")
    assert got.dtype == torch.float32 and torch.equal(got.double(), ref.detach())
    g = torch.tensor([1.0, -2.0, 0.5, 3.0])
    (ref_gp,) = torch.autograd.grad(ref, pr, g.double())
    assert torch.equal(_voxel_terms_grad_torch(p, g, res, C, kind, "sum").double(), ref_gp)
    mean = _voxel_terms_torch(p, res, C, kind, "mean")                 # one more rounding: the division by the count
    from nerfacc_amd.losses import _voxel_counts
    assert torch.equal(mean, got / torch.tensor(_voxel_counts(res, C), dtype=torch.float32))


# ----------------------------------------------------------------------------- voxel_regularization
def test_regularization_is_the_weighted_sum():
    from nerfacc_amd.losses import voxel_regularization, voxel_terms
    enc = _enc((5, 4, 7), 4)
    for kind in R.KINDS:
        t = voxel_terms(enc, kind).detach().double()
        got = voxel_regularization(enc, tv=0.3, l1=0.7, kind=kind)
        assert got.shape == () and got.dtype == torch.float32
        torch.testing.assert_close(got.double(), 0.3 * t[:3].sum() + 0.7 * t[3], rtol=1e-5, atol=0.0)
        got = voxel_regularization(enc, tv=100.0, l1=0.7, kind=kind, tv_xyz=(0.1, 0.0, 0.25))   # tv_xyz overrides tv
        torch.testing.assert_close(got.double(), 0.1 * t[0] + 0.25 * t[2] + 0.7 * t[3], rtol=1e-5, atol=0.0)
    ts = voxel_terms(enc, "huber", "sum").detach().double()
    torch.testing.assert_close(voxel_regularization(enc, tv=0.5, kind="huber", reduction="sum").double(), 0.5 * ts[:3].sum(),
                               rtol=1e-5, atol=0.0)
    voxel_regularization(enc, tv=1.0, l1=1.0).backward()
    assert torch.isfinite(enc.params.grad).all() and enc.params.grad.abs().sum() > 0
    assert float(voxel_regularization(enc).detach()) == 0.0


def test_regularization_weights_are_built_once():
    from nerfacc_amd import losses
    enc = _enc((5, 4, 7), 4)
    losses.voxel_regularization(enc, tv=0.25, l1=0.5)
    n = len(losses._VOXEL_WEIGHTS)
    w = losses._voxel_weights(enc, 0.25, 0.25, 0.25, 0.5)
    losses.voxel_regularization(enc, tv=0.25, l1=0.5)
    assert len(losses._VOXEL_WEIGHTS) == n and losses._voxel_weights(enc, 0.25, 0.25, 0.25, 0.5) is w
    assert w.shape == (4,) and w.tolist() == [0.25, 0.25, 0.25, 0.5]
    losses.voxel_regularization(enc, tv_xyz=(1.0, 2.0, 3.0), l1=4.0)
    assert losses._voxel_weights(enc, 1.0, 2.0, 3.0, 4.0).tolist() == [1.0, 2.0, 3.0, 4.0] and len(losses._VOXEL_WEIGHTS) == n + 1


# ----------------------------------------------------------------------------- voxel_tv_add_grad_ on CPU tensors
W = (0.3, 0.2, 0.15, 0.05)


def _G(enc, kind, reduction, w=W):
    from nerfacc_amd.losses import _voxel_terms_grad_torch
    return _voxel_terms_grad_torch(enc.params, torch.tensor(w), enc.resolution, enc.n_features, kind, reduction)


@pytest.mark.parametrize("kind,reduction", [("huber", "sum"), ("l2", "mean"), ("l1", "sum")])
@pytest.mark.parametrize("C", [1, 4])
def test_add_grad_dense_and_sparse(C, kind, reduction):
    from nerfacc_amd.losses import voxel_tv_add_grad_
    res = (5, 4, 7)
    enc = _enc(res, C)
    G = _G(enc, kind, reduction)
    grad = torch.randn(enc.params.numel(), generator=torch.Generator().manual_seed(4))
    enc.params.grad = grad.clone()
    voxel_tv_add_grad_(enc, *W[:3], l1=W[3], kind=kind, dense=True, reduction=reduction)
    assert torch.equal(_bits(enc.params.grad), _bits(grad + G))
    # sparse: zeros of either sign stay as they are, a NaN counts as non-zero
    grad[::3] = 0.0
    grad[1::6] = -0.0
    grad[5] = float("nan")
    enc.params.grad = grad.clone()
    voxel_tv_add_grad_(enc, *W[:3], l1=W[3], kind=kind, dense=False, reduction=reduction)
    got, zero = enc.params.grad, grad == 0
    assert zero.sum() > 10 and (~zero).sum() > 10
    assert torch.equal(_bits(got[zero]), _bits(grad[zero])) and torch.signbit(got[1]) and not torch.signbit(got[0])
    assert torch.equal(_bits(got[~zero]), _bits((grad + G)[~zero])) and torch.isnan(got[5])
    assert (got[~zero] != grad[~zero]).sum() > 10                     # (something was added)


def test_add_grad_without_a_gradient():
    from nerfacc_amd.losses import voxel_tv_add_grad_
    enc = _enc((5, 4, 7), 2)
    voxel_tv_add_grad_(enc, *W[:3], dense=False)
    assert enc.params.grad is None                                    # nothing to add to: nothing happens
    voxel_tv_add_grad_(enc, *W[:3], dense=True)
    assert torch.equal(_bits(enc.params.grad), _bits(torch.zeros_like(enc.params) + _G(enc, "huber", "sum", (*W[:3], 0.0))))
    assert not enc.params.grad.requires_grad


def test_add_grad_is_the_clamp_of_six_neighbours():
    """``reduction="sum", kind="huber"`` with w / 6 per axis, restated as a literal loop: per voxel the sum over its existing
    six neighbours of clamp(own - neighbour, -1, 1), times w / 6."""
    from nerfacc_amd.losses import voxel_tv_add_grad_
    res, w = (3, 4, 5), 0.6
    enc = _enc(res, 1)
    g = enc.grid().detach().double()[..., 0]                          # [R_z, R_y, R_x]
    want = torch.zeros_like(g)
    for z in range(res[2]):
        for y in range(res[1]):
            for x in range(res[0]):
                for dz, dy, dx in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if 0 <= zz < res[2] and 0 <= yy < res[1] and 0 <= xx < res[0]:
                        want[z, y, x] += max(-1.0, min(1.0, float(g[z, y, x] - g[zz, yy, xx]))) * (w / 6)
    voxel_tv_add_grad_(enc, w / 6, w / 6, w / 6)
    torch.testing.assert_close(enc.params.grad.double(), want.reshape(-1), rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------------------- the wrappers' errors
def test_wrappers_refuse_unknown_arguments():
    from nerfacc_amd import losses
    from nerfacc_amd.encodings import VMGridEncoding
    enc = _enc((5, 4, 7), 4)
    calls = {"voxel_terms": lambda **kw: losses.voxel_terms(kw.pop("enc", enc), **kw),
             "voxel_regularization": lambda **kw: losses.voxel_regularization(kw.pop("enc", enc), tv=1.0, **kw),
             "voxel_tv_add_grad_": lambda **kw: losses.voxel_tv_add_grad_(kw.pop("enc", enc), 1.0, 1.0, 1.0, **kw)}
    for name, fn in calls.items():
        who = "voxel_terms" if name == "voxel_regularization" else name
        with pytest.raises(ValueError, match=rf"{who}: kind must be 'l2', 'l1' or 'huber' \(got 'l3'\)"):
            fn(kind="l3")
        with pytest.raises(ValueError, match=rf"{who}: reduction must be 'mean' or 'sum' \(got 'max'\)"):
            fn(reduction="max")
        with pytest.raises(ValueError, match=rf"{who}: enc must be a VoxelGridEncoding \(got VMGridEncoding\)"):
            fn(enc=VMGridEncoding((4, 4, 4), n_components=4))


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_voxreg_partials": "n_features res",
    "nfa_voxreg_fwd": "params n_features res kind reduction partials n_partials terms stream",
    "nfa_voxreg_bwd": "params n_features res kind reduction grad_terms grad_params stream",
    "nfa_voxreg_add_grad": "params n_features res kind reduction weights dense grad stream",
}
_POINTERS = {"nfa_voxreg_fwd": "params partials terms", "nfa_voxreg_bwd": "params grad_terms grad_params",
             "nfa_voxreg_add_grad": "params weights grad"}
_ALIGNED = {"nfa_voxreg_fwd": "params partials", "nfa_voxreg_bwd": "params grad_params", "nfa_voxreg_add_grad": "params grad"}


def _res(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    base = {"n_features": 4, "res": _res(5, 7, 4), "kind": 2, "reduction": 1, "n_partials": 0, "dense": 1, "stream": None,
            "weights": (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


def test_c_abi_argument_errors():
    """Every check in its documented order with its text.  No case reaches a launch: every call carries a fault (the
    forward's default n_partials, 0, is one; the other two entries get a null or misaligned pointer where nothing else is
    wrong)."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert lib.nfa_version() == 403 and B.ABI_VERSION == 403
    assert [len(B._SIGS[fn]) for fn in _ARGS] == [2, 9, 8, 9]
    assert B._RESTYPES["nfa_voxreg_partials"] == ctypes.c_int64
    assert B.VOXREG_KIND_CODES == {"l2": 0, "l1": 1, "huber": 2} and B.VOXREG_REDUCTION_CODES == {"mean": 0, "sum": 1}
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        for bad in (0, 3, 6, 68):
            assert _call(lib, fn, n_features=bad) == (-1, f"{nm}: n_features must be 1, 2 or a multiple of 4 up to 64 (got {bad})")
        assert _call(lib, fn, res=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 1, 4)) == (-1, f"{nm}: axis 1 resolution 1 is below 2")
        big = _res(1 << 9, 1 << 9, 1 << 9)
        assert _call(lib, fn, n_features=16, res=big) == (-1, f"{nm}: too many parameters (at most 2^31 - 1 floats)")
        # the order is fixed: the first failing check speaks
        assert _call(lib, fn, n_features=5, res=None, kind=7, params=None)[1].startswith(f"{nm}: n_features must be")
        assert _call(lib, fn, res=None, kind=7, params=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 7, 0), kind=7, params=None) == (-1, f"{nm}: axis 2 resolution 0 is below 2")
    for fn in list(_ARGS)[1:]:
        nm = fn[len("nfa_"):]
        for bad in (-1, 3):
            assert _call(lib, fn, kind=bad, reduction=9, params=None) == (
                -1, f"{nm}: kind must be NFA_VOXREG_L2, NFA_VOXREG_L1 or NFA_VOXREG_HUBER (got {bad})")
        for bad in (-1, 2):
            assert _call(lib, fn, reduction=bad, params=None) == (-1, f"{nm}: reduction must be NFA_VOXREG_MEAN or NFA_VOXREG_SUM (got {bad})")
        for name in _POINTERS[fn].split():
            assert _call(lib, fn, **{name: None}) == (-1, f"{nm}: null pointer")
            if name != "params":                        # a null pointer speaks before the alignment
                assert _call(lib, fn, **{name: None, "params": P + 4}) == (-1, f"{nm}: null pointer")
        a, b = _ALIGNED[fn].split()
        for name in (a, b):
            assert _call(lib, fn, **{name: P + 4}) == (-1, f"{nm}: {a} and {b} must be 16-byte aligned")
    assert _call(lib, "nfa_voxreg_fwd", params=P + 8, n_partials=-1)[1] == "voxreg_fwd: params and partials must be 16-byte aligned"
    need = lib.nfa_voxreg_partials(4, _res(5, 7, 4))
    assert need == 1                                    # 140 quads: one workgroup
    assert _call(lib, "nfa_voxreg_fwd", n_partials=need - 1) == (-1, "voxreg_fwd: n_partials is below nfa_voxreg_partials (0 < 1)")
    assert _call(lib, "nfa_voxreg_fwd", n_partials=-5) == (-1, "voxreg_fwd: n_partials is below nfa_voxreg_partials (-5 < 1)")


def test_partial_rows_follow_the_shape():
    """nfa_voxreg_partials: one row per 2048 quads of the flat table (the last quad may be short); -1 for a refused shape."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for res, C in [((160, 160, 160), 1), ((160, 160, 160), 12), ((161, 161, 161), 4), ((2, 2, 2), 1), ((5, 7, 9), 1),
                   ((4, 4, (1 << 26) + 5), 1), ((1 << 10, 1 << 10, (1 << 11) - 1), 1)]:
        quads = -(-res[0] * res[1] * res[2] * C // 4)
        assert lib.nfa_voxreg_partials(C, _res(*res)) == -(-quads // 2048)
    assert lib.nfa_voxreg_partials(1, _res(1 << 10, 1 << 10, (1 << 11) - 1)) <= 1 << 18
    assert lib.nfa_voxreg_partials(5, _res(4, 4, 4)) == -1
    assert lib.nfa_last_error() == b"voxreg_partials: n_features must be 1, 2 or a multiple of 4 up to 64 (got 5)"


# ----------------------------------------------------------------------------- pins
def test_pins():
    import nerfacc_amd
    from nerfacc_amd import losses
    assert len(nerfacc_amd.__all__) == 22
    for name in ("voxel_terms", "voxel_regularization", "voxel_tv_add_grad_"):
        assert name in losses.__all__ and name not in nerfacc_amd.__all__

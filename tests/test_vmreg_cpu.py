"""CPU: the VM-grid regularisers of nerfacc_amd.losses -- the torch path of ``vm_terms`` and the float32 restatement of the
native gradient against the float64 TensoRF form of tests/vmreg_reference.py, the three TensoRF correspondences,
``vm_regularization``'s weighting, the C entries' argument checks (stand-in pointers, no device) and the pins the addition
must not move."""
import ctypes

import pytest
import torch

import vmreg_reference as R

SHAPES = [(res, C) for res in R.RESOLUTIONS for C in R.COMPONENTS]


def _enc(res, C, params=None):
    from nerfacc_amd.encodings import VMGridEncoding
    enc = VMGridEncoding(res, n_components=C)
    with torch.no_grad():
        enc.params.copy_(R.make_params(res, C) if params is None else params)
    return enc


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


# ----------------------------------------------------------------------------- the torch path against the reference
@pytest.mark.parametrize("res,C", SHAPES)
def test_torch_path_values_and_gradient_in_float64(res, C):
    from nerfacc_amd.losses import _vm_terms_torch
    p, g, ref, ref_gp = R.case(res, C)
    enc = _enc(res, C, p)
    pr = p.double().requires_grad_(True)
    got = _vm_terms_torch(pr, enc.table)
    assert got.shape == (3, 6) and got.dtype == torch.float64
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=0.0)
    (gp,) = torch.autograd.grad(got, pr, g.double())
    torch.testing.assert_close(gp, ref_gp, rtol=1e-10, atol=1e-10 * float(ref_gp.abs().mean()))


def test_vm_terms_on_cpu_tensors():
    """float32 and float64 parameters both give float32 terms on the parameters' device, differentiable by autograd."""
    from nerfacc_amd.losses import vm_terms
    res, C = (7, 6, 5), 24
    p, g, ref, ref_gp = R.case(res, C)
    enc = _enc(res, C, p)
    got = vm_terms(enc)
    assert got.shape == (3, 6) and got.dtype == torch.float32 and got.device == enc.params.device
    torch.testing.assert_close(got.double()[:, :5], ref[:, :5], rtol=1e-4, atol=0.0)
    # ortho cancels: R products summed in any order, then at most C^2 entries, each rounding at most 2^-24 of the magnitudes
    rows = torch.tensor([res[c] for _, _, c in R.VM_MODES], dtype=torch.float64)
    bound = (rows + C * C) * 2.0 ** -24 * R.ortho_scale(p, res, C)
    assert ((got.double()[:, 5] - ref[:, 5]).abs() <= bound).all()
    (gp,) = torch.autograd.grad(got, enc.params, g)
    torch.testing.assert_close(gp.double(), ref_gp, **_tol(ref_gp))
    got64 = vm_terms(enc.double())
    assert got64.dtype == torch.float32
    torch.testing.assert_close(got64.double(), ref, rtol=1e-6, atol=0.0)


def test_torch_path_differentiates_twice():
    from nerfacc_amd.losses import vm_terms
    enc = _enc((7, 6, 5), 4)
    (gp,) = torch.autograd.grad(vm_terms(enc).sum(), enc.params, create_graph=True)
    (ggp,) = torch.autograd.grad((gp * gp).sum(), enc.params)
    assert torch.isfinite(ggp).all() and ggp.abs().sum() > 0


# ----------------------------------------------------------------------------- TensoRF's three regularisers
@pytest.mark.parametrize("res,C", [((7, 6, 5), 24), ((2, 2, 2), 4)])
def test_tensorf_correspondences(res, C):
    from nerfacc_amd.losses import _vm_terms_torch
    p = R.make_params(res, C, seed=5).double()
    enc = _enc(res, C)
    t = _vm_terms_torch(p, enc.table)
    tensors = R.views(p, res, C)
    for m, (plane, line) in enumerate(tensors):
        assert plane.shape == (1, C, res[R.VM_MODES[m][1]], res[R.VM_MODES[m][0]]) and line.shape == (1, C, res[R.VM_MODES[m][2]], 1)
        torch.testing.assert_close(R.tv_loss(plane), 2.0 * (t[m, 0] + t[m, 1]), rtol=1e-12, atol=0.0)          # TVLoss()(plane)
    density_l1 = sum(torch.mean(torch.abs(plane)) + torch.mean(torch.abs(line)) for plane, line in tensors)
    torch.testing.assert_close(density_l1, (t[:, 2] + t[:, 4]).sum(), rtol=1e-12, atol=0.0)                   # density_L1
    comp_diffs = sum(R.vector_diff(line) for _, line in tensors)
    torch.testing.assert_close(comp_diffs, t[:, 5].sum(), rtol=1e-10, atol=0.0)                               # vector_comp_diffs


# ----------------------------------------------------------------------------- vm_regularization
def test_regularization_is_the_weighted_sum():
    from nerfacc_amd.losses import vm_regularization, vm_terms
    enc = _enc((7, 6, 5), 8)
    t = vm_terms(enc).detach().double()
    got = vm_regularization(enc, tv=0.3, l1=0.7, tv_line=0.11, ortho=0.05)
    assert got.shape == () and got.dtype == torch.float32
    want = 0.3 * (t[:, 0] + t[:, 1]).sum() + 0.7 * (t[:, 2] + t[:, 4]).sum() + 0.11 * t[:, 3].sum() + 0.05 * t[:, 5].sum()
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=0.0)
    # TensoRF: TV_loss_density(TVLoss()) * w is tv = 0.02 w; density_L1 * w is l1 = w; vector_comp_diffs * w is ortho = w
    w = 0.1
    tv_reg = sum(R.tv_loss(plane) * 1e-2 for plane, _ in R.views(enc.params.detach().double(), (7, 6, 5), 8))
    torch.testing.assert_close(vm_regularization(enc, tv=0.02 * w).double(), w * tv_reg, rtol=1e-5, atol=0.0)
    torch.testing.assert_close(vm_regularization(enc, l1=w).double(), w * (t[:, 2] + t[:, 4]).sum(), rtol=1e-5, atol=0.0)
    torch.testing.assert_close(vm_regularization(enc, ortho=w).double(), w * t[:, 5].sum(), rtol=1e-5, atol=0.0)
    # differentiable, and the default is nothing at all
    vm_regularization(enc, tv=1.0, l1=1.0, tv_line=1.0, ortho=1.0).backward()
    assert torch.isfinite(enc.params.grad).all() and enc.params.grad.abs().sum() > 0
    assert float(vm_regularization(enc).detach()) == 0.0


def test_regularization_weights_are_built_once():
    from nerfacc_amd import losses
    enc = _enc((7, 6, 5), 4)
    losses.vm_regularization(enc, tv=0.25, ortho=0.5)
    n = len(losses._VM_WEIGHTS)
    w = losses._vm_weights(enc, 0.25, 0.0, 0.0, 0.5)
    losses.vm_regularization(enc, tv=0.25, ortho=0.5)
    assert len(losses._VM_WEIGHTS) == n and losses._vm_weights(enc, 0.25, 0.0, 0.0, 0.5) is w
    assert w.shape == (3, 6) and all(row == [0.25, 0.25, 0.0, 0.0, 0.0, 0.5] for row in w.tolist())
    assert losses._vm_weights(enc, 1.0, 2.0, 3.0, 4.0)[1].tolist() == [1.0, 1.0, 2.0, 3.0, 2.0, 4.0]


# ----------------------------------------------------------------------------- the float32 restatement of the native gradient
@pytest.mark.parametrize("res,C", SHAPES)
def test_gradient_restatement_against_float64_autograd(res, C):
    from nerfacc_amd.losses import _vm_terms_grad_torch
    p, g, _, ref_gp = R.case(res, C)
    enc = _enc(res, C, p)
    got = _vm_terms_grad_torch(p, g, enc.table)
    assert got.dtype == torch.float32 and got.shape == p.shape
    torch.testing.assert_close(got.double(), ref_gp, **_tol(ref_gp))
    # a parameter that is exactly 0: the L1 terms contribute nothing there
    only_l1 = torch.zeros_like(g)
    only_l1[:, 2] = 1.0
    only_l1[:, 4] = 1.0
    got = _vm_terms_grad_torch(p, only_l1, enc.table)
    assert (p == 0.0).any() and (got[p == 0.0] == 0).all() and (got[p != 0.0] != 0).all()
    assert torch.equal(torch.sign(got), torch.sign(p))


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_vmreg_partials": "n_components res",
    "nfa_vmreg_fwd": "params n_components res partials n_partials signs terms stream",
    "nfa_vmreg_bwd": "params n_components res grad_terms signs grad_params stream",
}


def _res(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    base = {"n_components": 8, "res": _res(5, 7, 4), "n_partials": 0, "stream": None}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


def test_c_abi_argument_errors():
    """Every check in its documented order with its text.  No case reaches a launch: a call that passes every other check
    ends at n_partials (0 here), the last one; nfa_vmreg_bwd has no such check, so each of its cases carries a fault."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert lib.nfa_version() == 403 and B.ABI_VERSION == 403
    assert [len(B._SIGS[fn]) for fn in _ARGS] == [2, 8, 7]
    assert B._RESTYPES["nfa_vmreg_partials"] == ctypes.c_int64
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        for bad in (0, 2, 6, 100):
            assert _call(lib, fn, n_components=bad) == (-1, f"{nm}: n_components must be a multiple of 4 in 4..96 (got {bad})")
        assert _call(lib, fn, res=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 1, 4)) == (-1, f"{nm}: axis 1 resolution 1 is below 2")
        big = _res(1 << 13, 1 << 13, 1 << 13)
        assert _call(lib, fn, n_components=96, res=big) == (-1, f"{nm}: too many parameters (at most 2^31 - 1 floats)")
        # the order is fixed: the first failing check speaks
        assert _call(lib, fn, n_components=5, res=None, params=None)[1].startswith(f"{nm}: n_components must be")
        assert _call(lib, fn, res=None, params=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 7, 0), params=None) == (-1, f"{nm}: axis 2 resolution 0 is below 2")
    fwd_text = "vmreg_fwd: params, partials and signs must be 16-byte aligned"
    bwd_text = "vmreg_bwd: params, signs and grad_params must be 16-byte aligned"
    for fn, ptrs in (("nfa_vmreg_fwd", "params partials signs terms"), ("nfa_vmreg_bwd", "params grad_terms signs grad_params")):
        nm = fn[len("nfa_"):]
        for name in ptrs.split():
            assert _call(lib, fn, **{name: None}) == (-1, f"{nm}: null pointer")
            if name != "params":                        # a null pointer speaks before the alignment
                assert _call(lib, fn, **{name: None, "params": P + 4}) == (-1, f"{nm}: null pointer")
    for name in ("params", "partials", "signs"):
        assert _call(lib, "nfa_vmreg_fwd", **{name: P + 4}) == (-1, fwd_text)
    assert _call(lib, "nfa_vmreg_fwd", params=P + 8, n_partials=-1)[1] == fwd_text      # the alignment speaks before n_partials
    for name in ("params", "signs", "grad_params"):
        assert _call(lib, "nfa_vmreg_bwd", **{name: P + 12}) == (-1, bwd_text)
    need = lib.nfa_vmreg_partials(8, _res(5, 7, 4))
    assert need == 3                                    # three planes of at most 16 rows by 256 quads: one tile each
    assert _call(lib, "nfa_vmreg_fwd", n_partials=need - 1) == (-1, f"vmreg_fwd: n_partials is below nfa_vmreg_partials ({need - 1} < {need})")
    assert _call(lib, "nfa_vmreg_fwd") == (-1, f"vmreg_fwd: n_partials is below nfa_vmreg_partials (0 < {need})")


def test_partial_rows_follow_the_shape():
    """nfa_vmreg_partials: ceil(H / 16) * ceil(W C / 1024) tiles per plane, summed over the modes; -1 for a refused shape."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for res, C in [((70, 33, 9), 24), ((300, 300, 300), 48), ((2, 2, 2), 4), ((128, 64, 17), 96)]:
        tiles = sum(-(-res[b] // 16) * -(-res[a] * C // 1024) for a, b, _ in R.VM_MODES)
        assert lib.nfa_vmreg_partials(C, _res(*res)) == tiles
    assert lib.nfa_vmreg_partials(5, _res(4, 4, 4)) == -1
    assert lib.nfa_last_error() == b"vmreg_partials: n_components must be a multiple of 4 in 4..96 (got 5)"


# ----------------------------------------------------------------------------- pins
def test_pins():
    import nerfacc_amd
    from nerfacc_amd import losses
    assert len(nerfacc_amd.__all__) == 22
    for name in ("vm_terms", "vm_regularization"):
        assert name in losses.__all__ and name not in nerfacc_amd.__all__
    for name in ("distortion", "plane_terms", "plane_regularization"):
        assert name in losses.__all__

"""CPU: the plane-grid (K-Planes) encoding -- the torch path against the float64 grid_sample form of
tests/planegrid_reference.py in value and gradient, the parameter layout, the constructor's refusals, the initialisation,
edge inputs, the C entries' argument checks (stand-in pointers, no device) and the pins the addition must not move."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as TF

import planegrid_reference as R

RES, MS = R.RES, R.MS
REDUCES = ["product", "sum"]


def _enc(D, reduce="product", F=4, res=None, ms=MS, **kw):
    from nerfacc_amd.encodings import PlaneGridEncoding
    torch.manual_seed(7 * D + len(reduce))
    enc = PlaneGridEncoding(D, res or RES[D], ms, n_features=F, reduce=reduce, **kw)
    with torch.no_grad():
        enc.params.uniform_(-1.0, 1.0)
    return enc


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


# ----------------------------------------------------------------------------- the torch path against the reference
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("D,res,ms", [(3, RES[3], MS), (4, RES[4], MS), (3, (2, 3, 2), (1,)), (4, (3, 2, 5, 2), (1, 3))])
def test_torch_path_values(D, res, ms, reduce):
    enc = _enc(D, reduce, res=res, ms=ms)
    g = torch.Generator().manual_seed(D)
    x = torch.rand(700, D, generator=g) * 1.4 - 0.2
    x[:4] = torch.tensor([0.0, 1.0, 0.5, 0.25])[:, None]          # nodes and borders are fine for values
    got = enc(x)
    ref = R.planegrid_reference(x, enc.params.detach(), res, ms, 4, reduce)
    assert got.shape == (700, len(ms) * 4) and got.dtype == torch.float32
    torch.testing.assert_close(got.double(), ref, **_tol(ref))


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("D", [3, 4])
def test_torch_path_gradients(D, reduce):
    enc = _enc(D, reduce)
    x = R.off_node_points(500, RES[D], MS, seed=D, lo=-0.2, hi=1.2).requires_grad_(True)
    g = torch.randn(500, enc.n_output_dims, generator=torch.Generator().manual_seed(1))
    gx, gp = torch.autograd.grad(enc(x), (x, enc.params), g)
    xr, pr = x.detach().double().requires_grad_(True), enc.params.detach().double().requires_grad_(True)
    rx, rp = torch.autograd.grad(R.planegrid_reference(xr, pr, RES[D], MS, 4, reduce), (xr, pr), g.double())
    torch.testing.assert_close(gx.double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.double(), rp, **_tol(rp))
    outside = (x.detach() < 0) | (x.detach() > 1)
    assert outside.any() and (gx[outside] == 0).all()


# ----------------------------------------------------------------------------- layout
@pytest.mark.parametrize("D", [3, 4])
def test_layout(D):
    enc = _enc(D, F=8)
    res = R.scale_resolutions(RES[D], MS)
    assert enc.resolutions == res and enc.planes == list(itertools.combinations(range(D), 2))
    assert enc.n_output_dims == 16 and enc.n_scales == 2
    at = 0
    for s in range(2):
        for k, (a, b) in enumerate(enc.planes):
            assert enc.offsets[s][k] == at and enc.sizes[s][k] == res[s][a] * res[s][b] * 8
            v = enc.plane(s, k)
            assert v.shape == (res[s][b], res[s][a], 8)
            assert v.data_ptr() == enc.params.data_ptr() + 4 * at        # a view, not a copy
            at += enc.sizes[s][k]
    assert at == enc.params.numel() == enc.table.n_params
    if D == 4:   # the time axis keeps its resolution on every scale
        assert [r[3] for r in res] == [3, 3] and [r[0] for r in res] == [5, 10]
    # plane(s, k).permute(2, 0, 1)[None] is the image K-Planes samples: one plane's sample through grid_sample
    x = R.off_node_points(50, RES[D], MS, seed=3)
    for s, k in [(0, 0), (1, len(enc.planes) - 1)]:
        a, b = enc.planes[k]
        img = enc.plane(s, k).detach().permute(2, 0, 1)[None].double()
        u = 2.0 * x.double() - 1.0
        want = TF.grid_sample(img, torch.stack([u[:, a], u[:, b]], -1)[None, None], mode="bilinear", padding_mode="border",
                              align_corners=True)[0, :, 0].t()
        only = _enc(D, "sum", F=8)
        with torch.no_grad():
            only.params.zero_()
            only.plane(s, k).copy_(enc.plane(s, k))
        got = only(x)[:, s * 8: s * 8 + 8]
        torch.testing.assert_close(got.double(), want, **_tol(want))
    assert "reduce='product'" in repr(enc) and f"n_input_dims={D}" in repr(enc)


# ----------------------------------------------------------------------------- constructor
def test_constructor_errors():
    from nerfacc_amd.encodings import PlaneGridEncoding as E
    for D in (2, 5):
        with pytest.raises(ValueError, match="n_input_dims must be 3 or 4"):
            E(D, (4,) * D)
    for F in (1, 2, 3, 64):
        with pytest.raises(ValueError, match="n_features must be 4, 8, 16 or 32"):
            E(3, (4, 4, 4), n_features=F)
    with pytest.raises(ValueError, match="1..8 entries"):
        E(3, (4, 4, 4), ())
    with pytest.raises(ValueError, match="1..8 entries"):
        E(3, (4, 4, 4), (1,) * 9)
    with pytest.raises(ValueError, match="at least 2"):
        E(3, (4, 1, 4))
    with pytest.raises(ValueError, match="at least 2"):
        E(4, (4, 4, 4, 1))
    with pytest.raises(ValueError, match="resolution must have 4 entries"):
        E(4, (4, 4, 4))
    with pytest.raises(ValueError, match=r"parameters \(at most 2\^31 - 1\)"):
        E(3, (8192, 8192, 8192), n_features=32)                    # 3 * 2^26 * 32 floats; refused before any allocation
    with pytest.raises(ValueError, match="reduce must be 'product' or 'sum'"):
        E(3, (4, 4, 4), reduce="mean")
    with pytest.raises(ValueError, match="out_dtype"):
        E(3, (4, 4, 4), out_dtype=torch.float64)


# ----------------------------------------------------------------------------- initialisation
def test_initialisation():
    from nerfacc_amd.encodings import PlaneGridEncoding as E
    enc = E(4, (16, 16, 16, 9), (1, 2), n_features=8)
    for s in range(2):
        for k, (a, b) in enumerate(enc.planes):
            v = enc.plane(s, k).detach()
            if b == 3:
                assert (v == 1).all()
            else:
                assert v.min() >= 0.1 and v.max() <= 0.5 and v.std() > 0.05 and abs(float(v.mean()) - 0.3) < 0.02
    enc = E(4, (16, 16, 16, 9), n_features=8, reduce="sum", init=(-0.25, 0.25))
    p = enc.params.detach()
    assert p.min() >= -0.25 and p.max() <= 0.25 and p.std() > 0.1 and "init=(-0.25, 0.25)" in repr(enc)
    enc = E(3, (16, 16, 16))
    assert enc.n_features == 32 and enc.reduce == "product" and enc.params.min() >= 0.1 and enc.params.max() <= 0.5


# ----------------------------------------------------------------------------- edge inputs
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("D", [3, 4])
def test_edge_inputs(D, reduce):
    enc = _enc(D, reduce)
    x = R.edge_points(D).requires_grad_(True)
    y = enc(x)
    assert torch.isfinite(y).all()
    # a clamped coordinate samples the border: the same values as the border itself
    for row, border in [(2, 0), (3, 0), (5, 0), (8, 0), (9, 0), (4, 1), (6, 1), (7, 1)]:
        assert torch.equal(y[row], y[border]), (row, border)
    gx, gp = torch.autograd.grad(y, (x, enc.params), torch.ones_like(y))
    assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
    assert (gx[3:10, 0] == 0).all() and (gx[10:] == 0).all()      # zero on the axis that is outside or not finite
    assert (gx[:10, 1:] != 0).all()                                # the axes inside keep theirs


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_planegrid_fwd": "n_dims reduce elem x params n_points n_scales n_features res y stream",
    "nfa_planegrid_bwd": "n_dims reduce elem x params grad_y n_points n_scales n_features res grad_params grad_x stream",
}


def _res(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    base = {"n_dims": 3, "reduce": 0, "elem": 0, "n_points": 16, "n_scales": 2, "n_features": 4, "res": _res(5, 7, 4, 10, 14, 8),
            "stream": None}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


def test_c_abi_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        # n_points == 0 returns before any other check
        assert _call(lib, fn, n_points=0, n_dims=9, reduce=9, elem=9, n_features=5, n_scales=0, res=None, x=None)[0] == 0
        assert _call(lib, fn, n_points=-1) == (-1, f"{nm}: negative n_points")
        for bad in (2, 5):
            assert _call(lib, fn, n_dims=bad) == (-1, f"{nm}: n_dims must be 3 or 4 (got {bad})")
        assert _call(lib, fn, reduce=2) == (-1, f"{nm}: reduce must be NFA_PLANE_PRODUCT (0) or NFA_PLANE_SUM (1) (got 2)")
        assert _call(lib, fn, elem=3) == (-1, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)")
        for bad in (2, 12, 64):
            assert _call(lib, fn, n_features=bad) == (-1, f"{nm}: n_features must be 4, 8, 16 or 32 (got {bad})")
        for bad in (0, 9):
            assert _call(lib, fn, n_scales=bad) == (-1, f"{nm}: n_scales must be in 1..8 (got {bad})")
        assert _call(lib, fn, res=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 7, 4, 10, 1, 8)) == (-1, f"{nm}: scale 1 axis 1 resolution 1 is below 2")
        big = _res(1 << 13, 1 << 13, 1 << 13, 2, 2, 2)
        assert _call(lib, fn, n_features=32, res=big) == (-1, f"{nm}: too many parameters (at most 2^31 - 1 floats)")
        assert _call(lib, fn, res=_res(1 << 30, 1 << 30, 2, 2, 2, 2)) == (-1, f"{nm}: too many parameters (at most 2^31 - 1 floats)")
        # the order is fixed: the first failing check speaks
        assert _call(lib, fn, n_dims=5, reduce=2, elem=3)[1] == f"{nm}: n_dims must be 3 or 4 (got 5)"
        assert _call(lib, fn, reduce=2, elem=3, n_features=5)[1].startswith(f"{nm}: reduce must be")
        assert _call(lib, fn, n_features=5, n_scales=0, x=None)[1].startswith(f"{nm}: n_features must be")
        assert _call(lib, fn, res=None, x=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, x=None) == (-1, f"{nm}: null pointer")
        assert _call(lib, fn, params=None) == (-1, f"{nm}: null pointer")
    assert _call(lib, "nfa_planegrid_fwd", y=None) == (-1, "planegrid_fwd: null pointer")
    assert _call(lib, "nfa_planegrid_bwd", grad_y=None) == (-1, "planegrid_bwd: null pointer")
    assert _call(lib, "nfa_planegrid_bwd", grad_params=None, grad_x=None) == (-1, "planegrid_bwd: null pointer")
    assert B._SIGS["nfa_planegrid_fwd"][8] == ctypes.POINTER(ctypes.c_int32)


# ----------------------------------------------------------------------------- pins
def test_pins():
    import nerfacc_amd
    from nerfacc_amd import _backend as B, encodings
    assert B.load().nfa_version() == 403 and B.ABI_VERSION == 403
    assert "PlaneGridEncoding" not in nerfacc_amd.__all__ and len(nerfacc_amd.__all__) == 22
    assert "PlaneGridEncoding" in encodings.__all__
    assert B.PLANE_REDUCE_CODES == {"product": 0, "sum": 1}


def test_torch_path_differentiates_twice():
    """The torch path is plain autograd (any order); the native function is once_differentiable (GPU tier)."""
    enc = _enc(3)
    x = R.off_node_points(20, RES[3], MS, seed=5).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    (gp,) = torch.autograd.grad(gx.sum(), enc.params)
    assert torch.isfinite(gp).all()

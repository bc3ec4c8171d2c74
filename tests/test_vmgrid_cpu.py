"""CPU: the VM grid (TensoRF) encoding -- the torch path against the float64 grid_sample form of tests/vmgrid_reference.py
in value and gradient, the parameter layout, the initialisation, the constructor's refusals, the three C entries' argument
checks (stand-in pointers, no device), the pins the addition must not move, and ``resampled`` against F.interpolate."""
import ctypes

import pytest
import torch

import vmgrid_reference as R

REDUCES = ["concat", "sum"]
RESOLUTIONS = [R.RES_SMALL, R.RES_WIDE]


def _enc(res=R.RES_SMALL, C=4, reduce="concat", **kw):
    from nerfacc_amd.encodings import VMGridEncoding
    torch.manual_seed(13 * C + len(reduce))
    enc = VMGridEncoding(res, C, reduce, **kw)
    with torch.no_grad():
        enc.params.uniform_(-1.0, 1.0)
    return enc


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


F64 = dict(rtol=1e-10, atol=1e-12)   # float64 against float64: the orders of the sums differ, nothing else


# ----------------------------------------------------------------------------- the torch path against the reference
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("C", [4, 24, 48])
@pytest.mark.parametrize("res", RESOLUTIONS + [(2, 2, 2)])
def test_torch_path_values(res, C, reduce):
    enc = _enc(res, C, reduce).double()
    x = torch.rand(600, 3, generator=torch.Generator().manual_seed(C), dtype=torch.float64) * 1.4 - 0.2
    x[:4] = torch.tensor([0.0, 1.0, 0.5, 0.25], dtype=torch.float64)[:, None]      # nodes and borders are fine for values
    got = enc(x)
    ref = R.vmgrid_reference(x, enc.params.detach(), res, C, reduce)
    assert got.shape == ((600, 3 * C) if reduce == "concat" else (600, 1)) and got.dtype == torch.float64
    assert enc.n_output_dims == got.shape[1]
    torch.testing.assert_close(got, ref, **F64)
    y32 = _enc(res, C, reduce)(x.float())
    assert y32.dtype == torch.float32
    torch.testing.assert_close(y32.double(), ref, **_tol(ref))


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("C", [4, 48])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_torch_path_gradients(res, C, reduce):
    enc = _enc(res, C, reduce).double()
    x = R.off_node_points(500, res, seed=C, lo=-0.2, hi=1.2).double().requires_grad_(True)
    g = torch.randn(500, enc.n_output_dims, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gx, gp = torch.autograd.grad(enc(x), (x, enc.params), g)
    xr, pr = x.detach().clone().requires_grad_(True), enc.params.detach().clone().requires_grad_(True)
    rx, rp = torch.autograd.grad(R.vmgrid_reference(xr, pr, res, C, reduce), (xr, pr), g)
    torch.testing.assert_close(gx, rx, **F64)
    torch.testing.assert_close(gp, rp, **F64)
    outside = (x.detach() < 0) | (x.detach() > 1)
    assert outside.any() and (gx[outside] == 0).all()


def test_edge_inputs():
    from planegrid_reference import edge_points
    for reduce in REDUCES:
        enc = _enc(C=8, reduce=reduce)
        x = edge_points(3).requires_grad_(True)
        y = enc(x)
        assert torch.isfinite(y).all()
        for row, border in [(2, 0), (3, 0), (5, 0), (8, 0), (9, 0), (4, 1), (6, 1), (7, 1)]:   # clamped: the border's values
            assert torch.equal(y[row], y[border]), (row, border)
        gx, gp = torch.autograd.grad(y, (x, enc.params), torch.ones_like(y))
        assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
        assert (gx[3:10, 0] == 0).all() and (gx[10:] == 0).all() and (gx[:10, 1:] != 0).all()


def test_torch_path_differentiates_twice():
    enc = _enc()
    x = R.off_node_points(20, R.RES_SMALL, seed=5).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    (gp,) = torch.autograd.grad(gx.sum(), enc.params)
    assert torch.isfinite(gp).all()


def test_sum_order_is_the_lane_order():
    """``"sum"`` adds in the documented order: lane sums (mode outer, r inner), then the xor butterfly."""
    from nerfacc_amd.encodings import _vm_lanes
    assert [_vm_lanes(C) for C in (4, 8, 12, 16, 24, 48, 64, 96)] == [4, 8, 4, 16, 8, 16, 32, 32]
    C, res = 24, R.RES_SMALL
    cat, tot = _enc(res, C, "concat"), _enc(res, C, "sum")
    with torch.no_grad():
        tot.params.copy_(cat.params)
    x = torch.rand(200, 3, generator=torch.Generator().manual_seed(3))
    t = cat(x).detach()
    lanes = torch.zeros(200, 8)
    for m in range(3):
        for r in range(3):
            lanes = lanes + t[:, m * C + r * 8: m * C + r * 8 + 8]
    for off in (4, 2, 1):
        lanes = lanes + lanes[:, torch.arange(8) ^ off]
    assert torch.equal(tot(x).detach(), lanes[:, :1])


# ----------------------------------------------------------------------------- layout
def test_layout():
    import torch.nn.functional as TF
    res, C = R.RES_SMALL, 8
    enc = _enc(res, C)
    assert enc.modes == [(0, 1, 2), (0, 2, 1), (1, 2, 0)] and enc.n_output_dims == 24 and enc.n_input_dims == 3
    assert _enc(res, C, "sum").n_output_dims == 1
    at = 0
    for m, (a, b, c) in enumerate(enc.modes):
        assert (a, b) == R.MAT_MODE[m] and c == R.VEC_MODE[m]
        assert enc.offsets[m] == [at, at + res[a] * res[b] * C] and enc.sizes[m] == [res[a] * res[b] * C, res[c] * C]
        p, l = enc.plane(m), enc.line(m)
        assert p.shape == (res[b], res[a], C) and l.shape == (res[c], C)
        assert p.data_ptr() == enc.params.data_ptr() + 4 * at                      # views, not copies
        assert l.data_ptr() == enc.params.data_ptr() + 4 * enc.offsets[m][1]
        at += sum(enc.sizes[m])
    assert at == enc.params.numel() == enc.table.n_params
    # the permutes of the docstring give the tensors TensoRF samples: one mode's term through grid_sample
    x = R.off_node_points(50, res, seed=3)
    u = 2.0 * x.double() - 1.0
    kw = dict(mode="bilinear", padding_mode="border", align_corners=True)
    y = enc(x)
    for m, (a, b, c) in enumerate(enc.modes):
        plane = enc.plane(m).detach().permute(2, 0, 1)[None].double()
        line = enc.line(m).detach().t()[None, :, :, None].double()
        assert plane.shape == (1, C, res[b], res[a]) and line.shape == (1, C, res[c], 1)
        pv = TF.grid_sample(plane, torch.stack([u[:, a], u[:, b]], -1)[None, None], **kw)[0, :, 0].t()
        lv = TF.grid_sample(line, torch.stack([torch.zeros_like(u[:, c]), u[:, c]], -1)[None, None], **kw)[0, :, 0].t()
        torch.testing.assert_close(y[:, m * C: m * C + C].double(), pv * lv, **_tol(pv * lv))
    assert "reduce='concat'" in repr(enc) and "n_components=8" in repr(enc) and "resolution=(7, 6, 5)" in repr(enc)


def test_initialisation():
    from nerfacc_amd.encodings import VMGridEncoding as E
    enc = E((32, 32, 32))
    assert enc.n_components == 16 and enc.reduce == "concat" and enc.params.dtype == torch.float32 and enc.params.requires_grad
    p = enc.params.detach()
    assert abs(float(p.mean())) < 0.005 and abs(float(p.std()) - 0.1) < 0.005 and float(p.abs().max()) > 0.3
    for m in range(3):
        assert abs(float(enc.plane(m).detach().std()) - 0.1) < 0.01 and abs(float(enc.line(m).detach().std()) - 0.1) < 0.02
    enc = E((32, 32, 32), 48, "sum", init_scale=0.5)
    assert abs(float(enc.params.detach().std()) - 0.5) < 0.02 and "init_scale=0.5" in repr(enc)


def test_constructor_errors():
    from nerfacc_amd.encodings import VMGridEncoding as E
    for C in (0, 2, 6, 100, 128, 16.0):
        with pytest.raises(ValueError, match=r"VMGridEncoding: n_components must be a multiple of 4 in 4\.\.96"):
            E((4, 4, 4), C)
    with pytest.raises(ValueError, match="VMGridEncoding: reduce must be 'concat' or 'sum' \\(got 'product'\\)"):
        E((4, 4, 4), reduce="product")
    for res in ((4, 4), (4, 4, 4, 4)):
        with pytest.raises(ValueError, match=f"VMGridEncoding: resolution must have 3 entries \\(got {len(res)}\\)"):
            E(res)
    with pytest.raises(ValueError, match="VMGridEncoding: every resolution must be at least 2"):
        E((4, 1, 4))
    with pytest.raises(ValueError, match=r"VMGridEncoding: \d+ parameters \(at most 2\^31 - 1\)"):
        E((8192, 8192, 8192), 96)                                  # refused before any allocation
    with pytest.raises(ValueError, match="out_dtype"):
        E((4, 4, 4), out_dtype=torch.float64)


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_vmgrid_fwd": "reduce elem x params n_points n_components res y stream",
    "nfa_vmgrid_bwd": "reduce elem x params grad_y n_points n_components res grad_params grad_x stream",
    "nfa_vmgrid_resample": "src_params src_res dst_params dst_res n_components stream",
}


def _res(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    base = {"reduce": 0, "elem": 0, "n_points": 16, "n_components": 8, "res": _res(5, 7, 4), "src_res": _res(5, 7, 4),
            "dst_res": _res(9, 3, 4), "stream": None}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


_BAD_C = "n_components must be a multiple of 4 in 4..96"
_TOO_MANY = "parameters (at most 2^31 - 1 floats)"


def test_c_abi_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn in ("nfa_vmgrid_fwd", "nfa_vmgrid_bwd"):
        nm = fn[len("nfa_"):]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        # n_points == 0 returns before any other check
        assert _call(lib, fn, n_points=0, reduce=9, elem=9, n_components=5, res=None, x=None)[0] == 0
        assert _call(lib, fn, n_points=-1) == (-1, f"{nm}: negative n_points")
        assert _call(lib, fn, reduce=2) == (-1, f"{nm}: reduce must be NFA_VM_CONCAT (0) or NFA_VM_SUM (1) (got 2)")
        assert _call(lib, fn, elem=3) == (-1, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)")
        for bad in (0, 2, 6, 100):
            assert _call(lib, fn, n_components=bad) == (-1, f"{nm}: {_BAD_C} (got {bad})")
        assert _call(lib, fn, res=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 1, 4)) == (-1, f"{nm}: axis 1 resolution 1 is below 2")
        assert _call(lib, fn, n_components=96, res=_res(1 << 13, 1 << 13, 1 << 13)) == (-1, f"{nm}: too many {_TOO_MANY}")
        assert _call(lib, fn, res=_res(1 << 30, 1 << 30, 2)) == (-1, f"{nm}: too many {_TOO_MANY}")
        # the order is fixed: the first failing check speaks
        assert _call(lib, fn, n_points=-1, reduce=2)[1] == f"{nm}: negative n_points"
        assert _call(lib, fn, reduce=2, elem=3, n_components=5)[1].startswith(f"{nm}: reduce must be")
        assert _call(lib, fn, elem=3, n_components=5)[1].startswith(f"{nm}: elem must be")
        assert _call(lib, fn, n_components=5, res=None)[1] == f"{nm}: {_BAD_C} (got 5)"
        assert _call(lib, fn, res=None, x=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_res(5, 1, 4), x=None)[1] == f"{nm}: axis 1 resolution 1 is below 2"
        assert _call(lib, fn, x=None) == (-1, f"{nm}: null pointer")
        assert _call(lib, fn, params=None) == (-1, f"{nm}: null pointer")
    assert _call(lib, "nfa_vmgrid_fwd", y=None) == (-1, "vmgrid_fwd: null pointer")
    assert _call(lib, "nfa_vmgrid_bwd", grad_y=None) == (-1, "vmgrid_bwd: null pointer")
    assert _call(lib, "nfa_vmgrid_bwd", grad_params=None, grad_x=None) == (-1, "vmgrid_bwd: null pointer")

    fn, nm = "nfa_vmgrid_resample", "vmgrid_resample"
    assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
    assert _call(lib, fn, n_components=10, src_res=None) == (-1, f"{nm}: {_BAD_C} (got 10)")
    assert _call(lib, fn, src_res=None) == (-1, f"{nm}: null resolution table")
    assert _call(lib, fn, dst_res=None, src_params=None) == (-1, f"{nm}: null resolution table")
    assert _call(lib, fn, src_res=_res(1, 7, 4), dst_res=_res(1, 1, 1)) == (-1, f"{nm}: source axis 0 resolution 1 is below 2")
    big = _res(1 << 13, 1 << 13, 1 << 13)
    assert _call(lib, fn, n_components=96, src_res=big, dst_res=_res(2, 2, 1)) == (-1, f"{nm}: too many source {_TOO_MANY}")
    assert _call(lib, fn, dst_res=_res(2, 2, 1), dst_params=None) == (-1, f"{nm}: destination axis 2 resolution 1 is below 2")
    assert _call(lib, fn, n_components=96, dst_res=big, dst_params=None) == (-1, f"{nm}: too many destination {_TOO_MANY}")
    assert _call(lib, fn, src_params=None) == (-1, f"{nm}: null pointer")
    assert _call(lib, fn, dst_params=None) == (-1, f"{nm}: null pointer")
    assert B._SIGS["nfa_vmgrid_fwd"][6] == ctypes.POINTER(ctypes.c_int32)


# ----------------------------------------------------------------------------- pins
def test_pins():
    import nerfacc_amd
    from nerfacc_amd import _backend as B, encodings
    assert B.load().nfa_version() == 403 and B.ABI_VERSION == 403
    assert "VMGridEncoding" not in nerfacc_amd.__all__ and len(nerfacc_amd.__all__) == 22
    assert "VMGridEncoding" in encodings.__all__
    assert B.VM_REDUCE_CODES == {"concat": 0, "sum": 1} and B.PLANE_REDUCE_CODES == {"product": 0, "sum": 1}
    with pytest.raises(ValueError, match="unsupported tcnn encoding"):
        encodings.encoding_from_tcnn_config(3, {"otype": "VMGrid"})


# ----------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("C", [4, 48])
@pytest.mark.parametrize("src,dst", [(R.RES_SMALL, (13, 9, 20)), (R.RES_WIDE, (8, 40, 9)), ((2, 2, 2), (5, 5, 5)),
                                     (R.RES_WIDE, R.RES_SMALL)])
def test_resampled(src, dst, C):
    enc = _enc(src, C, "sum", out_dtype=torch.bfloat16)
    new = enc.resampled(dst)
    assert type(new) is type(enc) and new.resolution == tuple(dst) and new.n_components == C and new.reduce == "sum"
    assert new.out_dtype == torch.bfloat16 and new.params.requires_grad and new.params.device == enc.params.device
    assert new.params.shape == (new.table.n_params,) and new.params.grad_fn is None and new.params.dtype == torch.float32
    ref = R.resample_reference(enc.params.detach(), src, dst, C)
    torch.testing.assert_close(new.params.detach().double(), ref, **_tol(ref))
    # in float64 the torch form is F.interpolate's arithmetic
    from nerfacc_amd.encodings import _vm_resample_torch
    torch.testing.assert_close(_vm_resample_torch(enc.params.detach().double(), enc.table, new.table), ref, **F64)
    # the corner nodes are the source's corner nodes (align_corners)
    for m in range(3):
        torch.testing.assert_close(new.plane(m)[0, 0], enc.plane(m)[0, 0])
        torch.testing.assert_close(new.plane(m)[-1, -1], enc.plane(m)[-1, -1])
        torch.testing.assert_close(new.line(m)[-1], enc.line(m)[-1])


def test_resampled_identity():
    enc = _enc(R.RES_WIDE, 24)
    new = enc.resampled(R.RES_WIDE)
    assert new is not enc and new.params.data_ptr() != enc.params.data_ptr()
    assert torch.equal(new.params.detach().view(torch.int32), enc.params.detach().view(torch.int32))
    x = torch.rand(100, 3)
    assert torch.equal(new(x), enc(x))

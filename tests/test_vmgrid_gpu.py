"""GPU: the native VM grid (TensoRF) passes of csrc/vmgrid.hip -- the forward bit for bit against the torch restatement,
the backward against the float64 grid_sample form of tests/vmgrid_reference.py (both line-gradient paths), the
reproducible dL/dx, half element types, edge inputs, the input forms the module accepts, and the resampling."""
import functools

import pytest
import torch

import vmgrid_reference as R

pytestmark = pytest.mark.gpu

REDUCES = ["concat", "sum"]
RESOLUTIONS = [R.RES_SMALL, R.RES_WIDE]
N_BWD = 1000
RES_LONG_LINE = (4, 4, 400)   # with C = 96 one line is 153,600 bytes: beyond the 64 KiB a workgroup keeps in LDS


def _enc(res, C, reduce, dev=None, **kw):
    from nerfacc_amd.encodings import VMGridEncoding
    torch.manual_seed(17 * C + len(reduce) + res[0])
    enc = VMGridEncoding(res, C, reduce, **kw)
    with torch.no_grad():
        enc.params.uniform_(-1.0, 1.0)
    return enc.to(dev) if dev is not None else enc


def _torch_path(enc, x):
    from nerfacc_amd import _backend as B
    from nerfacc_amd.encodings import _vmgrid_torch
    return _vmgrid_torch(x, enc.params.detach(), enc.table, B.VM_REDUCE_CODES[enc.reduce])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tol(ref, part=1.0):
    return dict(rtol=1e-4 * part, atol=1e-3 * part * float(ref.abs().mean()))


def _lanes(C):
    return next(w for w in (32, 16, 8, 4) if C % w == 0)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("C", [4, 16, 24, 48, 96])
@pytest.mark.parametrize("reduce", REDUCES)
def test_forward_bit_for_bit(dev, reduce, C):
    per_wave = 64 // _lanes(C)
    g = torch.Generator().manual_seed(C)
    for res in RESOLUTIONS:
        enc = _enc(res, C, reduce, dev=dev)
        for n in sorted({1, per_wave - 1, per_wave, per_wave + 1, 1000}):
            x = (torch.rand(n, 3, generator=g) * 1.4 - 0.2).to(dev)
            y = enc(x)
            want = _torch_path(enc, x)
            assert y.shape == ((n, 3 * C) if reduce == "concat" else (n, 1)) and y.dtype == torch.float32
            assert torch.equal(_bits(y), _bits(want)), (res, n)


def _edge_rows(res):
    """planegrid_reference.edge_points (borders, outside, infinite and NaN rows) and rows on exact nodes."""
    from planegrid_reference import edge_points
    nodes = torch.tensor([[i / (res[0] - 1), j / (res[1] - 1), k / (res[2] - 1)]
                          for i, j, k in [(0, 0, 0), (1, 2, 3), (3, 1, 2), (res[0] - 1, res[1] - 1, res[2] - 1), (2, 0, res[2] - 1)]])
    return torch.cat([edge_points(3), nodes, torch.tensor([[0.5, 0.2, 0.25], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])])


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("C", [8, 48])
def test_edge_inputs(dev, reduce, C):
    enc = _enc(R.RES_SMALL, C, reduce, dev=dev)
    x = _edge_rows(R.RES_SMALL).to(dev).requires_grad_(True)
    y = enc(x)
    assert torch.equal(_bits(y), _bits(_torch_path(enc, x.detach()))) and torch.isfinite(y).all()
    gx, gp = torch.autograd.grad(y, (x, enc.params), torch.ones_like(y))
    assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
    assert (gx[3:10, 0] == 0).all() and (gx[10:13] == 0).all() and (gx[:10, 1:] != 0).all()
    # every add landed in its place: the table gradient is the torch path's (autograd, on the CPU; it takes NaN rows)
    cpu = _enc(R.RES_SMALL, C, reduce)
    yc = cpu(x.detach().cpu())
    (cp,) = torch.autograd.grad(yc, cpu.params, torch.ones_like(yc))
    torch.testing.assert_close(gp.cpu(), cp, **_tol(cp))


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("reduce,C", [("concat", 48), ("sum", 16), ("concat", 4)])
def test_half_outputs_are_the_float32_result_rounded_once(dev, reduce, C, half):
    enc = _enc(R.RES_WIDE, C, reduce, dev=dev)
    x = (torch.rand(1000, 3, generator=torch.Generator().manual_seed(2)) * 1.4 - 0.2).to(dev)
    y32 = enc(x)
    enc.out_dtype = half
    yh = enc(x)
    assert yh.dtype == half and torch.equal(_bits(yh), _bits(y32.to(half)))
    with torch.autocast("cuda", dtype=half):
        enc.out_dtype = "autocast"
        assert enc(x).dtype == half
        enc.out_dtype = None
        assert enc(x).dtype == torch.float32
        assert torch.equal(_bits(enc(x.to(half))), _bits(enc(x.to(half).float())))   # a half x is widened, not run in half


# ----------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _bwd_case(res, C, reduce, g_dtype=torch.float32, fixed_axis=None, exact_axis=None):
    """(enc on the CPU, x, g, reference dL/dx, reference dL/dparams): computed once per configuration, never modified.
    The incoming gradient is rounded to ``g_dtype`` before the reference sees it.  ``fixed_axis``: every point has the
    same coordinate on that axis, so all of them add into one cell of the line along it.  ``exact_axis``: the coordinates
    on that axis are odd multiples of 2^-12, so that x (R - 1) is exact in float32 up to R = 2^11 and never a node."""
    enc = _enc(res, C, reduce)
    x = R.off_node_points(N_BWD, res, seed=100 + C, lo=-0.1, hi=1.1)
    if fixed_axis is not None:
        x[:, fixed_axis] = x[0, fixed_axis].clamp(0.05, 0.95)
    if exact_axis is not None:
        x[:, exact_axis] = (torch.floor(x[:, exact_axis] * 2048.0) * 2.0 + 1.0) / 4096.0
    g = torch.randn(N_BWD, enc.n_output_dims, generator=torch.Generator().manual_seed(9)).to(g_dtype)
    xr, pr = x.double().requires_grad_(True), enc.params.detach().double().requires_grad_(True)
    rx, rp = torch.autograd.grad(R.vmgrid_reference(xr, pr, res, C, reduce), (xr, pr), g.double())
    return enc, x, g, rx, rp


def _check_cpu_float32(cpu, x, g, rx, rp):
    """The inputs are fit for the tolerance: float32 arithmetic alone (the torch path, on the CPU) uses a quarter of it."""
    xc = x.clone().requires_grad_(True)
    cx, cp = torch.autograd.grad(cpu(xc), (xc, cpu.params), g)
    torch.testing.assert_close(cx.double(), rx, **_tol(rx, 0.25))
    torch.testing.assert_close(cp.double(), rp, **_tol(rp, 0.25))


def _native_grads(case, dev, label):
    cpu, x, g, rx, rp = case
    enc = _enc(cpu.resolution, cpu.n_components, cpu.reduce, dev=dev)
    xd, gd = x.to(dev).requires_grad_(True), g.to(dev)
    gx, gp = torch.autograd.grad(enc(xd), (xd, enc.params), gd)
    print(f"{label}: max|dx err| {float((gx.cpu().double() - rx).abs().max()):.3e} (atol {_tol(rx)['atol']:.3e}), "
          f"max|dp err| {float((gp.cpu().double() - rp).abs().max()):.3e} (atol {_tol(rp)['atol']:.3e})")
    torch.testing.assert_close(gx.cpu().double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.cpu().double(), rp, **_tol(rp))
    return enc, xd, gd, gx, gp


@pytest.mark.parametrize("C", [16, 48, 96])
@pytest.mark.parametrize("reduce", REDUCES)
def test_backward_against_the_float64_reference(dev, reduce, C):
    res = R.RES_SMALL
    case = _bwd_case(res, C, reduce)
    cpu, x, g, rx, rp = case
    _check_cpu_float32(*case)
    enc, xd, gd, gx, gp = _native_grads(case, dev, f"{reduce} C={C} {res}")
    outside = (x < 0) | (x > 1)
    assert outside.any() and (gx.cpu()[outside] == 0).all()

    # dL/dx: the same bits on a second run, and when it is asked for alone; dL/dparams alone is the same sum
    gx2, _ = torch.autograd.grad(enc(xd), (xd, enc.params), gd)
    assert torch.equal(_bits(gx), _bits(gx2))
    (gx_alone,) = torch.autograd.grad(enc(xd), xd, gd)
    assert torch.equal(_bits(gx), _bits(gx_alone))
    (gp_alone,) = torch.autograd.grad(enc(xd.detach()), enc.params, gd)
    torch.testing.assert_close(gp_alone.cpu().double(), rp, **_tol(rp))
    torch.testing.assert_close(gp_alone, gp, rtol=1e-4, atol=_tol(rp)["atol"])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_line_gradient_lds_all_points_in_one_cell(dev, axis):
    case = _bwd_case(R.RES_SMALL, 16, "concat", fixed_axis=axis)
    assert (case[1][:, axis] == case[1][0, axis]).all()
    _check_cpu_float32(*case)
    _native_grads(case, dev, f"one cell of the line along axis {axis}")


@pytest.mark.parametrize("reduce,C", [("concat", 48), ("sum", 96)])
def test_line_gradient_lds_points_spread_over_a_long_line(dev, reduce, C):
    assert max(R.RES_WIDE) * C * 4 <= 65536
    case = _bwd_case(R.RES_WIDE, C, reduce)
    _check_cpu_float32(*case)
    _native_grads(case, dev, f"{reduce} C={C} {R.RES_WIDE}")


@pytest.mark.parametrize("reduce", REDUCES)
def test_line_gradient_fallback_without_lds(dev, reduce):
    # On a 400-node axis the float32 rounding of x (R - 1) alone (2.4e-5 of a cell near x = 1), summed by the 4-node lines
    # over all the points, exceeds the tolerance (the CPU check below fails with plain uniform points): the points get
    # coordinates on that axis whose product is exact, so that the case tests the fallback and not that rounding.
    assert max(RES_LONG_LINE) * 96 * 4 > 65536
    case = _bwd_case(RES_LONG_LINE, 96, reduce, exact_axis=2)
    _check_cpu_float32(*case)
    _native_grads(case, dev, f"{reduce} C=96 {RES_LONG_LINE}")


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("reduce,C", [("sum", 16), ("concat", 24)])
def test_half_gradient_is_read_directly(dev, reduce, C, half):
    _, x, g, rx, rp = _bwd_case(R.RES_SMALL, C, reduce, half)
    enc = _enc(R.RES_SMALL, C, reduce, dev=dev, out_dtype=half)
    xd = x.to(dev).requires_grad_(True)
    y = enc(xd)
    assert y.dtype == half
    gx, gp = torch.autograd.grad(y, (xd, enc.params), g.to(dev))
    assert gx.dtype == torch.float32 and gp.dtype == torch.float32
    torch.testing.assert_close(gx.cpu().double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.cpu().double(), rp, **_tol(rp))


def test_second_order_is_refused(dev):
    enc = _enc(R.RES_SMALL, 4, "concat", dev=dev)
    x = torch.rand(10, 3, device=dev).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    assert gx.requires_grad                                        # create_graph=True alone is harmless
    with pytest.raises(NotImplementedError, match="VMGridEncoding: the second order"):
        gx.sum().backward()


# ----------------------------------------------------------------------------- input forms
def test_input_forms(dev):
    enc = _enc(R.RES_SMALL, 8, "concat", dev=dev)
    g = torch.Generator().manual_seed(4)
    # empty
    assert enc(torch.empty(0, 3, device=dev)).shape == (0, 24)
    x0 = torch.empty(0, 3, device=dev, requires_grad=True)
    gx, gp = torch.autograd.grad(enc(x0).sum(), (x0, enc.params))
    assert gx.shape == (0, 3) and (gp == 0).all()
    # leading batch dimensions
    x = torch.rand(3, 5, 3, generator=g).to(dev)
    y = enc(x)
    assert y.shape == (3, 5, 24) and torch.equal(_bits(y.view(15, 24)), _bits(_torch_path(enc, x.view(15, 3))))
    # a non-contiguous x, and one whose first element is 4 bytes past a 16-byte boundary
    wide = torch.rand(33, 7, generator=g).to(dev)
    xs = wide[:, 1:4]
    assert not xs.is_contiguous()
    assert torch.equal(_bits(enc(xs)), _bits(_torch_path(enc, xs.contiguous())))
    buf = torch.rand(33 * 3 + 1, generator=g).to(dev)
    xm = buf[1:].view(33, 3)
    assert xm.data_ptr() % 16 == 4
    assert torch.equal(_bits(enc(xm)), _bits(_torch_path(enc, xm.clone())))
    xm = xm.detach().requires_grad_(True)
    (gm,) = torch.autograd.grad(enc(xm).sum(), xm)
    xa = xm.detach().clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(enc(xa).sum(), xa)
    assert torch.equal(_bits(gm), _bits(ga))


def test_native_path_is_taken(dev, monkeypatch):
    from nerfacc_amd import encodings

    def boom(*a, **k):
        raise AssertionError("the torch path ran for a float32 tensor on the device")
    enc = _enc(R.RES_SMALL, 16, "sum", dev=dev)
    x = torch.rand(100, 3, device=dev, requires_grad=True)
    want = _torch_path(enc, x.detach())
    small = enc.resampled((4, 5, 6))
    monkeypatch.setattr(encodings, "_vmgrid_torch", boom)
    monkeypatch.setattr(encodings, "_vm_resample_torch", boom)
    y = enc(x)
    assert torch.equal(_bits(y), _bits(want))
    y.sum().backward()
    assert x.grad is not None and enc.params.grad is not None and enc.params.grad.abs().sum() > 0
    again = enc.resampled((4, 5, 6))
    assert again.params.is_cuda and torch.equal(_bits(again.params.detach()), _bits(small.params.detach()))


# ----------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("C", [4, 48])
@pytest.mark.parametrize("src,dst", [(R.RES_SMALL, (13, 9, 20)), (R.RES_WIDE, (8, 40, 9)), (R.RES_WIDE, R.RES_WIDE),
                                     ((2, 2, 2), (5, 5, 5))])
def test_resampled(dev, src, dst, C):
    from nerfacc_amd.encodings import _vm_resample_torch
    enc = _enc(src, C, "concat", dev=dev)
    new = enc.resampled(dst)
    assert new.params.device == enc.params.device and new.resolution == tuple(dst) and new.params.requires_grad
    want = _vm_resample_torch(enc.params.detach(), enc.table, new.table)
    assert torch.equal(_bits(new.params.detach()), _bits(want))
    ref = R.resample_reference(enc.params.detach().cpu(), src, dst, C)
    torch.testing.assert_close(new.params.detach().cpu().double(), ref, **_tol(ref))
    if tuple(src) == tuple(dst):
        assert torch.equal(_bits(new.params.detach()), _bits(enc.params.detach()))
    x = (torch.rand(300, 3, generator=torch.Generator().manual_seed(6)) * 1.2 - 0.1).to(dev)
    assert torch.equal(_bits(new(x)), _bits(_torch_path(new, x)))

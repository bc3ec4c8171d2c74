"""GPU: the native plane-grid (K-Planes) passes of csrc/planes.hip -- the forward bit for bit against the torch
restatement, the backward against the float64 grid_sample form of tests/planegrid_reference.py, the reproducible dL/dx,
half element types, edge inputs and the input forms the module accepts."""
import functools

import pytest
import torch

import planegrid_reference as R

pytestmark = pytest.mark.gpu

RES, MS = R.RES, R.MS
REDUCES = ["product", "sum"]
N_BWD = 1000


def _enc(D, reduce, F, ms=MS, res=None, dev=None, **kw):
    from nerfacc_amd.encodings import PlaneGridEncoding
    torch.manual_seed(11 * D + F + len(reduce))
    enc = PlaneGridEncoding(D, res or RES[D], ms, n_features=F, reduce=reduce, **kw)
    with torch.no_grad():
        enc.params.uniform_(-1.0, 1.0)
    return enc.to(dev) if dev is not None else enc


def _torch_path(enc, x):
    from nerfacc_amd import _backend as B
    from nerfacc_amd.encodings import _planegrid_torch
    return _planegrid_torch(x, enc.params.detach(), enc.table, B.PLANE_REDUCE_CODES[enc.reduce])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tol(ref, part=1.0):
    return dict(rtol=1e-4 * part, atol=1e-3 * part * float(ref.abs().mean()))


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("F", [4, 8, 16, 32])
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("D", [3, 4])
def test_forward_bit_for_bit(dev, D, reduce, F):
    per_wave = 64 // F
    g = torch.Generator().manual_seed(F)
    for ms in [(1,), MS]:
        enc = _enc(D, reduce, F, ms=ms, dev=dev)
        for n in sorted({1, per_wave - 1, per_wave, per_wave + 1, 1000}):
            x = (torch.rand(n, D, generator=g) * 1.4 - 0.2).to(dev)
            y = enc(x)
            want = _torch_path(enc, x)
            assert y.shape == (n, len(ms) * F) and y.dtype == torch.float32
            assert torch.equal(_bits(y), _bits(want)), (ms, n)


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("F", [4, 32])
@pytest.mark.parametrize("D", [3, 4])
def test_half_outputs_are_the_float32_result_rounded_once(dev, D, F, half):
    enc = _enc(D, "product", F, dev=dev)
    x = (torch.rand(1000, D, generator=torch.Generator().manual_seed(2)) * 1.4 - 0.2).to(dev)
    y32 = enc(x)
    enc.out_dtype = half
    yh = enc(x)
    assert yh.dtype == half and torch.equal(_bits(yh), _bits(y32.to(half)))
    with torch.autocast("cuda", dtype=half):
        enc.out_dtype = "autocast"
        assert enc(x).dtype == half
        enc.out_dtype = None
        assert enc(x).dtype == torch.float32


# ----------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _bwd_case(D, reduce, F, g_dtype=torch.float32):
    """(enc on the CPU, x, g, reference dL/dx, reference dL/dparams): computed once per configuration, never modified.
    The incoming gradient is rounded to ``g_dtype`` before the reference sees it."""
    enc = _enc(D, reduce, F)
    x = R.off_node_points(N_BWD, RES[D], MS, seed=100 + D, lo=-0.1, hi=1.1)
    g = torch.randn(N_BWD, enc.n_output_dims, generator=torch.Generator().manual_seed(9)).to(g_dtype)
    xr, pr = x.double().requires_grad_(True), enc.params.detach().double().requires_grad_(True)
    rx, rp = torch.autograd.grad(R.planegrid_reference(xr, pr, RES[D], MS, F, reduce), (xr, pr), g.double())
    return enc, x, g, rx, rp


@pytest.mark.parametrize("F", [8, 32])
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("D", [3, 4])
def test_backward_against_the_float64_reference(dev, D, reduce, F):
    cpu, x, g, rx, rp = _bwd_case(D, reduce, F)
    # the inputs are fit for the tolerance: float32 arithmetic alone (the torch path, here on the CPU) uses a quarter of it
    xc = x.clone().requires_grad_(True)
    cx, cp = torch.autograd.grad(cpu(xc), (xc, cpu.params), g)
    torch.testing.assert_close(cx.double(), rx, **_tol(rx, 0.25))
    torch.testing.assert_close(cp.double(), rp, **_tol(rp, 0.25))

    enc = _enc(D, reduce, F, dev=dev)
    xd, gd = x.to(dev).requires_grad_(True), g.to(dev)
    gx, gp = torch.autograd.grad(enc(xd), (xd, enc.params), gd)
    print(f"D={D} {reduce} F={F}: max|dx err| {float((gx.cpu().double() - rx).abs().max()):.3e} (atol {_tol(rx)['atol']:.3e}), "
          f"max|dp err| {float((gp.cpu().double() - rp).abs().max()):.3e} (atol {_tol(rp)['atol']:.3e})")
    torch.testing.assert_close(gx.cpu().double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.cpu().double(), rp, **_tol(rp))
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


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D,reduce,F", [(3, "sum", 4), (4, "product", 16)])
def test_half_gradient_is_read_directly(dev, D, reduce, F, half):
    _, x, g, rx, rp = _bwd_case(D, reduce, F, half)
    enc = _enc(D, reduce, F, dev=dev, out_dtype=half)
    xd = x.to(dev).requires_grad_(True)
    y = enc(xd)
    assert y.dtype == half
    gx, gp = torch.autograd.grad(y, (xd, enc.params), g.to(dev))
    assert gx.dtype == torch.float32 and gp.dtype == torch.float32
    torch.testing.assert_close(gx.cpu().double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.cpu().double(), rp, **_tol(rp))


def test_second_order_is_refused(dev):
    enc = _enc(3, "product", 4, dev=dev)
    x = torch.rand(10, 3, device=dev).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    assert gx.requires_grad                                        # create_graph=True alone is harmless
    with pytest.raises(NotImplementedError, match="PlaneGridEncoding: the second order"):
        gx.sum().backward()


# ----------------------------------------------------------------------------- edge inputs and input forms
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("D", [3, 4])
def test_edge_inputs(dev, D, reduce):
    enc = _enc(D, reduce, 8, dev=dev)
    x = R.edge_points(D).to(dev).requires_grad_(True)
    y = enc(x)
    assert torch.equal(_bits(y), _bits(_torch_path(enc, x.detach()))) and torch.isfinite(y).all()
    gx, gp = torch.autograd.grad(y, (x, enc.params), torch.ones_like(y))
    assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
    assert (gx[3:10, 0] == 0).all() and (gx[10:] == 0).all() and (gx[:10, 1:] != 0).all()
    # every add landed in its place: the table gradient is the torch path's (autograd, on the CPU; it takes NaN rows)
    cpu = _enc(D, reduce, 8)
    yc = cpu(x.detach().cpu())
    (cp,) = torch.autograd.grad(yc, cpu.params, torch.ones_like(yc))
    torch.testing.assert_close(gp.cpu(), cp, **_tol(cp))


def test_input_forms(dev):
    enc = _enc(4, "product", 8, dev=dev)
    g = torch.Generator().manual_seed(4)
    # empty
    y = enc(torch.empty(0, 4, device=dev))
    assert y.shape == (0, 16)
    x0 = torch.empty(0, 4, device=dev, requires_grad=True)
    gx, gp = torch.autograd.grad(enc(x0).sum(), (x0, enc.params))
    assert gx.shape == (0, 4) and (gp == 0).all()
    # leading batch dimensions
    x = torch.rand(3, 5, 4, generator=g).to(dev)
    y = enc(x)
    assert y.shape == (3, 5, 16) and torch.equal(_bits(y.view(15, 16)), _bits(_torch_path(enc, x.view(15, 4))))
    # a non-contiguous x, and one whose first element is 4 bytes past a 16-byte boundary
    wide = torch.rand(33, 7, generator=g).to(dev)
    xs = wide[:, 1:5]
    assert not xs.is_contiguous()
    assert torch.equal(_bits(enc(xs)), _bits(_torch_path(enc, xs.contiguous())))
    buf = torch.rand(33 * 4 + 1, generator=g).to(dev)
    xm = buf[1:].view(33, 4)
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
    enc = _enc(3, "product", 16, dev=dev)
    x = torch.rand(100, 3, device=dev, requires_grad=True)
    want = _torch_path(enc, x.detach())
    monkeypatch.setattr(encodings, "_planegrid_torch", boom)
    y = enc(x)
    assert torch.equal(_bits(y), _bits(want))
    y.sum().backward()
    assert x.grad is not None and enc.params.grad is not None and enc.params.grad.abs().sum() > 0

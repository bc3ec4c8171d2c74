"""GPU: the native dense voxel grid (DVGO / TiNeuVox) passes of csrc/voxgrid.hip -- the forward bit for bit against the
torch restatement, the backward against the float64 grid_sample form of tests/voxgrid_reference.py, the reproducible dL/dx,
half element types, edge inputs, the input forms the module accepts, the resampling, a table beyond 4 GiB and graph capture."""
import functools

import pytest
import torch

import voxgrid_reference as R

pytestmark = pytest.mark.gpu

RESOLUTIONS = [R.RES_SMALL, R.RES_TINY, R.RES_ODD, R.RES_WIDE]
STRIDES = [(1,), (1, 2, 4), (2,)]
N_BWD = 1000


def _legal(res, strides):
    return all(-(-r // s) >= 2 for r in res for s in strides)


def _enc(res, C, strides=(1,), dev=None, **kw):
    from nerfacc_amd.encodings import VoxelGridEncoding
    torch.manual_seed(17 * C + len(strides) + res[0])
    enc = VoxelGridEncoding(res, C, strides, **kw)
    with torch.no_grad():
        enc.params.uniform_(-1.0, 1.0)
    return enc.to(dev) if dev is not None else enc


def _torch_path(enc, x):
    from nerfacc_amd.encodings import _voxgrid_torch
    return _voxgrid_torch(x, enc.params.detach(), enc.table)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tol(ref, part=1.0):
    return dict(rtol=1e-4 * part, atol=1e-3 * part * float(ref.detach().abs().mean()))


def _lanes(C):
    return 1 if C <= 2 else next(w for w in (32, 16, 8, 4) if C % w == 0)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("C", [1, 2, 4, 12, 16, 48, 64])
@pytest.mark.parametrize("strides", STRIDES)
def test_forward_bit_for_bit(dev, strides, C):
    per_wave = 64 // _lanes(C)
    g = torch.Generator().manual_seed(C)
    ran = 0
    for res in RESOLUTIONS:
        if not _legal(res, strides):      # (2, 2, 2) has stride 1 only, (5, 4, 7) no stride 4: the constructor refuses them
            continue
        enc = _enc(res, C, strides, dev=dev)
        for n in sorted({1, per_wave - 1, per_wave, per_wave + 1, 1000}):
            x = (torch.rand(n, 3, generator=g) * 1.4 - 0.2).to(dev)
            y = enc(x)
            want = _torch_path(enc, x)
            assert y.shape == (n, C * len(strides)) and y.dtype == torch.float32
            assert torch.equal(_bits(y), _bits(want)), (res, n)
            ran += 1
    assert ran >= 8      # at least two resolutions, four point counts each (C = 64: a wave holds 2 points, so 1 = per-wave - 1)


@pytest.mark.parametrize("C", [1, 2, 12, 48])
def test_edge_inputs(dev, C):
    res, strides = R.RES_ODD, (1, 2, 4)
    enc = _enc(res, C, strides, dev=dev)
    x = R.edge_rows(res).to(dev).requires_grad_(True)
    y = enc(x)
    assert torch.equal(_bits(y), _bits(_torch_path(enc, x.detach()))) and torch.isfinite(y).all()
    gx, gp = torch.autograd.grad(y, (x, enc.params), torch.ones_like(y))
    assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
    assert (gx[3:10, 0] == 0).all() and (gx[10:13] == 0).all() and (gx[:10, 1:] != 0).all() and (gx[:2, 0] != 0).all()
    # every add landed in its place: the table gradient is the torch path's (autograd, on the CPU; it takes NaN rows)
    cpu = _enc(res, C, strides)
    yc = cpu(x.detach().cpu())
    (cp,) = torch.autograd.grad(yc, cpu.params, torch.ones_like(yc))
    torch.testing.assert_close(gp.cpu(), cp, **_tol(cp))


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,strides", [(1, (1,)), (12, (1, 2, 4)), (64, (2,))])
def test_half_outputs_are_the_float32_result_rounded_once(dev, C, strides, half):
    enc = _enc(R.RES_WIDE, C, strides, dev=dev)
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
    enc.out_dtype = "autocast"
    assert enc(x).dtype == torch.float32                                             # no autocast active: float32


# ----------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _bwd_case(res, C, strides, g_dtype=torch.float32, one_cell=False, fixed_axis=None):
    """(enc on the CPU, x, g, reference dL/dx, reference dL/dparams): computed once per configuration, never modified.
    The incoming gradient is rounded to ``g_dtype`` before the reference sees it.  ``one_cell``: every point lies inside one
    cell of the stride-1 grid, so all of them add into the same 8 nodes (a coarser stride's cells do not nest in it: there
    they share a few more).  ``fixed_axis``: every point has the same coordinate on that axis."""
    enc = _enc(res, C, strides)
    if one_cell:
        cell = torch.tensor([2.0, 3.0, 4.0])
        rm1 = torch.tensor([r - 1.0 for r in res])
        x = R.off_node_points(N_BWD, res, strides, seed=100 + C, lo=(cell + 0.02) / rm1, hi=(cell + 0.98) / rm1)
        assert all(len(torch.unique(torch.floor(x[:, d].double() * (res[d] - 1)))) == 1 for d in range(3))
    else:
        x = R.off_node_points(N_BWD, res, strides, seed=100 + C, lo=-0.1, hi=1.1)
    if fixed_axis is not None:
        x[:, fixed_axis] = x[0, fixed_axis].clamp(0.05, 0.95)
    g = torch.randn(N_BWD, enc.n_output_dims, generator=torch.Generator().manual_seed(9)).to(g_dtype)
    xr, pr = x.double().requires_grad_(True), enc.params.detach().double().requires_grad_(True)
    rx, rp = torch.autograd.grad(R.voxgrid_reference(xr, pr, res, C, strides), (xr, pr), g.double())
    return enc, x, g, rx, rp


def _check_cpu_float32(cpu, x, g, rx, rp):
    """The inputs are fit for the tolerance: float32 arithmetic alone (the torch path, on the CPU) uses a quarter of it."""
    xc = x.clone().requires_grad_(True)
    cx, cp = torch.autograd.grad(cpu(xc), (xc, cpu.params), g)
    torch.testing.assert_close(cx.double(), rx, **_tol(rx, 0.25))
    torch.testing.assert_close(cp.double(), rp, **_tol(rp, 0.25))


def _native_grads(case, dev, label):
    cpu, x, g, rx, rp = case
    enc = _enc(cpu.resolution, cpu.n_features, cpu.strides, dev=dev)
    xd, gd = x.to(dev).requires_grad_(True), g.to(dev)
    gx, gp = torch.autograd.grad(enc(xd), (xd, enc.params), gd)
    print(f"{label}: max|dx err| {float((gx.cpu().double() - rx).abs().max()):.3e} (atol {_tol(rx)['atol']:.3e}), "
          f"max|dp err| {float((gp.cpu().double() - rp).abs().max()):.3e} (atol {_tol(rp)['atol']:.3e})")
    torch.testing.assert_close(gx.cpu().double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.cpu().double(), rp, **_tol(rp))
    return enc, xd, gd, gx, gp


@pytest.mark.parametrize("C,strides", [(1, (1,)), (2, (1, 2, 4)), (12, (1, 2, 4)), (12, (1,)), (16, (2,)), (64, (1, 2))])
def test_backward_against_the_float64_reference(dev, C, strides):
    res = R.RES_ODD
    case = _bwd_case(res, C, strides)
    cpu, x, g, rx, rp = case
    _check_cpu_float32(*case)
    enc, xd, gd, gx, gp = _native_grads(case, dev, f"C={C} {strides} {res}")
    outside = (x < 0) | (x > 1)
    assert outside.any() and (gx.cpu()[outside] == 0).all()

    # dL/dx: the same bits on a second run, and when it is asked for alone; dL/dparams alone is the same sum
    gx2, _ = torch.autograd.grad(enc(xd), (xd, enc.params), gd)
    assert torch.equal(_bits(gx), _bits(gx2))
    (gx_alone,) = torch.autograd.grad(enc(xd), xd, gd)
    assert torch.equal(_bits(gx), _bits(gx_alone))
    torch.testing.assert_close(gx_alone.cpu().double(), rx, **_tol(rx))
    (gp_alone,) = torch.autograd.grad(enc(xd.detach()), enc.params, gd)
    torch.testing.assert_close(gp_alone.cpu().double(), rp, **_tol(rp))
    torch.testing.assert_close(gp_alone, gp, rtol=1e-4, atol=_tol(rp)["atol"])


def _backward_pointers(monkeypatch):
    """Records (grad_params, grad_x) of every nfa_voxgrid_bwd call: the pointers the kernel is given."""
    from nerfacc_amd import _backend as B
    seen, call = [], B.call

    def logged(name, *args):
        if name == "nfa_voxgrid_bwd":
            seen.append((args[-3], args[-2]))
        return call(name, *args)
    monkeypatch.setattr(B, "call", logged)
    return seen


@pytest.mark.parametrize("C,strides", [(1, (1,)), (1, (2,)), (2, (1, 2, 4)), (12, (1, 2, 4)), (16, (2,)), (64, (1, 2))])
def test_each_gradient_alone_is_a_null_pointer_for_the_other(dev, monkeypatch, C, strides):
    """A frozen grid with trainable points hands the kernel a null grad_params, fixed points a null grad_x: dL/dx is then bit
    for bit the both-gradients run's and within the tolerance of the reference, dL/dparams within the tolerance of both."""
    case = _bwd_case(R.RES_ODD, C, strides)
    _, x, g, rx, rp = case
    enc, xd, gd, gx, gp = _native_grads(case, dev, f"C={C} {strides}")
    seen = _backward_pointers(monkeypatch)
    # x only: the table does not require a gradient
    enc.params.requires_grad_(False)
    (gx_only,) = torch.autograd.grad(enc(xd), xd, gd)
    assert len(seen) == 1 and seen[0][0] is None and seen[0][1] is not None
    assert torch.equal(_bits(gx_only), _bits(gx))
    torch.testing.assert_close(gx_only.cpu().double(), rx, **_tol(rx))
    outside = (x < 0) | (x > 1)
    assert outside.any() and (gx_only.cpu()[outside] == 0).all()
    # a half incoming gradient on that path, against the reference fed the rounded gradient
    _, xh, gh, rxh, _ = _bwd_case(R.RES_ODD, C, strides, torch.bfloat16)
    assert torch.equal(xh, x)
    enc.out_dtype = torch.bfloat16
    (gx_half,) = torch.autograd.grad(enc(xd), xd, gh.to(dev))
    enc.out_dtype = None
    assert seen[1][0] is None
    torch.testing.assert_close(gx_half.cpu().double(), rxh, **_tol(rxh))
    # params only: the points do not require a gradient
    enc.params.requires_grad_(True)
    (gp_only,) = torch.autograd.grad(enc(xd.detach()), enc.params, gd)
    assert len(seen) == 3 and seen[2][1] is None and seen[2][0] is not None
    torch.testing.assert_close(gp_only.cpu().double(), rp, **_tol(rp))
    torch.testing.assert_close(gp_only, gp, rtol=1e-4, atol=_tol(rp)["atol"])


@pytest.mark.parametrize("C,strides", [(1, (1,)), (12, (1, 2, 4)), (48, (1,))])
def test_backward_with_all_points_in_one_cell(dev, C, strides):
    case = _bwd_case(R.RES_ODD, C, strides, one_cell=True)
    _check_cpu_float32(*case)
    _, _, _, _, gp = _native_grads(case, dev, f"one cell, C={C} {strides}")
    if strides == (1,):
        assert int((gp.view(-1, C) != 0).any(-1).sum()) <= 8      # every atomic contends for the same 8 nodes


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_backward_with_one_fixed_coordinate(dev, axis):
    case = _bwd_case(R.RES_ODD, 12, (1, 2, 4), fixed_axis=axis)
    assert (case[1][:, axis] == case[1][0, axis]).all()
    _check_cpu_float32(*case)
    _native_grads(case, dev, f"fixed coordinate on axis {axis}")


@pytest.mark.parametrize("C,strides", [(12, (1, 2, 4)), (1, (1,)), (1, (1, 2))])
def test_grad_x_is_bitwise_reproducible(dev, C, strides):
    """C = 12 has three rounds per lane; C = 1 one lane per point.  Two runs and a run at another launch size (the point
    duplicated) give the same bits."""
    enc = _enc(R.RES_WIDE, C, strides, dev=dev)
    gen = torch.Generator().manual_seed(31)
    x = (torch.rand(3001, 3, generator=gen) * 1.2 - 0.1).to(dev).requires_grad_(True)
    g = torch.randn(3001, enc.n_output_dims, generator=gen).to(dev)
    (a,) = torch.autograd.grad(enc(x), x, g)
    (b,) = torch.autograd.grad(enc(x), x, g)
    assert torch.equal(_bits(a), _bits(b)) and (a != 0).any()
    x2 = torch.cat([x.detach(), x.detach()]).requires_grad_(True)
    (c,) = torch.autograd.grad(enc(x2), x2, torch.cat([g, g]))
    assert torch.equal(_bits(c[:3001]), _bits(a)) and torch.equal(_bits(c[3001:]), _bits(a))
    enc.params.requires_grad_(False)                               # without the table gradient (a null grad_params): the same bits
    (d,) = torch.autograd.grad(enc(x), x, g)
    assert torch.equal(_bits(d), _bits(a))


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,strides", [(2, (1,)), (12, (1, 2, 4))])
def test_half_gradient_is_read_directly(dev, C, strides, half):
    _, x, g, rx, rp = _bwd_case(R.RES_ODD, C, strides, half)
    enc = _enc(R.RES_ODD, C, strides, dev=dev, out_dtype=half)
    xd = x.to(dev).requires_grad_(True)
    y = enc(xd)
    assert y.dtype == half
    gx, gp = torch.autograd.grad(y, (xd, enc.params), g.to(dev))
    assert gx.dtype == torch.float32 and gp.dtype == torch.float32
    torch.testing.assert_close(gx.cpu().double(), rx, **_tol(rx))
    torch.testing.assert_close(gp.cpu().double(), rp, **_tol(rp))


# ----------------------------------------------------------------------------- input forms
def test_input_forms(dev):
    enc = _enc(R.RES_SMALL, 12, (1, 2), dev=dev)
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
    # float64 and CPU inputs take the torch path
    xd = torch.rand(20, 3, generator=g, dtype=torch.float64).to(dev)
    yd = enc(xd)
    assert yd.dtype == torch.float64
    ref = R.voxgrid_reference(xd.cpu(), enc.params.detach().cpu(), enc.resolution, 12, enc.strides)
    torch.testing.assert_close(yd.cpu(), ref, **_tol(ref))
    cpu = _enc(R.RES_SMALL, 12, (1, 2))
    xc = torch.rand(20, 3, generator=g)
    yc = cpu(xc)
    assert not yc.is_cuda
    torch.testing.assert_close(enc(xc.to(dev)).cpu(), yc, **_tol(yc))


def test_native_path_is_taken(dev, monkeypatch):
    from nerfacc_amd import encodings

    def boom(*a, **k):
        raise AssertionError("the torch path ran for a float32 tensor on the device")
    enc = _enc(R.RES_ODD, 12, (1, 2, 4), dev=dev)
    x = torch.rand(100, 3, device=dev, requires_grad=True)
    want = _torch_path(enc, x.detach())
    small = enc.resampled((9, 5, 6))
    monkeypatch.setattr(encodings, "_voxgrid_torch", boom)
    monkeypatch.setattr(encodings, "_voxel_resample_torch", boom)
    y = enc(x)
    assert torch.equal(_bits(y), _bits(want))
    y.sum().backward()
    assert x.grad is not None and enc.params.grad is not None and enc.params.grad.abs().sum() > 0
    again = enc.resampled((9, 5, 6))
    assert again.params.is_cuda and torch.equal(_bits(again.params.detach()), _bits(small.params.detach()))


# ----------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("C", [1, 2, 12, 64])
@pytest.mark.parametrize("src,dst", [(R.RES_SMALL, (13, 9, 20)), (R.RES_WIDE, (8, 40, 9)), (R.RES_WIDE, R.RES_WIDE),
                                     (R.RES_TINY, (5, 5, 5)), (R.RES_ODD, (66, 3, 9))])
def test_resampled(dev, src, dst, C):
    from nerfacc_amd.encodings import _voxel_resample_torch
    enc = _enc(src, C, dev=dev)
    new = enc.resampled(dst)
    assert new.params.device == enc.params.device and new.resolution == tuple(dst) and new.params.requires_grad
    assert isinstance(new.params, torch.nn.Parameter) and new.params.is_leaf and new.params.grad_fn is None
    want = _voxel_resample_torch(enc.params.detach(), enc.table, new.table)
    assert torch.equal(_bits(new.params.detach()), _bits(want))
    ref = R.resample_reference(enc.params.detach().cpu(), src, dst, C)
    torch.testing.assert_close(new.params.detach().cpu().double(), ref, **_tol(ref))
    if tuple(src) == tuple(dst):
        assert torch.equal(_bits(new.params.detach()), _bits(enc.params.detach()))
    x = (torch.rand(300, 3, generator=torch.Generator().manual_seed(6)) * 1.2 - 0.1).to(dev).requires_grad_(True)
    y = new(x)
    assert torch.equal(_bits(y), _bits(_torch_path(new, x.detach())))
    gx, gp = torch.autograd.grad(y.sum(), (x, new.params))
    assert torch.isfinite(gx).all() and gp.shape == new.params.shape


# ----------------------------------------------------------------------------- a table beyond 4 GiB
def test_table_beyond_4_gib(dev):
    """(1024, 1024, 260) x 4 features: 1.09 G floats, 4.36 GB, so a 32-bit byte offset wraps in the top z-slabs."""
    from nerfacc_amd.encodings import VoxelGridEncoding
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 12 * 10 ** 9:
        pytest.skip(f"needs about 9 GB of device memory, {free / 1e9:.1f} GB are free")
    res, C, n = (1024, 1024, 260), 4, 300
    enc = VoxelGridEncoding.__new__(VoxelGridEncoding)              # (no 4 GB random table is drawn on the host)
    torch.nn.Module.__init__(enc)
    enc._configure(res, C, (1,), 0.1, None)
    slab = res[0] * res[1] * C
    assert enc.table.n_params == slab * res[2] and enc.table.n_params * 4 > 1 << 32 and enc.table.n_params < 1 << 31
    p = torch.zeros(enc.table.n_params, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(12)
    p[-2 * slab:] = (torch.rand(2 * slab, generator=gen) * 2.0 - 1.0).to(dev)
    enc.params = torch.nn.Parameter(p)
    x = torch.rand(n, 3, generator=gen)
    x[:, 2] = (res[2] - 2 + 0.05 + 0.9 * x[:, 2]) / (res[2] - 1)     # z in the top cell
    x = x.to(dev).requires_grad_(True)
    y = enc(x)
    want = _torch_path(enc, x.detach())
    assert torch.equal(_bits(y), _bits(want)) and (y != 0).all()
    g = torch.randn(n, C, generator=gen).to(dev)
    gx, gp = torch.autograd.grad(y, (x, enc.params), g)
    assert torch.isfinite(gx).all() and (gx != 0).any()
    assert not bool(gp[:-2 * slab].any())                          # nothing wrapped into the low part of the table
    got, ref = gp[-2 * slab:].view(-1, C).double().sum(0).cpu(), g.double().sum(0).cpu()
    print(f"beyond 4 GiB: per-channel sums {got.tolist()} against {ref.tolist()}")
    torch.testing.assert_close(got, ref, **_tol(ref))


# ----------------------------------------------------------------------------- capture
def test_captured_step_replays_the_eager_bytes(dev):
    from nerfacc_amd.graphs import CapturedStep
    enc = _enc(R.RES_WIDE, 12, (1, 2, 4), dev=dev, out_dtype=torch.float16)
    gen = torch.Generator().manual_seed(21)
    xs = (torch.rand(4097, 3, generator=gen) * 1.2 - 0.1).to(dev).requires_grad_(True)
    gs = torch.randn(4097, enc.n_output_dims, generator=gen).to(dev).half()
    eager_x, eager_p = torch.autograd.grad(enc(xs), (xs, enc.params), gs)
    eager_x = eager_x.clone()
    step = CapturedStep(lambda: torch.autograd.grad(enc(xs), (xs, enc.params), gs), warmup=1)   # torch.cuda.graph inside
    for _ in range(2):
        for t in step.outputs:
            t.fill_(float("nan"))
        g_x, g_p = step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(g_x), _bits(eager_x))
        torch.testing.assert_close(g_p, eager_p, rtol=1e-4, atol=1e-3 * float(eager_p.abs().mean()))

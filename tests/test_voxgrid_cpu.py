"""CPU: the dense voxel grid (DVGO / TiNeuVox) encoding -- the torch path against the float64 grid_sample form of
tests/voxgrid_reference.py in value and gradient, the parameter layout with ``grid()`` / ``load_grid``, ``resampled`` against
F.interpolate, edge inputs, the constructor's refusals, the three C entries' argument checks (stand-in pointers, no device)
and the pins the addition must not move.  The refusal of the second order on the native path is the one GPU case."""
import ctypes

import pytest
import torch

import voxgrid_reference as R

# (resolution, strides): non-cubic grids, R = 2, and strides that do not divide R - 1
SHAPES = [(R.RES_SMALL, (1,)), (R.RES_SMALL, (1, 2)), (R.RES_TINY, (1,)), (R.RES_ODD, (1, 2, 4)), (R.RES_ODD, (2,)),
          (R.RES_WIDE, (1, 2, 4, 8))]
FEATURES = [1, 2, 4, 12]


def _enc(res=R.RES_SMALL, C=4, strides=(1,), **kw):
    from nerfacc_amd.encodings import VoxelGridEncoding
    torch.manual_seed(13 * C + len(strides))
    enc = VoxelGridEncoding(res, C, strides, **kw)
    with torch.no_grad():
        enc.params.uniform_(-1.0, 1.0)
    return enc


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


F64 = dict(rtol=0.0, atol=1e-12)   # float64 against float64: the issue's bound


# ----------------------------------------------------------------------------- the torch path against the reference
@pytest.mark.parametrize("C", FEATURES)
@pytest.mark.parametrize("res,strides", SHAPES)
def test_torch_path_values(res, strides, C):
    from nerfacc_amd.encodings import _voxgrid_torch
    enc = _enc(res, C, strides)
    x = torch.rand(600, 3, generator=torch.Generator().manual_seed(C), dtype=torch.float64) * 1.4 - 0.2
    x[:4] = torch.tensor([0.0, 1.0, 0.5, 0.25], dtype=torch.float64)[:, None]      # nodes and borders are fine for values
    x[4] = torch.tensor([-1e30, 0.3, 1e30], dtype=torch.float64)
    edges = R.edge_rows(res).double()
    x = torch.cat([x, edges[torch.isfinite(edges).all(-1)]])                       # (grid_sample's NaN / inf rule is not ours)
    got = _voxgrid_torch(x, enc.params.detach().double(), enc.table)
    ref = R.voxgrid_reference(x, enc.params.detach(), res, C, strides)
    assert got.shape == (x.shape[0], C * len(strides)) == ref.shape and got.dtype == torch.float64
    assert enc.n_output_dims == got.shape[1]
    torch.testing.assert_close(got, ref, **F64)
    assert torch.equal(enc.double()(x), got)                                        # the module's float64 path is that function
    y32 = _enc(res, C, strides)(x.float())
    assert y32.dtype == torch.float32
    torch.testing.assert_close(y32.double(), ref, **_tol(ref))


@pytest.mark.parametrize("C", [1, 12])
@pytest.mark.parametrize("res,strides", [(R.RES_SMALL, (1, 2)), (R.RES_ODD, (1, 2, 4))])
def test_torch_path_gradients(res, strides, C):
    enc = _enc(res, C, strides).double()
    x = R.off_node_points(500, res, strides, seed=C, lo=-0.2, hi=1.2).double().requires_grad_(True)
    g = torch.randn(500, enc.n_output_dims, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gx, gp = torch.autograd.grad(enc(x), (x, enc.params), g)
    xr, pr = x.detach().clone().requires_grad_(True), enc.params.detach().clone().requires_grad_(True)
    rx, rp = torch.autograd.grad(R.voxgrid_reference(xr, pr, res, C, strides), (xr, pr), g)
    torch.testing.assert_close(gx, rx, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(gp, rp, rtol=1e-10, atol=1e-12)
    outside = (x.detach() < 0) | (x.detach() > 1)
    assert outside.any() and (gx[outside] == 0).all()


def test_strides_are_the_sliced_grids():
    """Stride s of an R-node grid is stride 1 of the grid [::s, ::s, ::s], bit for bit (any R: the last node is s (n - 1))."""
    res, C = R.RES_ODD, 4
    enc = _enc(res, C, (1, 2, 4))
    x = torch.rand(300, 3, generator=torch.Generator().manual_seed(8)) * 1.2 - 0.1
    y = enc(x).detach()
    for k, s in enumerate(enc.strides):
        sub = enc.grid().detach()[::s, ::s, ::s].contiguous()
        small = _enc(tuple(sub.shape[2::-1]), C)
        assert small.resolution == tuple(-(-r // s) for r in res)
        with torch.no_grad():
            small.params.copy_(sub.reshape(-1))
        assert torch.equal(small(x).detach(), y[:, k * C: (k + 1) * C])


# ----------------------------------------------------------------------------- layout
def test_grid_and_load_grid():
    import torch.nn.functional as TF
    res, C = R.RES_SMALL, 12
    enc = _enc(res, C)
    g = enc.grid()
    assert g.shape == (res[2], res[1], res[0], C) and g.data_ptr() == enc.params.data_ptr()      # a view, x fastest
    assert enc.params.shape == (res[0] * res[1] * res[2] * C,) and enc.n_input_dims == 3 and enc.n_output_dims == C
    assert float(g.detach()[3, 2, 1, 5]) == float(enc.params.detach()[((3 * res[1] + 2) * res[0] + 1) * C + 5])
    dvgo = g.detach().permute(3, 2, 1, 0)[None]
    assert dvgo.shape == (1, C, *res)
    # the permute of the docstring gives the tensor DVGO samples, with its flipped coordinates
    x = R.off_node_points(50, res, (1,), seed=3)
    want = TF.grid_sample(dvgo.double(), (2.0 * x.double() - 1.0).flip(-1)[None, None, None], mode="bilinear", padding_mode="border",
                          align_corners=True)[0, :, 0, 0].t()
    torch.testing.assert_close(enc(x).double(), want, **_tol(want))
    # load_grid round-trips both forms
    t = torch.randn(1, C, *res, generator=torch.Generator().manual_seed(5))
    for form in (t, t[0]):
        other = _enc(res, C)
        other.load_grid(form)
        assert torch.equal(other.grid().detach().permute(3, 2, 1, 0)[None], t)
        assert float(other.params[((3 * res[1] + 2) * res[0] + 1) * C + 5]) == float(t[0, 5, 1, 2, 3])
    for bad in (t[:, :4], t.permute(0, 1, 4, 3, 2), t[0, 0]):
        with pytest.raises(ValueError, match="VoxelGridEncoding.load_grid: the grid must have shape"):
            enc.load_grid(bad)
    assert "n_features=12" in repr(enc) and "resolution=(5, 4, 7)" in repr(enc) and "strides=(1,)" in repr(enc)


def test_initialisation():
    from nerfacc_amd.encodings import VoxelGridEncoding as E
    enc = E((32, 32, 32))
    assert enc.n_features == 12 and enc.strides == (1,) and enc.params.dtype == torch.float32 and enc.params.requires_grad
    p = enc.params.detach()
    assert abs(float(p.mean())) < 0.005 and abs(float(p.std()) - 0.1) < 0.005 and float(p.abs().max()) > 0.3
    enc = E((32, 32, 32), 1, init_scale=0.5)
    assert abs(float(enc.params.detach().std()) - 0.5) < 0.02 and "init_scale=0.5" in repr(enc)


# ----------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("C", [1, 12])
@pytest.mark.parametrize("src,dst", [(R.RES_SMALL, (13, 9, 20)), (R.RES_WIDE, (8, 5, 9)), (R.RES_TINY, (5, 5, 5)),
                                     (R.RES_ODD, (3, 7, 20))])
def test_resampled(src, dst, C):
    from nerfacc_amd.encodings import _voxel_resample_torch
    enc = _enc(src, C, (1, 2), out_dtype=torch.bfloat16) if min(src) > 2 and min(dst) > 2 else _enc(src, C, out_dtype=torch.bfloat16)
    new = enc.resampled(dst)
    assert type(new) is type(enc) and new.resolution == tuple(dst) and new.n_features == C and new.strides == enc.strides
    assert new.out_dtype == torch.bfloat16 and new.params.requires_grad and new.params.device == enc.params.device
    assert new.params.shape == (new.table.n_params,) and new.params.grad_fn is None and new.params.dtype == torch.float32
    assert new.params.is_leaf and isinstance(new.params, torch.nn.Parameter)
    ref = R.resample_reference(enc.params.detach(), src, dst, C)
    torch.testing.assert_close(new.params.detach().double(), ref, **_tol(ref))
    # in float64 the torch form is F.interpolate's arithmetic
    torch.testing.assert_close(_voxel_resample_torch(enc.params.detach().double(), enc.table, new.table), ref, rtol=1e-10, atol=1e-12)
    # the corner nodes are the source's corner nodes (align_corners)
    torch.testing.assert_close(new.grid()[0, 0, 0], enc.grid()[0, 0, 0])
    torch.testing.assert_close(new.grid()[-1, -1, -1], enc.grid()[-1, -1, -1])
    torch.testing.assert_close(new.grid()[0, -1, 0], enc.grid()[0, -1, 0])


def test_resampled_identity():
    enc = _enc(R.RES_WIDE, 12, (1, 2, 4))
    new = enc.resampled(R.RES_WIDE)
    assert new is not enc and new.params.data_ptr() != enc.params.data_ptr()
    assert torch.equal(new.params.detach().view(torch.int32), enc.params.detach().view(torch.int32))
    x = torch.rand(100, 3)
    assert torch.equal(new(x), enc(x))


# ----------------------------------------------------------------------------- edge inputs
@pytest.mark.parametrize("C", [1, 4])
def test_edge_inputs(C):
    res, strides = R.RES_ODD, (1, 2, 4)
    enc = _enc(res, C, strides)
    x = R.edge_points(3).requires_grad_(True)
    y = enc(x)
    assert torch.isfinite(y).all()
    for row, border in [(2, 0), (3, 0), (5, 0), (8, 0), (9, 0), (4, 1), (6, 1), (7, 1)]:   # clamped: the border's values
        assert torch.equal(y[row], y[border]), (row, border)
    node0 = torch.cat([enc.grid().detach()[0, 0, 0]] * len(strides))
    assert torch.equal(y[10], node0) and torch.equal(y[12], node0)                        # NaN and -inf sample node 0
    gx, gp = torch.autograd.grad(y, (x, enc.params), torch.ones_like(y))
    assert torch.isfinite(gx).all() and torch.isfinite(gp).all()
    assert (gx[3:10, 0] == 0).all() and (gx[10:] == 0).all() and (gx[:10, 1:] != 0).all() and (gx[:2, 0] != 0).all()


@pytest.mark.parametrize("C", [2, 12])
def test_table_gradient_sums_to_the_incoming_gradient(C):
    """The eight weights of a stride sum to 1: per channel, dL/dparams sums to the sum of g, stride by stride and together."""
    res, strides = R.RES_ODD, (1, 2, 4)
    x = torch.cat([R.edge_rows(res), torch.rand(200, 3, generator=torch.Generator().manual_seed(2)) * 1.4 - 0.2])
    g = torch.randn(x.shape[0], C * len(strides), generator=torch.Generator().manual_seed(3))
    total = torch.zeros(C, dtype=torch.float64)
    for k, s in enumerate(strides):
        enc = _enc(res, C, (s,))
        gk = g[:, k * C: (k + 1) * C]
        (gp,) = torch.autograd.grad(enc(x), enc.params, gk)
        want = gk.double().sum(0)
        torch.testing.assert_close(gp.view(-1, C).double().sum(0), want, rtol=1e-4, atol=1e-3 * float(gk.abs().mean()))
        off_stride = gp.view(res[2], res[1], res[0], C)[1::s] if s > 1 else gp.new_zeros(1)
        assert (off_stride == 0).all()                                                # only the stride's nodes are touched
        total += want
    enc = _enc(res, C, strides)
    (gp,) = torch.autograd.grad(enc(x), enc.params, g)
    torch.testing.assert_close(gp.view(-1, C).double().sum(0), total, rtol=1e-4, atol=1e-3 * float(g.abs().mean()))


def test_torch_path_differentiates_twice():
    enc = _enc()
    x = R.off_node_points(20, R.RES_SMALL, (1,), seed=5).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    (gp,) = torch.autograd.grad(gx.sum(), enc.params)
    assert torch.isfinite(gp).all()


@pytest.mark.gpu
def test_second_order_is_refused(dev):
    enc = _enc(R.RES_SMALL, 4, (1, 2)).to(dev)
    x = torch.rand(10, 3, device=dev).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    assert gx.requires_grad                                        # create_graph=True alone is harmless
    with pytest.raises(NotImplementedError, match="VoxelGridEncoding: the second order"):
        gx.sum().backward()
    (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="VoxelGridEncoding: the second order"):
        torch.autograd.grad(gx.sum(), enc.params)


# ----------------------------------------------------------------------------- constructor
def test_constructor_errors():
    from nerfacc_amd.encodings import VoxelGridEncoding as E
    for C in (0, 3, 6, 68, 128, 4.0):
        with pytest.raises(ValueError, match=r"VoxelGridEncoding: n_features must be 1, 2 or a multiple of 4 up to 64"):
            E((4, 4, 4), C)
    for C in (1, 2, 4, 12, 64):
        assert E((4, 4, 4), C).n_output_dims == C
    for res in ((4, 4), (4, 4, 4, 4)):
        with pytest.raises(ValueError, match=f"VoxelGridEncoding: resolution must have 3 entries \\(got {len(res)}\\)"):
            E(res)
    with pytest.raises(ValueError, match="VoxelGridEncoding: every resolution must be at least 2"):
        E((4, 1, 4))
    for strides in ((0,), (1, 9), (-1,)):
        with pytest.raises(ValueError, match=r"VoxelGridEncoding: every stride must be in 1\.\.8"):
            E((20, 20, 20), 4, strides)
    for strides in ((), (1, 2, 3, 4, 5)):
        with pytest.raises(ValueError, match=r"VoxelGridEncoding: strides must have 1\.\.4 entries"):
            E((20, 20, 20), 4, strides)
    with pytest.raises(ValueError, match="VoxelGridEncoding: stride 4 leaves fewer than 2 nodes"):
        E((9, 4, 9), 4, (1, 2, 4))
    assert E((9, 5, 9), 4, (1, 2, 4)).n_output_dims == 12
    with pytest.raises(ValueError, match="VoxelGridEncoding: stride 4 leaves fewer than 2 nodes"):
        E((9, 9, 9), 4, (1, 4)).resampled((9, 9, 4))
    with pytest.raises(ValueError, match=r"VoxelGridEncoding: \d+ parameters \(at most 2\^31 - 1\)"):
        E((2048, 2048, 2048), 64)                                  # refused before any allocation
    with pytest.raises(ValueError, match="out_dtype"):
        E((4, 4, 4), out_dtype=torch.float64)


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_voxgrid_fwd": "elem x params n_points n_features res n_strides strides y stream",
    "nfa_voxgrid_bwd": "elem x params grad_y n_points n_features res n_strides strides grad_params grad_x stream",
    "nfa_voxgrid_resample": "src_params src_res dst_params dst_res n_features stream",
}


def _ints(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _call(lib, fn, **kw):
    from nerfacc_amd import _backend as B
    base = {"elem": 0, "n_points": 16, "n_features": 4, "res": _ints(5, 7, 4), "n_strides": 2, "strides": _ints(1, 2),
            "src_res": _ints(5, 7, 4), "dst_res": _ints(9, 3, 4), "stream": None}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


_BAD_C = "n_features must be 1, 2 or a multiple of 4 up to 64"
_TOO_MANY = "parameters (at most 2^31 - 1 floats)"


def test_c_abi_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn in ("nfa_voxgrid_fwd", "nfa_voxgrid_bwd"):
        nm = fn[len("nfa_"):]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        # n_points == 0 returns before any other check
        assert _call(lib, fn, n_points=0, elem=9, n_features=5, res=None, strides=None, x=None)[0] == 0
        assert _call(lib, fn, n_points=-1) == (-1, f"{nm}: negative n_points")
        assert _call(lib, fn, elem=3) == (-1, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)")
        for bad in (0, 3, 6, 68):
            assert _call(lib, fn, n_features=bad) == (-1, f"{nm}: {_BAD_C} (got {bad})")
        assert _call(lib, fn, res=None) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, res=_ints(5, 1, 4)) == (-1, f"{nm}: axis 1 resolution 1 is below 2")
        assert _call(lib, fn, n_features=64, res=_ints(1 << 11, 1 << 11, 1 << 11)) == (-1, f"{nm}: too many {_TOO_MANY}")
        assert _call(lib, fn, res=_ints(1 << 30, 1 << 30, 1 << 30)) == (-1, f"{nm}: too many {_TOO_MANY}")
        for bad in (0, 5):
            assert _call(lib, fn, n_strides=bad) == (-1, f"{nm}: n_strides must be in 1..4 (got {bad})")
        assert _call(lib, fn, strides=None) == (-1, f"{nm}: null stride table")
        assert _call(lib, fn, strides=_ints(1, 9)) == (-1, f"{nm}: stride 1 is 9 (must be in 1..8)")
        assert _call(lib, fn, strides=_ints(0, 1)) == (-1, f"{nm}: stride 0 is 0 (must be in 1..8)")
        assert _call(lib, fn, strides=_ints(1, 4)) == (-1, f"{nm}: stride 4 leaves fewer than 2 nodes along axis 2 (resolution 4)")
        # the order is fixed: the first failing check speaks
        assert _call(lib, fn, n_points=-1, elem=3)[1] == f"{nm}: negative n_points"
        assert _call(lib, fn, elem=3, n_features=5)[1].startswith(f"{nm}: elem must be")
        assert _call(lib, fn, n_features=5, res=None)[1] == f"{nm}: {_BAD_C} (got 5)"
        assert _call(lib, fn, res=None, n_strides=0) == (-1, f"{nm}: null resolution table")
        assert _call(lib, fn, n_strides=0, strides=None)[1].startswith(f"{nm}: n_strides must be")
        assert _call(lib, fn, strides=_ints(1, 9), x=None)[1].startswith(f"{nm}: stride 1 is 9")
        assert _call(lib, fn, x=None) == (-1, f"{nm}: null pointer")
        assert _call(lib, fn, params=None) == (-1, f"{nm}: null pointer")
    assert _call(lib, "nfa_voxgrid_fwd", y=None) == (-1, "voxgrid_fwd: null pointer")
    assert _call(lib, "nfa_voxgrid_bwd", grad_y=None) == (-1, "voxgrid_bwd: null pointer")
    assert _call(lib, "nfa_voxgrid_bwd", grad_params=None, grad_x=None) == (-1, "voxgrid_bwd: null pointer")

    fn, nm = "nfa_voxgrid_resample", "voxgrid_resample"
    assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
    assert _call(lib, fn, n_features=10, src_res=None) == (-1, f"{nm}: {_BAD_C} (got 10)")
    assert _call(lib, fn, src_res=None) == (-1, f"{nm}: null source resolution table")
    assert _call(lib, fn, dst_res=None, src_params=None) == (-1, f"{nm}: null destination resolution table")
    assert _call(lib, fn, src_res=_ints(1, 7, 4), dst_res=_ints(1, 1, 1)) == (-1, f"{nm}: source axis 0 resolution 1 is below 2")
    big = _ints(1 << 11, 1 << 11, 1 << 11)
    assert _call(lib, fn, n_features=64, src_res=big, dst_res=_ints(2, 2, 1)) == (-1, f"{nm}: too many source {_TOO_MANY}")
    assert _call(lib, fn, dst_res=_ints(2, 2, 1), dst_params=None) == (-1, f"{nm}: destination axis 2 resolution 1 is below 2")
    assert _call(lib, fn, n_features=64, dst_res=big, dst_params=None) == (-1, f"{nm}: too many destination {_TOO_MANY}")
    assert _call(lib, fn, src_params=None) == (-1, f"{nm}: null pointer")
    assert _call(lib, fn, dst_params=None) == (-1, f"{nm}: null pointer")


# ----------------------------------------------------------------------------- pins
def test_pins():
    import nerfacc_amd
    from nerfacc_amd import _backend as B, encodings
    assert B.load().nfa_version() == 403 and B.ABI_VERSION == 403
    assert "VoxelGridEncoding" not in nerfacc_amd.__all__ and len(nerfacc_amd.__all__) == 22
    assert "VoxelGridEncoding" in encodings.__all__
    with pytest.raises(ValueError, match="unsupported tcnn encoding"):
        encodings.encoding_from_tcnn_config(3, {"otype": "VoxelGrid"})

"""CPU: the hash grid with 2 and 4 input dimensions -- construction, the pinned level tables, the torch path against the
float64 restatement of tests/hashgrid_nd_reference.py and under gradcheck, the 3-D torch path bit for bit against a frozen
copy of what it was before the dimension became a parameter, the ``_d`` entries' argument checks (stand-in pointers, no
device), and the Python-side errors."""
import ctypes

import numpy as np
import pytest
import torch

import hashgrid_nd_reference as R

INTERPS = ["Linear", "Smoothstep"]


# ----------------------------------------------------------------------------- construction and level tables
@pytest.mark.parametrize("D", [2, 4])
def test_construction(D):
    from nerfacc_amd.encodings import HashGridEncoding
    enc = HashGridEncoding(D, n_levels=4, n_features_per_level=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.5)
    assert enc.n_input_dims == D and enc.table.n_dims == D and enc.n_output_dims == 8
    assert enc.params.numel() == 2 * sum(enc.sizes)
    assert f"n_input_dims={D}" in repr(enc)
    assert "n_input_dims" not in repr(HashGridEncoding(3, 2, 2, 10))
    y = enc(torch.rand(2, 3, D))
    assert y.shape == (2, 3, 8) and y.dtype == torch.float32


TABLES = [
    # D, n_levels, log2, base, scale, resolutions, sizes, hashed
    (2, 6, 12, 16, 2.0, [16, 32, 64, 128, 256, 512], [256, 1024, 4096, 4096, 4096, 4096], [False] * 3 + [True] * 3),
    (2, 4, 14, 10.5, 1.5, [11, 16, 24, 36], [128, 256, 576, 1296], [False] * 4),
    (4, 5, 12, 4, 1.5, [4, 6, 9, 14, 21], [256, 1296, 4096, 4096, 4096], [False] * 2 + [True] * 3),
    (4, 3, 12, 8, 1.0, [8, 8, 8], [4096, 4096, 4096], [False] * 3),
    (4, 3, 14, 4.5, 1.7, [5, 8, 14], [632, 4096, 16384], [False, False, True]),
]


@pytest.mark.parametrize("D,L,log2,base,scale,res,sizes,hashed", TABLES)
def test_level_tables(D, L, log2, base, scale, res, sizes, hashed):
    from nerfacc_amd.encodings import HashGridEncoding, LevelTable
    t = LevelTable(L, log2, base, scale, n_dims=D)
    assert t.resolutions == res and t.sizes == sizes and t.hashed == hashed
    assert t.offsets == [sum(sizes[:l]) for l in range(L)] and t.n_entries == sum(sizes)
    enc = HashGridEncoding(D, L, 1, log2, base, scale)
    assert enc.resolutions == res and enc.sizes == sizes
    r = R.Table(D, L, 1, log2, base, scale)                       # the restatement's own table agrees
    assert r.res == res and r.sizes == sizes and r.hashed == hashed and [float(s) for s in r.scales] == t.scales
    # scale and resolution do not depend on D
    t3 = LevelTable(L, log2, base, scale)
    assert t3.n_dims == 3 and t3.scales == t.scales and t3.resolutions == t.resolutions


# ----------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("n", [63, 65, 4097])
@pytest.mark.parametrize("name", list(R.GRIDS))
def test_points_cover_the_named_regions(name, n):
    """The points every tier below and the GPU tier use: an eighth of them in [-2, 3]^D (a row drawn there lies outside the
    unit box with probability 1 - 5^-D, so at most an eighth of the block may lie inside), at least half of the block half a box width or more outside
    (cells below -1 and past res), one huge row, and rows on the cell faces of every level that the out-of-range block does not overwrite."""
    enc = R.make_grid(name)
    x = R.make_points(n, enc, 1000 + n)
    far = n // 8
    outside, deep, faces = R.point_census(x, enc)
    assert outside >= far - max(1, far // 8), (outside, far)
    assert deep >= far // 2, (deep, far)
    assert float(x[n - far:].min()) >= -2.0 and float(x[n - far:].max()) <= 3.0
    assert float(x[0].abs().min()) >= 1e5
    assert len(faces) == enc.n_levels and min(faces) >= 1, faces
    assert bool((x[1:n - far] == 0.0).all(-1).any()) and bool((x[1:n - far] == 1.0).all(-1).any())


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("name", list(R.GRIDS))
def test_torch_path_matches_restatement(name, interp):
    """rtol 1e-5 is the project's float32 contract.  The absolute term is tests/test_encodings_cpu.py's (rtol 0, atol 2e-6
    there): where the corner terms of an output cancel, its error is relative to the terms (|T| <= 1, weights summing to 1:
    2^D + 1 roundings of 2^-24, 1e-6 at D = 4), not to the sum."""
    enc = R.make_grid(name, interp)
    x = R.make_points(65, enc, 3)
    y = enc(x)
    ref = R.forward(x.numpy(), enc.params.detach().numpy(), R.table_of(enc), interp == "Smoothstep")
    assert y.shape == ref.shape
    np.testing.assert_allclose(y.detach().numpy(), ref, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("D", [2, 4])
def test_torch_path_gradcheck(D, interp):
    from nerfacc_amd import _backend as B
    from nerfacc_amd.encodings import HashGridEncoding, _hashgrid_torch
    torch.manual_seed(D)
    enc = HashGridEncoding(D, n_levels=2, n_features_per_level=1, log2_hashmap_size=10, base_resolution=4,
                           per_level_scale=12.0 if D == 2 else 3.0, interpolation=interp)
    assert enc.table.hashed == [False, True]
    code = B.INTERP_CODES[interp]
    p = enc.params.detach().double().uniform_(-1, 1).requires_grad_(True)
    # interior points: 0.05 away from every cell face of both levels
    cells = torch.rand(5, D, dtype=torch.float64)
    x = cells.clone()
    for _ in range(100):
        bad = torch.zeros(5, dtype=torch.bool)
        for s in enc.scales:
            fr = (x * s + 0.5) % 1.0
            bad |= ((fr < 0.05) | (fr > 0.95)).any(-1)
        if not bad.any():
            break
        x[bad] = torch.rand(int(bad.sum()), D, dtype=torch.float64)
    assert not bad.any()
    x.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda p_: _hashgrid_torch(x.detach(), p_, enc.table, 1, code), (p,), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda x_: _hashgrid_torch(x_, p.detach(), enc.table, 1, code), (x,), eps=1e-7, atol=1e-5)
    # the restatement's gradients are those of the torch path
    g = torch.randn(5, 2, dtype=torch.float64)
    y = _hashgrid_torch(x, p, enc.table, 1, code)
    gx, gp = torch.autograd.grad(y, (x, p), g)
    x32 = x.detach().float()
    ref_p, _, _, ref_x = R.grads(x32.numpy(), p.detach().numpy(), R.table_of(enc), g.numpy(), interp == "Smoothstep")
    y32 = _hashgrid_torch(x32.double().requires_grad_(True), p, enc.table, 1, code)   # (the float32 points, as the reference sees them)
    np.testing.assert_allclose(torch.autograd.grad(y32, p, g)[0].numpy(), ref_p.reshape(-1), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(gx.numpy(), ref_x, rtol=1e-3, atol=1e-3 * float(np.abs(ref_x).mean()))


def _frozen_hashgrid_torch_3d(x, params, t, n_features, interp=0):
    """nerfacc_amd.encodings._hashgrid_torch as it was while the grid was 3-D only (kept here, frozen)."""
    M = 0xFFFFFFFF
    F = n_features
    table = params.view(-1, F)
    outs = []
    for l in range(len(t.scales)):
        p = x * t.scales[l] + 0.5
        fl = torch.floor(p)
        f = p - fl
        if interp == 1:
            f = (f * f) * (3.0 - 2.0 * f)
        g = fl.detach().clamp(-2147483648.0, 2147483520.0).to(torch.int64) & M
        lvl = table[t.offsets[l]: t.offsets[l] + t.sizes[l]]
        size, res = t.sizes[l], t.resolutions[l]
        acc = torch.zeros(x.shape[0], F, dtype=x.dtype, device=x.device)
        for c in range(8):
            b = [(c >> d) & 1 for d in range(3)]
            q = [(g[:, d] + b[d]) & M for d in range(3)]
            if t.hashed[l]:
                idx = (q[0] ^ ((q[1] * 2654435761) & M) ^ ((q[2] * 805459861) & M)) & (size - 1)
            else:
                idx = ((q[0] + q[1] * res + q[2] * (res * res & M)) & M) % size
            w = [f[:, d] if b[d] else 1.0 - f[:, d] for d in range(3)]
            wc = (w[0] * w[1]) * w[2]
            acc = acc + wc[:, None] * lvl[idx]
        outs.append(acc)
    return torch.cat(outs, -1)


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("cfg", [(4, 2, 10, 4, 2.5), (7, 8, 12, 16, 1.0), (4, 2, 16, 10.5, 1.5), (16, 2, 19, 16, 1.4472692)])
def test_3d_torch_path_unchanged(cfg, interp):
    from nerfacc_amd.encodings import HashGridEncoding, _hashgrid_torch
    torch.manual_seed(1)
    enc = HashGridEncoding(3, *cfg)
    p = enc.params.detach().uniform_(-1, 1)
    x = torch.rand(257, 3) * 5.0 - 2.0
    x[0] = torch.tensor([1e6, -1e7, 3e9])
    x[1] = torch.tensor([float("nan"), float("inf"), -float("inf")])
    x[2:5] = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.5]])
    got = _hashgrid_torch(x, p, enc.table, enc.n_features_per_level, interp)
    ref = _frozen_hashgrid_torch_3d(x, p, enc.table, enc.n_features_per_level, interp)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    xd = x[5:].double().requires_grad_(True)
    a = torch.autograd.grad(_hashgrid_torch(xd, p.double(), enc.table, enc.n_features_per_level, interp).sum(), xd)[0]
    b = torch.autograd.grad(_frozen_hashgrid_torch_3d(xd, p.double(), enc.table, enc.n_features_per_level, interp).sum(), xd)[0]
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- C ABI
P = 0x1000   # a stand-in address (16-byte aligned) that is never dereferenced
_SCALES = (ctypes.c_float * 2)(3.0, 11.0)
_RES = (ctypes.c_int32 * 2)(4, 12)
_SIZES = {2: (ctypes.c_int32 * 2)(16, 144), 3: (ctypes.c_int32 * 2)(64, 1024), 4: (ctypes.c_int32 * 2)(256, 1024)}
_NPARAMS = {2: 160, 3: 1088, 4: 1280}
_ARGS = {
    "nfa_hashgrid_fwd_d": "n_dims interp elem x params n_points n_levels n_features log2 scales res sizes n_params y stream",
    "nfa_hashgrid_bwd_d": "n_dims interp elem x params grad_y n_points n_levels n_features log2 scales res sizes n_params "
                          "grad_params grad_x stream",
    "nfa_hashgrid_bwd_sorted_d": "n_dims interp elem x params grad_y n_points n_levels n_features log2 scales res sizes n_params "
                                 "grad_params grad_x scratch scratch_bytes stream",
}


def _call(lib, fn, n_dims, **kw):
    from nerfacc_amd import _backend as B
    table = n_dims if n_dims in _SIZES else 3
    base = {"n_dims": n_dims, "interp": 0, "elem": 0, "n_points": 16, "n_levels": 2, "n_features": 1, "log2": 10,
            "scales": _SCALES, "res": _RES, "sizes": _SIZES[table], "n_params": _NPARAMS[table], "scratch_bytes": 1 << 40,
            "stream": None}
    args = [kw[a] if a in kw else base[a] if a in base else P for a in _ARGS[fn].split()]
    assert len(args) == len(B._SIGS[fn])
    lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
    rc = getattr(lib, fn)(*args)
    return rc, lib.nfa_last_error().decode()


def test_d_entries_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn in _ARGS:
        nm = fn[len("nfa_"):-2]
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        for bad in (1, 5):
            assert _call(lib, fn, bad) == (-1, f"{nm}: n_dims must be 2, 3 or 4 (got {bad})")
        # a table computed for res^3 handed in with n_dims = 2, and the other way round
        assert _call(lib, fn, 2, sizes=_SIZES[3], n_params=1088) == (-1, f"{nm}: level 0 size 64 is not min(roundup8(res^2), 2^10)")
        assert _call(lib, fn, 4, sizes=_SIZES[3], n_params=1088) == (-1, f"{nm}: level 0 size 64 is not min(roundup8(res^4), 2^10)")
        assert _call(lib, fn, 3, sizes=_SIZES[2], n_params=160) == (-1, f"{nm}: level 0 size 16 is not min(roundup8(res^3), 2^10)")
        for D in (2, 3, 4):
            assert _call(lib, fn, D, sizes=None) == (-1, f"{nm}: null level table")
            assert _call(lib, fn, D, scales=None) == (-1, f"{nm}: null level table")
            assert _call(lib, fn, D, interp=2)[1].startswith(f"{nm}: interp must be")
            assert _call(lib, fn, D, elem=3)[1].startswith(f"{nm}: elem must be")
            assert _call(lib, fn, D, x=None) == (-1, f"{nm}: null pointer")
            assert _call(lib, fn, D, n_points=0, x=None, params=None)[0] == 0
        for D in (2, 4):   # a point is one vector access
            assert _call(lib, fn, D, x=P + 8)[1].endswith(f"16-byte aligned at n_dims {D}")
    fn = "nfa_hashgrid_bwd_sorted_d"
    for D in (2, 3, 4):
        limit = 1 << (32 - D)
        assert _call(lib, fn, D, n_points=limit) == (
            -1, f"hashgrid_bwd_sorted: {1 << D} * n_points must be below 2^32 (got n_points {limit})")
        assert _call(lib, fn, D, scratch=None) == (
            -1, "hashgrid_bwd_sorted: scratch is null (a table gradient needs nfa_hashgrid_sorted_scratch_bytes bytes)")
        assert _call(lib, fn, D, scratch_bytes=R.scratch_bytes(D, 16, 2) - 1)[1].startswith("hashgrid_bwd_sorted: scratch too small")


def test_scratch_bytes_d():
    from nerfacc_amd import _backend as B
    lib = B.load()
    f, old = lib.nfa_hashgrid_sorted_scratch_bytes_d, lib.nfa_hashgrid_sorted_scratch_bytes
    for D in (2, 3, 4):
        assert f(D, 0, 16, 19) == 0 and f(D, -1, 16, 19) == 0
        for n in (1, 17, 63, 65, 257, 1025, 4097, 1 << 20, (1 << (32 - D)) - 1):
            for L in (1, 5, 16, 32):
                assert f(D, n, L, 19) == R.scratch_bytes(D, n, L) == f(D, n, L, 10), (D, n, L)
                if D == 3:
                    assert f(3, n, L, 19) == old(n, L, 19)
    # the items, not the points, size the scratch
    assert f(2, 1024, 4, 12) == f(3, 512, 4, 12) == f(4, 256, 4, 12)
    for bad in (1, 5):
        lib.nfa_set_tuning(b"", None)
        assert f(bad, 16, 2, 10) == -1
        assert lib.nfa_last_error().decode() == f"hashgrid_sorted_scratch_bytes: n_dims must be 2, 3 or 4 (got {bad})"


# ----------------------------------------------------------------------------- Python errors
def test_python_errors():
    from nerfacc_amd import encodings as E
    for bad in (1, 5):
        with pytest.raises(ValueError, match=f"n_input_dims must be 2, 3 or 4 .got {bad}."):
            E.HashGridEncoding(bad)
    enc = E.HashGridEncoding(2, 2, 2, 10)
    with pytest.raises(AssertionError, match=r"x must have shape \(\.\.\., 2\)"):
        enc(torch.rand(4, 3))
    with pytest.raises(AssertionError, match=r"x must have shape \(\.\.\., 4\)"):
        E.HashGridEncoding(4, 2, 2, 10)(torch.rand(4, 3))
    # encoding_from_tcnn_config stays 3-D, and says where to go
    with pytest.raises(ValueError, match="only 3 input dimensions"):
        E.encoding_from_tcnn_config(4, {"otype": "HashGrid"})
    assert "n_input_dims=2 or 4" in E.encoding_from_tcnn_config.__doc__


@pytest.mark.parametrize("D", [2, 3, 4])
def test_sorted_point_limit(D):
    from nerfacc_amd import encodings as E
    enc = E.HashGridEncoding(D, 2, 2, 10, deterministic=True)
    limit = (1 << (32 - D)) - 1
    assert E.sorted_max_points(D) == limit and E.SORTED_MAX_POINTS == E.sorted_max_points(3)
    with pytest.raises(ValueError, match=f"2\\^{32 - D} - 1 = {limit}"):
        E._sorted_scratch(enc, limit + 1, "meta")               # a meta device: no allocation is made
    assert E._sorted_scratch(enc, limit, "meta").numel() == R.scratch_bytes(D, limit, 2)
    assert E._sorted_scratch(enc, 65, "meta").numel() == R.scratch_bytes(D, 65, 2)


@pytest.mark.parametrize("D", [2, 4])
def test_double_backward(D):
    """The native second order is 3-D only: the backward function refuses to be differentiated again at D != 3 (called
    here directly, no device needed); the torch path on CPU tensors is differentiated by autograd."""
    from nerfacc_amd import encodings as E
    enc = E.HashGridEncoding(D, 2, 2, 10, 4, 2.0, interpolation="Smoothstep")

    class Ctx:
        pass
    ctx = Ctx()
    ctx.enc = enc
    with pytest.raises(NotImplementedError, match=f"3 input dimensions only .this grid has {D}."):
        E._HashGridBwdFn.backward(ctx, torch.zeros(4, D), None)
    x = (torch.rand(6, D, dtype=torch.float64) * 0.8 + 0.1).requires_grad_(True)
    y = enc(x)
    (gx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    (gxx,) = torch.autograd.grad(gx.sum(), x)
    assert gxx.shape == x.shape and bool(torch.isfinite(gxx).all()) and float(gxx.abs().sum()) > 0

"""GPU: the native voxel-grid regularisers of csrc/voxreg.hip -- ``voxel_terms`` against the float64 form of
tests/voxreg_reference.py, the table gradient bit for bit against the float32 torch restatement and within tolerance of
float64 autograd, the in-place add (dense and sparse), special values, a table beyond 4 GiB, dispatch without host
synchronisation, and training use (SGD, capture, FusedAdam's zero-gradient skip)."""
import ctypes

import pytest
import torch

import voxreg_reference as R

pytestmark = pytest.mark.gpu

# The kernels' constants (csrc/voxreg.hip): the table is walked as aligned 16-byte quads of the flat table; a workgroup of
# NFA_VXR_LANES lanes takes NFA_VXR_LANES * NFA_VXR_FWD_QUADS consecutive quads in the forward (one partial row each) and
# NFA_VXR_LANES * NFA_VXR_BWD_QUADS in the backward; a wave-instruction spans 64 lanes * 4 floats; the finish kernel has
# NFA_VXR_FIN lanes, and a lane starts a new run every NFA_VXR_RUN partial rows.
NFA_VXR_LANES, NFA_VXR_FWD_QUADS, NFA_VXR_BWD_QUADS, NFA_VXR_FIN, NFA_VXR_RUN, WAVE_FLOATS = 256, 8, 4, 512, 128, 256
FWD_TILE, BWD_TILE = 4 * NFA_VXR_LANES * NFA_VXR_FWD_QUADS, 4 * NFA_VXR_LANES * NFA_VXR_BWD_QUADS   # floats
MAX_ROWS = (1 << 29) // (NFA_VXR_LANES * NFA_VXR_FWD_QUADS)          # a table has fewer than 2^31 floats: at most 2^29 quads
# the longest chain of float32 additions a term passes through (csrc/voxreg.hip's header): 4 per quad in a lane of the
# forward, 6 + 3 for its workgroup, a run and the runs in a lane of the finish kernel, 6 + 7 for its workgroup
CHAIN = 4 * NFA_VXR_FWD_QUADS + 9 + (NFA_VXR_RUN - 1) + (MAX_ROWS // (NFA_VXR_FIN * NFA_VXR_RUN) - 1) + 13
assert CHAIN == 184 and CHAIN <= 1024
RTOL = CHAIN * 2.0 ** -24

SMALL = (2, 2, 2)
ODD = (5, 4, 7)          # 140 nodes; rows of 5 C floats: for C = 1 and C = 2 no whole number of quads
LARGE = (9, 17, 55)      # 8415 nodes: more than one tile of either pass for every C, a multiple of neither a tile nor a wave's span
FEATURES = (1, 2, 4, 12, 64)
for _C in FEATURES:
    _n = LARGE[0] * LARGE[1] * LARGE[2] * _C
    assert _n > FWD_TILE and _n % FWD_TILE and _n % BWD_TILE and _n % WAVE_FLOATS
assert (ODD[0] * 1) % 4 and (ODD[0] * 2) % 4 and (LARGE[0] * LARGE[1] * LARGE[2]) % 4 == 3   # C = 1: the last quad is short
# Beyond 4 GiB, and more partial rows than one run of the finish kernel's lanes
HUGE = (4, 4, (1 << 26) + 5)
assert 4 * HUGE[0] * HUGE[1] * HUGE[2] > 1 << 32
assert -(-HUGE[0] * HUGE[1] * HUGE[2] // FWD_TILE) > NFA_VXR_FIN * NFA_VXR_RUN
SHAPES = [(res, C) for res in (SMALL, ODD, LARGE) for C in FEATURES]
W = (0.3, 0.2, 0.15, 0.05)


def _enc(res, C, dev, params=None):
    from nerfacc_amd.encodings import VoxelGridEncoding
    enc = VoxelGridEncoding(res, n_features=C)
    with torch.no_grad():
        enc.params.copy_(R.make_params(res, C) if params is None else params)
    return enc.to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-3 * float(ref.abs().mean()))


def _codes(kind, reduction):
    from nerfacc_amd import _backend as B
    return B.VOXREG_KIND_CODES[kind], B.VOXREG_REDUCTION_CODES[reduction]


def _c_res(res):
    return (ctypes.c_int32 * 3)(*res)


def _native_fwd(params, res, C, kind, reduction="mean"):
    """nfa_voxreg_fwd into buffers that are full of NaN beforehand."""
    from nerfacc_amd import _backend as B
    n = B.load().nfa_voxreg_partials(C, _c_res(res))
    partials = torch.full((n, 4), float("nan"), device=params.device)
    terms = torch.full((4,), float("nan"), device=params.device)
    B.call("nfa_voxreg_fwd", B.ptr(params), C, _c_res(res), *_codes(kind, reduction), B.ptr(partials), n, B.ptr(terms), B.stream())
    return terms


def _native_grad(params, res, C, kind, g_terms, reduction="mean"):
    """nfa_voxreg_bwd into a buffer that is full of NaN beforehand."""
    from nerfacc_amd import _backend as B
    out = torch.full_like(params, float("nan"))
    B.call("nfa_voxreg_bwd", B.ptr(params), C, _c_res(res), *_codes(kind, reduction), B.ptr(g_terms), B.ptr(out), B.stream())
    return out


def _native_add(params, res, C, kind, weights, dense, grad, reduction="sum"):
    from nerfacc_amd import _backend as B
    B.call("nfa_voxreg_add_grad", B.ptr(params), C, _c_res(res), *_codes(kind, reduction), (ctypes.c_float * 4)(*weights), int(dense),
           B.ptr(grad), B.stream())
    return grad


# ----------------------------------------------------------------------------- values
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("res,C", SHAPES)
def test_values(dev, res, C, kind):
    from nerfacc_amd.losses import voxel_terms
    p, _, ref, _ = R.case(res, C, kind)
    enc = _enc(res, C, dev, p)
    with torch.no_grad():
        got = voxel_terms(enc, kind)
    assert got.shape == (4,) and got.dtype == torch.float32 and got.device == enc.params.device
    print("terms", got.tolist(), "reference", ref.tolist())
    torch.testing.assert_close(got.cpu().double(), ref, rtol=RTOL, atol=0.0)
    with torch.no_grad():
        total = voxel_terms(enc, kind, "sum")
    torch.testing.assert_close(total.cpu().double(), R.case(res, C, kind, 0, "sum")[2], rtol=RTOL, atol=0.0)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("res,C", [(ODD, 1), (LARGE, 1), (LARGE, 2), (LARGE, 12)])
def test_integer_valued_tables_are_exact(dev, res, C, kind):
    """Small integers: every sum stays far below 2^24, so whatever the order of the additions the terms and the gradient are
    the float64 reference's exactly."""
    p = torch.randint(-3, 4, (R.n_params(res, C),), generator=torch.Generator().manual_seed(2)).float()
    pr = p.double().requires_grad_(True)
    ref = R.terms_reference(pr, res, C, kind, "sum")
    g = torch.tensor([1.0, -2.0, 0.5, 3.0])
    (ref_gp,) = torch.autograd.grad(ref, pr, g.double())
    assert float(ref.detach().max()) < 2 ** 24
    pd = p.to(dev)
    assert torch.equal(_native_fwd(pd, res, C, kind, "sum").cpu().double(), ref.detach())
    assert torch.equal(_native_grad(pd, res, C, kind, g.to(dev), "sum").cpu().double(), ref_gp)


# ----------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("res,C", SHAPES)
def test_gradient_bit_for_bit_and_against_float64(dev, res, C, kind):
    from nerfacc_amd.losses import _voxel_terms_grad_torch, voxel_terms
    p, g, _, ref_gp = R.case(res, C, kind)
    enc = _enc(res, C, dev, p)
    pd, gd = enc.params.detach(), g.to(dev)
    terms = _native_fwd(pd, res, C, kind)
    assert not torch.isnan(terms).any()
    got = _native_grad(pd, res, C, kind, gd)
    assert not torch.isnan(got).any()                                   # every element is written
    want = _voxel_terms_grad_torch(pd, gd, res, C, kind, "mean")        # float32, on the device, operation for operation
    assert torch.equal(_bits(got), _bits(want))
    torch.testing.assert_close(got.cpu().double(), ref_gp, **_tol(ref_gp))
    assert torch.equal(_bits(_native_grad(pd, res, C, kind, gd)), _bits(got))   # the same bits on a second run
    t = voxel_terms(enc, kind)                                          # the same through autograd
    assert torch.equal(_bits(t.detach()), _bits(terms))
    (auto,) = torch.autograd.grad(t, enc.params, gd)
    assert torch.equal(_bits(auto), _bits(got))
    assert torch.equal(_bits(_native_fwd(pd, res, C, kind)), _bits(terms))


def test_sum_reduction_gradient_bit_for_bit(dev):
    from nerfacc_amd.losses import _voxel_terms_grad_torch
    for C in (1, 12):
        p, g, _, _ = R.case(LARGE, C, "huber")
        pd, gd = p.to(dev), g.to(dev)
        assert torch.equal(_bits(_native_grad(pd, LARGE, C, "huber", gd, "sum")), _bits(_voxel_terms_grad_torch(pd, gd, LARGE, C, "huber", "sum")))


# ----------------------------------------------------------------------------- the in-place add
@pytest.mark.parametrize("kind,reduction", [("huber", "sum"), ("l2", "mean"), ("l1", "sum")])
@pytest.mark.parametrize("res,C", [(ODD, 1), (ODD, 2), (LARGE, 1), (LARGE, 2), (LARGE, 4), (LARGE, 12), (SMALL, 64)])
def test_add_grad_dense_and_sparse(dev, res, C, kind, reduction):
    from nerfacc_amd.losses import _voxel_terms_grad_torch
    pd = R.make_params(res, C).to(dev)
    wd = torch.tensor(W, device=dev)
    G = _voxel_terms_grad_torch(pd, wd, res, C, kind, reduction)
    assert torch.equal(_bits(_native_grad(pd, res, C, kind, wd, reduction)), _bits(G))   # weights as grad_terms: the same bits
    grad = torch.randn(pd.numel(), generator=torch.Generator().manual_seed(4)).to(dev)
    got = _native_add(pd, res, C, kind, W, True, grad.clone(), reduction)
    assert torch.equal(_bits(got), _bits(grad + G))
    # sparse: runs of zeros (whole quads and parts of quads), zeros of either sign, a NaN
    grad[torch.rand(pd.numel(), generator=torch.Generator().manual_seed(5)).to(dev) < 0.5] = 0.0
    grad[16: min(64, pd.numel() // 2)] = 0.0
    grad[1::6] = -0.0
    grad[5] = float("nan")
    got = _native_add(pd, res, C, kind, W, False, grad.clone(), reduction)
    zero = grad == 0
    assert zero.any() and (~zero).any() and torch.signbit(grad[zero]).any()
    assert torch.equal(_bits(got[zero]), _bits(grad[zero]))             # untouched: the same bits, -0.0 included
    assert torch.equal(_bits(got[~zero]), _bits((grad + G)[~zero])) and torch.isnan(got[5])


def test_add_grad_through_the_wrapper(dev):
    from nerfacc_amd.losses import _voxel_terms_grad_torch, voxel_tv_add_grad_
    enc = _enc(LARGE, 4, dev)
    G = _voxel_terms_grad_torch(enc.params, torch.tensor((*W[:3], 0.0), device=dev), LARGE, 4, "huber", "sum")
    voxel_tv_add_grad_(enc, *W[:3], dense=False)
    assert enc.params.grad is None
    voxel_tv_add_grad_(enc, *W[:3])
    assert torch.equal(_bits(enc.params.grad), _bits(torch.zeros_like(G) + G))
    voxel_tv_add_grad_(enc, *W[:3])
    assert torch.equal(_bits(enc.params.grad), _bits((torch.zeros_like(G) + G) + G))


# ----------------------------------------------------------------------------- special values
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("C", [1, 4])
def test_special_values_stay_in_their_stencil(dev, C, kind):
    res = ODD
    p = R.make_params(res, C)
    gd = torch.tensor([0.7, -0.4, 0.3, 0.2], device=dev)
    clean = _native_grad(p.to(dev), res, C, kind, gd)
    g = p.clone().view(res[2], res[1], res[0], C)
    nan_at, inf_at = (3, 1, 2, C - 1), (6, 3, 2, 0)                    # an inner node, and one on the table's last row and slab
    g[nan_at], g[inf_at] = float("nan"), float("inf")

    def stencil(at):
        m = torch.zeros(res[2], res[1], res[0], C, dtype=torch.bool)
        m[at] = True
        for axis in range(3):
            for step in (-1, 1):
                nb = list(at)
                nb[axis] += step
                if 0 <= nb[axis] < m.shape[axis]:
                    m[tuple(nb)] = True
        return m.view(-1)
    near_nan, near_inf = stencil(nan_at), stencil(inf_at)
    assert int(near_nan.sum()) == 7 and int(near_inf.sum()) == 5 and not (near_nan & near_inf).any()
    pd = g.reshape(-1).to(dev)
    got = _native_grad(pd, res, C, kind, gd).cpu()
    assert torch.isnan(got[near_nan]).all()                             # the NaN reaches exactly its stencil
    assert not torch.isnan(got[~near_nan & ~near_inf]).any()
    rest = ~(near_nan | near_inf)
    assert torch.equal(_bits(got[rest]), _bits(clean.cpu()[rest]))      # elsewhere: the bits of the run without them
    if kind == "l2":
        assert not torch.isfinite(got[near_inf]).any()                  # l1 and huber bound the infinity's differences
    else:
        assert torch.isfinite(got[near_inf]).all()
    assert not torch.isfinite(_native_fwd(pd, res, C, kind)).any()      # every term's stencil touches them


# ----------------------------------------------------------------------------- beyond 4 GiB
def test_table_beyond_4_gib(dev):
    """(4, 4, 2^26 + 5) with C = 1: 2^30 + 80 floats, so byte offsets pass 2^32, and 131,073 partial rows: three runs of the
    finish kernel's lanes.  g[z, y, x] = a[x] + b[y] + (z mod 3): the terms have a closed form in integers."""
    from nerfacc_amd.losses import _voxel_terms_grad_torch
    Rx, Ry, Rz = HUGE
    a, b = [0, 1, 3, 2], [0, 2, 1, 1]
    g = (torch.arange(Rz, device=dev) % 3).float()[:, None, None] + torch.tensor(b, device=dev).float()[None, :, None] \
        + torch.tensor(a, device=dev).float()[None, None, :]
    pd = g.reshape(-1)
    assert pd.numel() == (1 << 30) + 80 and pd.data_ptr() % 16 == 0

    def rho(d):                                                        # huber
        return 0.5 * d * d if abs(d) <= 1 else abs(d) - 0.5
    n_down = (Rz - 1) // 3                                             # the z in [0, R_z - 1) with z mod 3 == 2: a step of -2
    n_up = Rz - 1 - n_down                                             # every other step is +1
    want = [Ry * Rz * sum(rho(a[i + 1] - a[i]) for i in range(3)), Rx * Rz * sum(rho(b[i + 1] - b[i]) for i in range(3)),
            Rx * Ry * (n_up * rho(1) + n_down * rho(-2)),
            Ry * Rz * sum(a) + Rx * Rz * sum(b) + Rx * Ry * sum(z % 3 for z in range(3)) * (Rz // 3) + Rx * Ry * sum(z % 3 for z in range(Rz % 3))]
    got = _native_fwd(pd, HUGE, 1, "huber", "sum").cpu().double()
    print("beyond 4 GiB: terms", got.tolist(), "closed form", want)
    torch.testing.assert_close(got, torch.tensor(want, dtype=torch.float64), rtol=RTOL, atol=0.0)
    gd = torch.tensor([1.0, 0.5, 0.25, 2.0], device=dev)
    out = _native_grad(pd, HUGE, 1, "huber", gd, "sum")
    assert not bool(torch.isnan(out).any())                            # every element is written
    slab, k = Rx * Ry, 8
    top = _voxel_terms_grad_torch(pd[:(k + 1) * slab], gd, (Rx, Ry, k + 1), 1, "huber", "sum")[:k * slab]
    bottom = _voxel_terms_grad_torch(pd[-(k + 1) * slab:], gd, (Rx, Ry, k + 1), 1, "huber", "sum")[slab:]
    assert torch.equal(_bits(out[:k * slab]), _bits(top)) and torch.equal(_bits(out[-k * slab:]), _bits(bottom))


# ----------------------------------------------------------------------------- dispatch
def test_native_path_is_taken_without_host_synchronisation(dev, monkeypatch):
    from nerfacc_amd import _backend as B, losses
    enc = _enc(LARGE, 12, dev)

    def step():
        enc.params.grad = None
        losses.voxel_regularization(enc, tv=0.5, l1=0.25, kind="huber").backward()
        losses.voxel_tv_add_grad_(enc, 0.1, 0.2, 0.3, dense=False)
        return enc.params.grad

    want = step()   # (library loaded, allocator warm, the weight tensor built)

    def boom(*a, **k):
        raise AssertionError("the torch path ran on CUDA float32 parameters")
    monkeypatch.setattr(losses, "_voxel_terms_torch", boom)
    monkeypatch.setattr(losses, "_voxel_terms_grad_torch", boom)
    names = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert names == ["nfa_voxreg_fwd", "nfa_voxreg_bwd", "nfa_voxreg_add_grad"]
    assert torch.equal(_bits(want), _bits(got))


def test_fallbacks_give_the_same_values(dev):
    """CPU and float64 parameters take the torch path; parameters or gradients at a 4-byte offset are copied (the terms) or
    take the torch path (the in-place add): the same values, for the add the same bits."""
    from nerfacc_amd.losses import voxel_terms, voxel_tv_add_grad_
    res, C, kind = ODD, 2, "huber"
    p, g, ref, _ = R.case(res, C, kind)
    enc = _enc(res, C, dev, p)
    t0 = voxel_terms(enc, kind)
    (g0,) = torch.autograd.grad(t0, enc.params, g.to(dev))
    for other in (_enc(res, C, "cpu", p), _enc(res, C, dev, p).double()):
        t = voxel_terms(other, kind)
        assert t.dtype == torch.float32 and t.device == other.params.device
        torch.testing.assert_close(t.cpu().double(), ref, rtol=1e-5, atol=0.0)
    store = torch.empty(p.numel() + 1, device=dev)
    store[1:] = p.to(dev)
    enc.params = torch.nn.Parameter(store[1:])
    assert enc.params.data_ptr() % 16 == 4
    t1 = voxel_terms(enc, kind)
    (g1,) = torch.autograd.grad(t1, enc.params, g.to(dev))
    assert torch.equal(_bits(t0.detach()), _bits(t1.detach())) and torch.equal(_bits(g0), _bits(g1))
    # the in-place add: aligned (native) against a gradient at a 4-byte offset and against CPU tensors (torch)
    start = torch.randn(p.numel(), generator=torch.Generator().manual_seed(6))
    start[::3] = 0.0
    results = []
    for where, offset in ((dev, 0), (dev, 1), ("cpu", 0)):
        e = _enc(res, C, where, p)
        buf = torch.empty(p.numel() + offset, device=where)
        e.params.grad = buf[offset:]
        e.params.grad.copy_(start)
        assert e.params.grad.data_ptr() % 16 == 4 * offset
        voxel_tv_add_grad_(e, *W[:3], l1=W[3], dense=False)
        results.append(e.params.grad.cpu())
    assert torch.equal(_bits(results[0]), _bits(results[1])) and torch.equal(_bits(results[0]), _bits(results[2]))
    assert (results[0] != start).any() and (results[0][start == 0] == 0).all()


def test_misaligned_pointers_are_refused_by_the_entries(dev):
    from nerfacc_amd import _backend as B
    store = torch.zeros(R.n_params(ODD, 4) + 4, device=dev)
    with pytest.raises(B.NativeError, match="voxreg_fwd: params and partials must be 16-byte aligned"):
        _native_fwd(store[1:-3], ODD, 4, "l2")
    with pytest.raises(B.NativeError, match="voxreg_bwd: params and grad_params must be 16-byte aligned"):
        _native_grad(store[1:-3], ODD, 4, "l2", torch.zeros(4, device=dev))
    with pytest.raises(B.NativeError, match="voxreg_add_grad: params and grad must be 16-byte aligned"):
        _native_add(store[:-4], ODD, 4, "l2", W, True, store[1:-3])


def test_second_order_is_refused(dev):
    from nerfacc_amd.losses import voxel_terms
    enc = _enc(ODD, 4, dev)
    (gp,) = torch.autograd.grad(voxel_terms(enc).sum(), enc.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="voxel_terms"):
        torch.autograd.grad(gp.sum(), enc.params)


# ----------------------------------------------------------------------------- training use
def test_sgd_steps_lower_the_regulariser(dev):
    from nerfacc_amd.losses import voxel_regularization
    enc = _enc(LARGE, 4, dev)
    opt = torch.optim.SGD(enc.parameters(), lr=0.05)
    track = []
    for _ in range(4):
        opt.zero_grad()
        loss = voxel_regularization(enc, tv=1.0, l1=0.1, kind="huber", reduction="sum")
        loss.backward()
        opt.step()
        track.append(loss.detach())
    track = torch.stack(track).cpu()
    assert (track[1:] < track[:-1]).all(), track


def test_captured_steps_replay_the_eager_bits(dev):
    from nerfacc_amd.graphs import CapturedStep
    from nerfacc_amd.losses import voxel_regularization, voxel_tv_add_grad_
    enc = _enc(LARGE, 12, dev)

    def fwd_bwd():
        loss = voxel_regularization(enc, tv_xyz=(0.5, 0.25, 1.0), l1=0.1, kind="l1")
        return loss.detach(), torch.autograd.grad(loss, enc.params)[0]
    eager = [t.clone() for t in fwd_bwd()]
    step = CapturedStep(fwd_bwd, warmup=1)
    for _ in range(2):
        for t in step.outputs:
            t.fill_(float("nan"))
        got = step()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, eager))
    # the in-place add: every replay adds to whatever the gradient holds
    start = torch.randn(enc.params.numel(), generator=torch.Generator().manual_seed(7)).to(dev)
    start[::2] = 0.0
    enc.params.grad = start.clone()
    voxel_tv_add_grad_(enc, *W[:3], l1=W[3], dense=False)
    eager = enc.params.grad.clone()
    step = CapturedStep(lambda: voxel_tv_add_grad_(enc, *W[:3], l1=W[3], dense=False), warmup=1)
    for _ in range(2):
        enc.params.grad.copy_(start)
        step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(enc.params.grad), _bits(eager))


def test_fused_adam_still_skips_the_untouched_voxels(dev):
    from nerfacc_amd.losses import voxel_tv_add_grad_
    from nerfacc_amd.optim import FusedAdam
    enc = _enc(LARGE, 1, dev)
    opt = FusedAdam(enc.parameters(), lr=1e-2, skip_zero_grad=True)
    before = enc.params.detach().clone()
    grad = torch.randn(before.numel(), generator=torch.Generator().manual_seed(8)).to(dev)
    grad[torch.rand(before.numel(), generator=torch.Generator().manual_seed(9)).to(dev) < 0.9] = 0.0
    enc.params.grad = grad.clone()
    voxel_tv_add_grad_(enc, *W[:3], dense=False)
    opt.step()
    untouched = grad == 0
    assert untouched.sum() > 1000 and (~untouched).sum() > 100
    assert torch.equal(_bits(enc.params.detach()[untouched]), _bits(before[untouched]))
    assert (enc.params.detach()[~untouched] != before[~untouched]).float().mean() > 0.99

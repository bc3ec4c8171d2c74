"""GPU: the native plane regularisers of csrc/planereg.hip -- ``plane_terms`` against the float64 slicing form of
tests/planereg_reference.py, its table gradient bit for bit against the float32 torch restatement and within tolerance of
float64 autograd, reproducibility, the boundary overlaps of the time stencil, alignment, special values, training through
``plane_regularization`` and the absence of host synchronisation."""
import ctypes

import pytest
import torch

import planereg_reference as R

pytestmark = pytest.mark.gpu

# The kernels' constants (csrc/plane_tiles.h, csrc/planereg.hip): a tile is NFA_PT_ROWS rows by NFA_PT_QUADS 16-byte pieces,
# one workgroup each; a wave-instruction spans 64 lanes * 4 floats of a row; the finish kernel has NFA_PR_FIN lanes per plane,
# and a lane starts a new run of partial rows every NFA_PR_RUN rows, i.e. a plane of more than NFA_PR_FIN * NFA_PR_RUN tiles
# takes the several-runs path.
NFA_PT_ROWS, NFA_PT_QUADS, NFA_PR_FIN, NFA_PR_RUN, WAVE_FLOATS = 16, 256, 256, 256, 256
# Scale 1 of LARGE has [66, 140, 8] planes: 66 rows are 5 row blocks (not a multiple of 16), W F = 1120 floats are 2 segments
# (not a multiple of the 1024 floats of a tile's row, nor of the 256 floats of a wave): 10 workgroups for that plane.
LARGE = ((70, 33, 9, 11), (1, 2), 8)
SHAPES = [(res, ms, F) for _, res, ms in R.CASES for F in R.FEATURES] + [LARGE]
assert (2 * 33) % NFA_PT_ROWS and (2 * 70 * 8) % (4 * NFA_PT_QUADS) and (2 * 70 * 8) % WAVE_FLOATS and 2 * 70 * 8 > 4 * NFA_PT_QUADS


def _enc(res, ms, F, dev, params=None):
    from nerfacc_amd.encodings import PlaneGridEncoding
    enc = PlaneGridEncoding(len(res), res, ms, n_features=F)
    with torch.no_grad():
        enc.params.copy_(R.make_params(res, ms, F) if params is None else params)
    return enc.to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tol(ref, part=1.0):
    return dict(rtol=1e-4 * part, atol=1e-3 * part * float(ref.abs().mean()))


def _native_grad(enc, params, g_terms):
    """nfa_planereg_bwd into a buffer that is full of NaN beforehand."""
    from nerfacc_amd import _backend as B
    out = torch.full_like(params, float("nan"))
    B.call("nfa_planereg_bwd", enc.n_input_dims, B.ptr(params), enc.n_scales, enc.n_features, enc.table.c_res, B.ptr(g_terms),
           B.ptr(out), B.stream())
    return out


# ----------------------------------------------------------------------------- values
@pytest.mark.parametrize("res,ms,F", SHAPES)
def test_values(dev, res, ms, F):
    """All summands are non-negative and the longest chain of float32 additions is 599 <= 1024 (csrc/planereg.hip's header):
    the relative error is below about 6e-5."""
    from nerfacc_amd.losses import plane_terms
    p, _, ref, _ = R.case(res, ms, F)
    enc = _enc(res, ms, F, dev, p)
    with torch.no_grad():
        got = plane_terms(enc)
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.device == enc.params.device
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-4, atol=0.0)
    for k, (a, b) in enumerate(enc.planes):
        if b != 3:
            assert (got[:, k, 2:] == 0).all()             # exactly 0 on a spatial plane
    if res[-1] == 2 and len(res) == 4:
        assert (got[:, :, 2] == 0).all()


def test_values_with_several_runs_of_partial_rows(dev):
    """A plane of more than NFA_PR_FIN * NFA_PR_RUN = 65536 tiles: the finish kernel's lanes add more than one run."""
    from nerfacc_amd.losses import plane_terms
    res, ms, F = (2, 2, NFA_PT_ROWS * (NFA_PR_FIN * NFA_PR_RUN + 2) + 8), (1,), 4
    enc = _enc(res, ms, F, dev, torch.zeros(1))
    with torch.no_grad():
        enc.params.copy_(1.0 + 0.5 * torch.randn(enc.params.numel(), generator=torch.Generator().manual_seed(3)).to(dev))
        got = plane_terms(enc)
        ref = R.terms_reference(enc.params.detach(), res, ms, F)      # float64, on the device
    from nerfacc_amd import _backend as B
    need = B.load().nfa_planereg_partials(3, 1, F, enc.table.c_res)
    assert need == 1 + 2 * (NFA_PR_FIN * NFA_PR_RUN + 3)
    torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=0.0)


# ----------------------------------------------------------------------------- reproducibility
def test_two_calls_give_the_same_bits(dev):
    from nerfacc_amd.losses import plane_terms
    res, ms, F = LARGE
    p, g, _, _ = R.case(res, ms, F)
    enc = _enc(res, ms, F, dev, p)
    outs = []
    for _ in range(2):
        t = plane_terms(enc)
        (gp,) = torch.autograd.grad(t, enc.params, g.to(dev))
        outs.append((t.detach(), gp))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))


# ----------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("res,ms,F", SHAPES)
def test_gradient_bit_for_bit_and_against_float64(dev, res, ms, F):
    from nerfacc_amd.losses import _plane_terms_grad_torch, plane_terms
    p, g, _, ref_gp = R.case(res, ms, F)
    enc = _enc(res, ms, F, dev, p)
    pd, gd = enc.params.detach(), g.to(dev)
    got = _native_grad(enc, pd, gd)
    assert not torch.isnan(got).any()                                   # every element is written
    want = _plane_terms_grad_torch(pd, gd, enc.table)                   # float32, on the device, operation for operation
    assert torch.equal(_bits(got), _bits(want))
    torch.testing.assert_close(got.cpu().double(), ref_gp, **_tol(ref_gp))
    (auto,) = torch.autograd.grad(plane_terms(enc), enc.params, gd)     # the same through autograd
    assert torch.equal(_bits(auto), _bits(got))


@pytest.mark.parametrize("T", [3, 4, 5])
def test_boundary_overlaps_of_the_time_stencil(dev, T):
    """Few time nodes: every row is within two of both borders (at T = 3 all three rows touch the single second difference).
    The smoothness term alone, element by element."""
    from nerfacc_amd.losses import plane_terms
    res, ms, F = (5, 4, 3, T), (1, 2), 4
    p = R.make_params(res, ms, F, seed=T)
    pr = p.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(R.terms_reference(pr, res, ms, F)[:, :, 2].sum(), pr)
    enc = _enc(res, ms, F, dev, p)
    (got,) = torch.autograd.grad(plane_terms(enc)[:, :, 2].sum(), enc.params)
    got = got.cpu().double()
    for s, k, time, view in R.plane_views(ref, res, ms, F):
        mine = R.plane_views(got, res, ms, F)[s * 6 + k][3]
        if not time:
            assert (mine == 0).all()
            continue
        assert view.shape[0] == T and (view != 0).any(-1).any(-1).all()     # every row takes part
        torch.testing.assert_close(mine, view, **_tol(view))


# ----------------------------------------------------------------------------- alignment
def test_params_at_a_four_byte_offset(dev):
    from nerfacc_amd.losses import plane_terms
    res, ms, F = (5, 4, 3, 5), (1, 2), 4
    p, g, _, _ = R.case(res, ms, F)
    enc = _enc(res, ms, F, dev, p)
    t0 = plane_terms(enc)
    (g0,) = torch.autograd.grad(t0, enc.params, g.to(dev))
    store = torch.empty(p.numel() + 1, device=dev)
    store[1:] = p.to(dev)
    enc.params = torch.nn.Parameter(store[1:])
    assert enc.params.data_ptr() % 16 == 4
    t1 = plane_terms(enc)
    (g1,) = torch.autograd.grad(t1, enc.params, g.to(dev))
    assert torch.equal(_bits(t0.detach()), _bits(t1.detach())) and torch.equal(_bits(g0), _bits(g1))


# ----------------------------------------------------------------------------- special values
def test_l1_gradient_is_zero_at_one(dev):
    from nerfacc_amd.losses import plane_regularization
    res, ms, F = (5, 4, 3, 5), (1,), 4
    p = R.make_params(res, ms, F)
    enc = _enc(res, ms, F, dev, p)
    (gp,) = torch.autograd.grad(plane_regularization(enc, l1_time=1.0), enc.params)
    gp = gp.cpu()
    time = torch.cat([torch.full((v.numel(),), t) for _, _, t, v in R.plane_views(p, res, ms, F)])
    assert (p == 1.0).any() and (gp[p == 1.0] == 0).all() and (gp[~time] == 0).all()
    other = time & (p != 1.0)
    assert (gp[other] != 0).all() and torch.equal(torch.sign(gp[other]), torch.sign(p[other] - 1.0))


def test_a_nan_stays_in_its_plane(dev):
    from nerfacc_amd.losses import plane_terms
    res, ms, F = (5, 4, 3, 5), (1, 2), 4
    enc = _enc(res, ms, F, dev)
    for s, k in [(0, 1), (1, 4)]:
        with torch.no_grad():
            enc.params.copy_(R.make_params(res, ms, F).to(dev))
            enc.plane(s, k)[1, 2, 3] = float("nan")
            got = plane_terms(enc).cpu()
        bad = torch.isnan(got)
        time = enc.planes[k][1] == 3
        want = torch.zeros_like(bad)
        want[s, k, :] = torch.tensor([True, True, time, time])          # (a spatial plane's smooth and l1 stay 0)
        assert torch.equal(bad, want), (s, k, got)


# ----------------------------------------------------------------------------- training
def test_backward_adds_to_an_existing_grad(dev):
    from nerfacc_amd.losses import plane_regularization
    res, ms, F = (5, 4, 3, 5), (1, 2), 4
    enc = _enc(res, ms, F, dev)
    plane_regularization(enc, tv=1.0, time_smoothness=1.0, l1_time=1.0).backward()
    once = enc.params.grad.clone()
    plane_regularization(enc, tv=1.0, time_smoothness=1.0, l1_time=1.0).backward()
    assert once.abs().sum() > 0 and torch.equal(enc.params.grad, once + once)


def test_a_short_run_follows_the_torch_path(dev):
    """50 Adam steps on the regularisers alone: the loss falls from step to step after the first few, and the native path's
    losses are those of the torch path."""
    from nerfacc_amd import losses
    res, ms, F = (8, 6, 5, 7), (1, 2), 4
    runs = {}
    for name in ("native", "torch"):
        enc = _enc(res, ms, F, dev)
        opt = torch.optim.Adam(enc.parameters(), lr=2e-3)
        w = losses._reg_weights(enc, 1.0, 1.0, 1.0, 1.0)
        track = []
        for _ in range(50):
            opt.zero_grad()
            if name == "native":
                loss = losses.plane_regularization(enc, tv=1.0, time_smoothness=1.0, l1_time=1.0)
            else:
                loss = (losses._plane_terms_torch(enc.params, enc.table) * w).sum()
            loss.backward()
            opt.step()
            track.append(loss.detach())
        runs[name] = torch.stack(track).cpu().double()
    native, ref = runs["native"], runs["torch"]
    assert (native[4:] < native[3:-1]).all() and native[-1] < 0.9 * native[0]
    torch.testing.assert_close(native, ref, **_tol(ref))


# ----------------------------------------------------------------------------- the native path, and only once
def test_native_path_is_taken_without_host_synchronisation(dev, monkeypatch):
    from nerfacc_amd import _backend as B, losses
    res, ms, F = LARGE
    enc = _enc(res, ms, F, dev)

    def step():
        enc.params.grad = None
        losses.plane_regularization(enc, tv=0.5, tv_time=0.25, time_smoothness=0.1, l1_time=0.01).backward()
        return enc.params.grad

    want = step()   # (library loaded, allocator warm, the weight tensor built)

    def boom(*a, **k):
        raise AssertionError("the torch path ran on CUDA float32 parameters")
    monkeypatch.setattr(losses, "_plane_terms_torch", boom)
    names = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert names == ["nfa_planereg_fwd", "nfa_planereg_bwd"]
    assert torch.equal(_bits(want), _bits(got))


def test_second_order_is_refused(dev):
    from nerfacc_amd.losses import plane_terms
    enc = _enc((5, 4, 3, 5), (1,), 4, dev)
    (gp,) = torch.autograd.grad(plane_terms(enc).sum(), enc.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="plane_terms"):
        torch.autograd.grad(gp.sum(), enc.params)


def test_misaligned_pointers_are_refused_by_the_entries(dev):
    from nerfacc_amd import _backend as B
    res, ms, F = (5, 4, 3, 5), (1,), 4
    enc = _enc(res, ms, F, dev)
    store = torch.zeros(enc.params.numel() + 4, device=dev)
    g = torch.zeros(1, 6, 4, device=dev)
    with pytest.raises(B.NativeError, match="16-byte aligned"):
        _native_grad(enc, store[1:-3], g)
    assert isinstance(enc.table.c_res, ctypes.Array)

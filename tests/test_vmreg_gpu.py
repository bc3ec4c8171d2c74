"""GPU: the native VM-grid regularisers of csrc/vmreg.hip -- ``vm_terms`` against the float64 TensoRF form of
tests/vmreg_reference.py, its table gradient bit for bit against the float32 torch restatement and within tolerance of
float64 autograd, both line paths (LDS copy and global memory), reproducibility, alignment, special values, training
through ``vm_regularization`` and the absence of host synchronisation."""
import ctypes

import pytest
import torch

import vmreg_reference as R

pytestmark = pytest.mark.gpu

# The kernels' constants (csrc/plane_tiles.h, csrc/vmreg.hip): a plane tile is NFA_PT_ROWS rows by NFA_PT_QUADS 16-byte
# pieces, one workgroup each; a wave-instruction spans 64 lanes * 4 floats of a row; the finish kernel has NFA_VR_FIN lanes
# per mode, and a lane starts a new run every NFA_VR_RUN partial rows (line quads), i.e. a plane of more than NFA_VR_FIN *
# NFA_VR_RUN tiles takes the several-runs path; a line is copied to LDS while 4 max(R) C + NFA_VR_SCRATCH <= NFA_VR_LDS_BYTES.
NFA_PT_ROWS, NFA_PT_QUADS, NFA_VR_FIN, NFA_VR_RUN, WAVE_FLOATS = 16, 256, 512, 128, 256
NFA_VR_LDS_BYTES, NFA_VR_SCRATCH = 65536, 256
# Mode 0 of LARGE has a [33, 70, 24] plane: 33 rows are 3 row blocks (not a multiple of 16), W C = 1680 floats are 2 segments
# (more than the 1024 floats of a tile's row, a multiple neither of them nor of the 256 floats of a wave): 6 workgroups.
LARGE = ((70, 33, 9), 24)
assert 33 % NFA_PT_ROWS and (70 * 24) % (4 * NFA_PT_QUADS) and (70 * 24) % WAVE_FLOATS and 70 * 24 > 4 * NFA_PT_QUADS
# A line too long for the LDS copy (153,600 bytes), and the longest that C = 96 components fit (170 rows: 65,280 + 256 bytes).
LONG_LINE = ((4, 4, 400), 96)
LDS_FULL = ((4, 4, 170), 96)
assert 4 * 400 * 96 + NFA_VR_SCRATCH > NFA_VR_LDS_BYTES >= 4 * 170 * 96 + NFA_VR_SCRATCH > NFA_VR_LDS_BYTES - 4 * 96
SHAPES = [(res, C) for res in R.RESOLUTIONS for C in R.COMPONENTS] + [LARGE, LONG_LINE, LDS_FULL, ((5, 4, 33), 48)]
# Two planes of more than NFA_VR_FIN * NFA_VR_RUN = 65536 tiles, and a line of 2049 quads per lane of the finish kernel (17 runs)
SEVERAL_RUNS = ((2, 2, NFA_PT_ROWS * (NFA_VR_FIN * NFA_VR_RUN + 2) + 8), 4)


def plane_chain():
    """The longest chain of float32 additions a plane term passes through (csrc/vmreg.hip's header): 64 in a lane of a
    tile, 6 + 3 for the tile, 127 + 256 for a lane of the finish kernel, 6 + 7 for its workgroup."""
    return 4 * NFA_PT_ROWS + 9 + (NFA_VR_RUN - 1) + 256 + 13


def line_chain(rows, C):
    """... and tv_line / l1_line: 4 additions per quad in runs of NFA_VR_RUN quads, the runs, the workgroup."""
    n = -(-rows * (C // 4) // NFA_VR_FIN)
    return 4 * min(n, NFA_VR_RUN) + -(-n // NFA_VR_RUN) + 12


ORTHO_CHAIN = 12 + 13   # the sum of |G_ij|: at most 12 in a lane (3 blocks of 2 x 2), 6 + 7 for the workgroup


def _enc(res, C, dev, params=None):
    from nerfacc_amd.encodings import VMGridEncoding
    enc = VMGridEncoding(res, n_components=C)
    with torch.no_grad():
        enc.params.copy_(R.make_params(res, C) if params is None else params)
    return enc.to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tol(ref, part=1.0):
    return dict(rtol=1e-4 * part, atol=1e-3 * part * float(ref.abs().mean()))


def _native_fwd(enc, params):
    """nfa_vmreg_fwd into buffers that are full of NaN beforehand: (terms, signs)."""
    from nerfacc_amd import _backend as B
    C = enc.n_components
    n = B.load().nfa_vmreg_partials(C, enc.table.c_res)
    partials = torch.full((n, 4), float("nan"), device=params.device)
    signs = torch.full((3, C, C), float("nan"), device=params.device)
    terms = torch.full((3, 6), float("nan"), device=params.device)
    B.call("nfa_vmreg_fwd", B.ptr(params), C, enc.table.c_res, B.ptr(partials), n, B.ptr(signs), B.ptr(terms), B.stream())
    return terms, signs


def _native_grad(enc, params, g_terms, signs):
    """nfa_vmreg_bwd into a buffer that is full of NaN beforehand."""
    from nerfacc_amd import _backend as B
    out = torch.full_like(params, float("nan"))
    B.call("nfa_vmreg_bwd", B.ptr(params), enc.n_components, enc.table.c_res, B.ptr(g_terms), B.ptr(signs), B.ptr(out), B.stream())
    return out


def _check_values(got, ref, scale, res, C):
    """The five terms of non-negative summands: every chain is at most 1024 additions, so the relative error is below about
    1024 * 2^-24 = 6e-5.  ortho cancels: each G_ij is a chain of R products, their |.| a chain of ORTHO_CHAIN, so the error
    is at most (R + chain) 2^-24 times the mean over the pairs of sum_r |l[r,i] l[r,j]|."""
    assert plane_chain() <= 1024 and all(line_chain(res[c], C) <= 1024 for _, _, c in R.VM_MODES)
    got, ref, scale = got.cpu().double(), ref.cpu(), scale.cpu()
    print("terms", got.tolist(), "reference", ref.tolist())
    torch.testing.assert_close(got[:, :5], ref[:, :5], rtol=1e-4, atol=0.0)
    rows = torch.tensor([res[c] for _, _, c in R.VM_MODES], dtype=torch.float64)
    bound = (rows + ORTHO_CHAIN) * 2.0 ** -24 * scale
    err = (got[:, 5] - ref[:, 5]).abs()
    print("ortho error", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all()


# ----------------------------------------------------------------------------- values
@pytest.mark.parametrize("res,C", SHAPES)
def test_values(dev, res, C):
    from nerfacc_amd.losses import vm_terms
    p, _, ref, _ = R.case(res, C)
    enc = _enc(res, C, dev, p)
    with torch.no_grad():
        got = vm_terms(enc)
    assert got.shape == (3, 6) and got.dtype == torch.float32 and got.device == enc.params.device
    _check_values(got, ref, R.ortho_scale(p, res, C), res, C)


def test_values_with_several_runs_of_partial_rows(dev):
    """Planes of more than NFA_VR_FIN * NFA_VR_RUN tiles and a line of more than NFA_VR_RUN quads per lane: the finish
    kernel's lanes add more than one run of either."""
    from nerfacc_amd import _backend as B
    from nerfacc_amd.losses import vm_terms
    res, C = SEVERAL_RUNS
    enc = _enc(res, C, dev, torch.zeros(1))
    with torch.no_grad():
        enc.params.copy_(0.5 * torch.randn(enc.params.numel(), generator=torch.Generator().manual_seed(3)).to(dev))
        got = vm_terms(enc)
        ref = R.terms_reference(enc.params.detach(), res, C)      # float64, on the device
        scale = R.ortho_scale(enc.params.detach(), res, C)
    assert B.load().nfa_vmreg_partials(C, enc.table.c_res) == 1 + 2 * (NFA_VR_FIN * NFA_VR_RUN + 3)
    assert -(-res[2] * (C // 4) // NFA_VR_FIN) > NFA_VR_RUN
    _check_values(got, ref, scale, res, C)


# ----------------------------------------------------------------------------- reproducibility
def test_two_calls_give_the_same_bits(dev):
    from nerfacc_amd.losses import vm_terms
    res, C = LARGE
    p, g, _, _ = R.case(res, C)
    enc = _enc(res, C, dev, p)
    outs = []
    for _ in range(2):
        t = vm_terms(enc)
        (gp,) = torch.autograd.grad(t, enc.params, g.to(dev))
        outs.append((t.detach(), gp))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))


# ----------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("res,C", SHAPES)
def test_gradient_bit_for_bit_and_against_float64(dev, res, C):
    from nerfacc_amd.losses import _sign0, _vm_terms_grad_torch, vm_terms
    p, g, _, ref_gp = R.case(res, C)
    enc = _enc(res, C, dev, p)
    pd, gd = enc.params.detach(), g.to(dev)
    terms, signs = _native_fwd(enc, pd)
    assert not torch.isnan(terms).any() and not torch.isnan(signs).any()   # every element of both is written
    assert (signs == signs.transpose(1, 2)).all() and (signs.diagonal(dim1=1, dim2=2) == 0).all()
    for m in range(3):                                                  # the signs of the float32 Gram matrix, off the diagonal
        l = enc.line(m).detach()
        gram = torch.zeros(C, C, device=dev)
        for r in range(l.shape[0]):
            gram = gram + l[r][:, None] * l[r][None, :]
        assert torch.equal(signs[m], _sign0(gram) * (1.0 - torch.eye(C, device=dev)))
    got = _native_grad(enc, pd, gd, signs)
    assert not torch.isnan(got).any()                                   # every element is written
    want = _vm_terms_grad_torch(pd, gd, enc.table)                      # float32, on the device, operation for operation
    assert torch.equal(_bits(got), _bits(want))
    torch.testing.assert_close(got.cpu().double(), ref_gp, **_tol(ref_gp))
    t = vm_terms(enc)                                                   # the same through autograd
    assert torch.equal(_bits(t.detach()), _bits(terms))
    (auto,) = torch.autograd.grad(t, enc.params, gd)
    assert torch.equal(_bits(auto), _bits(got))


# ----------------------------------------------------------------------------- alignment
def test_params_at_a_four_byte_offset(dev):
    from nerfacc_amd.losses import vm_terms
    res, C = (7, 6, 5), 24
    p, g, _, _ = R.case(res, C)
    enc = _enc(res, C, dev, p)
    t0 = vm_terms(enc)
    (g0,) = torch.autograd.grad(t0, enc.params, g.to(dev))
    store = torch.empty(p.numel() + 1, device=dev)
    store[1:] = p.to(dev)
    enc.params = torch.nn.Parameter(store[1:])
    assert enc.params.data_ptr() % 16 == 4
    t1 = vm_terms(enc)
    (g1,) = torch.autograd.grad(t1, enc.params, g.to(dev))
    assert torch.equal(_bits(t0.detach()), _bits(t1.detach())) and torch.equal(_bits(g0), _bits(g1))


def test_misaligned_pointers_are_refused_by_the_entries(dev):
    from nerfacc_amd import _backend as B
    res, C = (7, 6, 5), 4
    enc = _enc(res, C, dev)
    store = torch.zeros(enc.params.numel() + 4, device=dev)
    g = torch.zeros(3, 6, device=dev)
    signs = torch.zeros(3, C, C, device=dev)
    with pytest.raises(B.NativeError, match="vmreg_fwd: params, partials and signs must be 16-byte aligned"):
        _native_fwd(enc, store[1:-3])
    with pytest.raises(B.NativeError, match="vmreg_bwd: params, signs and grad_params must be 16-byte aligned"):
        _native_grad(enc, store[1:-3], g, signs)
    assert isinstance(enc.table.c_res, ctypes.Array)


# ----------------------------------------------------------------------------- special values
def test_l1_gradient_is_zero_at_zero(dev):
    from nerfacc_amd.losses import vm_regularization
    res, C = (7, 6, 5), 8
    p = R.make_params(res, C)
    enc = _enc(res, C, dev, p)
    (gp,) = torch.autograd.grad(vm_regularization(enc, l1=1.0), enc.params)
    gp = gp.cpu()
    assert (p == 0.0).any() and (gp[p == 0.0] == 0).all()
    assert (gp[p != 0.0] != 0).all() and torch.equal(torch.sign(gp), torch.sign(p))


def test_a_nan_stays_in_its_mode(dev):
    from nerfacc_amd.losses import vm_terms
    res, C = (7, 6, 5), 8
    for m in range(3):
        enc = _enc(res, C, dev)
        with torch.no_grad():
            enc.line(m)[2, 3] = float("nan")
        terms = vm_terms(enc)
        (gp,) = torch.autograd.grad(terms, enc.params, torch.ones(3, 6, device=dev))
        bad = torch.isnan(terms.detach()).cpu()
        want = torch.zeros(3, 6, dtype=torch.bool)
        want[m, 3:] = True                                               # the line's three terms; the mode's plane terms stay
        assert torch.equal(bad, want), (m, terms)
        gp = gp.detach().clone()
        assert torch.isnan(enc.table.line(gp, m)).all()                  # through the Gram matrix every line element sees it
        enc.table.line(gp, m).zero_()
        assert torch.isfinite(gp).all()                                  # the mode's plane and the other modes do not


# ----------------------------------------------------------------------------- training
def test_backward_adds_to_an_existing_grad(dev):
    from nerfacc_amd.losses import vm_regularization
    enc = _enc((7, 6, 5), 8, dev)
    vm_regularization(enc, tv=1.0, l1=1.0, tv_line=1.0, ortho=1.0).backward()
    once = enc.params.grad.clone()
    vm_regularization(enc, tv=1.0, l1=1.0, tv_line=1.0, ortho=1.0).backward()
    assert once.abs().sum() > 0 and torch.equal(enc.params.grad, once + once)


def test_a_short_run_follows_the_torch_path(dev):
    """3 Adam steps on the regularisers alone (every parameter moves in every step, so every term has moved after the
    first): the native path's terms are those of the torch path."""
    from nerfacc_amd import losses
    res, C = (9, 8, 7), 8
    runs = {}
    for name in ("native", "torch"):
        enc = _enc(res, C, dev)
        opt = torch.optim.Adam(enc.parameters(), lr=2e-3)
        w = losses._vm_weights(enc, 1.0, 1.0, 1.0, 1.0)
        track = []
        for _ in range(4):                                               # (the fourth evaluation sees the third step)
            opt.zero_grad()
            terms = losses.vm_terms(enc) if name == "native" else losses._vm_terms_torch(enc.params, enc.table)
            (terms * w).sum().backward()
            opt.step()
            track.append(terms.detach())
        runs[name] = torch.stack(track).cpu().double()
    native, ref = runs["native"], runs["torch"]
    assert (native[1:] != native[:-1]).all()
    torch.testing.assert_close(native, ref, **_tol(ref))


# ----------------------------------------------------------------------------- the native path, and only once
def test_native_path_is_taken_without_host_synchronisation(dev, monkeypatch):
    from nerfacc_amd import _backend as B, losses
    res, C = LARGE
    enc = _enc(res, C, dev)

    def step():
        enc.params.grad = None
        losses.vm_regularization(enc, tv=0.5, l1=0.25, tv_line=0.1, ortho=0.01).backward()
        return enc.params.grad

    want = step()   # (library loaded, allocator warm, the weight tensor built)

    def boom(*a, **k):
        raise AssertionError("the torch path ran on CUDA float32 parameters")
    monkeypatch.setattr(losses, "_vm_terms_torch", boom)
    names = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert names == ["nfa_vmreg_fwd", "nfa_vmreg_bwd"]
    assert torch.equal(_bits(want), _bits(got))


def test_second_order_is_refused(dev):
    from nerfacc_amd.losses import vm_terms
    enc = _enc((7, 6, 5), 4, dev)
    (gp,) = torch.autograd.grad(vm_terms(enc).sum(), enc.params, create_graph=True)
    with pytest.raises(NotImplementedError, match="vm_terms"):
        torch.autograd.grad(gp.sum(), enc.params)

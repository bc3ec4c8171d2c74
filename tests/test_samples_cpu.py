"""CPU: nerfacc_amd.samples.sample_positions on its torch path -- bit-identity with the reference's expression, the
contractions against a float64 restatement, gradients, argument errors, empty inputs -- and the C ABI of the two native
entry points.  The restatement and the derived error bounds below are shared with tests/test_samples_gpu.py."""
import ctypes as C

import pytest
import torch

EPS = 2.0 ** -24   # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ float64 restatement
def contract_f64(x, kind):
    """x (normalised to the box) -> contracted x, from the issue's formulas: u = 2x - 1, m = |u|_2 ("sphere") or |u|_inf
    ("cube", through its first argmax: the subgradient of that coordinate at ties); m > 1: u <- (2 - 1/m)(u / m);
    x = u / 4 + 0.5."""
    u = 2 * x - 1
    if kind == "sphere":
        m = (u * u).sum(-1, keepdim=True).sqrt()
    else:
        a = u.abs()
        m = a.gather(-1, a.argmax(-1, keepdim=True))
    ms = torch.where(m > 1, m, torch.ones_like(m))
    u = torch.where(m > 1, (2 - 1 / ms) * (u / ms), u)
    return u / 4 + 0.5


def restate_f64(o, d, ts, te, ri, aabb=None, contraction=None, dirs=None):
    """(p, x, dirs, selector) in float64 from the given (float32) inputs; ri None: batched, the ray is the row.
    p is returned with retain_grad so that g_p can be read after a backward."""
    o, d, ts, te = (t.to(torch.float64) for t in (o, d, ts, te))
    if ri is None:
        oo, dd = o[:, None, :], d[:, None, :].expand(*ts.shape, 3)
    else:
        oo, dd = o[ri], d[ri]
    p = oo + dd * (ts + te)[..., None] / 2
    if p.requires_grad:
        p.retain_grad()
    x, sel = p, None
    if aabb is not None:
        box = torch.as_tensor(aabb, dtype=torch.float32).to(device=p.device, dtype=torch.float64)
        x = (p - box[:3]) / (box[3:] - box[:3])
        if contraction is not None:
            x = contract_f64(x, contraction)
        sel = ((x > 0) & (x < 1)).all(-1)
    dr = None if dirs is None else (dd.contiguous() if dirs == "raw" else (dd + 1) / 2)
    return p, x, dr, sel


# ------------------------------------------------------------------------------------------------ derived bounds
def forward_bound(o, d, ts, te, ri, aabb, contraction):
    """First-order bound on |x_float32 - x_float64| per coordinate: (rounded operations) x 2^-24 x scale, the scale being
    the sum of the absolute values of the terms, carried through the divisions.  Tests allow twice this.

    x = (o + d (ts + te) / 2 - lo) / (hi - lo): 6 roundings (ts + te, d *, + o, - lo, hi - lo, /; the halving is exact),
        scale X = (|o| + |d| (|ts| + |te|) / 2 + |lo|) / |hi - lo|.
    u = 2x - 1: one more, 7 in all, scale S = 2X + 1.
    Not contracted (m <= 1): x' = u / 4 + 0.5 adds one: 8, scale S / 4 + 0.5.
    Contracted (m > 1): u'_k = (2 - 1/m) u_k / m.  The 7 roundings behind each u_j reach u'_k through the Jacobian
        J_kj = a [k = j] + c' u_k w_j (a = (2m - 1) / m^2, c' = 2 (1 - m) / m^3, w = dm/du: u / m or the unit vector of
        the argmax): T_k = sum_j |J_kj| S_j.  m costs 6 roundings for the 2-norm (3 squares, 2 sums, the root), none for
        the infinity norm; 1/m, 2 - 1/m, u/m and their product 4; each moves u'_k by at most 2^-24 x 2 |u_k| / m.
        With the final + 0.5: 18 (sphere) or 12 (cube) roundings, scale (T_k + 2 |u_k| / m) / 4 + 0.5.
    The map is continuous (and has a continuous Jacobian) across m = 1, so a float32 m on the other side of 1 than the
    float64 one costs second order only."""
    o, d, ts, te = (t.to(torch.float64) for t in (o, d, ts, te))
    if ri is None:
        oo, dd = o[:, None, :], d[:, None, :].expand(*ts.shape, 3)
    else:
        oo, dd = o[ri], d[ri]
    box = torch.as_tensor(aabb, dtype=torch.float32).to(device=o.device, dtype=torch.float64)
    lo, ext = box[:3], box[3:] - box[:3]
    X = (oo.abs() + dd.abs() * (ts.abs() + te.abs())[..., None] / 2 + lo.abs()) / ext.abs()
    if contraction is None:
        return 6 * EPS * X
    S = 2 * X + 1
    x = (oo + dd * (ts + te)[..., None] / 2 - lo) / ext
    u = 2 * x - 1
    if contraction == "sphere":
        m = (u * u).sum(-1, keepdim=True).sqrt()
        w = u / m
        n_ops = 18
    else:
        a_ = u.abs()
        k = a_.argmax(-1, keepdim=True)
        m = a_.gather(-1, k)
        w = torch.zeros_like(u).scatter(-1, k, 1.0)
        n_ops = 12
    a = (2 * m - 1) / m ** 2
    c = 2 * (m - 1).abs() / m ** 3
    T = a * S + c * u.abs() * (w.abs() * S).sum(-1, keepdim=True)
    inside = 8 * EPS * (S / 4 + 0.5)
    outside = n_ops * EPS * ((T + 2 * u.abs() / m) / 4 + 0.5)
    return torch.where(m > 1, outside, inside)


# ------------------------------------------------------------------------------------------------ cases
AABB = [-1.0, -1.5, -0.5, 1.0, 0.5, 1.5]


def random_case(seed, n_rays=9, n=200, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n_rays, 3, generator=g) - 0.5) * 2
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    ts = torch.rand(n, generator=g) * spread
    te = ts + torch.rand(n, generator=g) * 0.1
    ri = torch.randint(0, n_rays, (n,), generator=g)
    return o, d, ts, te, ri


def test_torch_path_is_the_reference_expression_bit_for_bit():
    from nerfacc_amd.samples import sample_positions
    rays_o, rays_d, t_starts, t_ends, ray_indices = random_case(0)
    t_origins = rays_o[ray_indices]
    t_dirs = rays_d[ray_indices]
    positions = t_origins + t_dirs * (t_starts + t_ends)[:, None] / 2.0
    out = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices, dirs="unit")
    assert out.selector is None and torch.equal(out.positions, positions)
    assert torch.equal(out.dirs, (t_dirs + 1) / 2)
    assert torch.equal(sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices, dirs="raw").dirs, t_dirs)
    # batched: the ray of an element is its row
    tb, eb = t_starts[:45].view(9, 5), t_ends[:45].view(9, 5)
    rows = torch.arange(9).repeat_interleave(5)
    want = (rays_o[rows] + rays_d[rows] * (tb + eb).reshape(-1)[:, None] / 2.0).view(9, 5, 3)
    got = sample_positions(rays_o, rays_d, tb, eb, dirs="raw")
    assert got.positions.shape == (9, 5, 3) and torch.equal(got.positions, want)
    assert got.dirs.shape == (9, 5, 3) and torch.equal(got.dirs, rays_d[rows].view(9, 5, 3))


# points (as ray origins with a zero direction, so p = o exactly) in the box [-1, 1]^3, where u = p
_BOX = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
_POINTS = [
    [0.3, -0.2, 0.5], [0.0, 0.0, 0.0],                       # inside
    [1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-1.0, 1.0, 0.25],     # |u| = 1 in one norm or the other
    [600.0, -800.0, 100.0], [-3.0, 1000.0, 999.0],           # far outside, m ~ 1e3
    [1.5, -0.2, 0.1], [0.9, 0.9, 0.9],                       # just outside / outside for the 2-norm only
]


@pytest.mark.parametrize("kind", ["sphere", "cube"])
def test_contractions_match_the_float64_restatement(kind):
    from nerfacc_amd.samples import sample_positions
    o = torch.tensor(_POINTS, dtype=torch.float32)
    d = torch.zeros_like(o)
    ts, te = torch.full((len(o),), 0.5), torch.full((len(o),), 0.75)
    ri = torch.arange(len(o))
    got = sample_positions(o, d, ts, te, ri, aabb=_BOX, contraction=kind, selector=True)
    _, x, _, sel = restate_f64(o, d, ts, te, ri, _BOX, kind)
    bound = forward_bound(o, d, ts, te, ri, _BOX, kind)
    err = (got.positions.double() - x).abs()
    assert bool((err <= 2 * bound).all()), float((err / bound).max())
    assert torch.equal(got.selector, sel) and bool(sel.all())   # everything lands strictly inside (0, 1)
    # the box lands on [0.25, 0.75]^3, far points just inside the ball / cube of radius 1/2
    assert torch.equal(got.positions[0], torch.tensor([0.3, -0.2, 0.5]) / 4 + 0.5)
    far = got.positions[5:7]
    r = (far - 0.5).norm(dim=-1) if kind == "sphere" else (far - 0.5).abs().amax(-1)   # |u'| / 4 = (2 - 1/m) / 4
    assert bool(((r > 0.499) & (r < 0.5)).all()) and bool(((far > 0) & (far < 1)).all())
    # random points too, spread over both branches
    o, d, ts, te, ri = random_case(1, spread=6.0)
    got = sample_positions(o, d, ts, te, ri, aabb=AABB, contraction=kind)
    _, x, _, _ = restate_f64(o, d, ts, te, ri, AABB, kind)
    err = (got.positions.double() - x).abs()
    assert bool((err <= 2 * forward_bound(o, d, ts, te, ri, AABB, kind)).all())
    m = (2 * restate_f64(o, d, ts, te, ri, AABB)[1] - 1).abs().amax(-1)
    assert 0.1 < float((m > 1).double().mean()) < 0.9


def test_selector_on_a_face_is_false():
    from nerfacc_amd.samples import sample_positions
    o = torch.tensor([[-1.0, 0.2, 0.3], [0.2, 1.0, 0.3], [0.2, 0.3, 0.999], [0.2, 0.3, -1.5]])
    d = torch.zeros_like(o)
    t = torch.ones(4)
    out = sample_positions(o, d, t, t, torch.arange(4), aabb=torch.tensor(_BOX), selector=True)
    assert out.positions[0, 0] == 0.0 and out.positions[1, 1] == 1.0
    assert out.selector.tolist() == [False, False, True, False]
    assert torch.equal(out.positions, (o + 1) / 2)


@pytest.mark.parametrize("mode", [None, "aabb", "sphere", "cube"])
@pytest.mark.parametrize("batched", [False, True])
def test_torch_path_gradients_match_float64_autograd(mode, batched):
    """The torch path in float64 against autograd of the restatement (both carry ~50 float64 roundings per element:
    rtol 1e-12), and in float32 against the same within 1e-4 of each gradient's largest entry (float32 rounding of a
    chain of that length on inputs of order 1..10)."""
    from nerfacc_amd.samples import sample_positions
    o, d, ts, te, ri = random_case(2, spread=6.0)
    if batched:
        ts, te, ri = ts[:45].view(9, 5), te[:45].view(9, 5), None
    aabb = None if mode is None else AABB
    contraction = mode if mode in ("sphere", "cube") else None
    g = torch.Generator().manual_seed(3)
    gx = torch.randn(*ts.shape, 3, generator=g, dtype=torch.float64)
    gd = torch.randn(*ts.shape, 3, generator=g, dtype=torch.float64)

    def grads(fn, dtype):
        xs = [t.to(dtype).requires_grad_(True) for t in (o, d, ts, te)]
        pos, dirs = fn(*xs)
        return torch.autograd.grad((pos * gx.to(dtype)).sum() + (dirs * gd.to(dtype)).sum(), xs)

    def ours(a, b, c, e):
        out = sample_positions(a, b, c, e, ri, aabb=aabb, contraction=contraction, dirs="unit", selector=aabb is not None)
        assert out.selector is None or not out.selector.requires_grad
        return out.positions, out.dirs

    def ref(a, b, c, e):
        _, x, dr, _ = restate_f64(a, b, c, e, ri, aabb, contraction, "unit")
        return x, dr

    want = grads(ref, torch.float64)
    for a, b in zip(grads(ours, torch.float64), want):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))
    for a, b in zip(grads(ours, torch.float32), want):
        assert a.dtype == torch.float32 and float((a.double() - b).abs().max()) <= 1e-4 * float(b.abs().max())


def test_value_errors():
    from nerfacc_amd.samples import sample_positions
    o, d, ts, te, ri = random_case(4)
    for kw in (dict(selector=True), dict(contraction="sphere"), dict(contraction="cube"), dict(aabb=AABB, contraction="tanh"),
               dict(dirs="normalized"), dict(aabb=AABB, contraction="Sphere"), dict(aabb=[0.0, 1.0])):
        with pytest.raises(ValueError):
            sample_positions(o, d, ts, te, ri, **kw)


def test_empty_inputs():
    from nerfacc_amd.samples import sample_positions
    o, d, _, _, _ = random_case(5)
    e = torch.empty(0)
    out = sample_positions(o, d, e, e, torch.empty(0, dtype=torch.int64), aabb=AABB, contraction="sphere", dirs="unit", selector=True)
    assert out.positions.shape == (0, 3) and out.dirs.shape == (0, 3) and out.selector.shape == (0,) and out.selector.dtype == torch.bool
    out = sample_positions(o, d, torch.empty(9, 0), torch.empty(9, 0), aabb=AABB, dirs="raw", selector=True)
    assert out.positions.shape == (9, 0, 3) and out.dirs.shape == (9, 0, 3) and out.selector.shape == (9, 0)
    z = torch.empty(0, 3)
    out = sample_positions(z, z, torch.empty(0, 4), torch.empty(0, 4), dirs="unit")
    assert out.positions.shape == (0, 4, 3) and out.dirs.shape == (0, 4, 3) and out.selector is None
    out = sample_positions(z, z, e, e, torch.empty(0, dtype=torch.int64))
    assert out.positions.shape == (0, 3) and out.dirs is None


# ------------------------------------------------------------------------------------------------ C ABI
P = 0x1000   # a stand-in address that is never dereferenced
_BOX6 = (C.c_float * 6)(*_BOX)
_FWD = "rays_o rays_d t_starts t_ends ray_indices n_rays n_elems samples_per_ray aabb_host aabb contraction dirs_mode " \
       "positions dirs selector stream"
_BWD = "rays_o rays_d t_starts t_ends ray_indices g_positions g_dirs packed_info tiles n_tiles n_rays n_elems samples_per_ray " \
       "aabb_host aabb contraction dirs_mode grad_rays_o grad_rays_d grad_t_starts grad_t_ends grad_p stream"
_DEFAULTS = dict(n_rays=4, n_elems=16, samples_per_ray=0, n_tiles=1, aabb_host=None, aabb=None, contraction=0, dirs_mode=0,
                 dirs=None, selector=None, g_dirs=None, grad_p=None, stream=None)
_CASES = [
    ("nfa_sample_positions_fwd", _FWD, [
        (dict(n_rays=-1), "sample_positions_fwd: negative size"),
        (dict(n_elems=-1), "sample_positions_fwd: negative size"),
        (dict(samples_per_ray=-2), "sample_positions_fwd: negative size"),
        (dict(n_rays=(1 << 31) - 64), "sample_positions_fwd: too many rays"),
        (dict(contraction=3, aabb_host=_BOX6), "sample_positions_fwd: contraction and dirs_mode must be 0, 1 or 2"),
        (dict(dirs_mode=-1), "sample_positions_fwd: contraction and dirs_mode must be 0, 1 or 2"),
        (dict(contraction=1), "sample_positions_fwd: contraction needs an aabb"),
        (dict(contraction=2, n_elems=0), "sample_positions_fwd: contraction needs an aabb"),
        (dict(selector=P), "sample_positions_fwd: the selector needs an aabb"),
        (dict(aabb_host=_BOX6, aabb=P), "sample_positions_fwd: aabb given twice"),
        (dict(n_elems=0, rays_o=None, rays_d=None, t_starts=None, t_ends=None, ray_indices=None, positions=None), None),
        *[({k: None}, "sample_positions_fwd: null pointer") for k in "rays_o rays_d t_starts t_ends positions".split()],
        (dict(dirs_mode=1), "sample_positions_fwd: dirs and dirs_mode must be given together"),
        (dict(dirs=P), "sample_positions_fwd: dirs and dirs_mode must be given together"),
        (dict(ray_indices=None), "sample_positions_fwd: without ray_indices n_elems must be n_rays * samples_per_ray"),
        (dict(ray_indices=None, samples_per_ray=3), "sample_positions_fwd: without ray_indices n_elems must be n_rays * samples_per_ray"),
        (dict(n_rays=0), "sample_positions_fwd: without ray_indices n_elems must be n_rays * samples_per_ray"),
    ]),
    ("nfa_sample_positions_bwd", _BWD, [
        (dict(n_rays=-1), "sample_positions_bwd: negative size"),
        (dict(n_elems=-1), "sample_positions_bwd: negative size"),
        (dict(n_rays=(1 << 31) - 64), "sample_positions_bwd: too many rays"),
        (dict(contraction=-1), "sample_positions_bwd: contraction and dirs_mode must be 0, 1 or 2"),
        (dict(dirs_mode=3), "sample_positions_bwd: contraction and dirs_mode must be 0, 1 or 2"),
        (dict(contraction=1), "sample_positions_bwd: contraction needs an aabb"),
        (dict(aabb_host=_BOX6, aabb=P), "sample_positions_bwd: aabb given twice"),
        (dict(n_elems=0, n_rays=0, rays_o=None, packed_info=None, tiles=None), None),
        (dict(n_elems=0, grad_rays_o=None, grad_rays_d=None, rays_o=None), None),
        *[({k: None}, "sample_positions_bwd: null pointer") for k in "rays_o rays_d t_starts t_ends".split()],
        (dict(g_dirs=P), "sample_positions_bwd: g_dirs needs dirs_mode"),
        (dict(packed_info=None), "sample_positions_bwd: packed_info/tiles is null"),
        (dict(tiles=None), "sample_positions_bwd: packed_info/tiles is null"),
        (dict(n_tiles=0), "sample_positions_bwd: packed_info/tiles is null"),
        (dict(g_positions=None), "sample_positions_bwd: per-ray sums need g_positions or g_dirs, and write no grad_p"),
        (dict(grad_p=P), "sample_positions_bwd: per-ray sums need g_positions or g_dirs, and write no grad_p"),
        # the flat form (no per-ray gradient asked for)
        (dict(grad_rays_o=None, grad_rays_d=None, g_positions=None), "sample_positions_bwd: null pointer"),
        (dict(grad_rays_o=None, grad_rays_d=None, grad_t_starts=None, grad_t_ends=None), "sample_positions_bwd: null pointer"),
        (dict(grad_rays_o=None, grad_rays_d=None, ray_indices=None),
         "sample_positions_bwd: without ray_indices n_elems must be n_rays * samples_per_ray"),
    ]),
]


def test_abi_symbols_and_argument_errors():
    """Both entry points are exported, bound, and reject bad arguments with a fixed text before anything reaches the GPU."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert lib.nfa_version() == B.ABI_VERSION
    for fn, names, cases in _CASES:
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn)
        assert len(B._SIGS[fn]) == len(names.split())
        for kw, msg in cases:
            args = [kw[a] if a in kw else _DEFAULTS.get(a, P) if a in _DEFAULTS else P for a in names.split()]
            lib.nfa_set_tuning(b"", None)   # leaves a known error text behind
            rc = getattr(lib, fn)(*args)
            if msg is None:
                assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
            else:
                assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())

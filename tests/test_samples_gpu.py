"""GPU: nerfacc_amd.samples.sample_positions on the native ops nfa_sample_positions_{fwd,bwd} -- bit-identity with the
torch expression, the box and the contractions against the float64 restatement under derived bounds, the selector,
gradients (per sample and the per-ray sums of the segmented engine), the scalar form on unaligned bases, batched and
unsorted input, determinism, composition with the hash grid, graph capture."""
import pytest
import torch

from test_distortion_gpu import ragged_case
from test_samples_cpu import EPS, forward_bound, restate_f64

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 64, 65, 257, 0, 1000]   # empty rays, a lane-sized tail, a wave boundary, multi-step rays
MODES = [None, "aabb", "sphere", "cube"]
AABB = [-6.0, -8.0, -5.0, 7.0, 6.0, 8.0]    # case A's rays reach t ~ 30: a good share of the samples on either side of its faces
_CACHE = {}


def _mode(mode):
    return (None if mode is None else AABB), (mode if mode in ("sphere", "cube") else None)


def case(dev, name):
    """Inputs of cases A-D (built once).  A: ragged rays, t on a 2^-8 grid, aligned bases.  B: the same tensors viewed
    from element 1 (bases off by 4 / 8 bytes: the scalar form).  C: batched (7, 5).  D: A with the samples permuted."""
    if not _CACHE:
        _, ts, te, ri, R = ragged_case(LENGTHS, seed=11)
        g = torch.Generator().manual_seed(12)
        o = (torch.rand(R, 3, generator=g) - 0.5) * 2
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        n = ts.numel()
        gx, gd = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
        perm = torch.randperm(n, generator=g)
        A = dict(o=o, d=d, ts=ts, te=te, ri=ri, gx=gx, gd=gd)
        A = {k: v.to(dev) for k, v in A.items()}
        _CACHE["A"] = A
        _CACHE["B"] = dict(A, **{k: A[k][1:] for k in ("ts", "te", "ri", "gx", "gd")})
        _CACHE["D"] = dict(A, perm=perm.to(dev), **{k: A[k][perm.to(dev)].contiguous() for k in ("ts", "te", "ri", "gx", "gd")})
        tb = (torch.rand(7, 5, generator=g) * 6).to(dev)
        _CACHE["C"] = dict(o=A["o"][:7].contiguous(), d=A["d"][:7].contiguous(), ts=tb, te=tb + 0.0625, ri=None,
                           gx=torch.randn(7, 5, 3, generator=g).to(dev), gd=torch.randn(7, 5, 3, generator=g).to(dev))
    return _CACHE[name]


def rows_of(c):
    return c["ri"] if c["ri"] is not None else torch.arange(c["ts"].shape[0], device=c["ts"].device).repeat_interleave(c["ts"].shape[1])


def run_native(c, mode, dirs="unit", with_gd=True, selector=False):
    """Forward outputs and the four gradients of sum(positions * gx) + sum(dirs * gd)."""
    from nerfacc_amd.samples import sample_positions
    aabb, contraction = _mode(mode)
    xs = [c[k].detach().clone().requires_grad_(True) for k in ("o", "d", "ts", "te")]
    if c["ri"] is not None and c["ts"].data_ptr() % 16:   # keep case B's bases unaligned: clone() would realign them
        for i, k in ((2, "ts"), (3, "te")):
            buf = torch.empty(c[k].numel() + 1, device=c[k].device)
            buf[1:] = c[k]
            xs[i] = buf[1:].detach().requires_grad_(True)
    out = sample_positions(*xs, c["ri"], aabb=aabb, contraction=contraction, dirs=dirs, selector=selector)
    loss = (out.positions * c["gx"]).sum()
    if with_gd and dirs is not None:
        loss = loss + (out.dirs * c["gd"]).sum()
    return out, torch.autograd.grad(loss, xs)


def run_f64(c, mode, dirs="unit", with_gd=True):
    aabb, contraction = _mode(mode)
    xs = [c[k].detach().double().requires_grad_(True) for k in ("o", "d", "ts", "te")]
    p, x, dr, sel = restate_f64(*xs, c["ri"], aabb, contraction, dirs)
    loss = (x * c["gx"].double()).sum()
    if with_gd and dirs is not None:
        loss = loss + (dr * c["gd"].double()).sum()
    grads = torch.autograd.grad(loss, xs + [p])
    return (x.detach(), dr, sel), grads[:4], grads[4].detach()


def grad_bounds(c, mode, g_p, dscale):
    """First-order bounds (tests allow twice) on the float32 gradients against float64 autograd of the restatement, from
    the float64 g_p = J^T g_x: (rounded operations) x 2^-24 x (sum of the absolute values of the terms).

    g_p per coordinate, B_p:
      no box      g_p = g_x: exact, 0.
      box         g_p = g_x / (hi - lo): 2 roundings (hi - lo, /), scale |g_p|.
      contracted  g_p = (2 / ext) (a g' + c (u . g') w), g' = g_x / 4, at the recomputed u (notation of
                  test_samples_cpu.forward_bound; not contracted where m <= 1).  Local roundings, each at most 2^-24 x
                  L_k, L_k = (2 / |ext_k|) (a |g'_k| + c^ |w_k| sum_j |u_j g'_j|) with c^ = 2 (1 + m) / m^3 (the absolute
                  values of the terms of 2 (1 - m)): m 6 for the 2-norm, counted twice because a and c^ move by up to
                  twice m's relative error (|m a'/a| < 1, |m c'/c^| < 2), none for the infinity norm; a 3 (2m - 1, m m,
                  /); c 4 (1 - m, m m m, /); the dot product 5; c (u . g') 1; w 1 (u / m; 0 for the cube); a g', the
                  product with w and their sum 3; hi - lo and / 2: 31 (sphere) or 18 (cube).  Input: the 7 roundings
                  behind each u_j (forward_bound, scale S_j) reach g_p,k through d g_p,k / d u_j, taken from float64
                  autograd: 7 x 2^-24 x sum_j |d g_p,k / d u_j| S_j.
    g_t_start = g_t_end = 1/2 d . g_p: 3 products and 2 sums on top: 1/2 sum_k |d_k| B_p,k + 5 x 2^-24 x 1/2 sum_k |d_k g_p,k|.
    g_o[r] = sum g_p: sum B_p + n_r x 2^-24 x sum |g_p| (one rounding per summed element).
    g_d[r] = sum (m g_p + s g_dirs), m = (ts + te) / 2: ts + te, m g_p and the sum with s g_dirs are 3 roundings (s = 1 or
        1/2 and the halving are exact): sum |m| B_p + (3 + n_r) x 2^-24 x sum (|m| |g_p| + s |g_dirs|), |m| <= (|ts| + |te|) / 2.
    Returns (B_t [n], B_o [R, 3], B_d [R, 3])."""
    aabb, contraction = _mode(mode)
    o, d, ts, te = (c[k].double() for k in ("o", "d", "ts", "te"))
    rows = rows_of(c)
    R = o.shape[0]
    ts, te = ts.reshape(-1), te.reshape(-1)
    oo, dd = o[rows], d[rows]
    gx = c["gx"].double().reshape(-1, 3)
    g_p = g_p.reshape(-1, 3)
    if aabb is None:
        Bp = torch.zeros_like(g_p)
    else:
        box = torch.tensor(aabb, dtype=torch.float32).to(device=o.device, dtype=torch.float64)
        lo, ext = box[:3], box[3:] - box[:3]
        if contraction is None:
            Bp = 2 * EPS * g_p.abs()
        else:
            X = (oo.abs() + dd.abs() * (ts.abs() + te.abs())[:, None] / 2 + lo.abs()) / ext.abs()
            S = 2 * X + 1
            u0 = 2 * ((oo + dd * (ts + te)[:, None] / 2 - lo) / ext) - 1
            gq = gx / 4

            def parts(u):
                if contraction == "sphere":
                    m = (u * u).sum(-1, keepdim=True).sqrt()
                    w = u / m
                else:
                    k = u.abs().argmax(-1, keepdim=True)
                    m = u.abs().gather(-1, k)
                    w = torch.zeros_like(u).scatter(-1, k, 1.0) * torch.sign(u)
                return m, w, (2 * m - 1) / m ** 2, 2 * (1 - m) / m ** 3

            def gp_of_u(u):
                m, w, a, cc = parts(u)
                gu = torch.where(m > 1, a * gq + cc * (u * gq).sum(-1, keepdim=True) * w, gq)
                return 2 * gu / ext

            u = u0.detach().requires_grad_(True)
            gp = gp_of_u(u)
            assert torch.allclose(gp.detach(), g_p, rtol=1e-9, atol=1e-12)   # the explicit Jacobian is autograd's
            inp = torch.stack([(torch.autograd.grad(gp[:, k].sum(), u, retain_graph=True)[0].abs() * S).sum(-1) for k in range(3)], -1)
            m, w, a, _ = parts(u0)
            chat = 2 * (1 + m) / m ** 3
            L = torch.where(m > 1, a * gq.abs() + chat * w.abs() * (u0 * gq).abs().sum(-1, keepdim=True), gq.abs()) * 2 / ext.abs()
            n_loc = torch.where(m > 1, 31.0 if contraction == "sphere" else 18.0, 2.0)
            Bp = EPS * (n_loc * L + 7 * inp)
    n_r = torch.bincount(rows, minlength=R).double()[:, None]
    add = lambda v: torch.zeros(R, 3, dtype=torch.float64, device=o.device).index_add(0, rows, v)
    B_t = 0.5 * (dd.abs() * Bp).sum(-1) + 5 * EPS * 0.5 * (dd * g_p).abs().sum(-1)
    B_o = add(Bp) + n_r * EPS * add(g_p.abs())
    am = ((ts.abs() + te.abs()) / 2)[:, None]
    B_d = add(am * Bp) + (3 + n_r) * EPS * add(am * g_p.abs() + dscale * c["gd"].double().reshape(-1, 3).abs())
    return B_t, B_o, B_d


def within(got, want, bound, what):
    err = (got.double() - want).abs()
    ok = err <= 2 * bound
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(ok.all()), \
        (what, int((~ok).sum()), float((err / bound.clamp_min(1e-300))[~ok].max()))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_without_a_box_the_outputs_are_the_torch_expression_bit_for_bit(dev, name):
    from nerfacc_amd.samples import sample_positions
    c = case(dev, name)
    rays_o, rays_d, t_starts, t_ends, rows = c["o"], c["d"], c["ts"].reshape(-1), c["te"].reshape(-1), rows_of(c)
    t_origins = rays_o[rows]
    t_dirs = rays_d[rows]
    positions = t_origins + t_dirs * (t_starts + t_ends)[:, None] / 2.0
    shape = tuple(c["ts"].shape)
    out = sample_positions(rays_o, rays_d, c["ts"], c["te"], c["ri"], dirs="unit")
    assert out.positions.shape == shape + (3,) and out.positions.dtype == torch.float32 and out.selector is None
    assert torch.equal(out.positions.reshape(-1, 3), positions)
    assert torch.equal(out.dirs.reshape(-1, 3), (t_dirs + 1) / 2)
    raw = sample_positions(rays_o, rays_d, c["ts"], c["te"], c["ri"], dirs="raw")
    assert torch.equal(raw.dirs.reshape(-1, 3), t_dirs) and torch.equal(raw.positions, out.positions)
    assert sample_positions(rays_o, rays_d, c["ts"], c["te"], c["ri"]).dirs is None


@pytest.mark.parametrize("mode", MODES[1:])
@pytest.mark.parametrize("name", ["A", "C"])
def test_box_and_contractions_match_float64_within_the_derived_bound(dev, name, mode):
    c = case(dev, name)
    out, _ = run_native(c, mode, selector=True)
    (x, _, sel), _, _ = run_f64(c, mode)
    aabb, contraction = _mode(mode)
    bound = forward_bound(c["o"], c["d"], c["ts"], c["te"], c["ri"], aabb, contraction)
    within(out.positions, x, bound, "positions")
    # the selector, wherever float64 x is further than the allowed error from both faces
    clear = ((x.abs() > 2 * bound) & ((x - 1).abs() > 2 * bound)).all(-1)
    assert float((~clear).double().mean()) <= 0.01
    assert out.selector.dtype == torch.bool and torch.equal(out.selector[clear], sel[clear])
    if name == "A":   # both outcomes, and both branches of the contraction, are exercised
        assert 0.02 < float(sel.double().mean()) < 0.98 or contraction is not None
        m = (2 * run_f64(c, "aabb")[0][0] - 1).abs().amax(-1)
        assert 0.02 < float((m > 1).double().mean()) < 0.98


def test_selector_on_a_face_is_false(dev):
    from nerfacc_amd.samples import sample_positions
    o = torch.tensor([[-1.0, 0.2, 0.3], [0.2, 1.0, 0.3], [0.2, 0.3, 0.999], [0.2, 0.3, -1.5], [0.0, 0.0, 0.0]], device=dev)
    t = torch.ones(5, device=dev)
    box = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    for aabb in (box, torch.tensor(box, device=dev)):   # by value, and read from the device
        out = sample_positions(o, torch.zeros_like(o), t, t, torch.arange(5, device=dev), aabb=aabb, selector=True)
        assert out.positions[0, 0] == 0.0 and out.positions[1, 1] == 1.0
        assert out.selector.tolist() == [False, False, True, False, True]


def test_scalar_form_equals_vector_form_bit_for_bit(dev):
    """Case B is case A from element 1 on: unaligned bases take the element-wise form of both kernels."""
    a, b = case(dev, "A"), case(dev, "B")
    assert a["ts"].data_ptr() % 16 == 0 and b["ts"].data_ptr() % 16 == 4 and b["ri"].data_ptr() % 16 == 8
    for mode in MODES:
        oa, ga = run_native(a, mode, selector=mode is not None)
        ob, gb = run_native(b, mode, selector=mode is not None)
        assert torch.equal(oa.positions[1:], ob.positions) and torch.equal(oa.dirs[1:], ob.dirs)
        assert mode is None or torch.equal(oa.selector[1:], ob.selector)
        assert torch.equal(ga[2][1:], gb[2]) and torch.equal(ga[3][1:], gb[3])   # per sample: no sum, the same bits


# ------------------------------------------------------------------------------------------------ backward
def check_grads(c, mode, with_gd, undo=None):
    dirs = "unit" if with_gd else None
    _, got = run_native(c, mode, dirs=dirs, with_gd=with_gd)
    _, want, g_p = run_f64(c, mode, dirs=dirs, with_gd=with_gd)
    cc = c if with_gd else dict(c, gd=torch.zeros_like(c["gd"]))
    B_t, B_o, B_d = grad_bounds(cc, mode, g_p, 0.5)
    shape = c["ts"].shape
    within(got[0], want[0], B_o, "g_rays_o")
    within(got[1], want[1], B_d, "g_rays_d")
    within(got[2], want[2], B_t.view(shape), "g_t_starts")
    within(got[3], want[3], B_t.view(shape), "g_t_ends")
    empty = torch.bincount(rows_of(c), minlength=c["o"].shape[0]) == 0
    assert bool((got[0][empty] == 0).all()) and bool((got[1][empty] == 0).all())
    return got


@pytest.mark.parametrize("with_gd", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_gradients_match_float64_autograd_within_the_derived_bound(dev, name, mode, with_gd):
    c = case(dev, name)
    if name == "A":
        assert int((torch.bincount(c["ri"], minlength=8) == 0).sum()) == 2
    check_grads(c, mode, with_gd)


def test_gradient_arriving_at_dirs_only(dev):
    from nerfacc_amd.samples import sample_positions
    c = case(dev, "A")
    for dirs, s in (("raw", 1.0), ("unit", 0.5)):
        xs = [c[k].detach().clone().requires_grad_(True) for k in ("o", "d", "ts", "te")]
        out = sample_positions(*xs, c["ri"], aabb=AABB, dirs=dirs)
        g = torch.autograd.grad((out.dirs * c["gd"]).sum(), xs)
        want = torch.zeros(8, 3, dtype=torch.float64, device=dev).index_add(0, c["ri"], c["gd"].double() * s)
        n_r = torch.bincount(c["ri"], minlength=8).double()[:, None]
        bound = n_r * EPS * torch.zeros(8, 3, dtype=torch.float64, device=dev).index_add(0, c["ri"], c["gd"].double().abs() * s)
        within(g[1], want, bound, "g_rays_d")
        assert not bool(g[0].any()) and not bool(g[2].any()) and not bool(g[3].any())


def test_backward_is_deterministic_and_takes_the_engine(dev, monkeypatch):
    from nerfacc_amd import _backend as B
    c = case(dev, "A")
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    _, g1 = run_native(c, "sphere")
    _, g2 = run_native(c, "sphere")
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    bwd = [a for name, a in calls if name == "nfa_sample_positions_bwd"]
    assert len(bwd) == 2 and all(a[7] is not None and a[8] is not None and a[17] is not None and a[21] is None for a in bwd)
    assert [name for name, _ in calls].count("nfa_sample_positions_fwd") == 2


@pytest.mark.parametrize("mode", [None, "sphere"])
def test_unsorted_indices_take_index_add_and_match(dev, mode, monkeypatch):
    """Case D: the forward is native for ray indices in any order; the backward reduces g_p with index_add_."""
    from nerfacc_amd import _backend as B
    a, dcase = case(dev, "A"), case(dev, "D")
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *args: (calls.append((name, args)), real(name, *args))[1])
    out_d, _ = run_native(dcase, mode)
    got = check_grads(dcase, mode, True)
    bwd = [args for name, args in calls if name == "nfa_sample_positions_bwd"]
    assert bwd and all(args[7] is None and args[17] is None and args[21] is not None for args in bwd)   # flat: grad_p, no per-ray output
    monkeypatch.undo()
    out_a, ga = run_native(a, mode)
    perm = dcase["perm"]
    assert torch.equal(out_d.positions, out_a.positions[perm]) and torch.equal(out_d.dirs, out_a.dirs[perm])
    assert torch.equal(got[2], ga[2][perm]) and torch.equal(got[3], ga[3][perm])   # per sample: the same arithmetic
    # the per-ray sums of both orders are within the same bound of float64 (check_grads above for D, here for A)
    check_grads(a, mode, True)


# ------------------------------------------------------------------------------------------------ with the rest of the library
def test_composes_with_the_hash_grid(dev):
    from nerfacc_amd.encodings import HashGridEncoding
    from nerfacc_amd.samples import sample_positions
    c = case(dev, "A")
    torch.manual_seed(0)
    enc = HashGridEncoding(3, n_levels=4, n_features_per_level=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.5).to(dev)
    o = c["o"].detach().clone().requires_grad_(True)
    out = sample_positions(o, c["d"], c["ts"], c["te"], c["ri"], aabb=[-8.0, -8.0, -8.0, 8.0, 8.0, 8.0], selector=True)
    y = enc(out.positions)
    assert y.shape == (c["ts"].numel(), 8) and out.selector.dtype == torch.bool
    (y[out.selector] ** 2).sum().backward()
    assert o.grad is not None and o.grad.shape == (8, 3) and bool(torch.isfinite(o.grad).all()) and bool(o.grad.any())
    assert enc.params.grad is not None and bool(enc.params.grad.any())


def test_forward_and_backward_capture_into_a_graph(dev):
    """Forward + backward on tagged ray_indices hold no host synchronisation: the step captures (nerfacc_amd.CapturedStep)
    and every replay gives the eager step's bits.  In a child process, as the other capture tests: a capture that fails
    takes its process down."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from nerfacc_amd.graphs import CapturedStep
from nerfacc_amd.samples import sample_positions
from nerfacc_amd._segments import seginfo_from_ray_indices
import test_samples_gpu as T
dev = torch.device("cuda:0")
c = T.case(dev, "A")
seginfo_from_ray_indices(c["ri"], 8)   # tagged, as sampling() tags what it returns: no read-back in the step
def leaves():
    return [c[k].detach().clone().requires_grad_(True) for k in ("o", "d", "ts", "te")]
def step(xs):
    out = sample_positions(*xs, c["ri"], aabb=T.AABB, contraction="sphere", dirs="unit", selector=True)
    grads = torch.autograd.grad((out.positions * c["gx"]).sum() + (out.dirs * c["gd"]).sum(), xs)
    return (out.positions.detach(), out.dirs.detach(), out.selector, *grads)
# The captured step gets leaves of its own, first used inside the capture: a leaf that an eager step has used keeps an
# AccumulateGrad node bound to the default stream (as long as anything refers to that step's graph), and the autograd
# engine then synchronises the capturing stream with the default one, which a capture does not survive.
xs = leaves()
graph = CapturedStep(lambda: step(xs), warmup=2)
eager = step(leaves())
ok = True
for _ in range(2):
    got = graph()
    torch.cuda.synchronize()
    ok = ok and len(got) == 7 and all(torch.equal(a, b) for a, b in zip(got, eager))
print("OK captured", ok, graph.replays)
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK captured True 2" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-500:])

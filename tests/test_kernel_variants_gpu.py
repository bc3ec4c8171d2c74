"""GPU: the forms of the packed-op engine (csrc/segscan.hip) the other tests do not reach.

Every packed op picks its 16-byte vector form only when all of its float arrays are 16-byte aligned and runs a scalar form
otherwise.  Contiguous views at an element offset (interval edges ``edges[:-1], edges[1:]``, one-row batches
``t[:, 1:]``, gradients that are slices of a larger buffer) reach the scalar form in normal use.  Here every op runs on
aligned inputs and again on the same values at offsets of 1-3 elements, with unaligned incoming gradients: outputs and
gradients must be bit-identical (the two forms load the same values and do the same arithmetic), the scalar form must
have been the one taken (an unaligned pointer reached the entry point), and the aligned result must agree with a float64
restatement (tests/seg_reference.py, checked on the CPU by test_seg_reference_cpu.py) within per-element bounds derived
from the float32 arithmetic.  The channel groups of accumulate_along_rays (D > 4: later groups read back and add to the
weight gradient) and its in-place and unsorted forms are covered the same way.
"""
import numpy as np
import pytest
import torch

import nerfacc_amd as na
import seg_reference as SR
from nerfacc_amd import _backend as B
from nerfacc_amd import volrend
from nerfacc_amd._segments import seginfo_from_ray_indices

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -126 * SR.K_ROUND    # results below float32's normal range have no relative precision


# ----------------------------------------------------------------------------- helpers
def shifted(x: torch.Tensor, k: int) -> torch.Tensor:
    """The values of x as a contiguous view at a storage offset of k elements (k = 1, 2, 3: not 16-byte aligned)."""
    assert k in (1, 2, 3)
    buf = torch.empty(x.numel() + 4, dtype=x.dtype, device=x.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + x.numel()].view(x.shape)
    v.copy_(x.detach())
    assert v.is_contiguous() and (x.numel() == 0 or v.data_ptr() % 16 != 0)
    return v


def ragged_counts(seed: int) -> torch.Tensor:
    """Ray lengths where the engine changes behaviour: 0-5 (a quad's phase moves with the offset), around a wave step
    (256) and the default tile (1024), one ray longer than 4 tiles, a run of more than SEG_TILE_ROWS (256) empty rays,
    short random rays; the total is not a multiple of 4."""
    rng = np.random.default_rng(seed)
    blocks = [[0, 1, 2, 3, 4, 5], [255], [256], [257], [1023], [1024], [1025], [4 * 1024 + 301], [0] * 300,
              list(rng.integers(0, 40, 400)), [5, 4, 3, 2, 1, 0]]
    order = rng.permutation(len(blocks))
    c = np.concatenate([np.asarray(blocks[i], np.int64) for i in order])
    if c.sum() % 4 == 0:
        c = np.append(c, 3)
    return torch.from_numpy(c)


class CallLog:
    """Records every native call (name, arguments) while installed, as test_native_path_taken does."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def unaligned(self, name: str) -> bool:
        """Some data pointer (the arguments before the stream) of a call to ``name`` is not 16-byte aligned."""
        return any(isinstance(v, int) and v > (1 << 32) and v % 16 != 0
                   for n, a in self.calls if n == name for v in a[:-1])

    def assert_scalar_form(self, *names):
        seen = {n for n, _ in self.calls}
        for n in names:
            assert n in seen, (n, sorted(seen))
            assert self.unaligned(n), f"{n} received only 16-byte aligned pointers"


def grads_like(outs, seed, which=None):
    """Seeded incoming gradients for the outputs (None where ``which`` excludes one)."""
    g = torch.Generator().manual_seed(seed)
    res = []
    for i, o in enumerate(outs):
        if (which is not None and not which[i]) or not o.is_floating_point():
            res.append(None)
        else:
            res.append(torch.randn(o.shape, generator=g).to(o.device))
    return res


def run_pair(fn, inputs, needs_grad, gouts, log, entries, shifts=(1, 3, 2, 1, 2, 3)):
    """fn(*inputs) -> outputs, run on aligned copies and on shifted ones (input i at offset shifts[i], incoming gradient
    j at offset shifts[j + 1]); outputs and gradients w.r.t. the inputs flagged in ``needs_grad`` must be bit-identical and
    each entry point must have run its scalar form.  Returns (outputs, gradients) of the aligned run."""
    res = []
    for unaligned in (False, True):
        xs = []
        for i, t in enumerate(inputs):
            if t is None:
                xs.append(None)
                continue
            x = shifted(t, shifts[i % len(shifts)]) if unaligned else t.detach().clone()
            xs.append(x.requires_grad_(needs_grad[i]))
        outs = fn(*xs)
        pairs = [(o, g) for o, g in zip(outs, gouts(outs)) if g is not None]
        if unaligned:
            pairs = [(o, shifted(g, shifts[(j + 1) % len(shifts)])) for j, (o, g) in enumerate(pairs)]
        wrt = [x for x, m in zip(xs, needs_grad) if m]
        grads = torch.autograd.grad([o for o, _ in pairs], wrt, [g for _, g in pairs]) if wrt else ()
        res.append(([o.detach() for o in outs], [g for g in grads]))
    (oa, ga), (ou, gu) = res
    for k, (a, b) in enumerate(zip(oa, ou)):
        assert torch.equal(a, b), ("output", k, float((a.double() - b.double()).abs().max()))
    for k, (a, b) in enumerate(zip(ga, gu)):
        assert torch.equal(a, b), ("gradient", k, float((a.double() - b.double()).abs().max()))
    log.assert_scalar_form(*entries)
    return oa, ga


def check(name, got, want, tol):
    """|got - want| <= tol element by element (NaN fails)."""
    err = (got.double() - want.double()).abs()
    tol = tol + TINY
    ok = err <= tol
    assert bool(ok.all()), (name, int((~ok).sum()), float((err / tol).max()))


def case(dev, seed=0, sig_max=2.0):
    counts = ragged_counts(seed)
    rays = SR.Rays(counts.to(dev))
    g = torch.Generator().manual_seed(seed + 100)
    n = rays.n
    ts = torch.rand(n, generator=g) * 4.0
    te = ts + 0.001 + torch.rand(n, generator=g) * 0.02
    sig = torch.rand(n, generator=g) * sig_max
    ri = rays.ray_ids.clone()
    return rays, ri, ts.to(dev), te.to(dev), sig.to(dev), g


def d64(*ts):
    return [None if t is None else t.detach().double() for t in ts]


# ----------------------------------------------------------------------------- scans
@pytest.mark.parametrize("kind", ["inclusive_sum", "exclusive_sum", "inclusive_prod", "exclusive_prod"])
def test_scans_scalar_form(dev, monkeypatch, kind):
    rays, _, _, _, _, g = case(dev, 1)
    prod = kind.endswith("prod")
    x = (torch.rand(rays.n, generator=g) * 0.1 + 0.95 if prod else torch.randn(rays.n, generator=g)).to(dev)
    pi = rays.packed_info()
    log = CallLog(monkeypatch)
    fn = lambda a: (getattr(na, kind)(a, pi),)
    gin = grads_like([x], 5)
    (y,), (gx,) = run_pair(fn, [x], [True], lambda outs: gin, log,
                           ["nfa_packed_scan"] + (["nfa_packed_prod_backward"] if prod else []))
    x64 = x.double().requires_grad_(True)
    y64 = SR.scan(rays, x64, kind)
    (g64,) = torch.autograd.grad(y64, x64, gin[0].double())
    s_f, s_b = SR.scan_scales(rays, x.double(), y64.detach(), gin[0].double(), kind)
    check("y", y, y64, SR.bound(rays, s_f))
    check("grad", gx, g64, SR.bound(rays, 2.0 * s_b if prod else s_b))   # (products: the y_j and then their sum round)


# ----------------------------------------------------------------------------- transmittance / weights
# The *_saturated tests run the same bodies with densities up to SIG_SAT: sigma * delta reaches 420, so alpha == 1 and T == 0
# exactly over most of a ray (tests/test_render_edges_gpu.py places such samples one by one).
SIG_SAT = 2e4


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("grad_t", [False, True])
def test_render_weight_from_density_scalar_form(dev, monkeypatch, prefix, grad_t):
    _render_weight_from_density_scalar_form(dev, monkeypatch, prefix, grad_t, 2.0)


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("grad_t", [False, True])
def test_render_weight_from_density_scalar_form_saturated(dev, monkeypatch, prefix, grad_t):
    _render_weight_from_density_scalar_form(dev, monkeypatch, prefix, grad_t, SIG_SAT)


def _render_weight_from_density_scalar_form(dev, monkeypatch, prefix, grad_t, sig_max):
    rays, ri, ts, te, sig, g = case(dev, 2, sig_max=sig_max)
    pf = (0.2 + 0.8 * torch.rand(rays.n, generator=g)).to(dev) if prefix else None
    R = rays.R
    log = CallLog(monkeypatch)
    fn = lambda a, b, s, p: na.render_weight_from_density(a, b, s, ray_indices=ri, n_rays=R, prefix_trans=p)
    gin = grads_like([sig] * 3, 6)
    outs, grads = run_pair(fn, [ts, te, sig, pf], [grad_t, grad_t, True, False], lambda o: gin, log,
                           ["nfa_render_from_density_fwd", "nfa_render_from_density_bwd"])
    ts64, te64, sig64, pf64 = d64(ts, te, sig, pf)
    leaves = [t.requires_grad_(True) for t in ((ts64, te64, sig64) if grad_t else (sig64,))]
    ref = SR.from_density(rays, ts64, te64, sig64, pf64)
    rgrads = torch.autograd.grad(ref, leaves, [x.double() for x in gin])
    w, T, a = (r.detach() for r in ref)
    s_w, s_t, s_a, s_gx = SR.density_scales(rays, ts64.detach(), te64.detach(), sig64.detach(), T, a, *d64(*gin))
    for name, got, want, sc in zip(("weights", "trans", "alphas"), outs, (w, T, a), (s_w, s_t, s_a)):
        check(name, got, want, SR.bound(rays, sc))
    dt, sg = (te64 - ts64).detach().abs(), sig64.detach().abs()
    scales = ([s_gx * sg, s_gx * sg] if grad_t else []) + [s_gx * dt]
    for name, got, want, sc in zip(("g_t_starts", "g_t_ends", "g_sigmas")[-len(grads):], grads, rgrads, scales):
        check(name, got, want, SR.bound(rays, sc))


@pytest.mark.parametrize("prefix", [False, True])
def test_render_weight_from_alpha_scalar_form(dev, monkeypatch, prefix):
    rays, ri, _, _, _, g = case(dev, 3)
    al = (torch.rand(rays.n, generator=g) * 0.05).to(dev)
    al[::97] = 0.9   # (1 - alpha)^-1 of the gradient at its largest
    pf = (0.2 + 0.8 * torch.rand(rays.n, generator=g)).to(dev) if prefix else None
    log = CallLog(monkeypatch)
    fn = lambda a, p: na.render_weight_from_alpha(a, ray_indices=ri, n_rays=rays.R, prefix_trans=p)
    gin = grads_like([al] * 2, 7)
    (w, T), (ga,) = run_pair(fn, [al, pf], [True, False], lambda o: gin, log,
                             ["nfa_render_from_alpha_fwd", "nfa_render_from_alpha_bwd"])
    al64, pf64 = d64(al, pf)
    al64.requires_grad_(True)
    ref = SR.from_alpha(rays, al64, pf64)
    (rg,) = torch.autograd.grad(ref, al64, [x.double() for x in gin])
    s_w, s_t, s_g = SR.alpha_scales(rays, al64.detach(), ref[1].detach(), *d64(*gin))
    check("weights", w, ref[0], SR.bound(rays, s_w))
    check("trans", T, ref[1], SR.bound(rays, s_t))
    check("g_alphas", ga, rg, SR.bound(rays, s_g))


# ----------------------------------------------------------------------------- rendering
def _incoming(opac, depth, g_o, g_d):
    """The per-ray gradients rendering's depth normalisation (depth_raw / opacity.clamp_min(eps)) hands to the packed
    pass, formed from the product's own float32 opacity and depth: (G_opacity, G_depth_raw, |G_opacity| scale)."""
    eps = torch.finfo(torch.float32).eps
    o, d = opac.double(), depth.double()
    oc = o.clamp_min(eps)
    live = (o >= eps).double()
    G_d = g_d / oc
    G_o = g_o - live * g_d * d / oc
    return G_o, G_d, g_o.abs() + live * (g_d * d / oc).abs()


@pytest.mark.parametrize("mode", ["sigma_extras", "sigma_colors", "alpha_extras", "alpha_colors"])
def test_rendering_scalar_form(dev, monkeypatch, mode):
    _rendering_scalar_form(dev, monkeypatch, mode, 2.0)


@pytest.mark.parametrize("mode", ["sigma_extras", "sigma_colors"])   # (the alpha modes' reference is autograd over a cumprod: not
def test_rendering_scalar_form_saturated(dev, monkeypatch, mode):     #  the contract at alpha == 1, see test_render_edges_gpu.py)
    _rendering_scalar_form(dev, monkeypatch, mode, SIG_SAT)


def _rendering_scalar_form(dev, monkeypatch, mode, sig_max):
    rays, ri, ts, te, sig, g = case(dev, 4, sig_max=sig_max)
    R, dens, extras = rays.R, mode.startswith("sigma"), mode.endswith("extras")
    rgb = torch.rand(rays.n, 3, generator=g).to(dev)
    al = (torch.rand(rays.n, generator=g) * 0.05).to(dev)
    field = sig if dens else al
    log = CallLog(monkeypatch)

    def fn(a, b, f, c):
        cb = (lambda *_: (c, f))
        kw = {"rgb_sigma_fn": cb} if dens else {"rgb_alpha_fn": cb}
        colors, opac, depth, ex = na.rendering(a, b, ri, n_rays=R, **kw)
        return (colors, opac, depth) + ((ex["weights"], ex["trans"]) + ((ex["alphas"],) if dens else ()) if extras else ())

    n_out = 3 + (0 if not extras else (3 if dens else 2))
    gl = [torch.randn(R, 3, generator=g), torch.randn(R, 1, generator=g), torch.randn(R, 1, generator=g)]
    gl = [x.to(dev) for x in gl] + [torch.randn(rays.n, generator=g).to(dev) for _ in range(n_out - 3)]
    entries = (["nfa_render_fused_fwd", "nfa_render_fused_bwd"] if dens else
               ["nfa_render_from_alpha_fwd", "nfa_render_from_alpha_bwd", "nfa_render_accumulate_fwd", "nfa_render_accumulate_bwd"])
    outs, (g_f, g_rgb) = run_pair(fn, [ts, te, field, rgb], [False, False, True, True], lambda o: gl, log, entries)
    if dens:   # the fused pass, with (X) and without extras' gradients
        fused_bwd = [a for n, a in log.calls if n == "nfa_render_fused_bwd"]
        assert all((a[8] is not None) == extras for a in fused_bwd)   # g_weights

    # float64: the packed part under autograd, with the incoming per-ray gradients torch forms from the product's outputs
    colors, opac, depth = outs[:3]
    ts64, te64, f64, rgb64 = d64(ts, te, field, rgb)
    f64.requires_grad_(True)
    rgb64.requires_grad_(True)
    if dens:
        w, T, a = SR.from_density(rays, ts64, te64, f64)
        parts = [w, T, a]
    else:
        w, T = SR.from_alpha(rays, f64)
        a = f64
        parts = [w, T]
    c_r, o_r, d_r = SR.render_accumulate(rays, w, rgb64, ts64, te64)
    G_o, G_d, G_o_abs = _incoming(opac, depth, gl[1].double(), gl[2].double())
    ex_g = [x.double() for x in gl[3:]]
    r_f, r_rgb = torch.autograd.grad([c_r, o_r, d_r] + parts[:len(ex_g)], [f64, rgb64], [gl[0].double(), G_o, G_d] + ex_g)
    _, _, ref_depth = SR.finish_rendering(c_r.detach(), o_r.detach(), d_r.detach())

    w, T, a = w.detach(), T.detach(), a.detach()
    mid = ((ts64 + te64) / 2.0).abs()
    gw_ex, gt_ex, ga_ex = (ex_g + [None] * 3)[:3]
    gw_abs = ((gl[0].double().abs()[ri] * rgb64.detach().abs()).sum(-1) + G_o_abs[ri, 0] + G_d.abs()[ri, 0] * mid
              + (0.0 if gw_ex is None else gw_ex.abs()))
    if dens:
        s_w, s_t, s_a, s_gx = SR.density_scales(rays, ts64, te64, f64.detach(), T, a, gw_abs, gt_ex, ga_ex)
        s_f = s_gx * (te64 - ts64).abs()
    else:
        s_w, s_t, s_f = SR.alpha_scales(rays, a, T, gw_abs, gt_ex)
    sw1 = s_w + w
    s_col = SR.accumulate(rays, sw1, rgb64.detach().abs())
    s_op = SR.accumulate(rays, sw1)
    s_dr = SR.accumulate(rays, sw1, mid[:, None])
    s_dep = (s_dr + ref_depth.abs() * s_op) / o_r.detach().clamp_min(torch.finfo(torch.float32).eps)
    check("colors", colors, c_r, SR.bound(rays, s_col, per_ray=True))
    check("opacities", opac, o_r, SR.bound(rays, s_op, per_ray=True))
    check("depths", depth, ref_depth, SR.bound(rays, s_dep, per_ray=True, extra=4))
    if extras:
        check("weights", outs[3], w, SR.bound(rays, s_w))
        check("trans", outs[4], T, SR.bound(rays, s_t))
        if dens:
            check("alphas", outs[5], a, SR.bound(rays, s_a))
    check("g_field", g_f, r_f, SR.bound(rays, s_f))
    check("g_rgbs", g_rgb, r_rgb, SR.bound(rays, gl[0].double().abs()[ri] * sw1[:, None]))


# ----------------------------------------------------------------------------- visibility, compaction, test-mode step
@pytest.mark.parametrize("density", [True, False])
@pytest.mark.parametrize("counts", [False, True])
def test_visibility_scalar_form(dev, monkeypatch, density, counts):
    _visibility_scalar_form(dev, monkeypatch, density, counts, 20.0)


@pytest.mark.parametrize("counts", [False, True])
def test_visibility_scalar_form_saturated(dev, monkeypatch, counts):
    _visibility_scalar_form(dev, monkeypatch, True, counts, SIG_SAT)


def _visibility_scalar_form(dev, monkeypatch, density, counts, sig_max):
    rays, ri, ts, te, sig, g = case(dev, 5, sig_max=sig_max)
    al = (torch.rand(rays.n, generator=g) * 0.2).to(dev)
    pf = (0.5 + 0.5 * torch.rand(rays.n, generator=g)).to(dev)
    seg = seginfo_from_ray_indices(ri, rays.R)
    eps, thre = 1e-2, 0.05
    log = CallLog(monkeypatch)
    res = []
    for k in (0, 1):
        sh = (lambda t, j: shifted(t, j)) if k else (lambda t, j: t.clone())
        v = sh(sig if density else al, 2)
        out = volrend._visibility_native(seg, sh(ts, 1) if density else None, sh(te, 3) if density else None, v, sh(pf, 1),
                                         eps, thre, want_counts=counts)
        res.append(out if counts else (out, None))
    (vis, cnt), (vis_u, cnt_u) = res
    assert torch.equal(vis, vis_u) and (cnt is None or torch.equal(cnt, cnt_u))
    log.assert_scalar_form("nfa_render_visibility")
    ts64, te64, sig64, al64, pf64 = d64(ts, te, sig, al, pf)
    if density:
        _, T, a = SR.from_density(rays, ts64, te64, sig64, pf64)
        _, s_t, s_a, _ = SR.density_scales(rays, ts64, te64, sig64, T, a)
    else:
        _, T = SR.from_alpha(rays, al64, pf64)
        a = al64
        s_t, s_a = T, torch.zeros_like(T)
    want = (T >= eps) & (a >= thre)
    band = ((T - eps).abs() <= SR.bound(rays, s_t) + TINY) | ((a - thre).abs() <= SR.bound(rays, s_a) + TINY)
    assert int(band.sum()) < rays.n // 100 and bool(want.any()) and bool((~want).any())
    assert torch.equal(vis[~band], want[~band])
    if counts:
        assert torch.equal(cnt, torch.zeros_like(cnt).index_add_(0, ri, vis.long()))


def test_compact_samples_scalar_form(dev, monkeypatch):
    """test_compact_samples_consecutive_and_arbitrary_output_offsets with t_starts / t_ends at element offsets and the
    visibility mask at a 1-byte offset."""
    from nerfacc_amd._segments import seginfo_from_packed
    counts = ragged_counts(6)
    rays = SR.Rays(counts.to(dev))
    rng = np.random.default_rng(6)
    n, R = rays.n, rays.R
    vis = (rng.random(n) < 0.6).astype(np.uint8)
    ts = rng.random(n).astype(np.float32)
    te = ts + 1
    cnt = counts.numpy()
    ray = np.repeat(np.arange(R), cnt)
    kept = np.bincount(ray[vis != 0], minlength=R).astype(np.int64)
    m = int(kept.sum())
    seg = seginfo_from_packed(rays.packed_info(), n)
    rank = np.concatenate([np.arange(c) for c in kept])
    log = CallLog(monkeypatch)
    for starts in (np.concatenate([[0], np.cumsum(kept)[:-1]]), np.concatenate([[0], np.cumsum(kept[::-1])[:-1]])[::-1].copy()):
        want_pos = starts[ray[vis != 0]] + rank
        e_ri = np.full(m, -1, np.int64); e_ts = np.full(m, -1, np.float32); e_te = np.full(m, -1, np.float32)
        e_ri[want_pos] = ray[vis != 0]; e_ts[want_pos] = ts[vis != 0]; e_te[want_pos] = te[vis != 0]
        st = torch.from_numpy(starts).to(dev)
        res = []
        for unaligned in (False, True):
            v = torch.from_numpy(vis).to(dev)
            t0, t1 = torch.from_numpy(ts).to(dev), torch.from_numpy(te).to(dev)
            if unaligned:
                vb = torch.zeros(n + 1, dtype=torch.uint8, device=dev)
                vb[1:] = v
                v, t0, t1 = vb[1:], shifted(t0, 1), shifted(t1, 3)
                assert v.data_ptr() % 4 != 0
            o_ri = torch.full((m,), -1, dtype=torch.int64, device=dev)
            o_ts = torch.full((m,), -1.0, device=dev); o_te = torch.full((m,), -1.0, device=dev)
            B.call("nfa_compact_samples", B.ptr(v), B.ptr(t0), B.ptr(t1), B.ptr(seg.packed_info), B.ptr(seg.tiles),
                   seg.n_tiles, B.ptr(st), R, n, B.ptr(o_ri), B.ptr(o_ts), B.ptr(o_te), m, B.stream())
            res.append((o_ri.cpu().numpy(), o_ts.cpu().numpy(), o_te.cpu().numpy()))
        for got in res:
            assert np.array_equal(got[0], e_ri) and np.array_equal(got[1], e_ts) and np.array_equal(got[2], e_te)
    log.assert_scalar_form("nfa_compact_samples")


@pytest.mark.parametrize("alpha_thre", [0.0, 0.01])
def test_render_step_accumulate_scalar_form(dev, monkeypatch, alpha_thre):
    _render_step_accumulate_scalar_form(dev, monkeypatch, alpha_thre, 4.0)


@pytest.mark.parametrize("alpha_thre", [0.0, 0.01])
def test_render_step_accumulate_scalar_form_saturated(dev, monkeypatch, alpha_thre):
    _render_step_accumulate_scalar_form(dev, monkeypatch, alpha_thre, SIG_SAT)


def _render_step_accumulate_scalar_form(dev, monkeypatch, alpha_thre, sig_max):
    from nerfacc_amd import marching
    rays, ri, ts, te, sig, g = case(dev, 7, sig_max=sig_max)
    R = rays.R
    rgbs = torch.rand(rays.n, 3, generator=g).to(dev)
    c0 = torch.rand(R, 3, generator=g).to(dev)
    o0 = (torch.rand(R, 1, generator=g) * 0.5).to(dev)
    d0 = torch.rand(R, 1, generator=g).to(dev)
    seg = seginfo_from_ray_indices(ri, R)
    log = CallLog(monkeypatch)
    res = []
    for k in (0, 1):
        sh = (lambda t, j: shifted(t, j)) if k else (lambda t, j: t.clone())
        c, o, d = c0.clone(), o0.clone(), d0.clone()
        nv = torch.zeros(marching._VISIBLE_SLOTS, dtype=torch.int64, device=dev) if alpha_thre > 0 else None
        marching._render_step_native(seg, sh(ts, 1), sh(te, 3), sh(sig, 2), sh(rgbs, 1), alpha_thre, c, o, d, nv)
        res.append((c, o, d, None if nv is None else int(nv.sum())))
    for a, b in zip(res[0], res[1]):
        assert (a == b) if not torch.is_tensor(a) else torch.equal(a, b)
    log.assert_scalar_form("nfa_render_step_accumulate")
    c, o, d, nv = res[0]
    ts64, te64, sig64, rgb64, o64 = d64(ts, te, sig, rgbs, o0)
    dc, do, dd, keep = SR.render_step(rays, ts64, te64, sig64, rgb64, o64[:, 0], alpha_thre)
    _, T, a = SR.from_density(rays, ts64, te64, sig64, 1.0 - o64[ri, 0])
    s_w, _, s_a, _ = SR.density_scales(rays, ts64, te64, sig64, T, a)
    band = (a - alpha_thre).abs() <= SR.bound(rays, s_a) + TINY if alpha_thre > 0 else torch.zeros_like(keep)
    ok_ray = torch.zeros(R, dtype=torch.bool, device=dev).index_fill_(0, ri[band], True).logical_not()
    assert int((~ok_ray).sum()) < R // 50
    sw1 = torch.where(keep, s_w + T * a, torch.zeros_like(s_w))
    mid = ((ts64 + te64) / 2.0).abs()
    for name, got, base, inc, sc in (("colors", c, c0, dc, SR.accumulate(rays, sw1, rgb64.abs())),
                                     ("opacity", o, o0, do, SR.accumulate(rays, sw1)),
                                     ("depth", d, d0, dd, SR.accumulate(rays, sw1, mid[:, None]))):
        tol = SR.bound(rays, sc + base.double().abs(), per_ray=True, extra=1)
        check(name, got[ok_ray], (base.double() + inc)[ok_ray], tol[ok_ray])
    if alpha_thre > 0:
        n_band = int(band.sum())
        assert abs(nv - int(keep.sum())) <= n_band


# ----------------------------------------------------------------------------- distortion, CDF rows
def test_distortion_scalar_form(dev, monkeypatch):
    from nerfacc_amd.losses import distortion
    from test_distortion_gpu import check_against_f64, ragged_case
    w, ts, te, ri, R = ragged_case(ragged_counts(8).numpy(), seed=8, offset=3.0)
    got = check_against_f64(w, ts, te, ri, R, dev)     # aligned vs float64 (per-element scales)
    rid = ri.to(dev)
    g = torch.rand(R, generator=torch.Generator().manual_seed(7), dtype=torch.float32).to(dev) + 0.5   # check_against_f64's
    log = CallLog(monkeypatch)
    xs = [shifted(t.to(dev), k).requires_grad_(True) for t, k in ((w, 1), (ts, 3), (te, 2))]
    loss = distortion(*xs, ray_indices=rid, n_rays=R)
    grads = torch.autograd.grad(loss, xs, shifted(g, 1))
    for k, (a, b) in enumerate(zip(got, (loss.detach(),) + grads)):
        assert torch.equal(a, b), k
    log.assert_scalar_form("nfa_distortion_fwd", "nfa_distortion_bwd")


@pytest.mark.parametrize("R,S", [(513, 64), (3, 1), (70, 1025), (1, 4097), (257, 255)])
def test_density_cdf_rows_scalar_form(dev, monkeypatch, R, S):
    from nerfacc_amd.estimators import prop_net as PN
    g = torch.Generator().manual_seed(R * 7 + S)
    t = torch.sort(torch.rand(R, S + 1, generator=g) * 5.0 + 0.1, -1).values.to(dev)
    ts, te = t[:, :-1].contiguous(), t[:, 1:].contiguous()
    sg = (torch.rand(R, S, generator=g) * 6.0).to(dev)
    gin = [torch.randn(R, S + 1, generator=g).to(dev)]
    log = CallLog(monkeypatch)
    (cd,), (g_sig,) = run_pair(lambda a, b, c: (PN._cdfs_from_density(a, b, c),), [ts, te, sg], [False, False, True],
                               lambda o: gin, log, ["nfa_density_cdf_rows_fwd", "nfa_density_cdf_rows_bwd"])
    ts64, te64, sg64 = d64(ts, te, sg)
    sg64.requires_grad_(True)
    ref = SR.cdf_rows(ts64, te64, sg64)
    (r_g,) = torch.autograd.grad(ref, sg64, gin[0].double())
    rays = SR.Rays(torch.full((R,), S, dtype=torch.int64, device=dev))
    flat = lambda x: x.reshape(-1)
    T = 1.0 - ref.detach()[:, :S]
    _, s_t, _, s_gx = SR.density_scales(rays, flat(ts64), flat(te64), flat(sg64.detach()), flat(T), torch.zeros_like(flat(T)),
                                        gt=-flat(gin[0].double()[:, :S]))
    check("cdfs", cd[:, :S].reshape(-1), flat(ref.detach()[:, :S]), SR.bound(rays, s_t + flat(ref.detach()[:, :S])))   # (+ 1 - T rounds)
    assert bool((cd[:, S] == 1.0).all())
    check("g_sigmas", flat(g_sig), flat(r_g), SR.bound(rays, s_gx * flat(te64 - ts64).abs()))


# ----------------------------------------------------------------------------- end to end: views at an offset in normal use
def test_one_row_batch_of_interval_edges(dev, monkeypatch):
    """render_weight_from_density(t[:, :-1], t[:, 1:], sigmas) on a (1, S) batch: the views are contiguous, the second
    starts 4 bytes in, and the batched path hands them to the native op as they are."""
    S = 1029
    g = torch.Generator().manual_seed(3)
    t0 = torch.sort(torch.rand(1, S + 1, generator=g) * 3.0, -1).values.to(dev)
    s0 = (torch.rand(1, S, generator=g) * 5.0).to(dev)
    gin = [torch.randn(1, S, generator=g).to(dev) for _ in range(3)]
    log = CallLog(monkeypatch)
    res = []
    for clone in (False, True):
        t = t0.clone().requires_grad_(True)
        sig = s0.clone().requires_grad_(True)
        a, b = t[:, :-1], t[:, 1:]
        if clone:
            a, b = a.clone(), b.clone()
        else:
            assert b.is_contiguous() and b.data_ptr() % 16 != 0
        outs = na.render_weight_from_density(a, b, sig)
        grads = torch.autograd.grad(outs, [t, sig], gin)
        res.append([o.detach() for o in outs] + list(grads))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    log.assert_scalar_form("nfa_render_from_density_fwd", "nfa_render_from_density_bwd")


def test_propnet_sampling_one_ray_with_tensor_planes(dev, monkeypatch):
    """PropNetEstimator.sampling with Tensor near / far planes and one ray: _resample slices t_vals[..., 1:] of a (1, k)
    row -- a contiguous view 4 bytes in -- and hands it to the fused CDF pass.  Everything must equal row 0 of the same
    ray sampled twice in one batch (there the views are copied, so aligned)."""
    p = torch.nn.Parameter(torch.tensor(3.0, device=dev))
    fn = lambda ts, te: torch.exp(-((ts + te) * 0.5 - 4.0) ** 2) * p + 0.1
    res = []
    log = CallLog(monkeypatch)
    for n_rays in (1, 2):
        est = na.PropNetEstimator().to(dev)
        near = torch.full((n_rays, 1), 2.0, device=dev)
        far = torch.full((n_rays, 1), 6.5, device=dev)
        ts, te = est.sampling([fn, fn], [63, 33], 17, n_rays, near, far, sampling_type="lindisp", requires_grad=True)
        cdfs = [c.detach()[:1] for _, c in est.prop_cache if c is not None]
        vals = [iv.vals[:1] for iv, _ in est.prop_cache]
        assert len(cdfs) == 2 and len(vals) == 3
        res.append([ts[:1], te[:1]] + cdfs + vals)
        if n_rays == 1:
            log.assert_scalar_form("nfa_density_cdf_rows_fwd")
    for k, (a, b) in enumerate(zip(*res)):
        assert a.shape == b.shape and torch.equal(a, b), k


# ----------------------------------------------------------------------------- accumulate_along_rays: channel groups
def _acc_case(dev, D, seed):
    counts = ragged_counts(seed)
    rays = SR.Rays(counts.to(dev))
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(rays.n, generator=g).to(dev)
    v = torch.randn(rays.n, D, generator=g).to(dev) if D else None
    return rays, rays.ray_ids.clone(), w, v, g


@pytest.mark.parametrize("D,grad", [(D, grad) for D in (1, 2, 3, 4, 5, 8, 9, 13) for grad in ("weights", "values", "both")]
                         + [(0, "weights")])   # D = 0: no values (the weights are accumulated)
def test_accumulate_channel_groups(dev, monkeypatch, D, grad):
    rays, ri, w, v, g = _acc_case(dev, D, 10 + D)
    need = [grad in ("weights", "both"), grad in ("values", "both")]
    gout = [torch.randn(rays.R, max(D, 1), generator=g).to(dev)]
    log = CallLog(monkeypatch)
    (out,), grads = run_pair(lambda a, b: (na.accumulate_along_rays(a, b, ri, rays.R),), [w, v], need, lambda o: gout, log,
                             ["nfa_accumulate_along_rays", "nfa_accumulate_along_rays_bwd"])
    w64, v64 = d64(w, v)
    leaves = [x.requires_grad_(True) for x, m in zip((w64, v64), need) if m]
    ref = SR.accumulate(rays, w64, v64)
    rgrads = torch.autograd.grad(ref, leaves, gout[0].double())
    vv = torch.ones_like(w64)[:, None] if v64 is None else v64.detach().abs()
    check("out", out, ref, SR.bound(rays, SR.accumulate(rays, w64.detach(), vv), per_ray=True))
    go = gout[0].double().abs()[ri]
    tols = []
    if need[0]:   # g_w = sum over the D channels of g_out * v: D terms, added group by group
        tols.append((max(D, 1) + SR.K_ROUND) * SR.EPS32 * (go * vv).sum(-1))
    if need[1]:   # g_v = g_out * w: one product
        tols.append(SR.K_ROUND * SR.EPS32 * go * w64.detach()[:, None])
    names = [n for n, m in zip(("g_weights", "g_values"), need) if m]
    for name, got, want, tol in zip(names, grads, rgrads, tols):
        check(name, got, want, tol)


@pytest.mark.parametrize("D", [0, 1, 2, 5, 9])
def test_accumulate_in_place_sorted_and_unsorted(dev, monkeypatch, D):
    """accumulate_along_rays_: sorted indices add the segmented sums into a non-zero output (accumulate = 1); unsorted
    indices take the atomic kernel, whose order of additions varies -- the bound holds for any order."""
    rays, ri, w, v, g = _acc_case(dev, D, 30 + D)
    Dc = max(D, 1)
    out0 = torch.randn(rays.R, Dc, generator=g).to(dev)
    w64, v64 = d64(w, v)
    vv = torch.ones_like(w64)[:, None] if v64 is None else v64.abs()
    want = out0.double() + SR.accumulate(rays, w64, v64)
    tol = SR.bound(rays, out0.double().abs() + SR.accumulate(rays, w64, vv), per_ray=True, extra=1)
    log = CallLog(monkeypatch)
    res = []
    with torch.no_grad():
        for unaligned in (False, True):
            o = out0.clone()
            volrend.accumulate_along_rays_(shifted(w, 1) if unaligned else w, None if v is None else (shifted(v, 3) if unaligned else v),
                                      ri, o)
            res.append(o)
    assert torch.equal(res[0], res[1])
    check("sorted", res[0], want, tol)
    log.assert_scalar_form("nfa_accumulate_along_rays")
    assert all(a[-3] == 1 for n, a in log.calls if n == "nfa_accumulate_along_rays")   # accumulate into the output
    perm = torch.randperm(rays.n, generator=torch.Generator().manual_seed(D)).to(dev)
    o = out0.clone()
    with torch.no_grad():
        volrend.accumulate_along_rays_(w[perm], None if v is None else v[perm], ri[perm], o)
    assert "nfa_accumulate_along_rays_atomic" in [n for n, _ in log.calls]
    check("atomic", o, want, tol)

"""GPU: the constant-step (`_cs`) passes -- t_ends formed from t_starts instead of loaded -- against the passes that load it.

Every case runs the same step (``sampling`` -> ``rendering`` -> backward) with ``volrend.DERIVE_T_ENDS`` on and off and
compares everything with ``torch.equal``: the sampler's outputs, the six outputs of the fused pass, the gradients arriving
at the field's outputs and the parameter gradient.  A log of the native calls says which entry points ran."""
import contextlib
import math

import numpy as np
import pytest
import torch

import nerfacc_amd as na
from nerfacc_amd import _backend as B
from nerfacc_amd import grid as G
from nerfacc_amd import volrend
from nerfacc_amd._segments import const_step_of, seginfo_from_packed

pytestmark = pytest.mark.gpu

CS = ["nfa_render_visibility_cs", "nfa_render_fused_fwd_cs", "nfa_render_fused_bwd_cs"]
SIBLINGS = ["nfa_render_visibility", "nfa_render_fused_fwd", "nfa_render_fused_bwd"]
BENCH_STEP = 2 * math.sqrt(3) / 1024


@contextlib.contextmanager
def call_log():
    """Names of the native calls made inside (a traversal's fill pass as ``nfa_traverse_grids[mode=1]``)."""
    names, real = [], B.call

    def logged(name, *a):
        names.append("%s[mode=%d]" % (name, a[0]._obj.mode) if name == "nfa_traverse_grids" else name)
        return real(name, *a)

    B.call = logged
    try:
        yield names
    finally:
        B.call = real


def engine_calls(names):
    return [n for n in names if n in CS or n in SIBLINGS]


def shell_grid(res, seed=42):
    """bench.py's grid: a shell of radius 0.50 .. 0.66 plus 2 % speckle."""
    rng = np.random.default_rng(seed)
    c = (np.arange(res) + 0.5) / res * 2 - 1
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    return (((r >= 0.50) & (r <= 0.66)) | (rng.random((res, res, res)) < 0.02))[None]


def random_rays(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((n, 3)).astype(np.float32) * np.float32(scale)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o, d


def estimator(dev, b):
    est = na.OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=b.shape[1], levels=1).to(dev)
    est.binaries = torch.from_numpy(b).to(dev)
    est.occs = est.binaries.reshape(-1).float()
    return est


def base_sigma(ts, te):
    return 4.0 * (0.5 + 0.5 * torch.sin(20.0 * (ts + te)))


def render(ts, te, ri, n_rays, p, extras, seed=11):
    """rendering + backward of a seeded linear loss; returns what is compared and the parameter with its gradient."""
    kept = {}

    def rgb_sigma_fn(a, b, _):
        kept["sigmas"] = base_sigma(a, b) * p[0]
        kept["rgbs"] = (a * p[1])[:, None].expand(-1, 3).contiguous()
        kept["sigmas"].retain_grad()
        kept["rgbs"].retain_grad()
        return kept["rgbs"], kept["sigmas"]

    colors, opac, depth, ex = na.rendering(ts, te, ri, n_rays=n_rays, rgb_sigma_fn=rgb_sigma_fn)
    g = torch.Generator().manual_seed(seed)
    w = lambda t: torch.randn(t.shape, generator=g).to(t.device)
    loss = (colors * w(colors)).sum() + (opac * w(opac)).sum() + (depth * w(depth)).sum()
    if extras:   # gradients arriving at the per-sample outputs too: the backward's other compile-time form
        loss = loss + (ex["weights"] * w(ex["weights"])).sum() + (ex["trans"] * w(ex["trans"])).sum() \
            + (ex["alphas"] * w(ex["alphas"])).sum()
    out = dict(colors=colors, opacities=opac, depths=depth, weights=ex["weights"], trans=ex["trans"], alphas=ex["alphas"])
    if ts.numel():   # (without samples the field is not called and nothing depends on the parameters)
        p.grad = None
        loss.backward()
        out.update(g_sigma=kept["sigmas"].grad, g_rgb=kept["rgbs"].grad, param_grad=p.grad.clone())
    return {k: v.detach() for k, v in out.items()}


def step_once(est, o, d, p0, derive, extras=False, touch=None, sample=None, **kw):
    """One step with DERIVE_T_ENDS = derive.  touch(ts, te) -> (ts, te) stands between sampling and rendering."""
    p = torch.nn.Parameter(torch.tensor([float(p0), 1.0], device=o.device))
    saved = volrend.DERIVE_T_ENDS
    volrend.DERIVE_T_ENDS = derive
    try:
        with call_log() as names:
            sigma_fn = lambda a, b, _: base_sigma(a, b) * float(p0)
            ri, ts, te = sample() if sample is not None else est.sampling(o, d, sigma_fn=sigma_fn, **kw)
            tagged = const_step_of(ts, te) is not None
            if touch is not None:
                ts, te = touch(ts, te)
            res = render(ts, te, ri, o.shape[0], p, extras)
    finally:
        volrend.DERIVE_T_ENDS = saved
    res.update(ray_indices=ri, t_starts=ts, t_ends=te)
    return res, names, tagged


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, a[k].shape, b[k].shape)


def on_off(est, o, d, p0, expect_off=SIBLINGS, **kw):
    on, names_on, tagged = step_once(est, o, d, p0, True, **kw)
    off, names_off, _ = step_once(est, o, d, p0, False, **kw)
    assert_same(on, off)
    assert engine_calls(names_off) == expect_off, names_off
    return on, names_on, tagged


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------------- 1, 2: the step of the benchmark, small
def test_base_case(dev):
    o, d = random_rays(4099, 39)
    est = estimator(dev, shell_grid(32))
    res, names, tagged = on_off(est, T(o, dev), T(d, dev), 1.0, render_step_size=BENCH_STEP)
    assert tagged and res["t_starts"].numel() > 20000
    assert engine_calls(names) == CS, names   # once each, none of the siblings


def test_compaction_keeps_the_tag(dev):
    o, d = random_rays(4099, 39)
    est = estimator(dev, shell_grid(32))
    ro, rd = T(o, dev), T(d, dev)
    total = est.sampling(ro, rd, render_step_size=BENCH_STEP)[0].numel()
    res, names, tagged = on_off(est, ro, rd, 16.0, extras=True, render_step_size=BENCH_STEP)
    assert 0 < res["t_starts"].numel() < total     # early termination dropped samples
    assert tagged and engine_calls(names) == CS, names


# ----------------------------------------------------------------------------- 3: binades, long rays, runs of empty rays
def test_binade_crossings_and_tile_boundaries(dev):
    # 32^3, near 0.9, step 1e-3: t crosses 1, 2 and 4.  A row of occupied cells along x with rays inside it gives rays of
    # ~2000 samples (a ray spans several tiles); 300 consecutive rays that miss the box give a tile boundary by rows.
    b = shell_grid(32)
    b[0, :, 16, 16] = True
    o, d = random_rays(3000, 39, scale=2.0)
    o[1200:1500] = [3.0, 3.0, 3.0]
    d[1200:1500] = np.float32(1 / math.sqrt(3))                      # away from the box
    o[2000:2008] = [-1.95, 0.03, 0.03]
    d[2000:2008] = [1.0, 0.0, 0.0]
    est = estimator(dev, b)
    res, names, tagged = on_off(est, T(o, dev), T(d, dev), 1.0, near_plane=0.9, render_step_size=1e-3)
    assert tagged and engine_calls(names) == CS, names
    per_ray = torch.bincount(res["ray_indices"], minlength=3000)
    assert int(per_ray.max()) > 1024 and int(per_ray[1200:1500].sum()) == 0
    ts = res["t_starts"]
    assert float(ts.min()) < 1.0 and float(ts.max()) > 4.0 and bool(((ts > 1.9) & (ts < 2.1)).any())

    o, d = random_rays(2000, 23)
    est = estimator(dev, shell_grid(16))
    res, names, tagged = on_off(est, T(o, dev), T(d, dev), 1.0, near_plane=0.2, render_step_size=0.0137)
    assert tagged and engine_calls(names) == CS and res["t_starts"].numel() > 1000, names


# ----------------------------------------------------------------------------- 4: rays filled by the serial kernel
def test_overflow_fill_branch(dev):
    # 32^3, iid 50 % cells, a quarter cell per step, rays from corner to corner.  Random cells give a ray about one run per
    # four cells crossed -- at most ~30 over the 94 cells of a diagonal -- so the cells within two cells of the main diagonal are
    # a 3-D checkerboard: the rays through them change cell state at every crossing (more than 40 runs on the CPU oracle).
    res, n = 32, 4099
    rng = np.random.default_rng(5)
    b = rng.random((1, res, res, res)) < 0.5
    i, j, k = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij")
    tube = (np.abs(i - j) <= 2) & (np.abs(j - k) <= 2) & (np.abs(i - k) <= 2)
    b[0][tube] = ((i + j + k) % 2 == 0)[tube]
    sgn = rng.choice([-1.0, 1.0], (n, 3))
    o = (sgn * (1.02 + 0.2 * rng.random((n, 3)))).astype(np.float32)
    tgt = (-sgn * (0.8 + 0.2 * rng.random((n, 3)))).astype(np.float32)
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    step = 0.0625 / 4 * 1.003
    est = estimator(dev, b)
    assert G.MAX_RUNS == 32
    out, names, tagged = on_off(est, T(o, dev), T(d, dev), 0.25, render_step_size=step)
    # the fill pass is launched only when the walk counted rays with more records than slots
    assert "nfa_traverse_grids[mode=1]" in names, names
    assert tagged and engine_calls(names) == CS, names
    # the identity on the device, for the sampler's whole output (no density callback: nothing dropped)
    ri, ts, te = est.sampling(T(o, dev), T(d, dev), render_step_size=step)
    assert ts.numel() > 100000 and const_step_of(ts, te) == np.float32(step)
    assert torch.equal(te, ts + torch.tensor(step, dtype=torch.float32, device=dev))


# ----------------------------------------------------------------------------- 5: jittered near planes, prefetched traversal
def test_stratified_with_planes_and_a_prefetched_traversal(dev):
    o, d = random_rays(4099, 39)
    est = estimator(dev, shell_grid(32))
    ro, rd = T(o, dev), T(d, dev)
    kw = dict(render_step_size=BENCH_STEP, stratified=True, t_min=torch.full((4099,), 0.3, device=dev),
              t_max=torch.full((4099,), 3.0, device=dev))

    def direct():
        torch.manual_seed(1234)
        return est.sampling(ro, rd, sigma_fn=lambda a, b, _: base_sigma(a, b), **kw)

    def prefetched():
        torch.manual_seed(1234)
        h = est.prefetch_traversal(ro, rd, **kw)
        return est.sampling(ro, rd, sigma_fn=lambda a, b, _: base_sigma(a, b), traversal=h, **kw)

    results = []
    for sample in (direct, prefetched):
        res, names, tagged = on_off(est, ro, rd, 1.0, sample=sample)
        assert tagged and engine_calls(names) == CS, names
        results.append(res)
    assert_same(*results)
    assert results[0]["t_starts"].numel() > 10000 and float(results[0]["t_starts"].min()) >= 0.3


# ----------------------------------------------------------------------------- 6: anything else loads t_ends
def test_invalidation(dev):
    o, d = random_rays(4099, 39)
    est = estimator(dev, shell_grid(32))
    ro, rd = T(o, dev), T(d, dev)
    want, _, _ = step_once(est, ro, rd, 1.0, False, render_step_size=BENCH_STEP)
    fwd_bwd = SIBLINGS[1:]
    for what, touch in (("in-place edit", lambda ts, te: (ts, te.add_(0))),
                        ("clone", lambda ts, te: (ts, te.clone())),
                        ("foreign t_starts", lambda ts, te: (ts.clone(), te))):
        got, names, tagged = step_once(est, ro, rd, 1.0, True, touch=touch, render_step_size=BENCH_STEP)
        assert tagged, what                              # the sampler's output was tagged, and ...
        assert const_step_of(got["t_starts"], got["t_ends"]) is None, what
        assert engine_calls(names) == [CS[0]] + fwd_bwd, (what, names)   # ... what reached rendering was not its output
        assert_same(got, want)

    # an in-place write inside the density callback: the sampler's own pass loads t_ends too
    saved = volrend.DERIVE_T_ENDS
    volrend.DERIVE_T_ENDS = True
    try:
        with call_log() as names:
            ri, ts, te = est.sampling(ro, rd, sigma_fn=lambda a, b, _: base_sigma(a, b.add_(0)), render_step_size=BENCH_STEP)
    finally:
        volrend.DERIVE_T_ENDS = saved
    assert engine_calls(names) == SIBLINGS[:1], names
    assert torch.equal(ri, want["ray_indices"]) and torch.equal(ts, want["t_starts"]) and torch.equal(te, want["t_ends"])

    # distance-dependent steps are never tagged
    got, names, tagged = on_off(est, ro, rd, 1.0, render_step_size=BENCH_STEP, cone_angle=0.004)
    assert not tagged and engine_calls(names) == SIBLINGS and got["t_starts"].numel() > 1000, names

    # nor are the API's traversal outputs
    def from_traverse_grids():
        iv, sm, _ = na.traverse_grids(ro, rd, est.binaries, est.aabbs, step_size=BENCH_STEP)
        return sm.ray_indices, iv.vals[iv.is_left], iv.vals[iv.is_right]

    got, names, tagged = on_off(est, ro, rd, 1.0, expect_off=fwd_bwd, sample=from_traverse_grids)
    assert not tagged and engine_calls(names) == fwd_bwd, names
    full = est.sampling(ro, rd, render_step_size=BENCH_STEP)
    assert torch.equal(got["t_starts"], full[1]) and torch.equal(got["t_ends"], full[2])


# ----------------------------------------------------------------------------- 7: the element-wise instances
def _shifted(t):
    """A copy of t one element off its allocation's start: not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("extra", [False, True])
def test_elementwise_instances(dev, extra):
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 90, 70)
    counts[[0, 7, 8, 9, 40, 69]] = 0
    counts[20], counts[21] = 300, 1      # a ray longer than a wave step, a single sample
    n, R = int(counts.sum()), len(counts)
    assert 2500 < n < 3500 and n % 4 != 0
    starts = np.cumsum(counts) - counts
    pi = T(np.stack([starts, counts], -1).astype(np.int64), dev)
    seg = seginfo_from_packed(pi, n, trusted=True)
    g = torch.Generator().manual_seed(5)
    step = 0.0137
    ts = _shifted((torch.rand(n, generator=g) * 5.0).to(dev))
    te = _shifted(ts + torch.tensor(step, dtype=torch.float32, device=dev))    # one fp32 add
    sig = _shifted((torch.rand(n, generator=g) * 40.0).to(dev))
    rgb = _shifted(torch.rand(n, 3, generator=g).to(dev))
    new = lambda *shape, dtype=torch.float32: _shifted(torch.zeros(*shape, dtype=dtype, device=dev))
    tail = (B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, R, n)

    def visibility(name, second):
        vis, cnt = new(n, dtype=torch.bool), torch.zeros(R, dtype=torch.int64, device=dev)
        B.call(name, B.ptr(ts), second, B.ptr(sig), None, 1e-2, 0.05, *tail, B.ptr(vis), B.ptr(cnt), B.stream())
        return vis, cnt

    def forward(name, second):
        out = [new(n), new(n), new(n), new(R, 3), new(R), new(R)]
        B.call(name, B.ptr(ts), second, B.ptr(sig), B.ptr(rgb), *tail, *(B.ptr(t) for t in out), B.stream())
        return out

    a, b = visibility("nfa_render_visibility_cs", step), visibility("nfa_render_visibility", B.ptr(te))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and 0 < int(a[1].sum()) < n
    fa, fb = forward("nfa_render_fused_fwd_cs", step), forward("nfa_render_fused_fwd", B.ptr(te))
    for x, y in zip(fa, fb):
        assert torch.equal(x, y)
    assert float(fa[4].max()) > 0.5
    trans, alphas = fa[1], fa[2]
    grads = [_shifted(torch.randn(s, generator=g).to(dev)) for s in ((R, 3), (R,), (R,))]
    grads += [_shifted(torch.randn(n, generator=g).to(dev)) if extra else None for _ in range(3)]

    def backward(name, second):
        out = [new(n), new(n, 3)]
        B.call(name, B.ptr(ts), second, B.ptr(rgb), B.ptr(trans), B.ptr(alphas), *(B.ptr(t) for t in grads), *tail,
               *(B.ptr(t) for t in out), B.stream())
        return out

    ba, bb = backward("nfa_render_fused_bwd_cs", step), backward("nfa_render_fused_bwd", B.ptr(te))
    assert torch.equal(ba[0], bb[0]) and torch.equal(ba[1], bb[1]) and bool(ba[0].any()) and bool(ba[1].any())


# ----------------------------------------------------------------------------- 8: nothing to do
def test_empty_inputs(dev):
    # rays that all miss the box: zero samples
    o = np.full((37, 3), 3.0, np.float32)
    d = np.full((37, 3), 1 / math.sqrt(3), np.float32)
    est = estimator(dev, shell_grid(16))
    res, names, tagged = on_off(est, T(o, dev), T(d, dev), 1.0, expect_off=SIBLINGS[:2], render_step_size=BENCH_STEP)
    assert res["t_starts"].numel() == 0 and tagged and engine_calls(names) == CS[:2], names
    assert not bool(res["colors"].any()) and not bool(res["opacities"].any())

    # no rays and no samples: accepted before anything else is looked at
    none = lambda k: [None] * k
    B.call("nfa_render_visibility_cs", None, 0.01, None, None, 1e-4, 0.0, None, None, 0, 0, 0, *none(3))
    B.call("nfa_render_fused_fwd_cs", None, 0.01, *none(4), 0, 0, 0, *none(7))
    B.call("nfa_render_fused_bwd_cs", None, 0.01, *none(11), 0, 0, 0, *none(3))
    # rays without samples: the visibility entry's counts are cleared
    pi = torch.zeros(4, 2, dtype=torch.int64, device=dev)
    seg = seginfo_from_packed(pi, 0, trusted=True)
    cnt = torch.full((4,), 7, dtype=torch.int64, device=dev)
    B.call("nfa_render_visibility_cs", None, 0.01, None, None, 1e-4, 0.0, B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles,
           4, 0, None, B.ptr(cnt), B.stream())
    assert cnt.tolist() == [0, 0, 0, 0]

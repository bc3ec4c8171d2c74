"""GPU: the half-precision field path -- fp16 / bf16 outputs and incoming gradients of the encodings
(nfa_hashgrid_{fwd,bwd}_t, nfa_sh_{fwd,bwd}_t) and fp16 / bf16 raw inputs of ``rendering_from_raw``
(nfa_render_raw_{fwd,bwd}_t).

The arithmetic of the half entries is the float32 one; only loads widen (exact) and stores round once to nearest even.  So
everything here is compared bit for bit with the project's own float32 path (which the existing suite pins to float64
references and the oracle): a half output must equal ``float32_output.to(dtype)``, a float32 output of a half call must
equal the float32 call on the widened inputs.  The one exception is the hash grid's parameter gradient, whose atomics have
no fixed order: it is held to the float64 bound of tests/test_encodings_gpu.py, restated below.
"""
import numpy as np
import pytest
import torch

import seg_reference as SR
from nerfacc_amd import _backend as B
from nerfacc_amd._segments import seginfo_from_ray_indices
from nerfacc_amd.encodings import HashGridEncoding, SphericalHarmonicsEncoding, encoding_from_tcnn_config
from nerfacc_amd.rawrender import rendering_from_raw

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
ELEM = {torch.float16: 1, torch.bfloat16: 2}   # include/nerfacc_hip.h: NFA_ELEM_F16 / NFA_ELEM_BF16
M32 = 0xFFFFFFFF

# (n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale): tests/test_encodings_gpu.py's
CONFIGS = {
    "density": (5, 2, 17, 16, np.exp((np.log(128) - np.log(16)) / 4).tolist()),
    "F1_L3": (3, 1, 14, 16, 2.0),          # 2-byte pieces
    "F4_L3": (3, 4, 14, 16, 2.0),          # 8-byte pieces, one idle lane
    "F8_L7_edge": (7, 8, 12, 16, 1.0),     # 16-byte pieces; every level exactly on the dense / hashed boundary
    "F2_L24": (24, 2, 16, 16, 1.2),        # 16 idle lanes per wave
}


class CallLog:
    def __init__(self, monkeypatch):
        self.calls = []
        real = B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def names(self):
        return [n for n, _ in self.calls]


def grid_pair(kind, d, dev, table_scale=1.0):
    """A float32 grid and one with out_dtype d that shares its parameters, both on dev."""
    torch.manual_seed(0)
    L, F, log2, base, scale = CONFIGS[kind]
    ref = HashGridEncoding(3, L, F, log2, base, scale)
    with torch.no_grad():
        ref.params.uniform_(-1, 1)
        ref.params.mul_(table_scale)
    ref = ref.to(dev)
    enc = HashGridEncoding(3, L, F, log2, base, scale, out_dtype=d)
    enc.params = ref.params
    return ref, enc


def points(n, seed, enc):
    """n points in [-0.25, 1.25]^3 with rows on cell boundaries of every level (x * scale_l + 0.5 an integer in float32) and
    the 0.0 / 1.0 corners (tests/test_encodings_gpu.py: with_cell_boundaries)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 1.5 - 0.25
    rows = []
    for s in enc.scales:
        k = torch.arange(0, int(s) + 2, dtype=torch.float32)
        c = (k - 0.5) / s
        c = c[(c * s + 0.5) == torch.floor(c * s + 0.5)]
        if c.numel():
            rows.append(c[torch.randint(0, c.numel(), (max(n // (4 * len(enc.scales)), 1), 3), generator=g)])
    rows.append(torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 0.5], [0.0, 0.0, 0.0]]))
    b = torch.cat(rows)[: max(n - 1, 1)]
    if n > 1:
        x[1: 1 + b.shape[0]] = b[: n - 1]
    else:
        x[0] = torch.tensor([1.0, 1.0, 1.0])
    return x


# ---------------------------------------------------------------- 1. hash grid forward
@pytest.mark.parametrize("n", [1, 63, 65, 4097])
@pytest.mark.parametrize("kind", list(CONFIGS))
@pytest.mark.parametrize("d", HALF)
def test_hashgrid_forward_bit_for_bit(dev, monkeypatch, d, kind, n):
    ref, enc = grid_pair(kind, d, dev)
    x = points(n, n, ref).to(dev)
    want = ref(x).to(d)
    log = CallLog(monkeypatch)
    got = enc(x)
    assert log.names() == ["nfa_hashgrid_fwd_t"] and log.calls[0][1][0] == ELEM[d]   # no cast kernel: d straight from the op
    assert got.dtype == d and got.shape == (n, ref.n_output_dims)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_hashgrid_forward_fp16_subnormal_results(dev):
    """The table scaled by 2^-16: every result lies below fp16's smallest normal (2^-14); a flushing convert gives zeros."""
    ref, enc = grid_pair("density", torch.float16, dev, table_scale=2.0 ** -16)
    x = points(4097, 3, ref).to(dev)
    got, want = enc(x), ref(x).to(torch.float16)
    assert float(want.float().abs().max()) < 2.0 ** -14 and int((want != 0).sum()) > want.numel() // 2
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------- 2. hash grid backward
def restate_grads(x, params, enc, g):
    """float64 scatter of w_c * g (weights from the float32 cell coordinates, as the kernels form them); per entry also
    the contribution count and the sum of |contribution| (tests/test_encodings_gpu.py: restate_grads)."""
    F = enc.n_features_per_level
    gp = torch.zeros(params.numel() // F, F, dtype=torch.float64)
    cnt = torch.zeros(params.numel() // F, dtype=torch.float64)
    absum = torch.zeros(params.numel() // F, F, dtype=torch.float64)
    for l in range(enc.n_levels):
        s = enc.scales[l]
        p = x * s + 0.5
        fl = torch.floor(p)
        f = (p - fl).double()
        gi = fl.clamp(-2147483648.0, 2147483520.0).to(torch.int64) & M32
        size, res, off = enc.sizes[l], enc.resolutions[l], enc.offsets[l]
        gl = g[:, l * F:(l + 1) * F].double()
        for c in range(8):
            b = [(c >> k) & 1 for k in range(3)]
            q = [(gi[:, k] + b[k]) & M32 for k in range(3)]
            if enc.table.hashed[l]:
                idx = (q[0] ^ ((q[1] * 2654435761) & M32) ^ ((q[2] * 805459861) & M32)) & (size - 1)
            else:
                idx = ((q[0] + q[1] * res + q[2] * res * res) & M32) % size
            wf = [f[:, k] if b[k] else 1.0 - f[:, k] for k in range(3)]
            contrib = (wf[0] * wf[1] * wf[2])[:, None] * gl
            gp.index_add_(0, off + idx, contrib)
            absum.index_add_(0, off + idx, contrib.abs())
            cnt.index_add_(0, off + idx, torch.ones_like(wf[0]))
    return gp.view(-1), cnt, absum.view(-1)


@pytest.mark.parametrize("kind", list(CONFIGS))
@pytest.mark.parametrize("d", HALF)
def test_hashgrid_backward(dev, monkeypatch, d, kind):
    ref, enc = grid_pair(kind, d, dev)
    n = 4097
    x = points(n, 11, ref)
    g = torch.randn(n, ref.n_output_dims, generator=torch.Generator().manual_seed(12)).to(d).to(dev)
    assert g.data_ptr() % 16 == 0

    x32 = x.to(dev).requires_grad_(True)
    ref(x32).backward(g.float())                       # the float32 op fed the exactly widened gradient
    gx32 = x32.grad.clone()
    ref.params.grad = None

    xh = x.to(dev).requires_grad_(True)
    y = enc(xh)
    log = CallLog(monkeypatch)
    y.backward(g)
    assert log.names() == ["nfa_hashgrid_bwd_t"]
    a = log.calls[0][1]
    assert a[0] == ELEM[d] and a[3] == g.data_ptr()    # the half gradient itself: no widened copy of [N, L F]
    assert torch.equal(xh.grad, gx32)                  # dL/dx: bit for bit
    gp = enc.params.grad
    assert gp.dtype == torch.float32

    # dL/dparams: float64 on the exactly widened gradient, the bound of the float32 path's test (one rounding per add of
    # the cnt contributions, and the product's two)
    ref_p, cnt, absum = restate_grads(x, ref.params.detach().cpu(), ref, g.float().cpu())
    bound = (cnt.repeat_interleave(ref.n_features_per_level) + 2) * 2.0 ** -23 * absum
    err = (gp.cpu().double() - ref_p).abs()
    print(f"{kind} {d}: worst err - bound {float((err - bound).max()):.3e}, entries hit {int((cnt > 0).sum())}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert int((cnt > 0).sum()) > 100


# ---------------------------------------------------------------- 3. spherical harmonics
@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("d", HALF)
def test_sh_bit_for_bit(dev, monkeypatch, d, degree, n):
    ref, sh = SphericalHarmonicsEncoding(3, degree), SphericalHarmonicsEncoding(3, degree, out_dtype=d)
    dirs = torch.rand(n, 3, generator=torch.Generator().manual_seed(degree)).to(dev)
    g = torch.randn(n, degree * degree, generator=torch.Generator().manual_seed(7)).to(d).to(dev)

    d32 = dirs.clone().requires_grad_(True)
    out32 = ref(d32)
    out32.backward(g.float())

    dh = dirs.clone().requires_grad_(True)
    log = CallLog(monkeypatch)
    out = sh(dh)
    out.backward(g)
    assert log.names() == ["nfa_sh_fwd_t", "nfa_sh_bwd_t"]
    assert log.calls[0][1][0] == ELEM[d] and log.calls[1][1][2] == g.data_ptr()
    assert out.dtype == d
    assert torch.equal(out.detach().view(torch.int16), out32.detach().to(d).view(torch.int16))
    assert torch.equal(dh.grad, d32.grad)


# ---------------------------------------------------------------- 4.-6. rendering_from_raw
BIAS = -1.0
_CASE = {}


def case(dev):
    """tests/test_rawrender_gpu.py's ray lengths and inputs: empty rays, one sample, a wave step's edge (255, 256, 257), a
    ray across the 1024-element tiles, 300 rays of 1-3 samples (more than the backward's 192 staged rays in one tile), a
    trailing empty ray; densities near trunc_exp's clamp; about 20 % masked.  Built once; the tests do not modify it."""
    if "c" in _CASE:
        return _CASE["c"]
    rng = np.random.default_rng(7)
    counts = np.concatenate([[0, 1, 3, 0, 255, 256, 257, 2500], rng.integers(1, 4, 300), [0]]).astype(np.int64)
    rays = SR.Rays(torch.from_numpy(counts).to(dev))
    g = torch.Generator().manual_seed(11)
    n = rays.n
    ts = torch.rand(n, generator=g) * 4.0
    te = ts + 0.001 + torch.rand(n, generator=g) * 0.02
    raw_sig = torch.rand(n, generator=g) * 12.0 - 6.0
    starts = np.cumsum(counts) - counts
    hot = torch.from_numpy(np.concatenate([starts[7] + [2440, 2470, 2499], starts[8::37]]))
    raw_sig[hot] = 16.0 + 4.0 * torch.rand(hot.numel(), generator=g) - BIAS
    raw_rgb = torch.rand(n, 3, generator=g) * 16.0 - 8.0
    sel = torch.rand(n, generator=g) > 0.2
    sel[hot[::2]] = True
    gl = {"colors": torch.randn(rays.R, 3, generator=g), "opacities": torch.randn(rays.R, 1, generator=g),
          "depths": torch.randn(rays.R, 1, generator=g), "weights": torch.randn(n, generator=g),
          "trans": torch.randn(n, generator=g), "alphas": torch.randn(n, generator=g)}
    c = dict(rays=rays, ri=rays.ray_ids.clone(), ts=ts.to(dev), te=te.to(dev), raw_sig=raw_sig.to(dev), raw_rgb=raw_rgb.to(dev),
             sel=sel.to(dev), gl={k: v.to(dev) for k, v in gl.items()})
    seginfo_from_ray_indices(c["ri"], rays.R)
    _CASE["c"] = c
    return c


def run(c, raw_sig, raw_rgb, dens, col, extras, tensors=None):
    """One forward (with the activated values) and backward; returns (outputs by name, (g_raw_sigmas, g_raw_rgbs))."""
    t = tensors or {k: c[k] for k in ("ts", "te", "sel", "gl")}
    rs, rc = raw_sig.detach().requires_grad_(True), raw_rgb.detach().requires_grad_(True)
    colors, opac, depth, ex = rendering_from_raw(t["ts"], t["te"], rc, rs, c["ri"], c["rays"].R, density_activation=dens,
                                                 density_bias=BIAS, rgb_activation=col, selector=t["sel"], return_activated=True)
    outs = {"colors": colors, "opacities": opac, "depths": depth, **ex}
    keys = ["colors", "opacities", "depths"] + (["weights", "trans", "alphas"] if extras else [])
    grads = torch.autograd.grad([outs[k] for k in keys], [rs, rc], [t["gl"][k] for k in keys])
    return {k: v.detach() for k, v in outs.items()}, grads


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.element_size() == 2 else a,
                                                                      b.view(torch.int16) if b.element_size() == 2 else b)


F32_OUT = ("colors", "opacities", "depths", "weights", "trans", "alphas")


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("col", ["sigmoid", "none"])
@pytest.mark.parametrize("dens", ["trunc_exp", "exp", "relu", "softplus", "none"])
@pytest.mark.parametrize("d", HALF)
def test_render_raw_bit_for_bit(dev, monkeypatch, d, dens, col, extras):
    c = case(dev)
    r_sig, r_rgb = c["raw_sig"].to(d), c["raw_rgb"].to(d)          # drawn in float32, rounded to d once
    want, (w_sig, w_rgb) = run(c, r_sig.float(), r_rgb.float(), dens, col, extras)
    log = CallLog(monkeypatch)
    got, (g_sig, g_rgb) = run(c, r_sig, r_rgb, dens, col, extras)
    assert log.names() == ["nfa_render_raw_fwd_t", "nfa_render_raw_bwd_t"]
    assert all(a[0] == ELEM[d] for _, a in log.calls)
    assert (log.calls[1][1][13] is not None) == extras             # g_weights: the backward's EXTRA variant
    for k in F32_OUT:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
    assert same_bits(got["sigmas"], want["sigmas"].to(d)) and same_bits(got["rgbs"], want["rgbs"].to(d))
    assert same_bits(g_sig, w_sig.to(d)), "g_raw_sigmas"
    assert same_bits(g_rgb, w_rgb.to(d)), "g_raw_rgbs"
    assert not bool(g_sig[~c["sel"]].any())                        # behind the mask: exact zeros


def shifted(x, k):
    """The values of x as a contiguous view at a storage offset of k elements."""
    buf = torch.empty(x.numel() + 16, dtype=x.dtype, device=x.device)
    v = buf[k:k + x.numel()].view(x.shape)
    v.copy_(x.detach())
    assert v.is_contiguous()
    return v


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("d", HALF)
def test_render_raw_scalar_form_equals_vector_form(dev, monkeypatch, d, extras):
    c = case(dev)
    r_sig, r_rgb = c["raw_sig"].to(d), c["raw_rgb"].to(d)
    aligned, g_aligned = run(c, r_sig, r_rgb, "trunc_exp", "sigmoid", extras)
    t = {"ts": shifted(c["ts"], 1), "te": shifted(c["te"], 3), "sel": shifted(c["sel"], 1),
         "gl": {k: shifted(v, 1 + i % 3) for i, (k, v) in enumerate(c["gl"].items())}}
    log = CallLog(monkeypatch)
    got, g_got = run(c, shifted(r_sig, 1), shifted(r_rgb, 1), "trunc_exp", "sigmoid", extras, tensors=t)
    assert log.names() == ["nfa_render_raw_fwd_t", "nfa_render_raw_bwd_t"]
    for name, a in log.calls:   # (elem, t_starts, t_ends, raw_sigmas, raw_rgbs, selector, ...)
        assert a[1] % 16 != 0 and a[2] % 16 != 0 and a[3] % 8 == 2 and a[4] % 8 == 2 and a[5] % 4 != 0, name
    for k in aligned:
        assert same_bits(aligned[k], got[k]), k
    assert same_bits(g_aligned[0], g_got[0]) and same_bits(g_aligned[1], g_got[1])


def small_case(dev):
    counts = torch.tensor([3, 0, 70, 1, 200], device=dev)
    ri = torch.repeat_interleave(torch.arange(5, device=dev), counts)
    g = torch.Generator().manual_seed(2)
    n = int(counts.sum())
    ts = (torch.rand(n, generator=g) * 2.0).to(dev)
    return ri, ts, ts + 0.01, (torch.rand(n, 3, generator=g) * 4 - 2).to(dev), (torch.rand(n, generator=g) * 4 - 2).to(dev)


def test_routing(dev, monkeypatch):
    ri, ts, te, rgb, sig = small_case(dev)
    raw = lambda names: [n for n in names if n.startswith("nfa_render_raw")]

    log = CallLog(monkeypatch)                                      # all float32: the unsuffixed entries, as ever
    s32, c32 = sig.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    colors, _, _, _ = rendering_from_raw(ts, te, c32, s32, ri, 5)
    colors.sum().backward()
    assert raw(log.names()) == ["nfa_render_raw_fwd", "nfa_render_raw_bwd"]

    for d in HALF:
        for kw in (dict(raw_rgbs=rgb.to(d), raw_sigmas=sig), dict(raw_rgbs=rgb, raw_sigmas=sig.to(d)),
                   dict(raw_rgbs=rgb.to(torch.float16), raw_sigmas=sig.to(torch.bfloat16)),
                   dict(raw_rgbs=rgb.to(d), raw_sigmas=sig.to(d), t_starts=ts.to(d)),
                   dict(raw_rgbs=rgb.to(d), raw_sigmas=sig.to(d), t_ends=te.to(d))):
            a = {"t_starts": ts, "t_ends": te, **kw}
            log.calls.clear()
            colors, opac, depth, ex = rendering_from_raw(a["t_starts"], a["t_ends"], a["raw_rgbs"], a["raw_sigmas"], ri, 5)
            assert raw(log.names()) == [], (d, list(kw))
            assert colors.shape == (5, 3) and all(bool(torch.isfinite(v.float()).all()) for v in (colors, opac, depth, ex["weights"]))


@pytest.mark.parametrize("d", HALF)
def test_empty_input(dev, d):
    ts = torch.zeros(0, device=dev)
    ri = torch.zeros(0, dtype=torch.int64, device=dev)
    rgb = torch.zeros(0, 3, dtype=d, device=dev, requires_grad=True)
    sig = torch.zeros(0, dtype=d, device=dev, requires_grad=True)
    colors, opac, depth, ex = rendering_from_raw(ts, ts, rgb, sig, ri, 3, return_activated=True)
    for v, shape in ((colors, (3, 3)), (opac, (3, 1)), (depth, (3, 1)), (ex["weights"], (0,)), (ex["trans"], (0,)), (ex["alphas"], (0,))):
        assert v.dtype == torch.float32 and v.shape == shape and not bool(v.any())
    assert ex["sigmas"].dtype == d and ex["sigmas"].shape == (0,) and ex["rgbs"].dtype == d and ex["rgbs"].shape == (0, 3)
    g_sig, g_rgb = torch.autograd.grad(colors.sum() + opac.sum(), [sig, rgb], allow_unused=True)
    for g, like in ((g_sig, sig), (g_rgb, rgb)):
        assert g is None or (g.dtype == d and g.shape == like.shape)

    x = torch.zeros(0, 3, device=dev, requires_grad=True)
    enc = HashGridEncoding(3, 4, 2, 12, 4, 1.5, out_dtype=d).to(dev)
    sh = SphericalHarmonicsEncoding(3, 4, out_dtype=d)
    y, s = enc(x), sh(x)
    assert y.shape == (0, 8) and y.dtype == d and s.shape == (0, 16) and s.dtype == d
    (y.float().sum() + s.float().sum()).backward()
    assert x.grad.shape == (0, 3) and float(enc.params.grad.abs().sum()) == 0.0


# ---------------------------------------------------------------- 7. an autocast step end to end
def test_autocast_step_trains(dev, monkeypatch):
    """tests/test_encodings_gpu.py's small NGP-shaped field under bf16 autocast: the encodings write bf16, the MLPs run in
    bf16, their raw outputs go straight into rendering_from_raw.  100 seeded steps at 48 x 48 rays; the loss must halve."""
    import nerfacc_amd as na
    torch.manual_seed(0)
    grid = encoding_from_tcnn_config(3, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2,
                                         "log2_hashmap_size": 15, "base_resolution": 8, "per_level_scale": 1.5},
                                     out_dtype="autocast")
    dirs_enc = encoding_from_tcnn_config(3, {"otype": "Composite", "nested": [
        {"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 4}]}, out_dtype="autocast")
    base = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.ReLU(), torch.nn.Linear(64, 16))
    head = torch.nn.Sequential(torch.nn.Linear(16 + 15, 64), torch.nn.ReLU(), torch.nn.Linear(64, 3))
    model = torch.nn.ModuleList([grid, base, head]).to(dev)
    est = na.OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=32).to(dev)
    est.binaries = torch.ones_like(est.binaries)
    est.occs = torch.ones_like(est.occs)

    H = W = 48
    v, u = torch.meshgrid(torch.linspace(-0.6, 0.6, H, device=dev), torch.linspace(-0.6, 0.6, W, device=dev), indexing="ij")
    d = torch.stack([u, v, torch.ones_like(u)], -1).view(-1, 3)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor([0.0, 0.0, -3.0], device=dev).expand_as(d).contiguous()
    r2 = (u * u + v * v).view(-1)
    target = torch.stack([(r2 < 0.2).float(), 0.5 * (r2 < 0.1).float(), 0.3 + 0.0 * r2], -1)
    seen = {}

    def step():
        ri, ts, te = est.sampling(o, d, render_step_size=2 * 3 ** 0.5 / 256, near_plane=0.0)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x = o[ri] + d[ri] * ((ts + te) / 2)[:, None]
            feat = grid((x + 1.0) / 2.0)
            sh = dirs_enc((d[ri] + 1.0) / 2.0)
            h = base(feat)
            raw_rgb = head(torch.cat([sh, h[:, 1:]], -1))
        seen.update(grid=feat.dtype, sh=sh.dtype, raw_sigma=h.dtype, raw_rgb=raw_rgb.dtype)
        colors, _, _, _ = rendering_from_raw(ts, te, raw_rgb, h[:, 0], ri, H * W, density_activation="trunc_exp", density_bias=1.0)
        loss = torch.nn.functional.mse_loss(colors, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return float(loss.detach())

    opt = torch.optim.Adam(model.parameters(), lr=1e-2, eps=1e-15)
    losses = [step() for _ in range(100)]
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert all(np.isfinite(losses))
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])

    log = CallLog(monkeypatch)
    step()
    names = log.names()
    assert all(v == torch.bfloat16 for v in seen.values()), seen
    assert "nfa_render_raw_fwd" not in names and "nfa_render_raw_bwd" not in names
    for n in ("nfa_hashgrid_fwd_t", "nfa_hashgrid_bwd_t", "nfa_sh_fwd_t", "nfa_render_raw_fwd_t", "nfa_render_raw_bwd_t"):
        assert names.count(n) == 1, (n, names)
    assert "nfa_hashgrid_fwd" not in names and "nfa_hashgrid_bwd" not in names and "nfa_sh_fwd" not in names
    assert model[0].params.grad.dtype == torch.float32

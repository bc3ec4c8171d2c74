"""GPU: nerfacc_amd.encodings on the native ops nfa_hashgrid_{fwd,bwd} and nfa_sh_{fwd,bwd} -- the hash grid's forward bit
for bit against the torch path, its gradients against float64, determinism of dL/dx, spherical harmonics against float64,
the native path being the one taken, empty input, and a small NGP-shaped field trained through OccGridEstimator."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


NGP_SCALE = np.exp((np.log(4096) - np.log(16)) / 15).tolist()
# (n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale)
CONFIGS = {
    "radiance": (16, 2, 19, 16, NGP_SCALE),                                    # NGPRadianceField
    "density": (5, 2, 17, 16, np.exp((np.log(128) - np.log(16)) / 4).tolist()),  # NGPDensityField
    "F1_L1": (1, 1, 14, 16, 2.0),          # one level: no cross-lane sum of dL/dx
    "F1_L32": (32, 1, 12, 16, 1.3),        # 2 points per wave
    "F1_L3_2p24": (3, 1, 24, 128, 4.0),    # 2 hashed levels of 2^24 entries (~142 MB of parameters)
    "F2_L24": (24, 2, 16, 16, 1.2),        # 16 idle lanes per wave
    "F4_L3": (3, 4, 14, 16, 2.0),          # one idle lane
    "F4_ngp": (16, 4, 19, 16, NGP_SCALE),  # the NGP radiance field's shape at F = 4
    "F8_L7_edge": (7, 8, 12, 16, 1.0),     # every level 16^3 = 2^12 entries: exactly on the dense / hashed boundary
    "F8_L32": (32, 8, 15, 16, 1.3),        # widest
    "F2_odd_res": (4, 2, 16, 10.5, 1.5),   # level 0: 11^3 entries, padded to 1336
}


def ngp_grid(kind, seed=0):
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(seed)
    L, F, log2, base, scale = CONFIGS[kind]
    enc = HashGridEncoding(3, L, F, log2, base, scale)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    return enc


def points(n, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g) * (hi - lo) + lo


def with_cell_boundaries(x, enc, seed):
    """x with rows replaced by points on cell boundaries of every level (x * scale_l + 0.5 an integer in float32) and by
    x = 1.0 and 0.0 coordinates."""
    g = torch.Generator().manual_seed(seed)
    x = x.clone()
    n = x.shape[0]
    rows = []
    for s in enc.scales:
        k = torch.arange(0, int(s) + 2, dtype=torch.float32)
        c = (k - 0.5) / s
        c = c[(c * s + 0.5) == torch.floor(c * s + 0.5)]   # (float32 arithmetic, as the kernels do it)
        if c.numel():
            rows.append(c[torch.randint(0, c.numel(), (max(n // (4 * len(enc.scales)), 1), 3), generator=g)])
    rows.append(torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 0.5], [0.0, 0.0, 0.0]]))
    b = torch.cat(rows)[: max(n - 1, 1)]
    x[1: 1 + b.shape[0]] = b[: n - 1] if n > 1 else x[1:]
    if n == 1:
        x[0] = torch.tensor([1.0, 1.0, 1.0])
    return x


ORIG = ("radiance", "density")
FWD_CASES = [pytest.param(kind, n, id=f"{n}-{kind}")
             for kind in CONFIGS for n in (1, 63, 65, 4097, 1 << 20) if n < (1 << 20) or kind in ORIG]


@pytest.mark.parametrize("kind,n", FWD_CASES)
def test_forward_bit_identical_to_torch_path(dev, kind, n):
    enc = ngp_grid(kind)
    x = points(n, n)
    if n > 8:   # out-of-range finite points as well
        x[: n // 8] = points(n // 8, n + 1, -2.0, 3.0)
        x[0] = torch.tensor([1e6, -1e7, 3e9])
    if kind not in ORIG:
        x = with_cell_boundaries(x, enc, n)
    ref = enc(x)                                   # CPU: the torch path
    got = enc.to(dev)(x.to(dev))
    assert got.shape == ref.shape == (n, enc.n_output_dims)
    assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32))


def test_forward_batch_dims_and_noncontiguous(dev):
    enc = ngp_grid("density")
    x = points(2 * 7 * 5, 3, -0.5, 1.5).view(2, 7, 5, 3)
    ref = enc(x)
    ref_t = enc(x.transpose(0, 2))
    encd = enc.to(dev)
    xd = x.to(dev)
    got = encd(xd)
    assert got.shape == (2, 7, 5, 10)
    assert torch.equal(got.cpu(), ref)
    xt = xd.transpose(0, 2)                        # non-contiguous
    assert not xt.is_contiguous()
    assert torch.equal(encd(xt).cpu(), ref_t)
    # the torch path on the GPU agrees too
    from nerfacc_amd.encodings import _hashgrid_torch
    t = _hashgrid_torch(xd.view(-1, 3), encd.params.detach(), encd.table, 2)
    assert torch.equal(t, got.view(-1, 10))


def test_nonfinite_inputs_do_not_fault(dev):
    enc = ngp_grid("radiance").to(dev)
    x = points(4096, 5).to(dev)
    x[::7, 0] = float("nan")
    x[1::7, 1] = float("inf")
    x[2::7, 2] = -float("inf")
    x.requires_grad_(True)
    y = enc(x)
    y.sum().backward()
    torch.cuda.synchronize()
    ok = torch.isfinite(x.detach()).all(-1)
    ref = enc(x.detach()[ok])
    assert torch.equal(y.detach()[ok], ref)


def restate_grads(x, params, enc, g):
    """float64 scatter of w_c * g (weights from the float32 cell coordinates, as the kernels form them); per entry also
    the contribution count and the sum of |contribution|.  dL/dx in float64 from the same cells."""
    F = enc.n_features_per_level
    x64 = x.double()
    gp = torch.zeros(params.numel() // F, F, dtype=torch.float64)
    cnt = torch.zeros(params.numel() // F, dtype=torch.float64)
    absum = torch.zeros(params.numel() // F, F, dtype=torch.float64)
    gx = torch.zeros_like(x64)
    P = params.double().view(-1, F)
    for l in range(enc.n_levels):
        s = enc.scales[l]
        p = x * s + 0.5
        fl = torch.floor(p)
        f = (p - fl).double()
        gi = fl.clamp(-2147483648.0, 2147483520.0).to(torch.int64) & M32
        size, res, off = enc.sizes[l], enc.resolutions[l], enc.offsets[l]
        gl = g[:, l * F:(l + 1) * F].double()
        for c in range(8):
            b = [(c >> d) & 1 for d in range(3)]
            q = [(gi[:, d] + b[d]) & M32 for d in range(3)]
            if enc.table.hashed[l]:
                idx = (q[0] ^ ((q[1] * 2654435761) & M32) ^ ((q[2] * 805459861) & M32)) & (size - 1)
            else:
                idx = ((q[0] + q[1] * res + q[2] * res * res) & M32) % size
            wf = [f[:, d] if b[d] else 1.0 - f[:, d] for d in range(3)]
            w = wf[0] * wf[1] * wf[2]
            contrib = w[:, None] * gl
            gp.index_add_(0, off + idx, contrib)
            absum.index_add_(0, off + idx, contrib.abs())
            cnt.index_add_(0, off + idx, torch.ones_like(w))
            dot = (gl * P[off + idx]).sum(-1)
            for d in range(3):
                o = [e for e in range(3) if e != d]
                gx[:, d] += (1.0 if b[d] else -1.0) * s * wf[o[0]] * wf[o[1]] * dot
    return gp.view(-1), cnt, absum.view(-1), gx


@pytest.mark.parametrize("kind", list(CONFIGS))
def test_backward_against_float64(dev, kind):
    enc = ngp_grid(kind)
    n = 1 << 16
    x = points(n, 11, -0.25, 1.25)
    if kind not in ORIG:
        x = with_cell_boundaries(x, enc, 11)
    g = torch.randn(n, enc.n_output_dims, generator=torch.Generator().manual_seed(12))
    encd = enc.to(dev)
    xd = x.to(dev).requires_grad_(True)
    encd(xd).backward(g.to(dev))
    ref_p, cnt, absum, ref_x = restate_grads(x, enc.params.detach().cpu(), enc, g)
    got_p = encd.params.grad.cpu().double()
    F = enc.n_features_per_level
    bound = (cnt.repeat_interleave(F) + 2) * 2.0 ** -23 * absum
    err = (got_p - ref_p).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert int((cnt > 0).sum()) > 1000
    torch.testing.assert_close(xd.grad.cpu().double(), ref_x, rtol=1e-4, atol=1e-3 * float(ref_x.abs().mean()))
    # dL/dx is bitwise reproducible; params-only and x-only backward give the same gradients
    gx1 = xd.grad.clone()
    gp1 = encd.params.grad.clone()
    xd.grad = None
    encd.params.grad = None
    encd.params.requires_grad_(False)
    encd(xd).backward(g.to(dev))
    assert torch.equal(xd.grad, gx1)
    encd.params.requires_grad_(True)
    xd2 = x.to(dev)
    encd.params.grad = None
    encd(xd2).backward(g.to(dev))
    assert bool(((encd.params.grad.cpu().double() - ref_p).abs() <= bound).all())   # (the order of the atomic adds varies)


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_against_float64(dev, degree):
    from nerfacc_amd.encodings import SphericalHarmonicsEncoding
    sh = SphericalHarmonicsEncoding(3, degree)
    d = torch.rand(5000, 3, generator=torch.Generator().manual_seed(degree))
    dd = d.to(dev).requires_grad_(True)
    out = sh(dd)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    out.backward(g.to(dev))
    d64 = d.double().requires_grad_(True)
    ref = sh(d64)                                  # CPU float64: the torch path
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=1e-5, atol=2e-6)
    if degree == 1:                                # a constant: no gradient
        assert float(dd.grad.abs().max()) == 0.0
    else:
        ref.backward(g.double())
        torch.testing.assert_close(dd.grad.cpu().double(), d64.grad, rtol=1e-4, atol=2e-5)
    # leading dims, non-contiguous input
    dv = d.to(dev).view(50, 100, 3).transpose(0, 1)
    torch.testing.assert_close(sh(dv).cpu(), sh(d.view(50, 100, 3).transpose(0, 1)), rtol=1e-5, atol=2e-6)


def test_native_path_taken(dev, monkeypatch):
    from nerfacc_amd import _backend as B
    from nerfacc_amd.encodings import SphericalHarmonicsEncoding
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    enc = ngp_grid("density").to(dev)
    sh = SphericalHarmonicsEncoding(3, 4)
    x = points(1000, 1).to(dev).requires_grad_(True)
    (enc(x).sum() + sh(x).sum()).backward()
    assert sorted(calls) == sorted(["nfa_hashgrid_fwd", "nfa_sh_fwd", "nfa_hashgrid_bwd", "nfa_sh_bwd"]), calls


def test_empty_input(dev):
    from nerfacc_amd.encodings import SphericalHarmonicsEncoding
    enc = ngp_grid("density").to(dev)
    sh = SphericalHarmonicsEncoding(3, 4)
    x = torch.zeros(0, 3, device=dev, requires_grad=True)
    y, s = enc(x), sh(x)
    assert y.shape == (0, 10) and s.shape == (0, 16)
    (y.sum() + s.sum()).backward()
    assert x.grad.shape == (0, 3) and float(enc.params.grad.abs().sum()) == 0.0


def test_autocast_float32(dev):
    enc = ngp_grid("density").to(dev)
    x = points(333, 2).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        y = enc(x)
    assert y.dtype == torch.float32
    assert torch.equal(y, enc(x))


def test_train_small_ngp_field(dev):
    """A small NGPRadianceField-shaped model (hash grid -> MLP -> density, SH(dir) + features -> MLP -> rgb) trained for 100
    seeded steps through OccGridEstimator.sampling and rendering towards a synthetic image: the loss must halve."""
    import nerfacc_amd as na
    from nerfacc_amd.encodings import encoding_from_tcnn_config
    torch.manual_seed(0)
    grid = encoding_from_tcnn_config(3, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2,
                                         "log2_hashmap_size": 15, "base_resolution": 8, "per_level_scale": 1.5})
    dirs_enc = encoding_from_tcnn_config(3, {"otype": "Composite", "nested": [
        {"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 4}]})
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
    # target: a coloured disc on black
    r2 = (u * u + v * v).view(-1)
    target = torch.stack([(r2 < 0.2).float(), 0.5 * (r2 < 0.1).float(), 0.3 + 0.0 * r2], -1)

    def field(ts, te, ri):
        x = o[ri] + d[ri] * ((ts + te) / 2)[:, None]
        h = base(grid((x + 1.0) / 2.0))
        sigma = torch.nn.functional.softplus(h[:, 0] - 1.0) * 10.0
        rgb = torch.sigmoid(head(torch.cat([dirs_enc((d[ri] + 1.0) / 2.0), h[:, 1:]], -1)))
        return rgb, sigma

    opt = torch.optim.Adam(model.parameters(), lr=1e-2, eps=1e-15)
    losses = []
    for _ in range(100):
        ri, ts, te = est.sampling(o, d, render_step_size=2 * 3 ** 0.5 / 256, near_plane=0.0)
        colors, _, _, _ = na.rendering(ts, te, ri, n_rays=H * W, rgb_sigma_fn=field)
        loss = torch.nn.functional.mse_loss(colors, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])


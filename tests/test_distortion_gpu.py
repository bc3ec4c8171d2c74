"""GPU: nerfacc_amd.losses.distortion on the native ops nfa_distortion_{fwd,bwd} -- values and gradients against a float64
pairwise restatement, the path taken, determinism, tiling invariance, composition with rendering(), batched input."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged_case(lengths, seed, offset=0.0, step=0.05):
    """Samples of rays with the given lengths: t increasing along each ray from `offset`, t values on a 2^-8 grid (so that
    midpoints and widths are exact in float32 also at t ~ 1e3), random weights.  float32, on the CPU."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    n = int(lengths.sum())
    ray_ids = np.repeat(np.arange(len(lengths)), lengths)
    q = lambda x: np.round(x * 256.0) / 256.0
    gap = q(rng.random(n) * step) + 1.0 / 256
    c = np.cumsum(gap)
    starts = np.cumsum(lengths) - lengths
    base = np.where(starts[ray_ids] > 0, c[np.maximum(starts[ray_ids] - 1, 0)], 0.0)
    te = c - base + offset + q(rng.random(len(lengths)) * 4.0)[ray_ids]
    ts = te - q(gap * rng.random(n))
    w = rng.random(n) * (2.0 / np.maximum(lengths[ray_ids], 1))
    T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    return T(w), T(ts), T(te), T(ray_ids, torch.int64), len(lengths)


def pairwise_f64(w, ts, te, ri, R):
    """float64 restatement, O(n^2) per ray (Barron et al. 2022, eq. 15); rays up to 64 samples are padded into one batch,
    longer ones run one by one."""
    w, ts, te = (t.to(torch.float64) for t in (w, ts, te))
    m, s = (ts + te) / 2, te - ts
    counts = torch.bincount(ri, minlength=R)
    starts = torch.cumsum(counts, 0) - counts
    out = [torch.zeros(R, dtype=torch.float64, device=w.device).index_add(0, ri, w * w * s / 3)]
    short = torch.nonzero((counts > 0) & (counts <= 64)).flatten()
    if short.numel():
        k = torch.arange(64, device=w.device)
        idx = starts[short, None] + k
        ok = k < counts[short, None]
        idx = torch.where(ok, idx, torch.zeros_like(idx))
        ww, mm = w[idx] * ok, m[idx]
        pair = (ww[:, :, None] * ww[:, None, :] * (mm[:, :, None] - mm[:, None, :]).abs()).sum((1, 2))
        out.append(torch.zeros(R, dtype=torch.float64, device=w.device).index_add(0, short, pair))
    for r in torch.nonzero(counts > 64).flatten().tolist():
        a, b = int(starts[r]), int(starts[r] + counts[r])
        pr = (w[a:b, None] * w[None, a:b] * (m[a:b, None] - m[None, a:b]).abs()).sum()
        out.append(torch.zeros(R, dtype=torch.float64, device=w.device).index_put((torch.tensor([r], device=w.device),), pr.view(1)))
    return sum(out)


def scales(w, ts, te, ri, R, g):
    """Per-ray scale W^2 (m_last - m_first) + sum w^2 s of the loss, and the matching per-element scales of its gradients:
    |g| (2 W span + w s) for weights, |g| (2 w W + w^2) for t_starts / t_ends."""
    w, ts, te = (t.to(torch.float64) for t in (w, ts, te))
    m, s = (ts + te) / 2, te - ts
    W = torch.zeros(R, dtype=torch.float64, device=w.device).index_add(0, ri, w)
    mmax = torch.full((R,), -np.inf, dtype=torch.float64, device=w.device).scatter_reduce(0, ri, m, "amax")
    mmin = torch.full((R,), np.inf, dtype=torch.float64, device=w.device).scatter_reduce(0, ri, m, "amin")
    span = torch.where(W > 0, mmax - mmin, torch.zeros_like(W)).clamp_min(0)
    loss_scale = W * W * span + torch.zeros_like(W).index_add(0, ri, w * w * s)
    gabs = g.abs().to(torch.float64)[ri]
    return loss_scale, gabs * (2 * W[ri] * span[ri] + w * s), gabs * (2 * w * W[ri] + w * w)


def run(fn, w, ts, te, g):
    xs = [t.detach().clone().requires_grad_(True) for t in (w, ts, te)]
    out = fn(*xs)
    return (out.detach(), *torch.autograd.grad(out, xs, g))


def check_against_f64(w, ts, te, ri, R, dev, **kw):
    from nerfacc_amd.losses import distortion
    wd, tsd, ted, rid = (t.to(dev) for t in (w, ts, te, ri))
    g = torch.rand(R, generator=torch.Generator().manual_seed(7), dtype=torch.float32).to(dev) + 0.5
    got = run(lambda a, b, c: distortion(a, b, c, ray_indices=rid, n_rays=R, **kw), wd, tsd, ted, g)
    ref = run(lambda a, b, c: pairwise_f64(a, b, c, rid, R), wd.double(), tsd.double(), ted.double(), g.double())
    ls, gws, gts = scales(wd, tsd, ted, rid, R, g)
    assert got[0].dtype == torch.float32 and got[0].shape == (R,)
    for name, a, b, sc in zip(("loss", "g_weights", "g_t_starts", "g_t_ends"), got, ref, (ls, gws, gts, gts)):
        err = (a.double() - b).abs()
        bad = err > 1e-5 * sc
        assert not bool(bad.any()), (name, int(bad.sum()), float((err / sc.clamp_min(1e-30)).max()))
    counts = torch.bincount(rid, minlength=R)
    assert bool((got[0][counts == 0] == 0).all())
    return got


LONG = [300, 1100, 2500]


def test_native_matches_float64_ragged(dev):
    rng = np.random.default_rng(0)
    lengths = np.concatenate([rng.integers(0, 40, 3000), LONG, [0, 1, 1, 0, 257, 1024, 1025]])
    rng.shuffle(lengths)
    check_against_f64(*ragged_case(lengths, seed=1), dev)


def test_native_matches_float64_far_offset(dev):
    """t around 1e3 (the far planes of unbounded scenes): the kernels work on m - m_first, so no cancellation."""
    rng = np.random.default_rng(2)
    lengths = np.concatenate([rng.integers(0, 40, 2000), LONG])
    check_against_f64(*ragged_case(lengths, seed=3, offset=1000.0, step=0.02), dev)


def test_native_matches_float64_occgrid_samples(dev):
    import nerfacc_amd as na
    rng = np.random.default_rng(4)
    R, res = 4096, 64
    o = torch.from_numpy(rng.standard_normal((R, 3)).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((R, 3)).astype(np.float32)), dim=-1).to(dev)
    est = na.OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=res).to(dev)
    b = torch.from_numpy(rng.random((1, res, res, res)) < 0.3).to(dev)
    est.binaries = b
    est.occs = b.reshape(-1).float()
    ri, ts, te = est.sampling(o, d, render_step_size=2 * 3 ** 0.5 / 512)
    assert ri.numel() > 10000
    w = torch.from_numpy(rng.random(ri.numel()).astype(np.float32)).to(dev) * 0.05
    check_against_f64(w.cpu(), ts.cpu(), te.cpu(), ri.cpu(), R, dev)


def _case(dev, seed=5):
    rng = np.random.default_rng(seed)
    lengths = np.concatenate([rng.integers(0, 60, 5000), LONG])
    w, ts, te, ri, R = ragged_case(lengths, seed=seed, offset=10.0)
    return w.to(dev), ts.to(dev), te.to(dev), ri.to(dev), R


def test_native_path_taken(dev, monkeypatch):
    from nerfacc_amd import _backend as B
    from nerfacc_amd import losses
    from nerfacc_amd._segments import seginfo_from_ray_indices
    w, ts, te, ri, R = _case(dev)
    seginfo_from_ray_indices(ri, R)   # cached on ri: the segment table is not part of the loss
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(losses, "_distortion_torch", lambda *a: pytest.fail("torch fallback taken"))
    ws = w.clone().requires_grad_(True)
    loss = losses.distortion(ws, ts, te, ray_indices=ri, n_rays=R)
    loss.sum().backward()
    assert calls == ["nfa_distortion_fwd", "nfa_distortion_bwd"], calls


def test_deterministic(dev):
    from nerfacc_amd.losses import distortion
    w, ts, te, ri, R = _case(dev)
    g = torch.linspace(0.5, 1.5, R, device=dev)
    a = run(lambda x, y, z: distortion(x, y, z, ray_indices=ri, n_rays=R), w, ts, te, g)
    b = run(lambda x, y, z: distortion(x, y, z, ray_indices=ri, n_rays=R), w, ts, te, g)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


_CHILD = r"""
import hashlib, sys
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_distortion_gpu import _case, run
from nerfacc_amd.losses import distortion
dev = torch.device("cuda:0")
w, ts, te, ri, R = _case(dev)
out = run(lambda x, y, z: distortion(x, y, z, ray_indices=ri, n_rays=R), w, ts, te, torch.linspace(0.5, 1.5, R, device=dev))
h = hashlib.sha256()
for t in out:
    h.update(t.cpu().numpy().tobytes())
print("digest", h.hexdigest())
"""


def test_tiling_invariance(dev):
    """Outputs are bit-identical across tile sizes: each size in a child process (NFA_SEG_TILE is read once)."""
    digests = []
    for tile in ("256", "1024", "3072"):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, NFA_SEG_TILE=tile))
        assert r.returncode == 0 and "digest " in r.stdout, (tile, r.returncode, r.stdout[-300:], r.stderr[-500:])
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1] == digests[2], digests


def test_composition_with_rendering(dev):
    """distortion(extras["weights"], ...).mean() added to a rendering() loss: sigma / rgb gradients match the same
    composition with the loss on the torch path."""
    import nerfacc_amd as na
    from nerfacc_amd import losses
    w0, ts, te, ri, R = _case(dev, seed=6)
    n = ts.numel()
    gen = torch.Generator().manual_seed(0)
    sig0 = (torch.rand(n, generator=gen) * 20.0).to(dev)
    rgb0 = torch.rand((n, 3), generator=gen).to(dev)

    def total(torch_path):
        sig, rgb = sig0.clone().requires_grad_(True), rgb0.clone().requires_grad_(True)
        colors, opac, depth, extras = na.rendering(ts, te, ri, n_rays=R, rgb_sigma_fn=lambda a, b, c: (rgb, sig))
        w = extras["weights"]
        if torch_path:
            dl = losses._distortion_torch(w, ts, te, ri, R)
        else:
            dl = losses.distortion(w, ts, te, ri, R)
        loss = (colors ** 2).sum() + 0.1 * opac.sum() + dl.mean()
        return torch.autograd.grad(loss, (sig, rgb))

    nat, ref = total(False), total(True)
    for a, b in zip(nat, ref):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * float(b.abs().max())), float((a - b).abs().max())


def test_batched_matches_packed(dev):
    from nerfacc_amd.losses import distortion
    R, S = 777, 48
    w, ts, te, ri, _ = ragged_case([S] * R, seed=8, offset=2.0)
    w, ts, te, ri = (t.to(dev) for t in (w, ts, te, ri))
    g = torch.linspace(0.5, 1.5, R, device=dev)
    packed = run(lambda a, b, c: distortion(a, b, c, ray_indices=ri, n_rays=R), w, ts, te, g)
    batched = run(lambda a, b, c: distortion(a, b, c), w.view(R, S), ts.view(R, S), te.view(R, S), g)
    assert batched[0].shape == (R,) and batched[1].shape == (R, S)
    for a, b in zip(packed, batched):
        assert torch.equal(a, b.reshape(a.shape))

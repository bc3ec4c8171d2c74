"""CPU: the float64 reference of the packed ops (tests/seg_reference.py, used by test_kernel_variants_gpu.py) against a
per-ray Python loop on a small ragged batch -- values and the autograd gradients the GPU tests take from it."""
import math

import torch

import seg_reference as SR

COUNTS = [0, 1, 2, 3, 4, 5, 0, 0, 9, 1, 17, 0]


def _case(seed=0):
    g = torch.Generator().manual_seed(seed)
    rays = SR.Rays(torch.tensor(COUNTS))
    n = rays.n
    ts = torch.rand(n, generator=g, dtype=torch.float64)
    te = ts + 0.05 + torch.rand(n, generator=g, dtype=torch.float64) * 0.2
    sig = torch.rand(n, generator=g, dtype=torch.float64) * 6
    return rays, ts, te, sig, g


def _loop_rays(rays):
    out = []
    for r, c in enumerate(rays.counts.tolist()):
        s = int(rays.starts[r])
        out.append((r, list(range(s, s + c))))
    return out


def test_layout_round_trip_and_scans():
    rays, ts, te, sig, g = _case()
    x = torch.rand(rays.n, generator=g, dtype=torch.float64) + 0.5
    assert torch.equal(rays.unpad(rays.pad(x)), x)
    assert rays.pad(x).shape == (len(COUNTS), max(COUNTS))
    for kind in ("inclusive_sum", "exclusive_sum", "inclusive_prod", "exclusive_prod"):
        got = SR.scan(rays, x, kind)
        want = torch.empty_like(x)
        for _, idx in _loop_rays(rays):
            acc = 0.0 if kind.endswith("sum") else 1.0
            for i in idx:
                if kind.startswith("inclusive"):
                    acc = acc + x[i].item() if kind.endswith("sum") else acc * x[i].item()
                    want[i] = acc
                else:
                    want[i] = acc
                    acc = acc + x[i].item() if kind.endswith("sum") else acc * x[i].item()
        torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-13)


def test_density_alpha_and_their_gradients():
    rays, ts, te, sig, g = _case(1)
    pf = torch.rand(rays.n, generator=g, dtype=torch.float64)
    gw, gt, ga = (torch.randn(rays.n, generator=g, dtype=torch.float64) for _ in range(3))
    sig_r = sig.clone().requires_grad_(True)
    w, T, a = SR.from_density(rays, ts, te, sig_r, pf)
    (w * gw + T * gt + a * ga).sum().backward()
    for _, idx in _loop_rays(rays):
        S = 0.0
        for k, i in enumerate(idx):
            x = sig[i].item() * (te[i] - ts[i]).item()
            Ti, ai = math.exp(-S) * pf[i].item(), 1.0 - math.exp(-x)
            assert abs(T[i].item() - Ti) < 1e-13 and abs(a[i].item() - ai) < 1e-13 and abs(w[i].item() - Ti * ai) < 1e-13
            # dL/dx_i = (gw_i T_i + ga_i)(1 - a_i) - sum_{j > i} (gw_j a_j + gt_j) T_j
            tail = 0.0
            S2 = S + x
            for j in idx[k + 1:]:
                xj = sig[j].item() * (te[j] - ts[j]).item()
                Tj, aj = math.exp(-S2) * pf[j].item(), 1.0 - math.exp(-xj)
                tail += (gw[j].item() * aj + gt[j].item()) * Tj
                S2 += xj
            gx = (gw[i].item() * Ti + ga[i].item()) * (1.0 - ai) - tail
            assert abs(sig_r.grad[i].item() - gx * (te[i] - ts[i]).item()) < 1e-12
            S += x
    al = (torch.rand(rays.n, generator=g, dtype=torch.float64) * 0.9).requires_grad_(True)
    w2, T2 = SR.from_alpha(rays, al, pf)
    for _, idx in _loop_rays(rays):
        P = 1.0
        for i in idx:
            assert abs(T2[i].item() - P * pf[i].item()) < 1e-13 and abs(w2[i].item() - P * pf[i].item() * al[i].item()) < 1e-13
            P *= 1.0 - al[i].item()


def test_accumulations_render_step_and_cdf_rows():
    rays, ts, te, sig, g = _case(2)
    w = torch.rand(rays.n, generator=g, dtype=torch.float64)
    v = torch.randn(rays.n, 5, generator=g, dtype=torch.float64)
    out = SR.accumulate(rays, w, v)
    op = SR.accumulate(rays, w)
    for r, idx in _loop_rays(rays):
        for ch in range(5):
            assert abs(out[r, ch].item() - sum(w[i].item() * v[i, ch].item() for i in idx)) < 1e-13
        assert abs(op[r, 0].item() - sum(w[i].item() for i in idx)) < 1e-13
    rgb = torch.rand(rays.n, 3, generator=g, dtype=torch.float64)
    opac0 = torch.rand(rays.R, 1, generator=g, dtype=torch.float64) * 0.5
    c, o, d, keep = SR.render_step(rays, ts, te, sig, rgb, opac0[:, 0], 0.3)
    for r, idx in _loop_rays(rays):
        S, acc = 0.0, [0.0] * 5
        for i in idx:
            x = sig[i].item() * (te[i] - ts[i]).item()
            Ti, ai = math.exp(-S) * (1.0 - opac0[r, 0].item()), 1.0 - math.exp(-x)
            if ai >= 0.3:
                wi = Ti * ai
                for ch in range(3):
                    acc[ch] += wi * rgb[i, ch].item()
                acc[3] += wi
                acc[4] += wi * (ts[i] + te[i]).item() / 2
            assert bool(keep[i]) == (ai >= 0.3)
            S += x
        assert max(abs(c[r, ch].item() - acc[ch]) for ch in range(3)) < 1e-13
        assert abs(o[r, 0].item() - acc[3]) < 1e-13 and abs(d[r, 0].item() - acc[4]) < 1e-13
    R, S_ = 4, 6
    t = torch.sort(torch.rand(R, S_ + 1, generator=g, dtype=torch.float64), -1).values
    s2 = torch.rand(R, S_, generator=g, dtype=torch.float64) * 3
    cd = SR.cdf_rows(t[:, :-1], t[:, 1:], s2)
    for r in range(R):
        acc = 0.0
        for k in range(S_):
            assert abs(cd[r, k].item() - (1.0 - math.exp(-acc))) < 1e-13
            acc += s2[r, k].item() * (t[r, k + 1] - t[r, k]).item()
        assert cd[r, S_].item() == 1.0


def test_error_scales_cover_a_float32_evaluation():
    """The scales the GPU tests turn into tolerances hold for a float32 evaluation of the same formulas on the CPU."""
    rays, ts, te, sig, g = _case(3)
    ts, te, sig = (t.float() for t in (ts, te, sig))
    gw, gt = (torch.randn(rays.n, generator=g) for _ in range(2))
    w32, T32, a32 = SR.from_density(rays, ts, te, sig)
    sig64 = sig.double().requires_grad_(True)
    w, T, a = SR.from_density(rays, ts.double(), te.double(), sig64)
    (w * gw.double() + T * gt.double()).sum().backward()
    s_w, s_t, s_a, s_gx = SR.density_scales(rays, ts.double(), te.double(), sig.double(), T, a, gw.double(), gt.double())
    for got, want, sc in ((w32, w, s_w), (T32, T, s_t), (a32, a, s_a)):
        assert bool(((got.double() - want).abs() <= SR.bound(rays, sc)).all())
    sig32 = sig.clone().requires_grad_(True)
    w32, T32, _ = SR.from_density(rays, ts, te, sig32)
    (w32 * gw + T32 * gt).sum().backward()
    dt = (te - ts).double()
    assert bool(((sig32.grad.double() - sig64.grad).abs() <= SR.bound(rays, s_gx * dt)).all())

"""The plane regularisers of nerfacc_amd.losses restated in float64 by slicing, differentiated by autograd: the reference of
tests/test_planereg_cpu.py and tests/test_planereg_gpu.py.

Plane ``(s, k)`` of a plane grid is a row-major ``[H, W, F]`` block ``p[j, i, f]`` (``H = R_b``, ``W = R_a``); a time plane is
one with ``b == 3``.  Four terms per plane, each a mean:

    tv_h   = sum (p[j+1] - p[j])^2 / (F (H-1) W)               tv_w = sum (p[:, i+1] - p[:, i])^2 / (F H (W-1))
    smooth = sum ((p[j+2] - p[j+1]) - (p[j+1] - p[j]))^2 / (F (H-2) W)      time planes only; 0 when H = 2
    l1     = sum |1 - p| / (F H W)                                           time planes only
"""
import functools
import itertools

import torch

# (n_dims, resolution, multiscale_res): D = 3, and D = 4 at every time resolution with its own boundary overlaps
CASES = [(3, (6, 5, 4), (1, 2))] + [(4, (5, 4, 3, T), (1, 2)) for T in (2, 3, 4, 5, 7)]
FEATURES = (4, 32)


def scale_resolutions(resolution, multiscale_res):
    D = len(resolution)
    return [[resolution[d] * m if d < 3 else resolution[d] for d in range(D)] for m in multiscale_res]


def plane_views(params, resolution, multiscale_res, F):
    """[(s, k, is_time, p[H, W, F])] over the flat table, scale-major, then ``itertools.combinations`` order."""
    D = len(resolution)
    out, at = [], 0
    for s, res in enumerate(scale_resolutions(resolution, multiscale_res)):
        for k, (a, b) in enumerate(itertools.combinations(range(D), 2)):
            H, W = res[b], res[a]
            out.append((s, k, b == 3, params[at: at + H * W * F].view(H, W, F)))
            at += H * W * F
    assert at == params.numel()
    return out


def n_params(resolution, multiscale_res, F):
    D = len(resolution)
    return sum(res[a] * res[b] * F for res in scale_resolutions(resolution, multiscale_res)
               for a, b in itertools.combinations(range(D), 2))


def terms_reference(params, resolution, multiscale_res, F):
    """``[n_scales, n_planes, 4]`` float64 (tv_h, tv_w, smooth, l1); differentiable towards a float64 ``params``."""
    p64 = params.to(torch.float64)
    rows = []
    for s, k, time, p in plane_views(p64, resolution, multiscale_res, F):
        H, W, _ = p.shape
        zero = p64.new_zeros(())
        tv_h = ((p[1:] - p[:-1]) ** 2).sum() / (F * (H - 1) * W)
        tv_w = ((p[:, 1:] - p[:, :-1]) ** 2).sum() / (F * H * (W - 1))
        smooth, l1 = zero, zero
        if time:
            if H > 2:
                smooth = (((p[2:] - p[1:-1]) - (p[1:-1] - p[:-2])) ** 2).sum() / (F * (H - 2) * W)
            l1 = (1.0 - p).abs().sum() / (F * H * W)
        rows.append(torch.stack([tv_h, tv_w, smooth, l1]))
    D = len(resolution)
    return torch.stack(rows).view(len(multiscale_res), D * (D - 1) // 2, 4)


def make_params(resolution, multiscale_res, F, seed=0):
    """Float32 parameters around 1 (so that ``|1 - p|`` sees both signs), a few of them exactly 1."""
    g = torch.Generator().manual_seed(seed)
    p = 1.0 + 0.5 * torch.randn(n_params(resolution, multiscale_res, F), generator=g)
    p[::37] = 1.0
    return p


@functools.lru_cache(maxsize=None)
def case(resolution, multiscale_res, F, seed=0):
    """(params float32, grad_terms float32, terms float64, grad_params float64) of one shape: computed once, never modified.
    ``grad_terms`` is random, with whole planes of zeros."""
    p = make_params(resolution, multiscale_res, F, seed)
    pr = p.double().requires_grad_(True)
    terms = terms_reference(pr, resolution, multiscale_res, F)
    g = torch.randn(terms.shape, generator=torch.Generator().manual_seed(seed + 1))
    g[0, 0] = 0.0
    g[-1, -1] = 0.0
    (gp,) = torch.autograd.grad(terms, pr, g.double())
    return p, g, terms.detach(), gp

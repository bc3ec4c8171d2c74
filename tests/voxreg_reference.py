"""The voxel-grid regularisers of nerfacc_amd.losses restated in float64 on the ``[1, C, N_x, N_y, N_z]`` view DVGO and TiNeuVox
keep (``grid().permute(3, 2, 1, 0)[None]``), differentiated by autograd: the reference of tests/test_voxreg_cpu.py and
tests/test_voxreg_gpu.py.  Independent of the slicing form in nerfacc_amd/losses.py: ``torch.diff`` along dims 2, 3, 4 and
``F.smooth_l1_loss`` / ``abs`` / ``pow(2)`` with ``reduction="sum"``, divided by the counts.
"""
import functools

import torch
import torch.nn.functional as F

TERMS = ("tv_x", "tv_y", "tv_z", "l1")
KINDS = ("l2", "l1", "huber")
RESOLUTIONS = [(2, 2, 2), (5, 4, 7), (9, 17, 33)]
FEATURES = (1, 2, 4, 12)


def n_params(res, C):
    return res[0] * res[1] * res[2] * C


def view(params, res, C):
    """DVGO's ``[1, C, N_x, N_y, N_z]`` tensor as a view of the flat ``[R_z, R_y, R_x, C]`` table."""
    return params.view(res[2], res[1], res[0], C).permute(3, 2, 1, 0)[None]


def penalty_sum(d, kind):
    if kind == "l2":
        return d.pow(2).sum()
    if kind == "l1":
        return d.abs().sum()
    return F.smooth_l1_loss(d, torch.zeros_like(d), reduction="sum", beta=1.0)


def terms_reference(params, res, C, kind, reduction="mean"):
    """``[4]`` float64 (tv_x, tv_y, tv_z, l1); differentiable towards a float64 ``params``."""
    v = view(params.to(torch.float64), res, C)
    out = []
    for dim in (2, 3, 4):
        d = torch.diff(v, dim=dim)
        out.append(penalty_sum(d, kind) / (d.numel() if reduction == "mean" else 1))
    out.append(v.abs().sum() / (v.numel() if reduction == "mean" else 1))
    return torch.stack(out)


def make_params(res, C, seed=0):
    """Float32 parameters ``1.5 * randn`` (so |d| lands on both sides of 1), a few of them exactly 0, and a few adjacent pairs
    (along x, y and z) that differ by exactly 0, +1 and -1: sign0 at 0 and the clamp's edges."""
    p = 1.5 * torch.randn(n_params(res, C), generator=torch.Generator().manual_seed(seed))
    p[::37] = 0.0
    g = p.view(res[2], res[1], res[0], C)
    for axis, delta in enumerate((0.0, 1.0, -1.0)):
        for lead in ((0, 0, 0), (1, 1, 1)):                      # the pair (lead, lead + 1 along `axis`), channel 0 and the last
            nxt = list(lead)
            nxt[axis] += 1
            if nxt[axis] < g.shape[axis]:
                for c in {0, C - 1}:
                    base = torch.round(g[lead][c] * 4.0) / 4.0       # (a quarter: base + 1 and base - 1 are exact)
                    g[lead][c] = base
                    g[tuple(nxt)][c] = base + delta
    return p


@functools.lru_cache(maxsize=None)
def case(res, C, kind, seed=0, reduction="mean"):
    """(params float32, grad_terms float32, terms float64, grad_params float64) of one shape: computed once, never modified.
    ``grad_terms`` is random, with tv_y's weight exactly 0."""
    p = make_params(res, C, seed)
    pr = p.double().requires_grad_(True)
    terms = terms_reference(pr, res, C, kind, reduction)
    g = torch.randn(4, generator=torch.Generator().manual_seed(seed + 1))
    g[1] = 0.0
    (gp,) = torch.autograd.grad(terms, pr, g.double())
    return p, g, terms.detach(), gp

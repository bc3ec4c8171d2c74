"""The VM-grid regularisers of nerfacc_amd.losses restated in float64 in the tensor form TensoRF's ``TensorVMSplit`` uses, on
the ``[1, C, H, W]`` plane and ``[1, C, R, 1]`` line views, differentiated by autograd: the reference of
tests/test_vmreg_cpu.py and tests/test_vmreg_gpu.py.  Independent of the slicing form in nerfacc_amd/losses.py.

    TVLoss(x[1, C, H, W])         = 2 (h_tv / count_h + w_tv / count_w),  count_h = C (H-1) W,  count_w = C H (W-1)
    density_L1                    = sum_m mean|plane_m| + mean|line_m|
    vector_comp_diffs             = sum_m mean |offdiag(V V^T)|,  V = line_m.view(C, R); the off-diagonal part by
                                    dotp.view(-1)[1:].view(C - 1, C + 1)[..., :-1]
"""
import functools

import torch

VM_MODES = ((0, 1, 2), (0, 2, 1), (1, 2, 0))
TERMS = ("tv_h", "tv_w", "l1_plane", "tv_line", "l1_line", "ortho")
RESOLUTIONS = [(2, 2, 2), (7, 6, 5), (33, 20, 9)]
COMPONENTS = (4, 24, 96)


def n_params(res, C):
    return sum((res[a] * res[b] + res[c]) * C for a, b, c in VM_MODES)


def views(params, res, C):
    """[(plane [1, C, H, W], line [1, C, R, 1])] per mode: TensoRF's tensors, as views of the flat table."""
    out, at = [], 0
    for a, b, c in VM_MODES:
        H, W, R = res[b], res[a], res[c]
        plane = params[at: at + H * W * C].view(H, W, C).permute(2, 0, 1)[None]
        at += H * W * C
        line = params[at: at + R * C].view(R, C).t()[None, :, :, None]
        at += R * C
        out.append((plane, line))
    assert at == params.numel()
    return out


def tv_parts(x):
    """TVLoss's two quotients of a ``[1, C, H, W]`` tensor: (h_tv / count_h, w_tv / count_w)."""
    h_x, w_x = x.size(2), x.size(3)
    count_h = x[:, :, 1:, :].numel() // x.size(0)
    count_w = x[:, :, :, 1:].numel() // x.size(0)
    h_tv = torch.pow(x[:, :, 1:, :] - x[:, :, :h_x - 1, :], 2).sum()
    w_tv = torch.pow(x[:, :, :, 1:] - x[:, :, :, :w_x - 1], 2).sum()
    return h_tv / count_h, w_tv / count_w


def tv_loss(x):
    """``TVLoss()`` (weight 1, batch 1)."""
    h, w = tv_parts(x)
    return 2 * (h + w)


def vector_diff(line):
    """One summand of ``vector_comp_diffs``: the mean |.| of the off-diagonal part of the components' dot products."""
    n_comp, n_size = line.shape[1:-1]
    v = line.reshape(n_comp, n_size)
    dotp = torch.matmul(v, v.transpose(-1, -2))
    non_diagonal = dotp.view(-1)[1:].view(n_comp - 1, n_comp + 1)[..., :-1]
    return torch.mean(torch.abs(non_diagonal))


def terms_reference(params, res, C):
    """``[3, 6]`` float64 (tv_h, tv_w, l1_plane, tv_line, l1_line, ortho); differentiable towards a float64 ``params``."""
    rows = []
    for plane, line in views(params.to(torch.float64), res, C):
        tv_h, tv_w = tv_parts(plane)
        # the h half of TVLoss on the line (its w half divides by an empty count: W = 1)
        tv_line = torch.pow(line[:, :, 1:, :] - line[:, :, :-1, :], 2).sum() / line[:, :, 1:, :].numel()
        rows.append(torch.stack([tv_h, tv_w, torch.mean(torch.abs(plane)), tv_line, torch.mean(torch.abs(line)), vector_diff(line)]))
    return torch.stack(rows)


def ortho_scale(params, res, C):
    """``[3]`` float64: mean_{i<j} sum_r |l[r,i] l[r,j]| per mode, the magnitude the rounding of a Gram entry scales with."""
    out = []
    for _, line in views(params.to(torch.float64), res, C):
        v = line.reshape(C, -1).abs()
        out.append(torch.triu(v @ v.t(), diagonal=1).sum() / (C * (C - 1) / 2))
    return torch.stack(out)


def make_params(res, C, seed=0):
    """Float32 parameters around 0 with both signs, a few of them exactly 0."""
    p = 0.5 * torch.randn(n_params(res, C), generator=torch.Generator().manual_seed(seed))
    p[::37] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def case(res, C, seed=0):
    """(params float32, grad_terms float32, terms float64, grad_params float64) of one shape: computed once, never modified.
    ``grad_terms`` is random, with mode 1's tv_w and mode 2's l1_line weight exactly 0."""
    p = make_params(res, C, seed)
    pr = p.double().requires_grad_(True)
    terms = terms_reference(pr, res, C)
    g = torch.randn(terms.shape, generator=torch.Generator().manual_seed(seed + 1))
    g[1, 1] = 0.0
    g[2, 4] = 0.0
    (gp,) = torch.autograd.grad(terms, pr, g.double())
    return p, g, terms.detach(), gp

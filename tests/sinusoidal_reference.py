"""The sinusoidal encoding in float64, plain torch, differentiable to any order by autograd: the formulas of
csrc/sinenc.hip's header restated, ``var`` and ``freq_weights`` included, and the error bounds of its accuracy contract.

With xb = 2^k x_d (exact in float32) and a = w_k exp(-0.5 4^k var_d):
    forward    every sine / cosine column within  2^-22 max(1, |xb|) a  (+ 2^-22 a with var or freq_weights: exp, products)
    gradients  within (2^-22 + (2 L + 2) 2^-24) sum |term|, each term's trigonometric factor weighted by max(1, |xb|)
With var, a can lie below float32's normal range (exp(-0.5 4^9 0.1) is far below it): there a float32 result is a multiple of
2^-149, so such a factor carries an absolute error of up to one such quantum (TINY: the roundings of exp and of two
products, half a quantum each at most) whatever its size, and the bounds with var add TINY times what multiplies a.
"""
import math

import torch

# (n_input_dims, min_deg, max_deg, use_identity)
REFERENCE_CONFIGS = [(3, 0, 10, True), (3, 0, 4, True), (1, 0, 4, True), (2, 0, 4, True)]
CONFIGS = REFERENCE_CONFIGS + [(4, -2, 6, False), (3, 0, 16, True), (3, 3, 4, True)]
POINT_COUNTS = [0, 1, 63, 64, 65, 1000, 4099]
U = 2.0 ** -22
TINY = 2.0 ** -148   # float32 underflow, see above


def scales(min_deg, max_deg, device=None):
    return torch.tensor([2.0 ** i for i in range(min_deg, max_deg)], dtype=torch.float64, device=device)


def _parts(x, min_deg, max_deg, var=None, freq_weights=None):
    """(xb, a) as [..., L, D] float64 tensors."""
    x = x.to(torch.float64)
    s = scales(min_deg, max_deg, x.device)
    xb = x[..., None, :] * s[:, None]
    a = torch.ones_like(xb)
    if freq_weights is not None:
        a = a * freq_weights.to(torch.float64)[:, None]
    if var is not None:
        a = a * torch.exp(-0.5 * (s * s)[:, None] * var.to(torch.float64)[..., None, :])
    return xb, a


def encode(x, min_deg, max_deg, use_identity=True, var=None, freq_weights=None):
    """x [..., D] (any float dtype) -> [..., K] in float64; columns: x, the sine block (k D + d), the cosine block."""
    x = x.to(torch.float64)
    if max_deg == min_deg:
        return x
    xb, a = _parts(x, min_deg, max_deg, var, freq_weights)
    blocks = [(a * torch.sin(xb)).flatten(-2), (a * torch.cos(xb)).flatten(-2)]
    return torch.cat(([x] if use_identity else []) + blocks, dim=-1)


def forward_bound(x, min_deg, max_deg, use_identity=True, var=None, freq_weights=None):
    """The contract's bound per column of ``encode`` (0 on the identity columns: they are bitwise x)."""
    xb, a = _parts(x, min_deg, max_deg, var, freq_weights)
    b = U * torch.clamp(xb.abs(), min=1.0) * a.abs()
    if var is not None or freq_weights is not None:
        b = b + U * a.abs()
    if var is not None:
        b = b + TINY
    b = b.flatten(-2)
    ident = [torch.zeros(*x.shape, dtype=torch.float64, device=x.device)] if use_identity else []
    return torch.cat(ident + [b, b], dim=-1)


def _split(g, D, L, use_identity):
    g = g.to(torch.float64)
    o = D if use_identity else 0
    g_id = g[..., :D] if use_identity else torch.zeros(*g.shape[:-1], D, dtype=torch.float64, device=g.device)
    g_sin = g[..., o:o + L * D].unflatten(-1, (L, D))
    g_cos = g[..., o + L * D:].unflatten(-1, (L, D))
    return g_id, g_sin, g_cos


def grad_bounds(x, g, min_deg, max_deg, use_identity=True, var=None, freq_weights=None):
    """(bound of grad_x, bound of grad_var) for the incoming gradient g [..., K]."""
    D, L = x.shape[-1], max_deg - min_deg
    s = scales(min_deg, max_deg, x.device)[:, None]
    xb, a = _parts(x, min_deg, max_deg, var, freq_weights)
    g_id, g_sin, g_cos = _split(g, D, L, use_identity)
    w = torch.clamp(xb.abs(), min=1.0)
    eps = U + (2 * L + 2) * 2.0 ** -24
    tx = g_id.abs() + (s * a.abs() * w * (g_sin.abs() * torch.cos(xb).abs() + g_cos.abs() * torch.sin(xb).abs())).sum(-2)
    tv = 0.5 * (s * s * a.abs() * w * (g_sin.abs() * torch.sin(xb).abs() + g_cos.abs() * torch.cos(xb).abs())).sum(-2)
    if var is None:
        return eps * tx, eps * tv
    gg = g_sin.abs() + g_cos.abs()
    return eps * tx + TINY * (s * gg).sum(-2), eps * tv + TINY * (s * s * gg).sum(-2)


def second_order_bounds(x, g, v, min_deg, max_deg, use_identity=True, freq_weights=None):
    """(bound of grad_grad_out [..., K], bound of the second-order grad_x [..., D]) for gg_x = v."""
    D, L = x.shape[-1], max_deg - min_deg
    s = scales(min_deg, max_deg, x.device)[:, None]
    xb, a = _parts(x, min_deg, max_deg, None, freq_weights)
    _, g_sin, g_cos = _split(g, D, L, use_identity)
    v = v.to(torch.float64)[..., None, :]
    w = torch.clamp(xb.abs(), min=1.0)
    eps = U + (2 * L + 2) * 2.0 ** -24
    b_sin = (eps * (v * s * a).abs() * w * torch.cos(xb).abs()).flatten(-2)
    b_cos = (eps * (v * s * a).abs() * w * torch.sin(xb).abs()).flatten(-2)
    ident = [torch.zeros(*x.shape, dtype=torch.float64, device=x.device)] if use_identity else []
    b_x = eps * ((v * s * s * a).abs() * w * (g_sin.abs() * torch.sin(xb).abs() + g_cos.abs() * torch.cos(xb).abs())).sum(-2)
    return torch.cat(ident + [b_sin, b_cos], dim=-1), b_x


def barf_window(alpha, n_freqs):
    k = torch.arange(n_freqs, dtype=torch.float64)
    return (1.0 - torch.cos(math.pi * torch.clamp(torch.as_tensor(alpha, dtype=torch.float64) - k, 0.0, 1.0))) / 2.0


def assert_within(got, want, bound, what=""):
    """|got - want| <= bound everywhere (float64 comparison), with the worst ratio in the message."""
    got, want, bound = got.detach().to(torch.float64).cpu(), want.detach().to(torch.float64).cpu(), bound.detach().cpu()
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    err = (got - want).abs()
    bad = err > bound
    if bad.any():
        ratio = (err / bound.clamp(min=1e-300))[bad].max()
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} values outside the bound, max err {float(err.max()):.3e}, "
                             f"worst err / bound {float(ratio):.3f}")


def draw(n, D, seed, span=1.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, D, generator=g) * 2.0 - 1.0) * span

"""Float64 autograd through a restatement of the Instant-NGP field with the chain's forward rounding points (each rounding is
straight-through: the rounded value, the identity's gradient), for the fused training pass of nerfacc_amd/csrc/ngp_field.hip.
The encoding and the harmonics are the package's op-for-op torch forms (as tests/ngp_field_reference.py)."""
import torch

import mlp_reference as R
from nerfacc_amd.encodings import _hashgrid_torch, _sh_torch
from nerfacc_amd.rawrender import activate_density


def _st(t, dtype):
    return t + (R.rnd(t.detach(), dtype) - t.detach())


def _net(h, ws, dtype):
    for l, w in enumerate(ws):
        z = h @ w.t()
        h = _st(torch.relu(z) if l < len(ws) - 1 else z, dtype)
    return h


def grads(field, positions, directions, g_rgb, g_sigma, activated):
    """``field``: a CPU module.  d(<g_rgb, rgb> + <g_sigma, sigma>) / d(table, base params, head params), float64, flat; the
    outputs are the raw ones or, ``activated``, sigmoid(rgb) and the module's density.  ``directions`` None: the density alone."""
    dtype = field.dtype
    leaf = lambda p: p.detach().double().requires_grad_()
    table, base = leaf(field.encoding.params), leaf(field.mlp_base.params)
    head = leaf(field.mlp_head.params) if directions is not None else None
    x, selector = field._normalise(positions.float())
    enc = _st(_hashgrid_torch(x.double(), table, field.encoding.table, 2, field.encoding.interp), dtype)
    y = _net(enc, [R.rnd(w, dtype).detach() + (w - w.detach()) for w in field.mlp_base._views(base)], dtype)
    sigma = y[:, 0]
    if activated:
        sigma = activate_density(sigma[:, None], field.density_activation, field.density_bias, selector[:, None])[:, 0]
    loss = (g_sigma.double() * sigma).sum()
    if head is not None:
        sh = R.rnd(_sh_torch((directions.float() + 1.0) / 2.0, 4).double(), dtype)
        rgb = _net(torch.cat([sh, y[:, 1:]], 1), [R.rnd(w, dtype).detach() + (w - w.detach()) for w in field.mlp_head._views(head)], dtype)
        loss = loss + (g_rgb.double() * (torch.sigmoid(rgb) if activated else rgb)).sum()
    return torch.autograd.grad(loss, [table, base] + ([head] if head is not None else []))

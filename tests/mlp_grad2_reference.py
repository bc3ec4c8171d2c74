"""Float64 restatement of the fused MLP's second order (nerfacc_amd/csrc/mlp.hip: nfa_mlp_tangent, and nfa_mlp_bwd_weights
run on the tangent activations), with the kernels' rounding points and a derived error bound per element.

With v the cotangent of dL/dx = g_x and s = <v, g_x> (notation of tests/mlp_reference.py, M_l = (H_l > 0)):
    T_{-1} = rnd(v),  T_l = rnd(M_l * (W_l T_{l-1})),  u = W_L T_{L-1} = ds/dg,  ds/dW_l = dZ_l^T T_{l-1},  ds/dx = 0.
The masks come from the ``hidden`` argument and the dZ_l from the ``dz`` argument, never recomputed here, so that both sides
of a comparison use one mask and one dZ.

Bound, by the rule of mlp_reference (layer l with K inputs, t with error e):
    e_pre  = |W| e + (K + 2) 2^-24 |W| |t|
    e_next = (e_pre + ulp(|z| + e_pre)) * M           a masked element is an exact zero on both sides
    e_dW   = |dZ|^T e_T + (N + 2) 2^-24 |dZ|^T |T| + ulp_32(|dZ|^T |T|)
"""
import torch

import mlp_reference as R


def tangent(v, weights, hidden, dtype, out_f32=False, exact=False):
    """v [N, n_in] float32 or dtype; hidden: [H_l] float64 values of ``dtype`` numbers.  Returns dict(u, e_u, t=[T_{-1}, T_0 ..
    T_{L-1}], e_t): u rounded to dtype unless ``out_f32``."""
    t = R.rnd(v.double(), dtype, exact)
    e = torch.zeros_like(t)
    ts, e_ts = [t], [e]
    for l, w in enumerate(weights):
        wq = R.rnd(w.double(), dtype, exact)
        z = t @ wq.t() + 0.0
        K = wq.shape[1]
        s_abs = t.abs() @ wq.abs().t()
        e_pre = e @ wq.abs().t() + (K + 2) * R.U32 * s_abs
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        if l < len(weights) - 1:
            mask = (hidden[l] > 0).double()
            t = R.rnd(torch.where(hidden[l] > 0, z, torch.zeros_like(z)), dtype, exact)
            e = (e_pre + R.ulp(dtype, z.abs() + e_pre)) * mask
            ts.append(t)
            e_ts.append(e)
        elif out_f32:
            u, e_u = z, e_pre
        else:
            u, e_u = R.rnd(z, dtype, exact), e_pre + R.ulp(dtype, z.abs() + e_pre)
    return dict(u=u, e_u=e_u, t=ts, e_t=e_ts)


def weight_grad2(dz, ts, e_ts, exact=False):
    """ds/dW_l = dZ_l^T T_{l-1} (float32 on the device, never rounded to the half type); dz = [dZ_0 .. dZ_L] and ts =
    [T_{-1} .. T_{L-1}] as float64.  Returns (dw=[...], e_dw=[...])."""
    N = ts[0].shape[0]
    dws, e_dws = [], []
    for d, t, e in zip(dz, ts, e_ts):
        dws.append(d.t() @ t + 0.0)
        s_abs = d.abs().t() @ t.abs()
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        e_dws.append(d.abs().t() @ e + (N + 2) * R.U32 * s_abs + R.ulp(torch.float32, s_abs))
    return dws, e_dws


def second_order(v, weights, hidden, dz, dtype, out_f32=False, exact=False):
    """Both passes: dict(u, e_u, t, e_t, dw, e_dw)."""
    r = tangent(v, weights, hidden, dtype, out_f32, exact)
    r["dw"], r["e_dw"] = weight_grad2(dz, r["t"], r["e_t"], exact)
    return r


def exact_tangent_input(N, n_in, dtype, mod=3):
    """v[n, i] = ((n + 2 i) mod 3) - 1: -1, 0, 1 (``mod=7``: -1 .. 5)."""
    n = torch.arange(N).view(-1, 1)
    return ((n + 2 * torch.arange(n_in).view(1, -1)) % mod - 1).to(dtype)


def autograd_float64(x, weights, g, v):
    """torch.autograd's own double backward of a plain ReLU nn.Linear(bias=False) stack in float64: (u, [ds/dW_l], ds/dx)
    of s = <v, dL/dx>, independent of the formulas above.  Only meaningful where nothing rounds (the exact data)."""
    from torch import nn
    lin = [nn.Linear(w.shape[1], w.shape[0], bias=False, dtype=torch.float64) for w in weights]
    with torch.no_grad():
        for l, w in zip(lin, weights):
            l.weight.copy_(w.double())
    xd = x.double().clone().requires_grad_(True)
    gd = g.double().clone().requires_grad_(True)
    h = xd
    for i, l in enumerate(lin):
        h = l(h)
        if i < len(lin) - 1:
            h = torch.relu(h)
    (g_x,) = torch.autograd.grad(h, xd, gd, create_graph=True)
    s = (g_x * v.double()).sum()
    grads = torch.autograd.grad(s, [gd] + [l.weight for l in lin] + [xd], allow_unused=True)
    return grads[0], list(grads[1:-1]), grads[-1]


# (N, n_in, n_out, x float32?, y and g float32?) of tests/test_mlp_gpu.py: the tile edges 31 / 32 / 33 and 127 / 128 / 129, rows
# that are not 16-byte aligned (the element-wise load path), 1 / 3 / 16 / 32 outputs, and 300 points: two split-K slices.
CONFIGS = [
    (1, 1, 1, True, False),
    (31, 16, 3, False, False),
    (32, 31, 16, True, True),
    (33, 32, 32, False, True),
    (127, 63, 3, False, False),
    (128, 32, 16, False, False),
    (129, 16, 1, True, True),
    (300, 32, 16, True, False),
]
WIDE_INPUT = (40, 150, 32, False, False)   # with 128 neurons: 10 k-steps of the first layer


def configs(family, width, n_hidden):
    """[(cfg, modulus of v)].  With the 'dense' first matrix of the wide-input case the mod-3 tangent input cancels: row o
    keeps the three columns i0, i0 + 50, i0 + 100 with ONE value ((7 * 50) mod 5 = 0), and v there is a permutation of -1, 0, 1
    ((2 * 50) mod 3 = 1), so T_0 and u are identically zero and only ds/dW_0 = dZ_0^T v is live.  That case stays, and the
    same shapes run once more with v mod 7, where every T_l, u and every ds/dW_l is live (and still an exact integer)."""
    wide = width == 128 and n_hidden <= 2
    return [(c, 3) for c in CONFIGS] + ([(WIDE_INPUT, 3)] if wide else []) + ([(WIDE_INPUT, 7)] if wide and family == "dense" else [])


def exact_case(family, dtype, width, n_hidden, cfg, v_mod=3):
    """Everything the exact tests compare against, for one case: (shape, ws, x, g, v, forward, backward, second order)."""
    N, n_in, n_out, x_f32, out_f32 = cfg
    shape = (n_in, n_out, width, n_hidden)
    ws = R.exact_weights(family, *shape)
    x, g = R.exact_inputs(N, n_in, n_out, torch.float32 if x_f32 else dtype, torch.float32 if out_f32 else dtype)
    v = exact_tangent_input(N, n_in, x.dtype, v_mod)
    f = R.forward(x, ws, dtype, out_f32, exact=True)
    b = R.backward(x, ws, f["hidden"], g, dtype, exact=True)
    s = second_order(v, ws, f["hidden"], b["dz"], dtype, out_f32, exact=True)
    if family == "dense" and cfg == WIDE_INPUT and v_mod == 3:   # see configs()
        assert not bool(s["u"].any()) and bool(R.flat(s["dw"]).any())
    elif N >= 31:   # a pass that writes zeros cannot agree
        assert bool(s["u"].any()) and bool(R.flat(s["dw"]).any())
    return shape, ws, x, g, v, f, b, s

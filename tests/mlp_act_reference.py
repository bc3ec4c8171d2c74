"""Float64 restatement of the fused MLP with activations (nerfacc_amd/csrc/mlp.hip: the nfa_mlp_act_* entries): forward, data
gradient, tangent and curvature pass with the kernels' rounding points and a propagated error bound per element.  It extends
tests/mlp_bias_skip_reference.py (same notation and conventions: the backward takes ``hidden`` and ``y`` as arguments, the
tangent ``hidden``, ``y`` and ``dz``, the curvature pass ``hidden`` and ``r``, so both sides of a comparison use one derivative
factor, one dZ and one R).

    H_l = rnd(f(z_l)),  y = rnd(f_out(z_L))
    dZ_L = rnd(g f_out'(y)),  dZ_l = rnd(dH_l f'(H_l))
    T_l = rnd(A_l f'(H_l)),  u = f_out'(y) A_L,  R_l = rnd((rho(H_l) dZ_l) A_l),  R_L = rnd((rho_out(y) dZ_L) A_L)
    E_L = R_L,  E_{l-1} = rnd((W_l^T E_l)[:W] f'(H_{l-1}) + R_{l-1}),  ds/dx = W_0^T E_0 + sum_cat W_l[:, W:]^T E_l

Bound.  The linear parts follow mlp_bias_skip_reference.  Through an activation: all seven are monotone, so a pre-activation
within e_pre of z gives a value between f(z - e_pre) and f(z + e_pre); the device evaluates f in float32 within C_F ulps of
float32 (measured, see C_F), and the result is rounded once to the half type:
    e_f    = max(f(z + e_pre) - f(z), f(z) - f(z - e_pre)) + C_F ulp_32(|f|)
    e_next = e_f + ulp_dtype(|f| + e_f)
A derivative factor is formed in float32 from a stored value that both sides share, so it carries no propagated error, only
its own evaluation: at most (2 C_F + 4) 2^-24 max(|f'|, 1) (one exp within C_F ulps whose argument beta y is itself a rounded
product -- t e^-t <= 0.37 bounds what that costs -- and at most three more roundings), and (2 C_F + 4) 2^-24 max(|rho|, beta)
for rho.  Each float32 product or sum after it adds 2^-24 of its magnitude.
"""
import torch

import mlp_bias_skip_reference as S
import mlp_grad2_reference as G
import mlp_reference as R
from mlp_reference import U32, rnd, ulp, worst_ratio  # noqa: F401

LEAKY = 0.009999999776482582   # 0.01f
NAMES = ("None", "ReLU", "LeakyReLU", "Sigmoid", "Tanh", "Softplus", "Exponential")
CURVED = ("Sigmoid", "Tanh", "Softplus", "Exponential")

# Float32 ulps of the device's evaluation of f (expf, log1pf, tanhf and the float32 arithmetic around them) against float64:
# TWICE the worst value that scripts/measure_mlp_act_ulps.py observed on the MI355X over every product of an fp16 number
# |x| <= 8 with five factors (184,330 pre-activations per activation; the tests' stay within |z| < 8).  Worst observed: Sigmoid
# 2.05, Tanh 1.307, Softplus 64.204 (beta 10) and 63.855 (beta 100), Exponential 0.792.  Softplus' figure is not the library's
# log1pf or expf: the argument -beta |z| is a rounded float32 product, and e^-t turns its half ulp into t / 2 ulps of the result
# (t up to 87 before e^-t leaves the normal range); the value there is below 1e-28.  LeakyReLU is one float32 product, restated
# exactly here: half an ulp for the pre-activation's own error.  The sample is not the worst case; a factor of two on a float32
# term is invisible beside one ulp of the half type (128 ulps of float32 are 2^-16, a half-type ulp is 2^-10 or 2^-7).
C_F = {"None": 0.0, "ReLU": 0.0, "LeakyReLU": 0.5, "Sigmoid": 4.1, "Tanh": 2.62, "Softplus": 128.5, "Exponential": 1.59}


def rnd32(t):
    return t.float().double()


def f(name, z, beta):
    if name == "ReLU":
        return torch.relu(z)
    if name == "LeakyReLU":
        return torch.where(z > 0, z, rnd32(z * LEAKY))   # one float32 rounding of the product
    if name == "Sigmoid":
        return torch.sigmoid(z)
    if name == "Tanh":
        return torch.tanh(z)
    if name == "Softplus":
        return z.clamp_min(0) + torch.log1p(torch.exp(-beta * z.abs())) / beta
    if name == "Exponential":
        return torch.exp(z)
    return z


def fprime(name, y, beta):
    """f' from the stored y (the multiplying activations only)."""
    if name == "Sigmoid":
        return y * (1 - y)
    if name == "Tanh":
        return 1 - y * y
    if name == "Softplus":
        return 1 - torch.exp(-beta * y)
    if name == "Exponential":
        return y
    return torch.ones_like(y)


def rho(name, y, beta):
    if name == "Sigmoid":
        return 1 - 2 * y
    if name == "Tanh":
        return -2 * y
    if name == "Softplus":
        return beta * torch.exp(-beta * y)
    if name == "Exponential":
        return torch.ones_like(y)
    return torch.zeros_like(y)


def times_deriv(name, d, e_d, y, beta):
    """(d f'(y), its error) for d with error e_d: a select for ReLU / LeakyReLU (whose 0.01f product is restated), a float32
    product for the others."""
    if name == "None":
        return d, e_d
    if name == "ReLU":
        return torch.where(y > 0, d, torch.zeros_like(d)), e_d * (y > 0)
    if name == "LeakyReLU":
        v = torch.where(y > 0, d, rnd32(d * LEAKY))
        return v, torch.where(y > 0, e_d, e_d * LEAKY + 2 * U32 * v.abs())
    fp = fprime(name, y, beta)
    v = d * fp
    return v, e_d * fp.abs() + d.abs() * (2 * C_F[name] + 4) * U32 * fp.abs().clamp_min(1.0) + U32 * v.abs()


def curvature_term(name, a, e_a, y, dz, beta):
    """(R = (rho(y) dZ) A unrounded, its error); dZ and y are shared."""
    if name not in CURVED:
        return torch.zeros_like(a), torch.zeros_like(a)
    rh = rho(name, y, beta)
    v = rh * dz * a
    e_rho = (2 * C_F[name] + 4) * U32 * rh.abs().clamp_min(beta if name == "Softplus" else 1.0)
    return v, (rh * dz).abs() * e_a + e_rho * (dz * a).abs() + 2 * U32 * v.abs()


def through(name, z, e_pre, beta, dtype=None):
    """(f(z) rounded to dtype (None: unrounded), its error) for z with error e_pre."""
    a = f(name, z, beta)
    if name in ("None", "ReLU"):
        e_f = e_pre
    else:
        e_f = torch.maximum(f(name, z + e_pre, beta) - a, a - f(name, z - e_pre, beta)) + C_F[name] * ulp(torch.float32, a)
    if dtype is None:
        return a, e_f
    return rnd(a, dtype), e_f + ulp(dtype, a.abs() + e_f)


def forward(x, weights, biases, skip_mask, dtype, act, out_f32=False, exact=False):
    """act = (hidden, output, beta).  Returns dict(y, hidden=[H_l], e_y, e_hidden)."""
    hid, out, beta = act
    x0 = rnd(x.double(), dtype, exact and x.dtype != torch.float32)
    h, e = x0, torch.zeros_like(x0)
    hidden, e_hidden = [], []
    for l, w in enumerate(weights):
        wq = rnd(w.double(), dtype, exact)
        hin, ein = S._cat(h, e, x0, l, skip_mask)
        b = biases[l].double() if biases is not None else torch.zeros(wq.shape[0], dtype=torch.float64)
        z = hin @ wq.t() + b + 0.0
        s_abs = hin.abs() @ wq.abs().t() + b.abs()
        e_pre = ein @ wq.abs().t() + (wq.shape[1] + 2 + (biases is not None)) * U32 * s_abs
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        if l < len(weights) - 1:
            h, e = through(hid, z, e_pre, beta, dtype)
            hidden.append(h)
            e_hidden.append(e)
        else:
            y, e_y = through(out, z, e_pre, beta, None if out_f32 else dtype)
    return dict(y=y, hidden=hidden, e_y=e_y, e_hidden=e_hidden)


def backward(x, weights, hidden, y, g, skip_mask, dtype, act, inject=None, exact=False):
    """hidden, y: float64 values as stored; g [N, n_out] float32 or dtype.  With ``inject`` = [R_0 .. R_{L-1}] the curvature
    pass: g is R_L, no output derivative, E_l = rnd(dH_l f'(H_l) + R_l).  Returns dict(dx, e_dx, dz=[dZ_0 .. dZ_L], e_dz, dw,
    e_dw, db, e_db); dx rounded to x's dtype."""
    hid, out, beta = act
    N, W = x.shape[0], weights[0].shape[0]
    x0 = rnd(x.double(), dtype, exact)
    if inject is not None or out == "None":
        dz, e = rnd(g.double(), dtype, exact), torch.zeros(g.shape, dtype=torch.float64)
    else:
        v, e_v = times_deriv(out, g.double(), torch.zeros(g.shape, dtype=torch.float64), y, beta)
        dz, e = rnd(v, dtype), e_v + (ulp(dtype, v.abs() + e_v) if out != "ReLU" else 0.0)
    L = len(weights)
    dzs, e_dzs, dws, e_dws, dbs, e_dbs = [dz], [e], [], [], [], []
    skip_dx, skip_e, skip_abs, skip_K = 0.0, 0.0, 0.0, 0
    for l in range(L - 1, -1, -1):
        h_prev = hidden[l - 1] if l > 0 else x0
        hin, _ = S._cat(h_prev, h_prev, x0, l, skip_mask)
        dws.append(dz.t() @ hin + 0.0)
        s_abs = dz.abs().t() @ hin.abs()
        e_dws.append(e.t() @ hin.abs() + (N + 2) * U32 * s_abs + ulp(torch.float32, s_abs))
        dbs.append(dz.sum(0) + 0.0)
        b_abs = dz.abs().sum(0)
        e_dbs.append(e.sum(0) + (N + 2) * U32 * b_abs + ulp(torch.float32, b_abs))
        wq = rnd(weights[l].double(), dtype, exact)
        K = wq.shape[0]
        if l > 0:
            wh = wq[:, :W]
            if S.is_cat(skip_mask, l):
                wx = wq[:, W:]
                skip_dx = skip_dx + dz @ wx
                skip_e = skip_e + e @ wx.abs()
                skip_abs = skip_abs + dz.abs() @ wx.abs()
                skip_K += K
            dh = dz @ wh + 0.0
            e_pre = e @ wh.abs() + (K + 2) * U32 * (dz.abs() @ wh.abs())
            v, e_v = times_deriv(hid, dh, e_pre, h_prev, beta)
            if inject is not None:
                v = v + inject[l - 1]
                e_v = e_v + U32 * v.abs()
            dz = rnd(v, dtype, exact and hid in ("None", "ReLU"))
            e = e_v + ulp(dtype, v.abs() + e_v)
            if hid == "ReLU" and inject is None:
                e = e * (h_prev > 0)   # a masked element is an exact zero on both sides
            dzs.append(dz)
            e_dzs.append(e)
        else:
            dh = dz @ wq + skip_dx + 0.0
            s_abs = dz.abs() @ wq.abs() + skip_abs
            e_pre = e @ wq.abs() + skip_e + (K + skip_K + 2) * U32 * s_abs
            dx = rnd(dh, x.dtype, exact and hid in ("None", "ReLU") and out in ("None", "ReLU"))
            e_dx = e_pre + ulp(x.dtype, dh.abs() + e_pre)
    return dict(dx=dx, e_dx=e_dx, dz=dzs[::-1], e_dz=e_dzs[::-1], dw=dws[::-1], e_dw=e_dws[::-1], db=dbs[::-1], e_db=e_dbs[::-1])


def tangent(v, weights, hidden, y, dz, skip_mask, dtype, act, out_f32=False, exact=False):
    """dz = [dZ_0 .. dZ_L] as stored.  Returns dict(u, e_u, t=[T_{-1} .. T_{L-1}], e_t, r=[R_0 .. R_L], e_r)."""
    hid, out, beta = act
    t0 = rnd(v.double(), dtype, exact)
    t, e = t0, torch.zeros_like(t0)
    ts, e_ts, rs, e_rs = [t], [e], [], []
    for l, w in enumerate(weights):
        wq = rnd(w.double(), dtype, exact)
        tin, ein = S._cat(t, e, t0, l, skip_mask)
        a = tin @ wq.t() + 0.0
        s_abs = tin.abs() @ wq.abs().t()
        e_pre = ein @ wq.abs().t() + (wq.shape[1] + 2) * U32 * s_abs
        last = l == len(weights) - 1
        name, yy = (out, y) if last else (hid, hidden[l])
        r_v, e_r = curvature_term(name, a, e_pre, yy, dz[l], beta)
        rs.append(rnd(r_v, dtype))
        e_rs.append(e_r + ulp(dtype, r_v.abs() + e_r) if name in CURVED else e_r)
        d, e_d = times_deriv(name, a, e_pre, yy, beta)
        if not last:
            t = rnd(d, dtype, exact and hid in ("None", "ReLU"))
            e = e_d + ulp(dtype, d.abs() + e_d)
            if hid == "ReLU":
                e = e * (hidden[l] > 0)
            ts.append(t)
            e_ts.append(e)
        elif out_f32:
            u, e_u = d, e_d
        else:
            u, e_u = rnd(d, dtype), e_d + ulp(dtype, d.abs() + e_d)
    return dict(u=u, e_u=e_u, t=ts, e_t=e_ts, r=rs, e_r=e_rs)


def tangent_weight_grad(dz, t, skip_mask):
    """ds/dW_l, first part: dZ_l^T [T_{l-1}(, v)] and its bound (t: the dict of :func:`tangent`)."""
    t0 = t["t"][0]
    cat = [S._cat(tt, ee, t0, l, skip_mask) for l, (tt, ee) in enumerate(zip(t["t"], t["e_t"]))]
    return G.weight_grad2(dz, [c[0] for c in cat], [c[1] for c in cat])


# ---------------------------------------------------------------- torch.autograd in float64, independent of the formulas above

def torch_act(name, z, beta):
    if name == "ReLU":
        return torch.relu(z)
    if name == "LeakyReLU":
        return torch.where(z > 0, z, z * LEAKY)
    if name == "Sigmoid":
        return torch.sigmoid(z)
    if name == "Tanh":
        return torch.tanh(z)
    if name == "Softplus":
        return torch.nn.functional.softplus(z, beta=beta, threshold=1e9)
    if name == "Exponential":
        return torch.exp(z)
    return z


def autograd_float64(x, weights, biases, skip_mask, act, g, v):
    """(y, dx, [dW_l], [db_l], u = ds/dg, ds/dx, [ds/dW_l], [ds/db_l]) of s = <v, dL/dx> by torch.autograd with
    create_graph=True; biases may be None (then the bias lists are empty)."""
    hid, out, beta = act
    ws = [w.double().clone().requires_grad_(True) for w in weights]
    bs = [b.double().clone().requires_grad_(True) for b in biases] if biases is not None else []
    xd, gd = x.double().clone().requires_grad_(True), g.double().clone().requires_grad_(True)
    h = xd
    for l, w in enumerate(ws):
        hin = torch.cat([h, xd], 1) if S.is_cat(skip_mask, l) else h
        z = hin @ w.t() + (bs[l] if bs else 0.0)
        h = torch_act(hid if l < len(ws) - 1 else out, z, beta)
    first = torch.autograd.grad(h, [xd] + ws + bs, gd, create_graph=True)
    s = (first[0] * v.double()).sum()
    second = torch.autograd.grad(s, [gd, xd] + ws + bs, allow_unused=True)
    n = len(ws)
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    return dict(y=h.detach(), dx=first[0].detach(), dw=[t.detach() for t in first[1:1 + n]], db=[t.detach() for t in first[1 + n:]],
                u=second[0], sx=zero(second[1], xd), sw=[zero(t, w) for t, w in zip(second[2:2 + n], ws)],
                sb=[zero(t, b) for t, b in zip(second[2 + n:], bs)])


def random_net(shape, skip_layer, seed=7, N=1000, dtype=torch.float16, f32_ends=False, scale=1.0):
    """Xavier matrices, biases in [-0.5, 0.5), standard normal x, g, v (``scale`` shrinks x: Exponential stays in range)."""
    skip_mask = S.skip_mask_of(skip_layer, shape[3])
    gen = torch.Generator().manual_seed(seed)
    ws = [(torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 for o, i in S.layer_dims(*shape, skip_mask)]
    bs = [torch.rand(w.shape[0], generator=gen) - 0.5 for w in ws]
    end = torch.float32 if f32_ends else dtype
    x, g, v = (torch.randn(N, n, generator=gen).to(end) for n in (shape[0], shape[1], shape[0]))
    return skip_mask, ws, bs, (x * scale).to(end), g, v

"""Float64 restatement of the fused MLP with biases and skip connections (nerfacc_amd/csrc/mlp.hip behind nfa_mlp_desc): forward,
backward (with db) and tangent, with the kernels' rounding points and a derived error bound per element, plus the
integer-valued data on which every pass must agree bit for bit.  It extends tests/mlp_reference.py and
tests/mlp_grad2_reference.py (same notation, same conventions: the backward takes ``hidden`` as an argument and the tangent
takes ``hidden`` and ``dz``, so both sides of a comparison use one mask and one dZ).

    z_l = b_l + W_l in_l,  in_l = [H_{l-1}, x] at a cat layer (bit l of ``skip_mask``), H_{l-1} elsewhere,  in_0 = x
    dx  = dZ_0 W_0 + sum over the cat layers dZ_l W_l[:, W:]         one float32 sum, rounded once
    dW_l = dZ_l^T in_l,  db_l = sum_p dZ_l[p, :]                     float32
    T_l = rnd(M_l * (W_l [T_{l-1}(, v)])),  u = W_L [T_{L-1}(, v)],  ds/dW_l = dZ_l^T [T_{l-1}(, v)],  ds/db_l = 0

Bound, by the rule of mlp_reference (layer l with K inputs, input h with error e):
    e_pre = |W| e + (K + 2 + [bias]) 2^-24 (|W| |h| + |b|)
A layer with a bias has one more float32 rounding (the sum starts from b instead of from zero) and b enters the magnitude; the
bias itself is float32 on both sides and carries no error.  A cat layer has K = W + n_in, and the x columns of its input carry
no error (x is rounded identically on both sides).  dx sums out_0 + sum_cat out_l products in one accumulator, so that is its K.
    e_db = sum_p e_dZ + (N + 2) 2^-24 sum_p |dZ| + ulp_32(sum_p |dZ|)

Against numbers that were computed WITHOUT the roundings (the golden fixture: the reference's MLP class in float64) the same
recursion bounds the distance, since every rounding moves a value by at most the ulp the recursion already adds and ReLU is
1-Lipschitz; but the two sides no longer share one mask and one H.  ``backward(..., free=forward's dict)`` adds what that costs:
a neuron whose pre-activation is within its own error of zero (|z| <= e_z) may be on for one side and off for the other, so
its dZ may differ by all of |dH| + e; and dW_l gains |dZ|^T e_H + e_dZ^T e_H.
"""
import torch

import mlp_grad2_reference as G
import mlp_reference as R
from mlp_reference import U32, rnd, ulp, worst_ratio  # noqa: F401  (worst_ratio: for the tests that import this module)


def skip_mask_of(skip_layer, n_hidden):
    """Bit l: layer l takes [H_{l-1}, x].  The reference appends x after hidden layer i when i > 0 and i % skip_layer == 0."""
    mask = 0
    if skip_layer is not None:
        for i in range(n_hidden):
            if i > 0 and i % skip_layer == 0:
                mask |= 1 << (i + 1)
    return mask


def is_cat(skip_mask, l):
    return bool((skip_mask >> l) & 1)


def layer_dims(n_in, n_out, width, n_hidden, skip_mask=0):
    return [(o, i + (n_in if is_cat(skip_mask, l) else 0)) for l, (o, i) in enumerate(R.layer_dims(n_in, n_out, width, n_hidden))]


def _cat(h, e, x0, l, skip_mask):
    if is_cat(skip_mask, l):
        return torch.cat([h, x0], 1), torch.cat([e, torch.zeros_like(x0)], 1)
    return h, e


def forward(x, weights, biases, skip_mask, dtype, out_f32=False, exact=False):
    """x [N, n_in] (float32 or dtype); weights float32 [out, in_l]; biases: float32 [out_l] each, or None.  Returns
    dict(y, hidden=[H_l], e_y, e_hidden)."""
    x0 = rnd(x.double(), dtype, exact and x.dtype != torch.float32)
    if exact:
        assert torch.equal(x0, x.double())
    h, e = x0, torch.zeros_like(x0)
    hidden, e_hidden, zs, e_zs = [], [], [], []
    for l, w in enumerate(weights):
        wq = rnd(w.double(), dtype, exact)
        hin, ein = _cat(h, e, x0, l, skip_mask)
        b = biases[l].double() if biases is not None else torch.zeros(wq.shape[0], dtype=torch.float64)
        z = hin @ wq.t() + b + 0.0
        K = wq.shape[1]
        s_abs = hin.abs() @ wq.abs().t() + b.abs()
        e_pre = ein @ wq.abs().t() + (K + 2 + (biases is not None)) * U32 * s_abs
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        if l < len(weights) - 1:
            h = rnd(torch.relu(z), dtype, exact)
            e = e_pre + ulp(dtype, z.abs() + e_pre)
            hidden.append(h)
            e_hidden.append(e)
            zs.append(z)
            e_zs.append(e_pre)
        elif out_f32:
            y, e_y = z, e_pre
        else:
            y, e_y = rnd(z, dtype, exact), e_pre + ulp(dtype, z.abs() + e_pre)
    return dict(y=y, hidden=hidden, e_y=e_y, e_hidden=e_hidden, z=zs, e_z=e_zs)


def backward(x, weights, hidden, g, skip_mask, dtype, exact=False, free=None):
    """hidden: [H_l] float64 values of ``dtype`` numbers; g [N, n_out] float32 or dtype.  Returns dict(dx, e_dx, dz=[dZ_0 ..
    dZ_L], e_dz, dw, e_dw, db, e_db); dx rounded to x's dtype.  db is returned whether or not the network has biases.
    ``free``: the dict of :func:`forward` when the other side has a mask and an H of its own (see the module's docstring)."""
    N, W = x.shape[0], weights[0].shape[0]
    x0 = rnd(x.double(), dtype, exact)
    dz = rnd(g.double(), dtype, exact)
    e = torch.zeros_like(dz)
    L = len(weights)
    dzs, e_dzs, dws, e_dws, dbs, e_dbs = [dz], [e], [], [], [], []
    skip_dx, skip_e, skip_abs, skip_K = 0.0, 0.0, 0.0, 0
    for l in range(L - 1, -1, -1):
        h_prev = hidden[l - 1] if l > 0 else x0
        hin, _ = _cat(h_prev, h_prev, x0, l, skip_mask)
        dws.append(dz.t() @ hin + 0.0)
        s_abs = dz.abs().t() @ hin.abs()
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        e_dw = e.t() @ hin.abs() + (N + 2) * U32 * s_abs + ulp(torch.float32, s_abs)
        if free is not None and l > 0:
            _, e_hin = _cat(h_prev, free["e_hidden"][l - 1], x0, l, skip_mask)
            e_dw = e_dw + (dz.abs() + e).t() @ e_hin
        e_dws.append(e_dw)
        dbs.append(dz.sum(0) + 0.0)
        b_abs = dz.abs().sum(0)
        e_dbs.append(e.sum(0) + (N + 2) * U32 * b_abs + ulp(torch.float32, b_abs))
        wq = rnd(weights[l].double(), dtype, exact)
        K = wq.shape[0]
        if l > 0:
            wh = wq[:, :W]
            if is_cat(skip_mask, l):   # the x columns feed dx only
                wx = wq[:, W:]
                skip_dx = skip_dx + dz @ wx
                skip_e = skip_e + e @ wx.abs()
                skip_abs = skip_abs + dz.abs() @ wx.abs()
                skip_K += K
            dh = dz @ wh + 0.0
            e_pre = e @ wh.abs() + (K + 2) * U32 * (dz.abs() @ wh.abs())
            mask = (h_prev > 0).double()
            dz = rnd(torch.where(h_prev > 0, dh, torch.zeros_like(dh)), dtype, exact)   # a select
            e = (e_pre + ulp(dtype, dh.abs() + e_pre)) * mask
            if free is not None:
                unsure = free["z"][l - 1].abs() <= free["e_z"][l - 1]
                e = torch.where(unsure, dh.abs() + e_pre + ulp(dtype, dh.abs() + e_pre), e)
            dzs.append(dz)
            e_dzs.append(e)
        else:
            dh = dz @ wq + skip_dx + 0.0
            s_abs = dz.abs() @ wq.abs() + skip_abs
            if exact:
                assert float(s_abs.max()) < 2 ** 24
            e_pre = e @ wq.abs() + skip_e + (K + skip_K + 2) * U32 * s_abs
            dx = rnd(dh, x.dtype, exact)
            e_dx = e_pre + ulp(x.dtype, dh.abs() + e_pre)
    return dict(dx=dx, e_dx=e_dx, dz=dzs[::-1], e_dz=e_dzs[::-1], dw=dws[::-1], e_dw=e_dws[::-1], db=dbs[::-1], e_db=e_dbs[::-1])


def tangent(v, weights, hidden, skip_mask, dtype, out_f32=False, exact=False):
    """As mlp_grad2_reference.tangent; a cat layer sees [T_{l-1}, v].  No bias enters.  Returns dict(u, e_u, t=[T_{-1} ..
    T_{L-1}], e_t)."""
    t0 = rnd(v.double(), dtype, exact)
    t, e = t0, torch.zeros_like(t0)
    ts, e_ts = [t], [e]
    for l, w in enumerate(weights):
        wq = rnd(w.double(), dtype, exact)
        tin, ein = _cat(t, e, t0, l, skip_mask)
        z = tin @ wq.t() + 0.0
        K = wq.shape[1]
        s_abs = tin.abs() @ wq.abs().t()
        e_pre = ein @ wq.abs().t() + (K + 2) * U32 * s_abs
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        if l < len(weights) - 1:
            mask = (hidden[l] > 0).double()
            t = rnd(torch.where(hidden[l] > 0, z, torch.zeros_like(z)), dtype, exact)
            e = (e_pre + ulp(dtype, z.abs() + e_pre)) * mask
            ts.append(t)
            e_ts.append(e)
        elif out_f32:
            u, e_u = z, e_pre
        else:
            u, e_u = rnd(z, dtype, exact), e_pre + ulp(dtype, z.abs() + e_pre)
    return dict(u=u, e_u=e_u, t=ts, e_t=e_ts)


def second_order(v, weights, hidden, dz, skip_mask, dtype, out_f32=False, exact=False):
    """Both passes: dict(u, e_u, t, e_t, dw, e_dw) with ds/dW_l = dZ_l^T [T_{l-1}(, v)]; ds/db is zero."""
    r = tangent(v, weights, hidden, skip_mask, dtype, out_f32, exact)
    t0 = r["t"][0]
    cat = [_cat(t, e, t0, l, skip_mask) for l, (t, e) in enumerate(zip(r["t"], r["e_t"]))]
    r["dw"], r["e_dw"] = G.weight_grad2(dz, [c[0] for c in cat], [c[1] for c in cat], exact)
    return r


def flat_params(mats, biases=None):
    """The module's flat layout: all matrices, then all biases."""
    return torch.cat([m.reshape(-1) for m in mats] + ([b.reshape(-1) for b in biases] if biases is not None else []))


# ---------------------------------------------------------------- exact data: every intermediate is a small integer

def exact_weights(family, n_in, n_out, width, n_hidden, skip_mask=0):
    """The families of mlp_reference for the H part of every layer; the x part of a cat layer is (a) 'perm': one signed entry
    per row, another column per layer; (b) 'dense': two or three entries of +-1 per row.  Layers >= 2 of a network with a
    skip are thinned once more (every other kept entry of the H part goes), since each cat layer feeds x in again and the
    magnitudes must stay integers that bf16 holds (|v| <= 256)."""
    base = R.exact_weights(family, n_in, n_out, width, n_hidden)
    ws = []
    for l, w in enumerate(base):
        if skip_mask and family == "dense" and l >= 2:
            o = torch.arange(w.shape[0]).view(-1, 1)
            i = torch.arange(w.shape[1]).view(1, -1)
            w = w * (((o + i) % 2) == 0)
        if is_cat(skip_mask, l):
            o = torch.arange(w.shape[0]).view(-1, 1)
            i = torch.arange(n_in).view(1, -1)
            if family == "perm":
                wx = (i == ((3 * o + l) % n_in)) * (1 - 2 * ((o + l) % 2))
            else:
                wx = (((7 * o + 3 * i + l) % max(n_in // 2, 1)) == 0) * (1 - 2 * ((o + i) % 2))
            w = torch.cat([w, wx.float()], 1)
        ws.append(w.float())
    return ws


def exact_biases(n_out, width, n_hidden):
    """Integer biases -2 .. 2, and -40 on one neuron in eight of the hidden layers: large enough to switch those neurons off,
    so that the masks differ from the bias-free network's."""
    bs = []
    for l in range(n_hidden + 1):
        o = torch.arange(n_out if l == n_hidden else width)
        b = (3 * o + l) % 5 - 2
        if l < n_hidden:
            b = torch.where(o % 8 == (5 + l) % 8, torch.full_like(b, -40), b)
        bs.append(b.float())
    return bs


def exact_case(family, dtype, width, n_hidden, cfg, bias, skip_layer, v_mod=3):
    """Everything the exact tests compare against, for one case of cfg = (N, n_in, n_out, x float32?, y and g float32?):
    (shape, skip_mask, ws, bs, x, g, v, forward, backward, second order).  Every rounding is asserted to be a no-op."""
    N, n_in, n_out, x_f32, out_f32 = cfg
    shape = (n_in, n_out, width, n_hidden)
    skip_mask = skip_mask_of(skip_layer, n_hidden)
    ws = exact_weights(family, *shape, skip_mask)
    bs = exact_biases(n_out, width, n_hidden) if bias else None
    x, g = R.exact_inputs(N, n_in, n_out, torch.float32 if x_f32 else dtype, torch.float32 if out_f32 else dtype)
    v = G.exact_tangent_input(N, n_in, x.dtype, v_mod)
    f = forward(x, ws, bs, skip_mask, dtype, out_f32, exact=True)
    b = backward(x, ws, f["hidden"], g, skip_mask, dtype, exact=True)
    s = second_order(v, ws, f["hidden"], b["dz"], skip_mask, dtype, out_f32, exact=True)
    return shape, skip_mask, ws, bs, x, g, v, f, b, s


# The covering set of the exact GPU and CPU tests: (family, width, n_hidden, skip_layer, bias, cfg).  cfg as above.
#   types: every case runs in fp16 and bf16;  widths 64 and 128;  N 1, 31, 32, 33, 129, 300 (two weight-gradient slices, the
#   second short);  n_in 5 (element-wise loads), 36 (three k-steps, the last partial, rows of 72 B: not 16-byte rows), 40
#   (16-byte rows), 150 with width 64 (five 32-column dx blocks, a cat layer of 214 inputs);  n_out 1, 3, 32;  float32 and half
#   ends;  bias only, skip only, both;  one inner cat layer (n_hidden 4, skip_layer 2), a cat OUTPUT layer (n_hidden 3,
#   skip_layer 2), three cat layers at once (n_hidden 4, skip_layer 1: 64 wide only, 128 wide they do not fit the LDS).
CASES = [
    # bias only
    ("dense", 64, 2, None, True, (1, 5, 1, True, True)),
    ("dense", 64, 1, None, True, (33, 36, 3, False, False)),
    ("perm", 128, 4, None, True, (129, 40, 32, False, True)),
    ("dense", 128, 2, None, True, (300, 36, 3, True, False)),
    # skip only
    ("perm", 64, 4, 2, False, (31, 36, 3, True, True)),
    ("dense", 64, 3, 2, False, (32, 40, 32, False, False)),
    ("dense", 64, 4, 1, False, (33, 5, 3, False, True)),
    ("dense", 128, 3, 1, False, (129, 40, 1, False, True)),    # 128 wide: an inner and the output layer take [H, x]
    ("dense", 64, 4, 2, False, (129, 150, 3, False, False)),
    # both
    ("dense", 64, 4, 2, True, (300, 36, 3, True, True)),       # the T-NeRF warp shape
    ("perm", 64, 4, 2, True, (129, 36, 3, False, False)),
    ("dense", 64, 3, 2, True, (129, 5, 32, True, False)),
    ("dense", 64, 3, 2, True, (31, 150, 1, False, True)),      # cat output layer of 214 inputs
    ("dense", 64, 4, 1, True, (300, 40, 3, False, False)),
    ("perm", 128, 3, 1, True, (32, 36, 32, True, True)),
    ("dense", 128, 3, 2, True, (1, 40, 1, False, False)),
    ("dense", 128, 4, 2, True, (300, 5, 3, False, True)),
    ("dense", 64, 4, 4, True, (33, 36, 3, False, False)),      # a skip_layer that selects nothing
]

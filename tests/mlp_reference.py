"""Float64 restatement of the fused MLP (nerfacc_amd/csrc/mlp.hip) with the kernels' rounding points and a derived error
bound per element, plus the integer-valued data on which every pass must agree bit for bit.

Rounding points: x and W to ``dtype``, every hidden activation after its ReLU, every dZ_l after its mask, y (unless it is
float32) and dL/dx as stored.  Roundings of INPUTS (x, W, g) are deterministic functions of the same float32 values on
both sides and carry no error.  The backward takes the hidden activations as an argument and never recomputes the ReLU mask.

Bound (forward propagation; layer l with K_l inputs, h with error e):
    e_pre  = |W| e + (K_l + 2) 2^-24 |W| |h|            float32 products are exact, the sum has K_l roundings
    e_next = e_pre + ulp_dtype(|z| + e_pre)             one whole ulp: a value near a tie may round to the neighbour
The backward products follow the same rule (K = the layer's outputs; K = N for the weight gradient, which stays float32).
"""
import torch

U32 = 2.0 ** -24
_MANT = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}
_EMIN = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}


def ulp(dtype, v):
    """Spacing of ``dtype`` at magnitude ``v`` (float64 tensor), the subnormal spacing below the smallest normal."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -200))).clamp_min(_EMIN[dtype])
    return torch.exp2(e - _MANT[dtype])


def rnd(t, dtype, exact=False):
    """``t`` (float64) rounded once to ``dtype``; with ``exact`` the rounding must be a no-op."""
    r = t.to(dtype).double()
    if exact:
        assert torch.equal(r, t), f"not exact in {dtype}: max |v| = {float(t.abs().max())}"
    return r + 0.0   # -0 -> +0: an MFMA accumulator that starts at +0 never ends at -0


def layer_dims(n_in, n_out, width, n_hidden):
    return list(zip([width] * n_hidden + [n_out], [n_in] + [width] * n_hidden))


def forward(x, weights, dtype, out_f32=False, exact=False):
    """x [N, n_in] (float32 or dtype), weights: float32 [out, in] each.  Returns dict(y, hidden=[H_l], e_y, e_hidden)."""
    h = rnd(x.double(), dtype, exact and x.dtype != torch.float32)
    if exact:
        assert torch.equal(h, x.double())
    e = torch.zeros_like(h)
    hidden, e_hidden = [], []
    for l, w in enumerate(weights):
        wq = rnd(w.double(), dtype, exact)
        z = h @ wq.t() + 0.0
        K = wq.shape[1]
        e_pre = e @ wq.abs().t() + (K + 2) * U32 * (h.abs() @ wq.abs().t())
        if exact:
            assert float((h.abs() @ wq.abs().t()).max()) < 2 ** 24
        if l < len(weights) - 1:
            h = rnd(torch.relu(z), dtype, exact)
            e = e_pre + ulp(dtype, z.abs() + e_pre)
            hidden.append(h)
            e_hidden.append(e)
        elif out_f32:
            y, e_y = z, e_pre
        else:
            y, e_y = rnd(z, dtype, exact), e_pre + ulp(dtype, z.abs() + e_pre)
    return dict(y=y, hidden=hidden, e_y=e_y, e_hidden=e_hidden)


def backward(x, weights, hidden, g, dtype, exact=False):
    """hidden: [H_l] as float64 values of ``dtype`` numbers (the forward's, or the kernel's own); g [N, n_out] float32 or
    dtype.  Returns dict(dx, e_dx, dz=[dZ_0 .. dZ_L], e_dz, dw=[dW_l], e_dw); dx rounded to x's dtype."""
    N = x.shape[0]
    xq = rnd(x.double(), dtype, exact)
    dz = rnd(g.double(), dtype, exact)
    e = torch.zeros_like(dz)
    L = len(weights)
    dzs, e_dzs, dws, e_dws = [dz], [e], [], []
    for l in range(L - 1, -1, -1):
        h_prev = hidden[l - 1] if l > 0 else xq
        dws.append(dz.t() @ h_prev + 0.0)
        s_abs = dz.abs().t() @ h_prev.abs()
        if exact:
            assert float(s_abs.max()) < 2 ** 24
        e_dws.append(e.t() @ h_prev.abs() + (N + 2) * U32 * s_abs + ulp(torch.float32, s_abs))
        wq = rnd(weights[l].double(), dtype, exact)
        dh = dz @ wq + 0.0
        K = wq.shape[0]
        e_pre = e @ wq.abs() + (K + 2) * U32 * (dz.abs() @ wq.abs())
        if l > 0:
            mask = (h_prev > 0).double()
            dz = rnd(torch.where(h_prev > 0, dh, torch.zeros_like(dh)), dtype, exact)   # a select
            e = (e_pre + ulp(dtype, dh.abs() + e_pre)) * mask
            dzs.append(dz)
            e_dzs.append(e)
        else:
            dx = rnd(dh, x.dtype, exact)
            e_dx = e_pre + ulp(x.dtype, dh.abs() + e_pre)
    return dict(dx=dx, e_dx=e_dx, dz=dzs[::-1], e_dz=e_dzs[::-1], dw=dws[::-1], e_dw=e_dws[::-1])


def flat(mats):
    return torch.cat([m.reshape(-1) for m in mats])


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0); the test asserts it is <= 1."""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0


# ---------------------------------------------------------------- exact data: every intermediate is a small integer

def exact_weights(family, n_in, n_out, width, n_hidden):
    """(a) 'perm': signed, scaled permutations, another permutation per layer: every output is one traceable input, so a
    wrong lane, register or k mapping shows.  (b) 'dense': asymmetric small integers ((3 o + 7 i + l) mod 5) - 2 (1 instead of 0), thinned to
    about three entries per row (eight in the last layer, so that a single output sees live neurons) so that magnitudes stay representable."""
    ws = []
    for l, (o_n, i_n) in enumerate(layer_dims(n_in, n_out, width, n_hidden)):
        o = torch.arange(o_n).view(-1, 1)
        i = torch.arange(i_n).view(1, -1)
        if family == "perm":
            col = ((5 + 6 * l) * o + 3 * l + 1) % i_n   # odd multiplier: a permutation of the columns when out == in == 64 / 128
            # one row in four negative in the first and the last layer: the zeros that the first ReLU makes travel through the
            # permutations of the layers between, so every layer's mask is exercised and a deep network stays alive
            sign = 1 - 2 * (((o + l) % 4 == 3) & (l in (0, n_hidden)))
            scale = 2 if l == 1 else 1
            w = (i == col) * sign * scale
        else:
            keep = ((5 * o + i + 2 * l) % max(i_n // (8 if l == n_hidden else 3), 1)) == 0
            v = ((3 * o + 7 * i + l) % 5) - 2
            w = torch.where(v == 0, torch.ones_like(v), v) * keep   # -2, -1, 1, 2: a kept entry is never zero
            if l >= 2:
                w = w.clamp(-1, 1)
        ws.append(w.float())
    return ws


def exact_inputs(N, n_in, n_out, x_dtype, g_dtype):
    n = torch.arange(N).view(-1, 1)
    x = ((3 * n + 5 * torch.arange(n_in).view(1, -1) + 3) % 7 - 1).to(x_dtype)   # -1 .. 5: mostly positive, so deep networks stay alive
    g = ((2 * n + 3 * torch.arange(n_out).view(1, -1)) % 5 - 2).to(g_dtype)
    return x, g


# ---------------------------------------------------------------- random data: the NGP networks

NGP_SHAPES = [(32, 16, 64, 1), (32, 3, 64, 2), (10, 1, 64, 1)]   # (n_in, n_out, width, n_hidden): base, head, proposal


def xavier_weights(n_in, n_out, width, n_hidden, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 for o, i in layer_dims(n_in, n_out, width, n_hidden)]

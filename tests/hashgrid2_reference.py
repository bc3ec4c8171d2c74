"""float64 restatement of the hash grid's second order (csrc/encoding.hip, "Second order"): the three gradients of
S = sum_n v[n] . g_x[n], where g_x is the first backward's dL/dx for the incoming dL/dy = g.

Per point n, level l (s = scale_l), corner c with bits b_d, signs sg_d = +-1, factors w_d = (b_d ? f_d : 1 - f_d) and
D_d(c) = sg_d prod_{e != d} w_e, T_c the corner's F parameters, g the point's piece of dL/dy of that level:

    a_c          = s sum_d v_d D_d(c)
    gg_y[n,l,j]  = sum_c a_c T_c[j]                                            (towards g)
    G2_T[idx_c]  += a_c g                                                      (towards params)
    x2[n,e]      = sum_l s^2 sum_c (sum_{d != e} v_d sg_d sg_e w_k) (g . T_c),  k the third dimension   (towards x)

The cell index and the fractions come from the float32 p = x * s + 0.5, as the kernels form them; everything after that is
float64.  With every output come, per element, the number of summed terms k and the sum of their magnitudes:
a term is one  s v_d D_d(c) T_c[j]  for gg_y (24 per element), one  s v_d D_d(c) g[j]  for G2_T (3 per point that touches
the entry with a corner; ``hits`` counts those touches), one  s^2 v_d sg_d sg_e w_k g[j] T_c[j]  for x2 (16 L F per element).
"""
import torch

M32 = 0xFFFFFFFF


def restate_grad2(x, params, enc, g, v):
    """x [N, 3] float32, params flat, g [N, L F], v [N, 3] (CPU tensors) -> dict of float64 tensors:
    gg_y, gg_y_k, gg_y_abs [N, L F];  g2_params, g2_params_k, g2_params_abs [n_params], hits [n_entries];
    x2, x2_k, x2_abs [N, 3]."""
    assert x.dtype == torch.float32
    L, F = enc.n_levels, enc.n_features_per_level
    N = x.shape[0]
    P = params.detach().double().view(-1, F)
    E = P.shape[0]
    g64, v64 = g.detach().double(), v.detach().double()
    gg_y = torch.zeros(N, L * F, dtype=torch.float64)
    gg_y_abs = torch.zeros_like(gg_y)
    gT = torch.zeros(E, F, dtype=torch.float64)
    gT_abs = torch.zeros_like(gT)
    hits = torch.zeros(E, dtype=torch.float64)
    x2 = torch.zeros(N, 3, dtype=torch.float64)
    x2_abs = torch.zeros_like(x2)
    for l in range(L):
        s = enc.scales[l]
        p = x * s + 0.5                      # float32, as the kernels form it
        fl = torch.floor(p)
        f = (p - fl).double()
        gi = fl.clamp(-2147483648.0, 2147483520.0).to(torch.int64) & M32
        size, res, off = enc.sizes[l], enc.resolutions[l], enc.offsets[l]
        gl = g64[:, l * F:(l + 1) * F]
        for c in range(8):
            b = [(c >> d) & 1 for d in range(3)]
            sg = [1.0 if b[d] else -1.0 for d in range(3)]
            q = [(gi[:, d] + b[d]) & M32 for d in range(3)]
            if enc.table.hashed[l]:
                idx = (q[0] ^ ((q[1] * 2654435761) & M32) ^ ((q[2] * 805459861) & M32)) & (size - 1)
            else:
                idx = ((q[0] + q[1] * res + q[2] * res * res) & M32) % size
            idx = off + idx
            w = [f[:, d] if b[d] else 1.0 - f[:, d] for d in range(3)]
            Tc = P[idx]                                                   # [N, F]
            # the three terms s v_d D_d(c) of a_c
            terms = [s * v64[:, d] * sg[d] * w[(d + 1) % 3] * w[(d + 2) % 3] for d in range(3)]
            a = terms[0] + terms[1] + terms[2]
            a_abs = terms[0].abs() + terms[1].abs() + terms[2].abs()
            gg_y[:, l * F:(l + 1) * F] += a[:, None] * Tc
            gg_y_abs[:, l * F:(l + 1) * F] += a_abs[:, None] * Tc.abs()
            gT.index_add_(0, idx, a[:, None] * gl)
            gT_abs.index_add_(0, idx, a_abs[:, None] * gl.abs())
            hits.index_add_(0, idx, torch.ones(N, dtype=torch.float64))
            dot = (gl * Tc).sum(-1)
            dot_abs = (gl * Tc).abs().sum(-1)
            for e in range(3):
                for d in range(3):
                    if d == e:
                        continue
                    k = 3 - d - e
                    m = (s * s) * v64[:, d] * sg[d] * sg[e] * w[k]
                    x2[:, e] += m * dot
                    x2_abs[:, e] += m.abs() * dot_abs
    return dict(
        gg_y=gg_y, gg_y_k=torch.full_like(gg_y, 24.0), gg_y_abs=gg_y_abs,
        g2_params=gT.view(-1), g2_params_k=(3.0 * hits).repeat_interleave(F), g2_params_abs=gT_abs.view(-1), hits=hits,
        x2=x2, x2_k=torch.full_like(x2, 16.0 * L * F), x2_abs=x2_abs)


def interior_points(n, enc, seed, lo=0.0, hi=1.0, margin=1e-3, grid=None):
    """n points of [lo, hi)^3 whose float32 p = x * scale_l + 0.5 stays at least ``margin`` of a cell away from every cell
    boundary of every level (rejection-sampled).  With ``grid`` the coordinates are multiples of 1 / grid."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    have = 0
    while have < n:
        x = torch.rand(2 * n + 16, 3, generator=gen) * (hi - lo) + lo
        if grid is not None:
            x = torch.floor(x * grid) / grid
        ok = torch.ones(x.shape[0], dtype=torch.bool)
        for s in enc.scales:
            p = x * s + 0.5
            f = p - torch.floor(p)
            ok &= ((f >= margin) & (f <= 1.0 - margin)).all(-1)
        out.append(x[ok])
        have += int(ok.sum())
    return torch.cat(out)[:n].contiguous()

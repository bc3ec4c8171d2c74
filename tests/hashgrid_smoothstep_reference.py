"""Restatements of the hash grid with ``interpolation="Smoothstep"`` (csrc/encoding.hip, "Smoothstep interpolation"), in the
conventions of tests/hashgrid2_reference.py (float64, with the number of summed terms and the sum of their magnitudes per
output element) and tests/hashgrid_sorted_reference.py (numpy float32, the sorted table gradient in its documented order).

Per point, level l (s = scale_l) and dimension d, from the float32 fraction f_d of p_d = x_d * s + 0.5, in float32 and in
exactly the kernels' operations:

    S_d = (f_d * f_d) * (3 - 2 * f_d),   S'_d = (6 * f_d) * (1 - f_d),   S''_d = 6 - 12 * f_d,   w_d = (c_d ? S_d : 1 - S_d)

The float64 restatement takes these float32 values (1 - S included: it cancels near f -> 1, and a float64 factor would make a
comparison measure that rounding instead of the kernel) and does everything after them in float64.  With sg_d = +-1 by the
corner bit, T_c the corner's F parameters, g the point's piece of dL/dy and dot_c = g . T_c:

    y[n,l,j]     = sum_c w_0 w_1 w_2 T_c[j]
    G_T[idx_c]  += w_0 w_1 w_2 g                                      (1 term per touching corner)
    g_x[n,d]     = sum_l s S'_d sum_c sg_d prod_{e != d} w_e dot_c
    a_c          = s sum_d v_d sg_d S'_d prod_{e != d} w_e
    gg_y[n,l,j]  = sum_c a_c T_c[j]                                   (24 terms per element)
    G2_T[idx_c] += a_c g                                              (3 terms per touching corner)
    x2[n,e]      = sum_l s^2 sum_c dot_c [sum_{d != e} v_d sg_d S'_d sg_e S'_e w_k + v_e sg_e S''_e prod_{k != e} w_k]
                                                                      (24 L F terms per element; the linear grid has 16 L F)
"""
import numpy as np
import torch

from hashgrid2_reference import interior_points  # noqa: F401  (the tests take it from here)
from hashgrid_sorted_reference import NS, _ordered_sum, check_bound, configs, make_inputs  # noqa: F401

TILE = 256
M32 = 0xFFFFFFFF
P1, P2 = 2654435761, 805459861


def grids():
    """configs() and, for a grid with four features per level, the F4_L3 grid of tests/test_hashgrid_grad2_gpu.py."""
    return dict(configs(), F4_L3=(3, 4, 14, 16, 2.0))


def make_grid(kind, out_dtype=None, deterministic=False, interpolation="Smoothstep"):
    """The grid of hashgrid_sorted_reference.make_grid (same seed, same table) with an interpolation."""
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(0)
    L, F, log2, base, scale = grids()[kind]
    enc = HashGridEncoding(3, L, F, log2, base, scale, out_dtype=out_dtype, deterministic=deterministic,
                           interpolation=interpolation)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    return enc


def face_points(enc, d, n=64):
    """n float32 points of a one-level grid whose fraction along d is exactly 0 (x_d * scale + 0.5 an integer)."""
    s = enc.scales[0]
    x = torch.rand(n, 3, generator=torch.Generator().manual_seed(d)) * 1.5 - 0.25
    k = torch.arange(0, int(s) + 2, dtype=torch.float32)
    c = (k - 0.5) / s
    c = c[(c * s + 0.5) == torch.floor(c * s + 0.5)]
    assert c.numel() > 4
    x[:, d] = c[torch.arange(n) % c.numel()]
    p = x[:, d] * s + 0.5
    assert bool((p - torch.floor(p) == 0).all())
    return x


def level_cell(x, enc, l):
    """x [N, 3] float32 tensor -> (gi int64 [N, 3] cell, S, S1, S2 float32 [N, 3]) of level l, formed as the kernels do."""
    assert x.dtype == torch.float32
    p = x * enc.scales[l] + 0.5
    fl = torch.floor(p)
    f = p - fl
    gi = fl.clamp(-2147483648.0, 2147483520.0).to(torch.int64) & M32
    S = (f * f) * (3.0 - 2.0 * f)
    S1 = (6.0 * f) * (1.0 - f)
    S2 = 6.0 - 12.0 * f
    assert S.dtype == S1.dtype == S2.dtype == torch.float32
    return gi, S, S1, S2


def corner_index(gi, b, enc, l):
    size, res = enc.sizes[l], min(enc.resolutions[l], 1 << 30)
    q = [(gi[:, d] + b[d]) & M32 for d in range(3)]
    if enc.table.hashed[l]:
        return (q[0] ^ ((q[1] * P1) & M32) ^ ((q[2] * P2) & M32)) & (size - 1)
    return ((q[0] + ((q[1] * res) & M32) + ((q[2] * ((res * res) & M32)) & M32)) & M32) % size


def restate(x, params, enc, g, v=None):
    """x [N, 3] float32, params flat, g [N, L F], v [N, 3] or None (CPU tensors) -> dict of float64 tensors:
    y [N, L F];  g_params, g_params_abs [n_params], hits [n_entries] (first order: one term per touch);  g_x [N, 3];
    and with v:  gg_y, gg_y_k, gg_y_abs [N, L F];  g2_params, g2_params_k, g2_params_abs [n_params];  x2, x2_k, x2_abs [N, 3]."""
    L, F = enc.n_levels, enc.n_features_per_level
    N = x.shape[0]
    P = params.detach().double().view(-1, F)
    E = P.shape[0]
    g64 = g.detach().double()
    v64 = None if v is None else v.detach().double()
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)   # noqa: E731
    y, gT, gT_abs, hits, g_x = z(N, L * F), z(E, F), z(E, F), z(E), z(N, 3)
    gg_y, gg_y_abs, g2T, g2T_abs, x2, x2_abs = z(N, L * F), z(N, L * F), z(E, F), z(E, F), z(N, 3), z(N, 3)
    for l in range(L):
        s = enc.scales[l]
        gi, S, S1, S2 = level_cell(x, enc, l)
        one_minus_S = 1.0 - S                                   # float32, as the kernels form it
        S1, S2 = S1.double(), S2.double()
        gl = g64[:, l * F:(l + 1) * F]
        sl = slice(l * F, (l + 1) * F)
        for c in range(8):
            b = [(c >> d) & 1 for d in range(3)]
            sg = [1.0 if b[d] else -1.0 for d in range(3)]
            idx = enc.offsets[l] + corner_index(gi, b, enc, l)
            w = [(S[:, d] if b[d] else one_minus_S[:, d]).double() for d in range(3)]
            Tc = P[idx]
            wc = w[0] * w[1] * w[2]
            y[:, sl] += wc[:, None] * Tc
            gT.index_add_(0, idx, wc[:, None] * gl)
            gT_abs.index_add_(0, idx, (wc[:, None] * gl).abs())
            hits.index_add_(0, idx, torch.ones(N, dtype=torch.float64))
            dot = (gl * Tc).sum(-1)
            dot_abs = (gl * Tc).abs().sum(-1)
            for d in range(3):
                g_x[:, d] += s * S1[:, d] * sg[d] * w[(d + 1) % 3] * w[(d + 2) % 3] * dot
            if v is None:
                continue
            u = [v64[:, d] * sg[d] * S1[:, d] for d in range(3)]
            terms = [s * u[d] * w[(d + 1) % 3] * w[(d + 2) % 3] for d in range(3)]
            a = terms[0] + terms[1] + terms[2]
            a_abs = terms[0].abs() + terms[1].abs() + terms[2].abs()
            gg_y[:, sl] += a[:, None] * Tc
            gg_y_abs[:, sl] += a_abs[:, None] * Tc.abs()
            g2T.index_add_(0, idx, a[:, None] * gl)
            g2T_abs.index_add_(0, idx, a_abs[:, None] * gl.abs())
            for e in range(3):
                ka, kb = [k for k in range(3) if k != e]
                for d, k in ((ka, kb), (kb, ka)):                               # the mixed partials
                    m = (s * s) * u[d] * sg[e] * S1[:, e] * w[k]
                    x2[:, e] += m * dot
                    x2_abs[:, e] += m.abs() * dot_abs
                m = (s * s) * v64[:, e] * sg[e] * S2[:, e] * w[ka] * w[kb]     # the pure second partial
                x2[:, e] += m * dot
                x2_abs[:, e] += m.abs() * dot_abs
    out = dict(y=y, g_params=gT.view(-1), g_params_abs=gT_abs.view(-1), hits=hits, g_x=g_x)
    if v is not None:
        out.update(gg_y=gg_y, gg_y_k=torch.full_like(gg_y, 24.0), gg_y_abs=gg_y_abs,
                   g2_params=g2T.view(-1), g2_params_k=(3.0 * hits).repeat_interleave(F), g2_params_abs=g2T_abs.view(-1),
                   x2=x2, x2_k=torch.full_like(x2, 24.0 * L * F), x2_abs=x2_abs)
    return out


# ---------------------------------------------------------------- the sorted table gradient, numpy float32
def _terms(x, enc, l, g, v):
    """keys [8 N] in item order i = 8 n + c, float32 terms [8 N, F] with the pinned coefficient expressions, the float64
    terms and their magnitudes [8 N, F] of level l; v None: first order."""
    f32 = np.float32
    F = enc.n_features_per_level
    N = x.shape[0]
    s = f32(enc.scales[l])
    gi, S, S1, _ = level_cell(torch.from_numpy(x), enc, l)
    S, S1 = S.numpy(), S1.numpy()
    assert S.dtype == np.float32
    c = np.arange(8)
    bits = [((c >> d) & 1).astype(bool)[None, :] for d in range(3)]                      # [1, 8]
    key = torch.stack([corner_index(gi, [(k >> d) & 1 for d in range(3)], enc, l) for k in range(8)], 1).numpy()
    w = [np.where(bits[d], S[:, d:d + 1], f32(1.0) - S[:, d:d + 1]).astype(f32).reshape(-1) for d in range(3)]
    gl = np.repeat(g[:, l * F:(l + 1) * F], 8, axis=0)
    w64 = [a.astype(np.float64) for a in w]
    g64 = gl.astype(np.float64)
    if v is None:
        coef = (w[0] * w[1]) * w[2]
        t64 = (w64[0] * w64[1] * w64[2])[:, None] * g64
        return key.reshape(-1), coef[:, None] * gl, t64, np.abs(t64)
    u = [(np.where(bits[d], v[:, d:d + 1], -v[:, d:d + 1]).astype(f32) * S1[:, d:d + 1]).astype(f32).reshape(-1)
         for d in range(3)]
    coef = ((u[0] * (w[1] * w[2]) + u[1] * (w[0] * w[2])) + u[2] * (w[0] * w[1])) * s
    assert coef.dtype == np.float32
    parts = [float(s) * u[d].astype(np.float64) * w64[(d + 1) % 3] * w64[(d + 2) % 3] for d in range(3)]
    t64 = (parts[0] + parts[1] + parts[2])[:, None] * g64
    tabs = (np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2]))[:, None] * np.abs(g64)
    return key.reshape(-1), coef[:, None] * gl, t64, tabs


def sorted_table_grad(x, enc, g, v=None):
    """hashgrid_sorted_reference.sorted_table_grad with the smoothstep terms: the same items, stable sort, tiles of 256,
    segment sums left to right and run sums in tile order.  Returns (grad float32 [n_params], info)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    v = None if v is None else np.ascontiguousarray(v, dtype=np.float32)
    F = enc.n_features_per_level
    grad = np.zeros((enc.table.n_entries, F), dtype=np.float32)
    entries, sums, absums, cnts = [], [], [], []
    if x.shape[0] == 0:
        z = np.zeros((0, F))
        return grad.reshape(-1), dict(entry=np.zeros(0, np.int64), sum64=z, abs64=z, cnt=np.zeros(0, np.int64))
    for l in range(enc.n_levels):
        key, t32, t64, tabs = _terms(x, enc, l, g, v)
        assert t32.dtype == np.float32
        order = np.argsort(key, kind="stable")
        key, t32, t64, tabs = key[order], t32[order], t64[order], tabs[order]
        M = key.shape[0]
        run_start = np.ones(M, dtype=bool)
        run_start[1:] = key[1:] != key[:-1]
        seg_start = np.nonzero(run_start | (np.arange(M) % TILE == 0))[0]
        seg_sum = _ordered_sum(t32, seg_start, np.diff(np.append(seg_start, M)))
        first_seg = np.nonzero(run_start[seg_start])[0]
        run_sum = _ordered_sum(seg_sum, first_seg, np.diff(np.append(first_seg, seg_start.shape[0])))
        rs = np.nonzero(run_start)[0]
        grad[enc.offsets[l] + key[rs]] = run_sum
        entries.append(enc.offsets[l] + key[rs])
        sums.append(np.add.reduceat(t64, rs, axis=0))
        absums.append(np.add.reduceat(tabs, rs, axis=0))
        cnts.append(np.diff(np.append(rs, M)))
    return grad.reshape(-1), dict(entry=np.concatenate(entries), sum64=np.concatenate(sums), abs64=np.concatenate(absums),
                                  cnt=np.concatenate(cnts))

"""float64 / numpy restatement of the hash grid for any number of input dimensions D, written from the definition in
csrc/encoding.hip's header ("Other dimensions"), not from ``nerfacc_amd.encodings._hashgrid_torch``:

    p_d = x_d * scale_l + 0.5 (float32, two roundings), g_d = (uint32)(int32)clamp(floor p_d), f_d = p_d - floor p_d (float32);
    under Smoothstep S_d = (f_d f_d)(3 - 2 f_d) and S'_d = (6 f_d)(1 - f_d) in float32 as the kernels form them, then widened;
    corner c = sum_d c_d 2^d in the order 0 .. 2^D - 1, q_d = g_d + c_d (uint32, wrapping);
    dense:  idx = (sum_d q_d res^d mod 2^32) mod size;   hashed: idx = (q_0 ^ q_1 P_1 ^ q_2 P_2 ^ q_3 P_3) & (size - 1);
    size_l = min(roundup8(res_l^D), 2^log2), hashed when roundup8(res_l^D) is the larger;
    w_c = prod_d (c_d ? f_d : 1 - f_d);  y = sum_c w_c T_c;  table-gradient term w_c g;
    dL/dx_e = s (S'_e) sum_c (c_e ? + : -) (prod_{d != e} w_d) dot_c.

Holds the level table, the forward, the gradients with per-entry count and sum |term|, and the sorted order of the
reproducible table gradient for items 2^D n + c (tests/hashgrid_sorted_reference.py's order, any D).
"""
import ctypes
import ctypes.util
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PRIMES = (1, 2654435761, 805459861, 3674653429)
TILE = 256
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp2f.restype = _libm.log2f.restype = ctypes.c_float
_libm.exp2f.argtypes = _libm.log2f.argtypes = [ctypes.c_float]


class Table:
    """The level table of a D-dimensional grid: scales (float32 values), resolutions, sizes, offsets, hashed."""

    def __init__(self, n_dims, n_levels, n_features, log2, base, scale):
        f32 = np.float32
        self.D, self.L, self.F, self.log2 = n_dims, n_levels, n_features, log2
        lg = f32(_libm.log2f(float(f32(scale))))
        self.scales, self.res, self.sizes, self.offsets, self.hashed = [], [], [], [], []
        off = 0
        for l in range(n_levels):
            s = f32(f32(_libm.exp2f(float(f32(f32(l) * lg)))) * f32(base)) - f32(1.0)
            r = int(math.ceil(float(s))) + 1
            dense = (r ** n_dims + 7) // 8 * 8
            self.scales.append(f32(s))
            self.res.append(r)
            self.sizes.append(min(dense, 1 << log2))
            self.hashed.append(dense > (1 << log2))
            self.offsets.append(off)
            off += self.sizes[-1]
        self.n_entries = off


def table_of(enc):
    return Table(enc.n_input_dims, enc.n_levels, enc.n_features_per_level, enc.log2_hashmap_size, enc.base_resolution,
                 enc.per_level_scale)


def scratch_bytes(n_dims, n_points, n_levels):
    """The documented formula of nfa_hashgrid_sorted_scratch_bytes_d."""
    if n_points <= 0:
        return 0
    m = (1 << n_dims) * n_points
    level = 16 * m + 1024 * ((m + 4095) // 4096 + 1) + 64 * ((m + 255) // 256)
    return n_levels * level if n_levels * level <= 1 << 29 else max(1 << 29, level)


def _level(x, t, l, smooth):
    """Per level: idx [N, 2^D] int64, w [D][N, 2^D] float32 factors, d1 [N, D] float32 (S', ones for Linear), bits."""
    D = t.D
    s = t.scales[l]
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x * s).astype(np.float32) + np.float32(0.5)
        fl = np.floor(p)
        f = (p - fl).astype(np.float32)
        cl = np.where(np.isnan(fl), np.float32(-2147483648.0), np.clip(fl, np.float32(-2147483648.0), np.float32(2147483520.0)))
        g = cl.astype(np.int64).astype(np.uint64) & M32
        d1 = np.ones_like(f)
        if smooth:
            d1 = ((np.float32(6.0) * f) * (np.float32(1.0) - f)).astype(np.float32)
            f = ((f * f) * (np.float32(3.0) - np.float32(2.0) * f)).astype(np.float32)
    c = np.arange(1 << D, dtype=np.uint64)[None, :]
    bits = [((c >> np.uint64(d)) & np.uint64(1)) for d in range(D)]
    q = [(g[:, d:d + 1] + bits[d]) & M32 for d in range(D)]
    size = np.uint64(t.sizes[l])
    if t.hashed[l]:
        idx = q[0]
        for d in range(1, D):
            idx = idx ^ ((q[d] * np.uint64(PRIMES[d])) & M32)
        idx = idx & (size - np.uint64(1))
    else:
        idx, power = q[0], np.uint64(t.res[l]) & M32
        for d in range(1, D):
            idx = (idx + ((q[d] * power) & M32)) & M32
            power = (power * (np.uint64(t.res[l]) & M32)) & M32
        idx = idx % size
    with np.errstate(invalid="ignore"):
        w = [np.where(bits[d].astype(bool), f[:, d:d + 1], np.float32(1.0) - f[:, d:d + 1]).astype(np.float32) for d in range(D)]
    return idx.astype(np.int64), w, d1, [b.astype(bool) for b in bits]


def forward(x, params, t, smooth=False):
    """float64 [N, L F]: weights from the float32 factors widened, products and sums in float64."""
    x = np.ascontiguousarray(x, np.float32)
    P = np.asarray(params, np.float64).reshape(-1, t.F)
    out = np.zeros((x.shape[0], t.L * t.F))
    for l in range(t.L):
        idx, w, _, _ = _level(x, t, l, smooth)
        wc = np.ones(idx.shape)
        for d in range(t.D):
            wc = wc * w[d].astype(np.float64)
        out[:, l * t.F:(l + 1) * t.F] = (wc[:, :, None] * P[t.offsets[l] + idx]).sum(1)
    return out


def grads(x, params, t, g, smooth=False):
    """(sum64 [E, F], cnt [E], abs64 [E, F], gx [N, D]): float64 table gradient, per-entry contribution count and
    sum |term|, and dL/dx, from the float32 cell coordinates (and float32 S, S') widened."""
    x = np.ascontiguousarray(x, np.float32)
    P = np.asarray(params, np.float64).reshape(-1, t.F)
    g = np.asarray(g, np.float64)
    gp = np.zeros((t.n_entries, t.F))
    ab = np.zeros((t.n_entries, t.F))
    cnt = np.zeros(t.n_entries)
    gx = np.zeros((x.shape[0], t.D))
    for l in range(t.L):
        idx, w, d1, bits = _level(x, t, l, smooth)
        w64 = [a.astype(np.float64) for a in w]
        gl = g[:, l * t.F:(l + 1) * t.F]
        wc = np.ones(idx.shape)
        for d in range(t.D):
            wc = wc * w64[d]
        term = wc[:, :, None] * gl[:, None, :]
        e = (t.offsets[l] + idx).reshape(-1)
        np.add.at(gp, e, term.reshape(-1, t.F))
        np.add.at(ab, e, np.abs(term).reshape(-1, t.F))
        np.add.at(cnt, e, 1.0)
        dot = (gl[:, None, :] * P[t.offsets[l] + idx]).sum(-1)
        for a in range(t.D):
            o = np.ones(idx.shape)
            for d in range(t.D):
                if d != a:
                    o = o * w64[d]
            sign = np.where(bits[a], 1.0, -1.0)
            gx[:, a] += (sign * o * dot).sum(1) * d1[:, a].astype(np.float64) * float(t.scales[l])
    return gp, cnt, ab, gx


def _ordered_sum(term, start, length):
    acc = term[start].copy()
    for p in range(1, int(length.max()) if length.size else 0):
        live = np.nonzero(length > p)[0]
        acc[live] = acc[live] + term[start[live] + p]
    return acc


def sorted_table_grad(x, t, g, smooth=False):
    """The reproducible table gradient in float32 with the documented order of additions: items i = 2^D n + c, stable sort
    by entry, tiles of 256 sorted items, segments summed left to right from their first term, a run across tile borders the
    sum of its segments' sums in tile order.  x [N, D] float32, g [N, L F] float32 (a half gradient: widened exactly)."""
    x = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(g, np.float32)
    grad = np.zeros((t.n_entries, t.F), np.float32)
    if x.shape[0] == 0:
        return grad.reshape(-1)
    C = 1 << t.D
    for l in range(t.L):
        idx, w, _, _ = _level(x, t, l, smooth)
        coef = w[0]
        for d in range(1, t.D):
            coef = (coef * w[d]).astype(np.float32)                      # ((w0 w1) w2) w3, float32
        key = idx.reshape(-1)
        t32 = (coef.reshape(-1)[:, None] * np.repeat(g[:, l * t.F:(l + 1) * t.F], C, axis=0)).astype(np.float32)
        order = np.argsort(key, kind="stable")
        key, t32 = key[order], t32[order]
        M = key.shape[0]
        run_start = np.ones(M, bool)
        run_start[1:] = key[1:] != key[:-1]
        seg_start = np.nonzero(run_start | (np.arange(M) % TILE == 0))[0]
        seg_sum = _ordered_sum(t32, seg_start, np.diff(np.append(seg_start, M)))
        first_seg = np.nonzero(run_start[seg_start])[0]
        run_sum = _ordered_sum(seg_sum, first_seg, np.diff(np.append(first_seg, seg_start.shape[0])))
        grad[t.offsets[l] + key[run_start]] = run_sum
    return grad.reshape(-1)


# ---------------------------------------------------------------- the grids and points both tiers use
# name: (D, n_levels, F, log2, base, scale).  The first five are the pinned level tables of tests/test_hashgrid_nd_cpu.py.
GRIDS = {
    "d2_boundary": (2, 6, 2, 12, 16, 2.0),      # level 2 dense with res^2 == 2^12; hashed from level 3
    "d2_odd": (2, 4, 4, 14, 10.5, 1.5),         # 11^2 = 121 padded to 128
    "d4_mixed": (4, 5, 1, 12, 4, 1.5),          # hashed from level 2
    "d4_edge": (4, 3, 8, 12, 8, 1.0),           # every level 8^4 = 2^12: dense, on the boundary
    "d4_last_hashed": (4, 3, 4, 14, 4.5, 1.7),  # 5^4 = 625 padded to 632; only the last level hashed
    "d2_L32": (2, 32, 1, 10, 4, 1.3),           # 2 points per wave
    "d4_L24": (4, 24, 2, 10, 2, 1.2),           # 16 idle lanes; levels of 16 entries
    "d2_wide": (2, 3, 8, 12, 16, 2.0),          # F = 8 at D = 2
    "d2_collide": (2, 2, 2, 10, 64, 2.0),       # both levels hashed into 1,024 entries
    "d4_collide": (4, 2, 2, 10, 64, 2.0),
}


def make_grid(name, interpolation="Linear", out_dtype=None, deterministic=False):
    import torch
    from nerfacc_amd.encodings import HashGridEncoding
    D, L, F, log2, base, scale = GRIDS[name]
    torch.manual_seed(0)
    enc = HashGridEncoding(D, L, F, log2, base, scale, out_dtype=out_dtype, deterministic=deterministic,
                           interpolation=interpolation)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    return enc


def make_points(n, enc, seed, same_point=False):
    """x [n, D] float32: uniform in [0, 1]^D; row 0 huge coordinates; from row 1 on rows on cell faces of every level
    (x * scale_l + 0.5 an integer in float32) and at 0.0 and 1.0 (with_cell_boundaries of test_encodings_gpu.py, any D);
    the LAST n // 8 rows uniform in [-2, 3]^D (cells below -1 and far above res: q wraps in uint32 on dense and hashed
    levels).  The face rows never reach the out-of-range block: ``point_census`` counts both, and the CPU tier asserts it."""
    import torch
    D = enc.n_input_dims
    gen = torch.Generator().manual_seed(seed)
    if same_point:
        return torch.tensor([0.3217, 0.6127, 0.4519, 0.7731][:D]).repeat(n, 1)
    x = torch.rand(n, D, generator=gen)
    far = n // 8 if n > 8 else 0
    if far:
        x[n - far:] = torch.rand(far, D, generator=gen) * 5.0 - 2.0
        x[0] = torch.tensor([1e6, -1e7, 3e9, -2e5][:D])
    rows = []
    for s in enc.scales:
        k = torch.arange(0, int(s) + 2, dtype=torch.float32)
        c = (k - 0.5) / s                                        # (and its float32 neighbours: one of the three usually hits)
        c = torch.cat([c, torch.nextafter(c, c + 1.0), torch.nextafter(c, c - 1.0)])
        c = c[(c * s + 0.5) == torch.floor(c * s + 0.5)]
        if c.numel():
            rows.append(c[torch.randint(0, c.numel(), (max(n // (4 * len(enc.scales)), 1), D), generator=gen)])
    rows.append(torch.tensor([[1.0] * D, [1.0, 0.0, 0.5, 0.0][:D], [0.0] * D]))
    b = torch.cat(rows)[: max(n - 1 - far, 1)]
    if n > 1:
        x[1: 1 + b.shape[0]] = b[: n - 1 - far]
    else:
        x[0] = torch.tensor([1.0] * D)
    return x


def point_census(x, enc):
    """(rows of the out-of-range block, the last n // 8, with a coordinate outside [0, 1]; of those the rows with a coordinate at
    least half the box's width outside it, below -0.5 or above 1.5: cells below -1 and past res on every level of scale >= 3;
    per level the rows between row 0 and that block with every coordinate on a cell face)."""
    import torch
    n = x.shape[0]
    far = n // 8 if n > 8 else 0
    r = x[n - far:]
    outside = ((r < 0.0) | (r > 1.0)).any(-1)
    deep = (r < -0.5).any(-1) | (r > 1.5).any(-1)
    faces = []
    for s in enc.scales:
        p = x[1: n - far] * s + 0.5
        faces.append(int((p == torch.floor(p)).all(-1).sum()))
    return int(outside.sum()), int((outside & deep).sum()), faces

// encoding.hip -- input encodings of Instant-NGP radiance fields: the multiresolution hash grid (D = 2, 3 or 4 input
// dimensions, linear or smoothstep interpolation) and the spherical-harmonics direction encoding, as tiny-cuda-nn's
// `HashGrid` and `SphericalHarmonics` define them (Mueller et al. 2022, "Instant Neural Graphics Primitives", sec. 3).
//
// The formulas below are written out for D = 3; "Other dimensions" after them states what D = 2 and D = 4 change.  D is a
// template parameter of every step that depends on it; the second order is D = 3 only.
//
// Hash grid, per point x and level l (all integer arithmetic uint32, wrapping):
//   p_d = x_d * scale_l + 0.5 (a multiply, then an add: the library builds with -ffp-contract=off)
//   g_d = (uint32)(int32)floor(p_d) (floor clamped to [-2^31, 2^31 - 128] first, so every finite input converts),
//   f_d = p_d - floor(p_d)
//   corner c = c0 + 2 c1 + 4 c2 in the order 0..7, q_d = g_d + c_d:
//     dense level:  idx = (q0 + q1 res + q2 res^2) mod size_l
//     hashed level: idx = (q0 ^ q1 * 2654435761 ^ q2 * 805459861) & (size_l - 1)
//     w_c = ((c0 ? f0 : 1 - f0) * (c1 ? f1 : 1 - f1)) * (c2 ? f2 : 1 - f2)
//   y[n, l F + j] = sum_c w_c params[(offset_l + idx_c) F + j], summed from 0 in corner order.
// Every index is reduced modulo the level's size, so any input (NaN and inf included) reads and writes inside the table.
// nerfacc_amd/encodings.py restates the same operations in torch, bit for bit.
//
// Layout: the forward runs one level per workgroup row and one lane per point; the backward one lane per (point, level),
// the level varying fastest inside a wave, so a wave covers 64 / L points x all L levels (64 mod L lanes idle).  A
// corner's F features are one vector load (F = 2: float2).  The per-level constants are a kernarg table.
// The backward scatters w_c * dL/dy with no-return global_atomic_add_f32 into a zeroed float32 table gradient; dL/dx
// (optional) is formed per (point, level) and summed over the point's levels in level order across lanes, so it is
// bitwise reproducible.
// The `_sorted` entries form the same table gradient (of both orders) without float atomics, by a stable sort of the (point,
// corner) items by entry and a segmented sum in a fixed order: "reproducible table gradient" below.
//
// Second order (hashgrid_bwd_bwd_kernel): the derivative of the backward's dL/dx output.  With g the point's dL/dy piece of the
// level, v = gg_x[n] the gradient that arrives for dL/dx[n], s = scale_l, w_d = (c_d ? f_d : 1 - f_d), u_d = (c_d ? v_d : -v_d)
// and T_c the corner's F parameters, per corner in the order 0..7:
//   a_c = ((u_0 * (w_1 * w_2) + u_1 * (w_0 * w_2)) + u_2 * (w_0 * w_1)) * s
//   gg_y[n, l F + j] = sum_c a_c * T_c[j], summed from 0 in corner order           (towards dL/dy; element type of dL/dy)
//   G2_T[idx_c][j]  += a_c * g[j]                                                   (towards params; float atomics as above)
//   dot_c = sum_j g[j] * T_c[j] from 0 in feature order;
//   h_0 = (u_1 * w_2 + u_2 * w_1) * dot_c, h_1 = (u_0 * w_2 + u_2 * w_0) * dot_c, h_2 = (u_0 * w_1 + u_1 * w_0) * dot_c
//   x2_l[e] = ((sum_c (c_e ? + : -) h_e) * s) * s;  x2[n, e] = sum_l x2_l[e] in level order across lanes (towards x)
// x2 has mixed partials only (linear interpolation has no pure second derivative); floor() contributes no gradient and the
// cell is the one locate() gives.  Same lane layout as the backward; each output is optional, and the corner parameters are
// read only for gg_y and x2.
//
// Smoothstep interpolation (NFA_INTERP_SMOOTHSTEP; tiny-cuda-nn's "interpolation": "Smoothstep"): everything up to f_d, g_d and
// the corner index is as above.  Per dimension d of a (point, level), float32, formed once in exactly these operations:
//   S_d = (f_d * f_d) * (3 - 2 * f_d),   S'_d = (6 * f_d) * (1 - f_d),   S''_d = 6 - 12 * f_d
//   w_d = (c_d ? S_d : 1 - S_d)                                    (replaces c_d ? f_d : 1 - f_d everywhere above)
//   forward:   w_c = (w_0 * w_1) * w_2 and the sum over the corners as above; the table gradient term is w_c * g[j].
//   backward:  the corner sum of dL/dx_d as above (sign of c_d, the two other factors, dot_c), then dL/dx_d = (sum * S'_d) * s,
//              summed over the levels as above.  S'(0) = 0: dL/dx_d vanishes on the cell faces of a level, the grid is C^1.
//   second order: u_d = (c_d ? v_d : -v_d) * S'_d (one multiply; the kernels form v_d * S'_d once and negate, the same bits);
//              a_c, gg_y and G2_T as above with this u_d;
//              h_e = (S'_e * (u_a * w_b + u_b * w_a) + (v_e * S''_e) * (w_a * w_b)) * dot_c, (a, b) = (1, 2), (0, 2), (0, 1)
//              for e = 0, 1, 2, with v_e * S''_e formed once per (point, level);
//              x2_l[e] = ((sum_c (c_e ? + : -) h_e) * s) * s, summed over the levels as above.
//              The second summand of h_e is the pure second partial d2/dx_e2 that the linear grid lacks.
// The interpolation is a template parameter of the kernels that form a weight (forward, backward, second order, hs_term of the
// sorted path); the Linear instantiations are the code they were before it existed.
//
// Other dimensions (D = 2, 4; forward, first-order backward and the sorted table gradient).  x is [N, D], contiguous and
// 16-byte aligned, a point being one 8-byte (D = 2) or 16-byte (D = 4) load; p_d, g_d, f_d (and S_d, S'_d) per dimension as above.
//   corner c = sum_d c_d 2^d in the order 0 .. 2^D - 1, q_d = g_d + c_d
//     dense level:  idx = (sum_d q_d res^d mod 2^32) mod size_l, the powers formed as wrapping products and the sum taken in
//                   ascending d
//     hashed level: idx = (q0 ^ q1 * 2654435761 ^ q2 * 805459861 ^ q3 * 3674653429) & (size_l - 1), the first D terms
//                   (tiny-cuda-nn's primes of dimensions 0..3)
//     size_l = min(roundup8(res_l^D), 2^log2_hashmap_size), hashed when roundup8(res_l^D) is the larger; scale_l and res_l
//                   do not depend on D
//     w_c = ((w_0 * w_1) * w_2) * w_3, the left-associated product of the first D factors
//   forward and table-gradient term as above over the 2^D corners.
//   dL/dx_e: per corner (sign of c_e) (prod_{d != e} w_d) * dot_c, the product over the other dimensions in ascending d,
//     left-associated; then the corner sum * s (Linear) or (* S'_e) * s (Smoothstep), summed over the levels as above.
//   The sorted path numbers its items i = 2^D n + c (2^D n_points < 2^32) and is otherwise unchanged.
// At D = 4 the 16 corners of a (point, level) are visited in groups, in corner order, a group's gathers being consumed before
// the next group's start (corner_group below; DESIGN.md "Hash grid: 2-D and 4-D inputs").
//
// Element types: y / dL/dy (and the spherical harmonics' out / dL/dout) are float, fp16 or bf16 (NFA_ELEM_*, common.hip.h).
// The arithmetic is the float32 one whatever the type; a point's F values of a level are converted once and moved as one
// vector of 2 F bytes.  The forward keeps its layout for half outputs: with F = 2 a wave writes 4-byte pieces at a 64-byte
// stride, and still takes 0.80-0.85 of the time of one lane per (point, level) (DESIGN.md "Half-precision field path").
#include "common.hip.h"

namespace nfa {

#define NFA_HG_MAX_LEVELS 32

struct HashGridLevels {
    float scale[NFA_HG_MAX_LEVELS];
    uint32_t res[NFA_HG_MAX_LEVELS];
    uint32_t offset[NFA_HG_MAX_LEVELS];   // in entries
    uint32_t size[NFA_HG_MAX_LEVELS];     // in entries; a power of two on hashed levels
    uint32_t hashed;                      // bit l: level l is hashed
    int32_t n_levels;
    int32_t pts_per_wave;                 // 64 / n_levels
};

template <int F> struct FVec;
template <> struct FVec<1> { float v[1]; };
template <> struct FVec<2> { float v[2]; } __attribute__((aligned(8)));
template <> struct FVec<4> { float v[4]; } __attribute__((aligned(16)));
template <> struct FVec<8> { float v[8]; } __attribute__((aligned(16)));

// K consecutive halves (E = fp16 or bf16) at p from / as floats, K = 1, 2, 4 or a multiple of 8: pieces of 2, 4, 8 or 16
// bytes; p is aligned to the piece.
template <int K, class E>
__device__ __forceinline__ void store_elems(E *p, const float *v)
{
    if constexpr (K == 1) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)half_bits<E>(v[0]);
    } else if constexpr (K == 2) {
        *reinterpret_cast<uint32_t *>(p) = pack_halves<E>(v[0], v[1]);
    } else if constexpr (K == 4) {
        const nfa_v2u w = {pack_halves<E>(v[0], v[1]), pack_halves<E>(v[2], v[3])};
        *reinterpret_cast<nfa_v2u *>(p) = w;
    } else {
        static_assert(K % 8 == 0, "K must be 1, 2, 4 or a multiple of 8");
#pragma unroll
        for (int k = 0; k < K; k += 8) {
            const nfa_v4u w = {pack_halves<E>(v[k], v[k + 1]), pack_halves<E>(v[k + 2], v[k + 3]),
                               pack_halves<E>(v[k + 4], v[k + 5]), pack_halves<E>(v[k + 6], v[k + 7])};
            *reinterpret_cast<nfa_v4u *>(p + k) = w;
        }
    }
}
template <int K, class E>
__device__ __forceinline__ void load_elems(const E *p, float *v)
{
    if constexpr (K == 1) {
        v[0] = half_value<E>(*reinterpret_cast<const uint16_t *>(p));
    } else if constexpr (K == 2) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
        v[0] = unpack_half<E>(w, 0); v[1] = unpack_half<E>(w, 1);
    } else if constexpr (K == 4) {
        const nfa_v2u w = *reinterpret_cast<const nfa_v2u *>(p);
        v[0] = unpack_half<E>(w.x, 0); v[1] = unpack_half<E>(w.x, 1); v[2] = unpack_half<E>(w.y, 0); v[3] = unpack_half<E>(w.y, 1);
    } else {
        static_assert(K % 8 == 0, "K must be 1, 2, 4 or a multiple of 8");
#pragma unroll
        for (int k = 0; k < K; k += 8) {
            const nfa_v4u w = *reinterpret_cast<const nfa_v4u *>(p + k);
            v[k] = unpack_half<E>(w.x, 0); v[k + 1] = unpack_half<E>(w.x, 1); v[k + 2] = unpack_half<E>(w.y, 0);
            v[k + 3] = unpack_half<E>(w.y, 1); v[k + 4] = unpack_half<E>(w.z, 0); v[k + 5] = unpack_half<E>(w.z, 1);
            v[k + 6] = unpack_half<E>(w.w, 0); v[k + 7] = unpack_half<E>(w.w, 1);
        }
    }
}

#define NFA_HG_MAX_DIMS 4

template <int D> struct Cell {
    uint32_t g[D];
    float f[D];
};

// The cell of the point at p on a level.  D = 2 and 4 read the point as one 8- or 16-byte load (x is 16-byte aligned).
template <int D>
__device__ __forceinline__ Cell<D> locate(const float *__restrict__ p, float scale)
{
    float xp[D];
    if constexpr (D == 2) {
        const float2 v = *reinterpret_cast<const float2 *>(p);
        xp[0] = v.x; xp[1] = v.y;
    } else if constexpr (D == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        xp[0] = v.x; xp[1] = v.y; xp[2] = v.z; xp[3] = v.w;
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = p[d];
    }
    Cell<D> c;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float p = xp[d] * scale + 0.5f;
        const float fl = floorf(p);
        c.f[d] = p - fl;
        const float cl = fminf(fmaxf(fl, -2147483648.0f), 2147483520.0f);   // NaN -> -2^31
        c.g[d] = (uint32_t)(int32_t)cl;
    }
    return c;
}

// A level's constants, read once out of the kernarg table
struct LevelRef {
    float scale;
    uint32_t res, size, offset;
    bool hashed;
    __device__ __forceinline__ LevelRef(const HashGridLevels &T, int l)
        : scale(T.scale[l]), res(T.res[l]), size(T.size[l]), offset(T.offset[l]), hashed((T.hashed >> l) & 1u) {}
};

// tiny-cuda-nn's hash primes of dimensions 1..3 (dimension 0: 1)
__host__ __device__ constexpr uint32_t hash_prime(int d) { return d == 1 ? 2654435761u : d == 2 ? 805459861u : 3674653429u; }

template <int D>
__device__ __forceinline__ uint32_t corner_index(const Cell<D> &c, int corner, const LevelRef &L)
{
    uint32_t q[D];
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = c.g[d] + ((corner >> d) & 1);
    if (L.hashed) {
        uint32_t h = q[0];
#pragma unroll
        for (int d = 1; d < D; ++d) h ^= q[d] * hash_prime(d);
        return h & (L.size - 1u);
    }
    uint32_t idx = q[0], power = L.res;
#pragma unroll
    for (int d = 1; d < D; ++d) {
        idx += q[d] * power;
        power *= L.res;
    }
    return idx % L.size;
}

// Smoothstep (header): the cell's fractions become S_d, so that Corner gives w_d; d1 = S', d2 = S''
template <int D>
__device__ __forceinline__ void smoothstep(Cell<D> &c, float *d1, float *d2)
{
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float f = c.f[d];
        d1[d] = (6.0f * f) * (1.0f - f);
        d2[d] = 6.0f - 12.0f * f;
        c.f[d] = (f * f) * (3.0f - 2.0f * f);
    }
}

// The terms of one corner (header).  This is the one place where a table-gradient coefficient is written down: the atomic
// kernels and hs_term of the sorted path both take it from here, so each sorted term is the float32 value the atomic pass adds.
template <int D> struct Corner {
    int bits;
    float w[D];   // w_d = (c_d ? f_d : 1 - f_d), f_d being S_d under Smoothstep
    __device__ __forceinline__ Corner(const Cell<D> &c, int corner) : bits(corner)
    {
#pragma unroll
        for (int d = 0; d < D; ++d) w[d] = ((corner >> d) & 1) ? c.f[d] : 1.0f - c.f[d];
    }
    // u_d = (c_d ? v_d : -v_d); Smoothstep: v holds v_d * S'_d, formed once per (point, level)
    __device__ __forceinline__ void signed_v(const float *v, float *u) const
    {
#pragma unroll
        for (int d = 0; d < D; ++d) u[d] = ((bits >> d) & 1) ? v[d] : -v[d];
    }
    __device__ __forceinline__ float first_order() const                                                     // w_c
    {
        float p = w[0];
#pragma unroll
        for (int d = 1; d < D; ++d) p = p * w[d];
        return p;
    }
    // prod_{d != e} w_d in ascending d, left-associated: the factor of dot_c in dL/dx_e
    template <int E> __device__ __forceinline__ float others() const
    {
        constexpr int a = E == 0 ? 1 : 0;
        float p = w[a];
        if constexpr (D > 2) {
            constexpr int b = a + 1 == E ? a + 2 : a + 1;
            p = p * w[b];
            if constexpr (D > 3) p = p * w[b + 1 == E ? b + 2 : b + 1];
        }
        return p;
    }
    __device__ __forceinline__ float second_order(const float *u, float s) const                             // a_c
    {
        static_assert(D == 3, "the second order is 3-D only");
        return ((u[0] * (w[1] * w[2]) + u[1] * (w[0] * w[2])) + u[2] * (w[0] * w[1])) * s;
    }
    // dx_d = (c_d ? dx_d + t_d : dx_d - t_d)
    __device__ __forceinline__ void accumulate(float *dx, const float *t) const
    {
#pragma unroll
        for (int d = 0; d < D; ++d) dx[d] = ((bits >> d) & 1) ? dx[d] + t[d] : dx[d] - t[d];
    }
    // the first-order terms t_e = (prod_{d != e} w_d) * dot_c, e = 0 .. D - 1
    template <size_t... E> __device__ __forceinline__ void accumulate_dot(float *dx, float dot, std::index_sequence<E...>) const
    {
        const float t[D] = {(others<(int)E>() * dot)...};
        accumulate(dx, t);
    }
};

// A point's F values of a level (piece = n * n_levels + l) from / as floats: float as one FVec<F>, halves as 2 F bytes
template <int F, class E>
__device__ __forceinline__ FVec<F> load_piece(const E *__restrict__ p, int64_t piece)
{
    FVec<F> v;
    if constexpr (std::is_same<E, float>::value) v = reinterpret_cast<const FVec<F> *>(p)[piece];
    else load_elems<F>(p + piece * F, v.v);
    return v;
}
template <int F, class E>
__device__ __forceinline__ void store_piece(E *__restrict__ p, int64_t piece, const float *v)
{
    if constexpr (std::is_same<E, float>::value) {
        FVec<F> out;
#pragma unroll
        for (int j = 0; j < F; ++j) out.v[j] = v[j];
        reinterpret_cast<FVec<F> *>(p)[piece] = out;
    } else {
        store_elems<F>(p + piece * F, v);
    }
}

// Forward: one level per workgroup row (blockIdx.y), one lane per point.  A wave's 64 points read one level's table, which
// stays in one XCD's L2 (4 MiB: a hashed level of the NGP grid), and write their F-float pieces at a stride of L F floats.
// Measured against one lane per (point, level) with the level fastest in the wave (coalesced output rows): 0.83-0.90 of
// its time at 2^20 points (DESIGN.md "Input encodings").
// The corners of a (point, level) are visited in groups of corner_group<D, F>(): the loop over the groups is a real loop,
// the group itself unrolled, so a group's gathers are in flight together and are consumed before the next group's start.
// Up to D = 3 the group is all 2^D corners.  At D = 4 it is 8 corners, 4 from F = 4: with all 16 gathers in flight the
// forward holds 16 F values (146 VGPRs at F = 8, 3 waves per SIMD; DESIGN.md "Hash grid: 2-D and 4-D inputs").  The corner
// order of the sums does not depend on the grouping.
template <int D, int F>
__host__ __device__ constexpr int corner_group() { return D <= 3 ? 1 << D : F >= 4 ? 4 : 8; }
// (the backward holds a point's F values of dL/dy and its D shares of dL/dx next to a corner's values: at D = 4 all 16
// corners are unrolled up to F = 2, F = 4 takes them in pairs and F = 8 one by one)
template <int D, int F>
__host__ __device__ constexpr int corner_group_bwd() { return D <= 3 || F < 4 ? 1 << D : F < 8 ? 2 : 1; }

template <int D, int F, class E, int I>
__global__ __launch_bounds__(256) void hashgrid_fwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                           int64_t n_points, const HashGridLevels T, E *__restrict__ y)
{
    const int l = (int)blockIdx.y;
    const LevelRef L(T, l);
    const FVec<F> *tab = reinterpret_cast<const FVec<F> *>(params) + L.offset;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < n_points; n += stride) {
        Cell<D> c = locate<D>(x + n * D, L.scale);
        if constexpr (I == NFA_INTERP_SMOOTHSTEP) {
            float d1[D], d2[D];
            smoothstep(c, d1, d2);
        }
        float acc[F];
#pragma unroll
        for (int j = 0; j < F; ++j) acc[j] = 0.0f;
#pragma nounroll
        for (int first = 0; first < (1 << D); first += corner_group<D, F>()) {
#pragma unroll
            for (int corner = first; corner < first + corner_group<D, F>(); ++corner) {
                const FVec<F> v = tab[corner_index(c, corner, L)];
                const float wc = Corner<D>(c, corner).first_order();
#pragma unroll
                for (int j = 0; j < F; ++j) acc[j] = acc[j] + wc * v.v[j];
            }
        }
        store_piece<F>(y, n * T.n_levels + l, acc);
    }
}

// The wave loop of the two (point, level) kernels and the (point, level) of this lane in it: a wave covers 64 / L points x
// all L levels (64 mod L lanes idle).  The dL/dx shares go to sum_levels() by value: handed over as a pointer to the
// kernel's array they cost the second-order kernels 4-6 VGPRs and a wave per SIMD.
struct LaneItems {
    int64_t w, n_waves, wave_stride, n_points, n;
    int n_levels, pts_per_wave, l;
    bool active;   // false for the idle lanes of a wave
    __device__ __forceinline__ LaneItems(const HashGridLevels &T, int64_t n_points_)
        : w(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64), n_waves(ceil_div64(n_points_, T.pts_per_wave)),
          wave_stride((int64_t)gridDim.x * (blockDim.x / 64)), n_points(n_points_), n_levels(T.n_levels),
          pts_per_wave(T.pts_per_wave) { item(); }
    __device__ __forceinline__ void item()
    {
        const int lane = (int)(threadIdx.x & 63);
        const int p = lane / n_levels;
        l = lane - p * n_levels;
        n = w * pts_per_wave + p;
        active = p < pts_per_wave && n < n_points;
    }
    __device__ __forceinline__ bool more() const { return w < n_waves; }
    __device__ __forceinline__ void next() { w += wave_stride; item(); }
    // dx summed over the point's L lanes in level order; the level-0 lane writes (call under a wave-uniform branch)
    // (g_x [N, D]: one 8- or 16-byte store per point at D = 2, 4, which need it 16-byte aligned like x)
    // (share: this lane's D shares, s: the D running sums, all by value and as scalars; see above.  S... is deduced from the
    // Shares tag alone, so both packs have D floats.  For D = 3, sum_levels(dx, g_x, ..) calls
    //   sum_shares(g_x, Shares<float, float, float>{}, dx[0], dx[1], dx[2], 0.0f, 0.0f, 0.0f), whose loop body reads
    //   v0 = __shfl(share0, src, 64), v1 = .., v2 = ..;  s0 = k == 0 ? v0 : s0 + v0;  s1 = ..;  s2 = ..;
    // the three scalar sums of the 3-D code this came from.)
    template <class... S> struct Shares {};
    template <class... S>
    __device__ __forceinline__ void sum_shares(float *__restrict__ g_x, Shares<S...>, S... share, S... s) const
    {
        constexpr int D = sizeof...(S);
        const int first = (int)(threadIdx.x & 63) - l;
        for (int k = 0; k < n_levels; ++k) {
            const int src = min(first + k, 63);
            [&](auto... v) { ((s = k == 0 ? v : s + v), ...); }(__shfl(share, src, 64)...);
        }
        if (active && l == 0) {
            const float out[D] = {s...};
            if constexpr (D == 2) {
                reinterpret_cast<float2 *>(g_x)[n] = make_float2(out[0], out[1]);
            } else if constexpr (D == 4) {
                reinterpret_cast<float4 *>(g_x)[n] = make_float4(out[0], out[1], out[2], out[3]);
            } else {
#pragma unroll
                for (int d = 0; d < D; ++d) g_x[n * D + d] = out[d];
            }
        }
    }
    template <int D, size_t... K>
    __device__ __forceinline__ void sum_levels(const float (&dx)[D], float *__restrict__ g_x, std::index_sequence<K...>) const
    {
        sum_shares(g_x, Shares<decltype(+dx[K])...>{}, dx[K]..., ((void)K, 0.0f)...);
    }
};

// A (point, level)'s corner sums of dL/dx_d, d = 0 .. D - 1, times s (Linear) or (* S'_d) * s (Smoothstep).  Written as a
// pack expansion, like the level sum above: as loops over d the D = 3 kernels come out with other registers.
template <int I, int D, size_t... K>
__device__ __forceinline__ void scale_dx(float (&dx)[D], const float *d1, float s, std::index_sequence<K...>)
{
    if constexpr (I == NFA_INTERP_SMOOTHSTEP) ((dx[K] = (dx[K] * d1[K]) * s), ...);
    else ((dx[K] *= s), ...);
}

template <int D, int F, class E, int I>
__global__ __launch_bounds__(256) void hashgrid_bwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                           const E *__restrict__ g_y, int64_t n_points,
                                                           const HashGridLevels T, float *__restrict__ g_params,
                                                           float *__restrict__ g_x)
{
    for (LaneItems it(T, n_points); it.more(); it.next()) {
        float dx[D] = {};
        if (it.active) {
            const int64_t n = it.n;
            const int l = it.l;
            const LevelRef L(T, l);
            Cell<D> c = locate<D>(x + n * D, L.scale);
            float d1[D], d2[D];
            if constexpr (I == NFA_INTERP_SMOOTHSTEP) smoothstep(c, d1, d2);
            const FVec<F> g = load_piece<F>(g_y, n * T.n_levels + l);
#pragma nounroll
            for (int first = 0; first < (1 << D); first += corner_group_bwd<D, F>())
#pragma unroll
            for (int corner = first; corner < first + corner_group_bwd<D, F>(); ++corner) {
                const uint32_t e = L.offset + corner_index(c, corner, L);
                const Corner<D> k(c, corner);
                if (g_params) {
                    const float wc = k.first_order();
                    float *dst = g_params + (size_t)e * F;
#pragma unroll
                    for (int j = 0; j < F; ++j) unsafeAtomicAdd(dst + j, wc * g.v[j]);
                }
                if (g_x) {
                    const FVec<F> v = reinterpret_cast<const FVec<F> *>(params)[e];
                    float dot = 0.0f;
#pragma unroll
                    for (int j = 0; j < F; ++j) dot = dot + g.v[j] * v.v[j];
                    k.accumulate_dot(dx, dot, std::make_index_sequence<D>{});
                }
            }
            if (g_x) {
                const float s = L.scale;
                scale_dx<I>(dx, d1, s, std::make_index_sequence<D>{});
            }
        }
        if (g_x) it.sum_levels(dx, g_x, std::make_index_sequence<D>{});
    }
}

// Second order: the derivative of the backward's dL/dx output, given its incoming gradient v = gg_x[n] (header: "Second
// order").  Shape of hashgrid_bwd_kernel; every output is optional, and the corners are read only for gg_y and x2.
template <int F, class E, int I>
__global__ __launch_bounds__(256) void hashgrid_bwd_bwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                               const E *__restrict__ g_y, const float *__restrict__ gg_x,
                                                               int64_t n_points, const HashGridLevels T,
                                                               E *__restrict__ gg_y, float *__restrict__ g_params,
                                                               float *__restrict__ g_x)
{
    for (LaneItems it(T, n_points); it.more(); it.next()) {
        float dx[3] = {0.0f, 0.0f, 0.0f};
        if (it.active) {
            const int64_t n = it.n;
            const int l = it.l;
            const LevelRef L(T, l);
            const float s = L.scale;
            Cell<3> c = locate<3>(x + n * 3, s);
            float v[3] = {gg_x[n * 3 + 0], gg_x[n * 3 + 1], gg_x[n * 3 + 2]};
            float d1[3], p[3];   // Smoothstep: S'_d, v_d * S''_d; v_d becomes v_d * S'_d
            if constexpr (I == NFA_INTERP_SMOOTHSTEP) {
                float d2[3];
                smoothstep(c, d1, d2);
                p[0] = v[0] * d2[0]; p[1] = v[1] * d2[1]; p[2] = v[2] * d2[2];
                v[0] = v[0] * d1[0]; v[1] = v[1] * d1[1]; v[2] = v[2] * d1[2];
            }
            const int64_t piece = n * T.n_levels + l;
            FVec<F> g = {};
            if (g_params || g_x) g = load_piece<F>(g_y, piece);
            float acc[F];
#pragma unroll
            for (int j = 0; j < F; ++j) acc[j] = 0.0f;
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                const uint32_t e = L.offset + corner_index(c, corner, L);
                const Corner<3> k(c, corner);
                const float *w = k.w;
                float u[3];
                k.signed_v(v, u);
                const float a = k.second_order(u, s);
                if (g_params) {
                    float *dst = g_params + (size_t)e * F;
#pragma unroll
                    for (int j = 0; j < F; ++j) unsafeAtomicAdd(dst + j, a * g.v[j]);
                }
                if (gg_y || g_x) {
                    const FVec<F> t = reinterpret_cast<const FVec<F> *>(params)[e];
#pragma unroll
                    for (int j = 0; j < F; ++j) acc[j] = acc[j] + a * t.v[j];
                    if (g_x) {
                        float dot = 0.0f;
#pragma unroll
                        for (int j = 0; j < F; ++j) dot = dot + g.v[j] * t.v[j];
                        if constexpr (I == NFA_INTERP_SMOOTHSTEP) {
                            const float t[3] = {(d1[0] * (u[1] * w[2] + u[2] * w[1]) + p[0] * (w[1] * w[2])) * dot,
                                                (d1[1] * (u[0] * w[2] + u[2] * w[0]) + p[1] * (w[0] * w[2])) * dot,
                                                (d1[2] * (u[0] * w[1] + u[1] * w[0]) + p[2] * (w[0] * w[1])) * dot};
                            k.accumulate(dx, t);
                        } else {
                            const float t[3] = {(u[1] * w[2] + u[2] * w[1]) * dot, (u[0] * w[2] + u[2] * w[0]) * dot,
                                                (u[0] * w[1] + u[1] * w[0]) * dot};
                            k.accumulate(dx, t);
                        }
                    }
                }
            }
            if (gg_y) store_piece<F>(gg_y, piece, acc);
            if (g_x) {
                dx[0] = (dx[0] * s) * s; dx[1] = (dx[1] * s) * s; dx[2] = (dx[2] * s) * s;
            }
        }
        if (g_x) it.sum_levels(dx, g_x, std::make_index_sequence<3>{});
    }
}

// ---------------------------------------------------------------- spherical harmonics
// tiny-cuda-nn's convention: directions d in [0, 1]^3, u = 2 d - 1 (not renormalised); degree^2 outputs per point.
#define SH_C0 0.28209479177387814f
#define SH_C1 0.48860251190291987f
#define SH_C2A 1.0925484305920792f
#define SH_C2B 0.94617469575755997f
#define SH_C2C 0.31539156525251999f
#define SH_C2D 0.54627421529603959f
#define SH_C3A 0.59004358992664352f
#define SH_C3B 2.8906114426405538f
#define SH_C3C 0.45704579946446572f
#define SH_C3D 0.3731763325901154f
#define SH_C3E 1.4453057213202769f

template <int DEG>
__device__ __forceinline__ void sh_eval(float x, float y, float z, float *o)
{
    o[0] = SH_C0;
    if constexpr (DEG > 1) {
        o[1] = -SH_C1 * y;
        o[2] = SH_C1 * z;
        o[3] = -SH_C1 * x;
    }
    if constexpr (DEG > 2) {
        const float xy = x * y, yz = y * z, xz = x * z, x2 = x * x, y2 = y * y, z2 = z * z;
        o[4] = SH_C2A * xy;
        o[5] = -SH_C2A * yz;
        o[6] = SH_C2B * z2 - SH_C2C;
        o[7] = -SH_C2A * xz;
        o[8] = SH_C2D * (x2 - y2);
        if constexpr (DEG > 3) {
            o[9] = SH_C3A * y * (-3.0f * x2 + y2);
            o[10] = SH_C3B * xy * z;
            o[11] = SH_C3C * y * (1.0f - 5.0f * z2);
            o[12] = SH_C3D * z * (5.0f * z2 - 3.0f);
            o[13] = SH_C3C * x * (1.0f - 5.0f * z2);
            o[14] = SH_C3E * z * (x2 - y2);
            o[15] = SH_C3A * x * (-x2 + 3.0f * y2);
        }
    }
}

// dL/du of sum_k g_k Y_k(u)
template <int DEG>
__device__ __forceinline__ void sh_grad(float x, float y, float z, const float *g, float *du)
{
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if constexpr (DEG > 1) {
        gy += -SH_C1 * g[1];
        gz += SH_C1 * g[2];
        gx += -SH_C1 * g[3];
    }
    if constexpr (DEG > 2) {
        gx += SH_C2A * y * g[4];
        gy += SH_C2A * x * g[4];
        gy += -SH_C2A * z * g[5];
        gz += -SH_C2A * y * g[5];
        gz += 2.0f * SH_C2B * z * g[6];
        gx += -SH_C2A * z * g[7];
        gz += -SH_C2A * x * g[7];
        gx += 2.0f * SH_C2D * x * g[8];
        gy += -2.0f * SH_C2D * y * g[8];
        if constexpr (DEG > 3) {
            const float x2 = x * x, y2 = y * y, z2 = z * z;
            gx += -6.0f * SH_C3A * x * y * g[9];
            gy += SH_C3A * (-3.0f * x2 + 3.0f * y2) * g[9];
            gx += SH_C3B * y * z * g[10];
            gy += SH_C3B * x * z * g[10];
            gz += SH_C3B * x * y * g[10];
            gy += SH_C3C * (1.0f - 5.0f * z2) * g[11];
            gz += -10.0f * SH_C3C * y * z * g[11];
            gz += SH_C3D * (15.0f * z2 - 3.0f) * g[12];
            gx += SH_C3C * (1.0f - 5.0f * z2) * g[13];
            gz += -10.0f * SH_C3C * x * z * g[13];
            gx += 2.0f * SH_C3E * x * z * g[14];
            gy += -2.0f * SH_C3E * y * z * g[14];
            gz += SH_C3E * (x2 - y2) * g[14];
            gx += SH_C3A * (-3.0f * x2 + 3.0f * y2) * g[15];
            gy += 6.0f * SH_C3A * x * y * g[15];
        }
    }
    du[0] = gx;
    du[1] = gy;
    du[2] = gz;
}

// Row of K floats: float4 pieces when K is a multiple of 4 (rows stay 16-byte aligned), single floats otherwise.
// Row of K halves (2 K bytes from a 16-byte aligned base: 2, 8, 18 or 32): K = 16 two 16-byte pieces, K = 4 one 8-byte
// piece, single halves otherwise.
template <int K, class E>
__device__ __forceinline__ void store_row(E *dst, const float *v)
{
    if constexpr (K % 8 == 0 || K == 4) {
        store_elems<K>(dst, v);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) store_elems<1>(dst + k, v + k);
    }
}
template <int K, class E>
__device__ __forceinline__ void load_row(const E *src, float *v)
{
    if constexpr (K % 8 == 0 || K == 4) {
        load_elems<K>(src, v);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) load_elems<1>(src + k, v + k);
    }
}
template <int K>
__device__ __forceinline__ void store_row(float *dst, const float *v)
{
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int k = 0; k < K; k += 4) reinterpret_cast<float4 *>(dst)[k / 4] = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) dst[k] = v[k];
    }
}
template <int K>
__device__ __forceinline__ void load_row(const float *src, float *v)
{
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int k = 0; k < K; k += 4) {
            const float4 q = reinterpret_cast<const float4 *>(src)[k / 4];
            v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = src[k];
    }
}

template <int DEG, class E>
__global__ __launch_bounds__(256) void sh_fwd_kernel(const float *__restrict__ dirs, int64_t n, E *__restrict__ out)
{
    constexpr int K = DEG * DEG;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float x = 2.0f * dirs[i * 3 + 0] - 1.0f, y = 2.0f * dirs[i * 3 + 1] - 1.0f, z = 2.0f * dirs[i * 3 + 2] - 1.0f;
        float o[K];
        sh_eval<DEG>(x, y, z, o);
        store_row<K>(out + i * K, o);
    }
}

template <int DEG, class E>
__global__ __launch_bounds__(256) void sh_bwd_kernel(const float *__restrict__ dirs, const E *__restrict__ g_out,
                                                     int64_t n, float *__restrict__ g_dirs)
{
    constexpr int K = DEG * DEG;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float x = 2.0f * dirs[i * 3 + 0] - 1.0f, y = 2.0f * dirs[i * 3 + 1] - 1.0f, z = 2.0f * dirs[i * 3 + 2] - 1.0f;
        float g[K], du[3];
        load_row<K>(g_out + i * K, g);
        sh_grad<DEG>(x, y, z, g, du);
        g_dirs[i * 3 + 0] = 2.0f * du[0];   // du / dd = 2
        g_dirs[i * 3 + 1] = 2.0f * du[1];
        g_dirs[i * 3 + 2] = 2.0f * du[2];
    }
}

// ---------------------------------------------------------------- argument checks
// The grid description of a call, filled at the extern "C" boundary
struct GridArgs {
    int32_t n_dims;   // 2, 3 or 4
    int64_t n_points;
    int32_t n_levels, n_features, log2_hashmap_size;
    const float *scales_host;
    const int32_t *resolutions_host, *sizes_host;
    int64_t n_params;
};

static int hashgrid_table(const char *name, const GridArgs &G, HashGridLevels &T)
{
    NFA_REQUIRE(G.n_dims >= 2 && G.n_dims <= NFA_HG_MAX_DIMS, "%s: n_dims must be 2, 3 or 4 (got %d)", name, G.n_dims);
    NFA_REQUIRE(G.n_points >= 0 && G.n_params >= 0, "%s: negative size", name);
    NFA_REQUIRE(G.n_features == 1 || G.n_features == 2 || G.n_features == 4 || G.n_features == 8,
                "%s: n_features must be 1, 2, 4 or 8 (got %d)", name, G.n_features);
    NFA_REQUIRE(G.n_levels >= 1 && G.n_levels <= NFA_HG_MAX_LEVELS, "%s: n_levels must be in 1..32 (got %d)", name, G.n_levels);
    NFA_REQUIRE(G.log2_hashmap_size >= 10 && G.log2_hashmap_size <= 24, "%s: log2_hashmap_size must be in 10..24 (got %d)",
                name, G.log2_hashmap_size);
    NFA_REQUIRE(G.n_params < ((int64_t)1 << 31), "%s: too many parameters (%lld)", name, (long long)G.n_params);
    NFA_REQUIRE(G.scales_host && G.resolutions_host && G.sizes_host, "%s: null level table", name);
    const int64_t table = (int64_t)1 << G.log2_hashmap_size;
    int64_t offset = 0;
    T = {};
    for (int l = 0; l < G.n_levels; ++l) {
        const int64_t r = G.resolutions_host[l], s = G.sizes_host[l];
        NFA_REQUIRE(r >= 1, "%s: level %d resolution %lld out of range", name, l, (long long)r);
        const int64_t big = (int64_t)1 << 40;   // past every table: res^D stops here (no overflow; hashed anyway)
        int64_t cells = r > (1 << 20) ? big : 1;
        for (int d = 0; d < G.n_dims && cells < big; ++d) cells *= r;
        const int64_t dense = cells >= big ? INT64_MAX : (cells + 7) / 8 * 8;
        NFA_REQUIRE(s == (dense < table ? dense : table), "%s: level %d size %lld is not min(roundup8(res^%d), 2^%d)",
                    name, l, (long long)s, G.n_dims, G.log2_hashmap_size);
        T.scale[l] = G.scales_host[l];
        T.res[l] = (uint32_t)r;
        T.offset[l] = (uint32_t)offset;
        T.size[l] = (uint32_t)s;
        if (dense > table) T.hashed |= 1u << l;
        offset += s;
    }
    NFA_REQUIRE(offset * G.n_features == G.n_params, "%s: n_params %lld != %lld entries x %d features", name,
                (long long)G.n_params, (long long)offset, G.n_features);
    T.n_levels = G.n_levels;
    T.pts_per_wave = 64 / G.n_levels;
    return NFA_OK;
}

static unsigned hashgrid_grid(int64_t n_points, const HashGridLevels &T)
{
    return grid_1d(ceil_div64(n_points, T.pts_per_wave) * 64, 256);
}

// ---------------------------------------------------------------- the entries, one implementation per element type
// Each pass is a check of its arguments (which builds the level table) and a launch with the checked table; the `_sorted`
// passes check once under their own name and call the launch half of the plain pass.
static int check_interp(const char *name, int32_t interp)
{
    NFA_REQUIRE(interp == NFA_INTERP_LINEAR || interp == NFA_INTERP_SMOOTHSTEP,
                "%s: interp must be NFA_INTERP_LINEAR (0) or NFA_INTERP_SMOOTHSTEP (1) (got %d)", name, interp);
    return NFA_OK;
}

// Host-side dispatch of a run-time value to a compile-time one, f(std::integral_constant<int, V>), for the V... it was
// checked to be one of; of a grid's (n_dims, n_features, interp) to f(.. <int, D>, .. <int, F>, .. <int, I>) for the Dims... a
// pass is instantiated for (all three, or 3 alone: the second order); and of the spherical-harmonics degree.
template <int... V, class Fn>
static void dispatch_int(int32_t v, Fn &&f)
{
    (void)((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}
template <int... Dims, class Fn>
static void dispatch_grid(const GridArgs &G, int32_t interp, Fn &&f)
{
    dispatch_int<Dims...>(G.n_dims, [&](auto d) {
        dispatch_int<NFA_INTERP_LINEAR, NFA_INTERP_SMOOTHSTEP>(interp, [&](auto i) {
            dispatch_int<1, 2, 4, 8>(G.n_features, [&](auto n) { f(d, n, i); });
        });
    });
}
template <class Fn>
static void dispatch_degree(int32_t degree, Fn &&f)
{
    dispatch_int<1, 2, 3, 4>(degree, f);
}

template <class E>
static int hashgrid_fwd(int32_t interp, const float *x, const float *params, const GridArgs &G, E *y, nfa_stream_t stream)
{
    HashGridLevels T;
    const int rc = hashgrid_table("hashgrid_fwd", G, T);
    if (rc != NFA_OK) return rc;
    if (G.n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && params && y, "hashgrid_fwd: null pointer");
    NFA_REQUIRE(G.n_dims == 3 || aligned16(x), "hashgrid_fwd: x must be 16-byte aligned at n_dims %d", G.n_dims);
    NFA_REQUIRE((std::is_same<E, float>::value) || aligned16(y), "hashgrid_fwd: a half y must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const dim3 grid(grid_1d(G.n_points, 256, 256 * 16 / G.n_levels + 1), G.n_levels), block(256);
    dispatch_grid<2, 3, 4>(G, interp, [&](auto d, auto f, auto i) {
        hipLaunchKernelGGL((hashgrid_fwd_kernel<d(), f(), E, i()>), grid, block, 0, s, x, params, G.n_points, T, y);
    });
    NFA_CHECK_LAUNCH("hashgrid_fwd");
    return NFA_OK;
}

template <class E>
static int hashgrid_bwd_launch(int32_t interp, const float *x, const float *params, const E *grad_y, const GridArgs &G,
                               const HashGridLevels &T, float *grad_params, float *grad_x, hipStream_t s)
{
    const dim3 grid(hashgrid_grid(G.n_points, T)), block(256);
    dispatch_grid<2, 3, 4>(G, interp, [&](auto d, auto f, auto i) {
        hipLaunchKernelGGL((hashgrid_bwd_kernel<d(), f(), E, i()>), grid, block, 0, s, x, params, grad_y, G.n_points, T,
                           grad_params, grad_x);
    });
    NFA_CHECK_LAUNCH("hashgrid_bwd");
    return NFA_OK;
}

template <class E>
static int hashgrid_bwd(int32_t interp, const float *x, const float *params, const E *grad_y, const GridArgs &G,
                        float *grad_params, float *grad_x, nfa_stream_t stream)
{
    HashGridLevels T;
    const int rc = hashgrid_table("hashgrid_bwd", G, T);
    if (rc != NFA_OK) return rc;
    if (G.n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && grad_y && (grad_params || grad_x) && (params || !grad_x), "hashgrid_bwd: null pointer");
    NFA_REQUIRE(G.n_dims == 3 || all_aligned16(x, grad_x), "hashgrid_bwd: x and grad_x must be 16-byte aligned at n_dims %d",
                G.n_dims);
    NFA_REQUIRE((std::is_same<E, float>::value) || aligned16(grad_y), "hashgrid_bwd: a half grad_y must be 16-byte aligned");
    return hashgrid_bwd_launch(interp, x, params, grad_y, G, T, grad_params, grad_x, as_stream(stream));
}

template <class E>
static int hashgrid_bwd_bwd_launch(int32_t interp, const float *x, const float *params, const E *grad_y,
                                   const float *grad_grad_x, const GridArgs &G, const HashGridLevels &T, E *grad_grad_y,
                                   float *grad_params, float *grad_x, hipStream_t s)
{
    const dim3 grid(hashgrid_grid(G.n_points, T)), block(256);
    dispatch_grid<3>(G, interp, [&](auto, auto f, auto i) {
        hipLaunchKernelGGL((hashgrid_bwd_bwd_kernel<f(), E, i()>), grid, block, 0, s, x, params, grad_y, grad_grad_x,
                           G.n_points, T, grad_grad_y, grad_params, grad_x);
    });
    NFA_CHECK_LAUNCH("hashgrid_bwd_bwd");
    return NFA_OK;
}

template <class E>
static int hashgrid_bwd_bwd(int32_t interp, const float *x, const float *params, const E *grad_y, const float *grad_grad_x,
                            const GridArgs &G, E *grad_grad_y, float *grad_params, float *grad_x, nfa_stream_t stream)
{
    HashGridLevels T;
    const int rc = hashgrid_table("hashgrid_bwd_bwd", G, T);
    if (rc != NFA_OK) return rc;
    if (G.n_points == 0) return NFA_OK;
    NFA_REQUIRE(grad_grad_x, "hashgrid_bwd_bwd: grad_grad_x is null");
    NFA_REQUIRE(grad_grad_y || grad_params || grad_x, "hashgrid_bwd_bwd: no output requested");
    NFA_REQUIRE(x && (grad_y || !(grad_params || grad_x)) && (params || !(grad_grad_y || grad_x)), "hashgrid_bwd_bwd: null pointer");
    NFA_REQUIRE((std::is_same<E, float>::value) || (aligned16(grad_y) && aligned16(grad_grad_y)),
                "hashgrid_bwd_bwd: half grad_y and grad_grad_y must be 16-byte aligned");
    return hashgrid_bwd_bwd_launch(interp, x, params, grad_y, grad_grad_x, G, T, grad_grad_y, grad_params, grad_x,
                                   as_stream(stream));
}

template <class E>
static int sh_fwd(const float *dirs, int64_t n_points, int32_t degree, E *out, nfa_stream_t stream)
{
    NFA_REQUIRE(n_points >= 0, "sh_fwd: negative size");
    NFA_REQUIRE(degree >= 1 && degree <= 4, "sh_fwd: degree must be in 1..4 (got %d)", degree);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(dirs && out, "sh_fwd: null pointer");
    NFA_REQUIRE(aligned16(out), "sh_fwd: out must be 16-byte aligned");
    const dim3 grid(grid_1d(n_points, 256)), block(256);
    hipStream_t s = as_stream(stream);
    dispatch_degree(degree, [&](auto deg) {
        hipLaunchKernelGGL((sh_fwd_kernel<deg(), E>), grid, block, 0, s, dirs, n_points, out);
    });
    NFA_CHECK_LAUNCH("sh_fwd");
    return NFA_OK;
}

template <class E>
static int sh_bwd(const float *dirs, const E *grad_out, int64_t n_points, int32_t degree, float *grad_dirs, nfa_stream_t stream)
{
    NFA_REQUIRE(n_points >= 0, "sh_bwd: negative size");
    NFA_REQUIRE(degree >= 1 && degree <= 4, "sh_bwd: degree must be in 1..4 (got %d)", degree);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(dirs && grad_out && grad_dirs, "sh_bwd: null pointer");
    NFA_REQUIRE(aligned16(grad_out), "sh_bwd: grad_out must be 16-byte aligned");
    const dim3 grid(grid_1d(n_points, 256)), block(256);
    hipStream_t s = as_stream(stream);
    dispatch_degree(degree, [&](auto deg) {
        hipLaunchKernelGGL((sh_bwd_kernel<deg(), E>), grid, block, 0, s, dirs, grad_out, n_points, grad_dirs);
    });
    NFA_CHECK_LAUNCH("sh_bwd");
    return NFA_OK;
}

// ---------------------------------------------------------------- reproducible table gradient: sort and segmented sum
// nfa_hashgrid_bwd_sorted / nfa_hashgrid_bwd_bwd_sorted form the table gradient without float atomics.  THE ORDER OF THE SUM,
// per level (tests/hashgrid_sorted_reference.py restates it; for any D tests/hashgrid_nd_reference.py):
//   items   i = 2^D n + c (D = 3: 8 n + c) for point n and corner c, in that order; key_i = the corner's entry index inside
//           the level (locate / corner_index as above); term_i[j] = coef_i * g[n][j] in float32, coef_i = w_c, the left-
//           associated product of the first D factors (D = 3: (w_0 * w_1) * w_2), at first order and a_c (header, "Second
//           order"; D = 3 only) at second order, g the point's dL/dy piece of the level converted once.
//   sort    the items are sorted by key with a stable LSD radix sort (8-bit digits over the ceil(log2 size_l) significant bits):
//           equal keys stay in ascending i, that is ascending point and then corner.
//   tiles   the sorted array is cut into tiles of NFA_HS_TILE = 256 consecutive items.  A run of equal keys is cut into
//           segments at the tile borders; a segment's sum starts from its first term and adds the following ones left to
//           right, s = (..((t_0 + t_1) + t_2) + ..).
//   carry   a run that lies inside one tile is its segment.  A run that crosses tile borders is the sum of its segments'
//           sums in tile order, starting from the first segment's, P = (..((s_0 + s_1) + s_2) + ..).
//   Every entry that received an item is written once with a plain store; the others are not touched (the caller zeroes).
// Nothing here depends on arrival order: launch shapes follow from (n_points, n_levels, the level sizes) alone and nothing
// is read back, so a step can be captured.
//
// Scratch: levels are processed in groups of G, one level per workgroup row, each with its own slab of
//   level_bytes = 16 M + 1024 (B + 1) + 64 Tn,  M = 2^D n_points, B = ceil(M / 4096), Tn = ceil(M / 256):
//   two key and two id buffers of M uint32 (ping-pong), 256 B block counts + 256 digit totals, Tn x {head, tail} x 8 floats;
//   G = min(n_levels, max(1, floor(2^29 / level_bytes))); scratch = n_levels level_bytes where that is at most 2^29, else
//   max(2^29, level_bytes): at least G level_bytes, and monotone in n_points.
// Radix pass p of a level (skipped by levels with fewer significant bits): hs_count (digit counts per block of 4096 items,
// digit-major), hs_scan (exclusive prefix of each digit's row over the blocks, and the digit's total), hs_scatter (a wave
// owns 1024 consecutive items, 64 at a time in lane order; equal digits are ranked by lane inside the wave, waves and blocks
// in order: stable).  Pass 0 takes the id from the position.  The work of hs_sum is bounded by the tile: the 256 terms are
// formed in parallel into LDS and the thread at each segment's first item adds at most 256 of them; hs_carry walks a crossing
// run's segment sums, one thread per (run, feature).
#define NFA_HS_TILE 256
#define NFA_HS_BLOCK_ITEMS 4096
#define NFA_HS_BUDGET ((int64_t)1 << 29)

struct HashSortPlan {
    int64_t items, n_blocks, n_tiles, level_bytes, scratch_bytes;
    int32_t group;
};

static HashSortPlan hashsort_plan(int64_t n_points, int32_t n_levels, int32_t n_dims)
{
    HashSortPlan p;
    p.items = n_points << n_dims;   // 2^D items per point
    p.n_blocks = ceil_div64(p.items, NFA_HS_BLOCK_ITEMS);
    p.n_tiles = ceil_div64(p.items, NFA_HS_TILE);
    p.level_bytes = 16 * p.items + 1024 * (p.n_blocks + 1) + 64 * p.n_tiles;
    int64_t g = p.level_bytes > 0 ? NFA_HS_BUDGET / p.level_bytes : n_levels;
    g = g < 1 ? 1 : (g > n_levels ? n_levels : g);
    p.group = (int32_t)g;
    p.scratch_bytes = n_levels * p.level_bytes <= NFA_HS_BUDGET ? n_levels * p.level_bytes
                                                                : (p.level_bytes > NFA_HS_BUDGET ? p.level_bytes : NFA_HS_BUDGET);
    return p;
}

struct HashSortArgs {
    unsigned char *scratch;
    int64_t level_bytes;
    int64_t items;       // < 2^32
    int64_t n_blocks;
    int64_t n_tiles;
    int64_t n_points;
    int32_t first_level;   // the group's first level; blockIdx.y counts from it
};

struct HashSortView {
    uint32_t *keys0, *keys1, *ids0, *ids1, *hist, *totals;
    float *part;   // [n_tiles][2 (head, tail)][8]
    // (selects, not arrays: a dynamically indexed member would be moved to LDS)
    __device__ __forceinline__ uint32_t *keys(int which) const { return which ? keys1 : keys0; }
    __device__ __forceinline__ uint32_t *ids(int which) const { return which ? ids1 : ids0; }
};

__device__ __forceinline__ HashSortView hs_view(const HashSortArgs &A, int slot)
{
    unsigned char *b = A.scratch + (int64_t)slot * A.level_bytes;
    HashSortView v;
    v.keys0 = reinterpret_cast<uint32_t *>(b);
    v.keys1 = v.keys0 + A.items;
    v.ids0 = v.keys1 + A.items;
    v.ids1 = v.ids0 + A.items;
    v.hist = v.ids1 + A.items;
    v.totals = v.hist + 256 * A.n_blocks;
    v.part = reinterpret_cast<float *>(v.totals + 256);
    return v;
}

// radix passes of a level: 8-bit digits over the significant bits of its keys (size >= 8: at least one)
__host__ __device__ static inline int hs_passes(uint32_t size)
{
    int bits = 1;
    while (bits < 32 && (1u << bits) < size) ++bits;
    return (bits + 7) / 8;
}

__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t v)
{
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < NFA_WAVE; off <<= 1) {
        const uint32_t u = __shfl_up(v, off, NFA_WAVE);
        if (lane >= off) v += u;
    }
    return v;
}

// exclusive prefix of v over the 256 threads of a workgroup (ws: 4 words of LDS, used once)
__device__ __forceinline__ uint32_t block_excl_sum_256(uint32_t v, uint32_t *ws, uint32_t &total)
{
    const int w = (int)(threadIdx.x >> 6);
    const uint32_t incl = wave_incl_sum_u32(v);
    if ((threadIdx.x & 63) == 63) ws[w] = incl;
    __syncthreads();
    uint32_t pre = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) pre += k < w ? ws[k] : 0u;
    total = ws[0] + ws[1] + ws[2] + ws[3];
    return pre + incl - v;
}

template <int D>
__global__ __launch_bounds__(256) void hs_keys_kernel(const float *__restrict__ x, const HashGridLevels T, const HashSortArgs A)
{
    const LevelRef L(T, A.first_level + (int)blockIdx.y);
    uint32_t *keys = hs_view(A, (int)blockIdx.y).keys0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.items; i += stride) {
        const Cell<D> c = locate<D>(x + (i >> D) * D, L.scale);
        keys[i] = corner_index(c, (int)(i & ((1 << D) - 1)), L);
    }
}

__global__ __launch_bounds__(256) void hs_count_kernel(const HashGridLevels T, const HashSortArgs A, int pass)
{
    __shared__ uint32_t h[256];
    const int l = A.first_level + (int)blockIdx.y;
    if (pass >= hs_passes(T.size[l])) return;
    const HashSortView V = hs_view(A, (int)blockIdx.y);
    const uint32_t *keys = V.keys(pass & 1);
    const int shift = 8 * pass;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * NFA_HS_BLOCK_ITEMS + threadIdx.x;
    uint32_t key[NFA_HS_BLOCK_ITEMS / 256];   // the loads first, all in flight together
#pragma unroll
    for (int k = 0; k < NFA_HS_BLOCK_ITEMS / 256; ++k) key[k] = base + k * 256 < A.items ? keys[base + k * 256] : 0u;
#pragma unroll
    for (int k = 0; k < NFA_HS_BLOCK_ITEMS / 256; ++k)
        if (base + k * 256 < A.items) atomicAdd(&h[(key[k] >> shift) & 255u], 1u);   // (integer counts: any order)
    __syncthreads();
    V.hist[(int64_t)threadIdx.x * A.n_blocks + blockIdx.x] = h[threadIdx.x];
}

// one workgroup per (digit, level): the digit's block counts -> their exclusive prefix over the blocks, and the total
__global__ __launch_bounds__(256) void hs_scan_kernel(const HashGridLevels T, const HashSortArgs A, int pass)
{
    __shared__ uint32_t ws[4];
    const int l = A.first_level + (int)blockIdx.y;
    if (pass >= hs_passes(T.size[l])) return;
    const HashSortView V = hs_view(A, (int)blockIdx.y);
    uint32_t *row = V.hist + (int64_t)blockIdx.x * A.n_blocks;
    const int64_t per = ceil_div64(A.n_blocks, 256);
    const int64_t lo = (int64_t)threadIdx.x * per < A.n_blocks ? (int64_t)threadIdx.x * per : A.n_blocks;
    const int64_t hi = lo + per < A.n_blocks ? lo + per : A.n_blocks;
    uint32_t sum = 0;
    for (int64_t j = lo; j < hi; ++j) sum += row[j];
    uint32_t total;
    uint32_t run = block_excl_sum_256(sum, ws, total);
    for (int64_t j = lo; j < hi; ++j) {
        const uint32_t v = row[j];
        row[j] = run;
        run += v;
    }
    if (threadIdx.x == 0) V.totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void hs_scatter_kernel(const HashGridLevels T, const HashSortArgs A, int pass)
{
    __shared__ uint32_t woff[4][256];   // per wave and digit: the count, then the next output position
    __shared__ uint32_t ws[4];
    const int l = A.first_level + (int)blockIdx.y;
    if (pass >= hs_passes(T.size[l])) return;
    const HashSortView V = hs_view(A, (int)blockIdx.y);
    const uint32_t *kin = V.keys(pass & 1), *iin = pass ? V.ids(pass & 1) : nullptr;
    uint32_t *kout = V.keys((pass + 1) & 1), *iout = V.ids((pass + 1) & 1);
    const int shift = 8 * pass;
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) woff[k][tid] = 0;
    __syncthreads();
    constexpr int ROUNDS = NFA_HS_BLOCK_ITEMS / 256;   // a wave's 1024 items, 64 at a time
    const int64_t base = (int64_t)blockIdx.x * NFA_HS_BLOCK_ITEMS + w * (ROUNDS * 64) + lane;
    uint32_t key[ROUNDS], id[ROUNDS];   // all loads are issued before the ranking loop, whose rounds depend on each other
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = base + r * 64;
        key[r] = i < A.items ? kin[i] : 0u;
        id[r] = iin && i < A.items ? iin[i] : (uint32_t)i;
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        if (base + r * 64 < A.items) atomicAdd(&woff[w][(key[r] >> shift) & 255u], 1u);
    __syncthreads();
    {   // thread = digit: where the block's items of this digit start, then each wave's share in wave order
        uint32_t total;
        const uint32_t digit_base = block_excl_sum_256(V.totals[tid], ws, total);
        uint32_t o = digit_base + V.hist[(int64_t)tid * A.n_blocks + blockIdx.x];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = woff[k][tid];
            woff[k][tid] = o;
            o += c;
        }
    }
    __syncthreads();
    volatile uint32_t *my = woff[w];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = base + r * 64;
        const bool valid = i < A.items;
        const uint32_t d = (key[r] >> shift) & 255u;
        unsigned long long same = __ballot(valid);   // the valid lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const int rank = __popcll(same & below);
        uint32_t off = 0;
        if (valid) {
            off = my[d];
            const uint32_t pos = off + (uint32_t)rank;
            if ((int64_t)pos < A.items) {
                kout[pos] = key[r];
                iout[pos] = id[r];
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) my[d] = off + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
    }
}

// term of item (n, corner) of level l: coef * g[j] (header of this section), coef being Corner's
template <int D, int F, class E, bool SECOND, int I>
__device__ __forceinline__ void hs_term(const float *__restrict__ x, const E *__restrict__ g_y, const float *__restrict__ gg_x,
                                        const HashGridLevels &T, int l, int64_t n, int corner, float *out)
{
    const float s = LevelRef(T, l).scale;
    Cell<D> c = locate<D>(x + n * D, s);
    float d1[D], d2[D];
    if constexpr (I == NFA_INTERP_SMOOTHSTEP) smoothstep(c, d1, d2);
    const FVec<F> g = load_piece<F>(g_y, n * T.n_levels + l);
    const Corner<D> k(c, corner);
    float coef;
    if constexpr (SECOND) {
        static_assert(D == 3, "the second order is 3-D only");
        float v[3] = {gg_x[n * 3 + 0], gg_x[n * 3 + 1], gg_x[n * 3 + 2]}, u[3];
        if constexpr (I == NFA_INTERP_SMOOTHSTEP) { v[0] = v[0] * d1[0]; v[1] = v[1] * d1[1]; v[2] = v[2] * d1[2]; }
        k.signed_v(v, u);
        coef = k.second_order(u, s);
    } else {
        coef = k.first_order();
    }
#pragma unroll
    for (int j = 0; j < F; ++j) out[j] = coef * g.v[j];
}

template <int D, int F, class E, bool SECOND, int I>
__global__ __launch_bounds__(256) void hs_sum_kernel(const float *__restrict__ x, const E *__restrict__ g_y,
                                                     const float *__restrict__ gg_x, const HashGridLevels T,
                                                     const HashSortArgs A, float *__restrict__ g_params)
{
    __shared__ uint32_t sk[NFA_HS_TILE];
    __shared__ float sv[F * NFA_HS_TILE];
    const int l = A.first_level + (int)blockIdx.y;
    const HashSortView V = hs_view(A, (int)blockIdx.y);
    const int sorted = hs_passes(T.size[l]) & 1;
    const uint32_t *keys = V.keys(sorted), *ids = V.ids(sorted);
    const int64_t t0 = (int64_t)blockIdx.x * NFA_HS_TILE;
    const int cnt = (int)(A.items - t0 < NFA_HS_TILE ? A.items - t0 : NFA_HS_TILE);
    const int tid = (int)threadIdx.x;
    uint32_t key = 0;
    if (tid < cnt) {
        key = keys[t0 + tid];
        const uint32_t id = ids[t0 + tid];
        const int64_t n = (int64_t)(id >> D);
        float term[F];
#pragma unroll
        for (int j = 0; j < F; ++j) term[j] = 0.0f;
        if (n < A.n_points) hs_term<D, F, E, SECOND, I>(x, g_y, gg_x, T, l, n, (int)(id & ((1u << D) - 1u)), term);
#pragma unroll
        for (int j = 0; j < F; ++j) sv[j * NFA_HS_TILE + tid] = term[j];
    }
    sk[tid] = key;
    __syncthreads();
    if (tid < cnt && (tid == 0 || sk[tid - 1] != key)) {   // the first item of a segment
        float acc[F];
#pragma unroll
        for (int j = 0; j < F; ++j) acc[j] = sv[j * NFA_HS_TILE + tid];
        int p = tid;
        while (p + 1 < cnt && sk[p + 1] == key) {
            ++p;
#pragma unroll
            for (int j = 0; j < F; ++j) acc[j] = acc[j] + sv[j * NFA_HS_TILE + p];
        }
        const bool open_left = tid == 0 && t0 > 0 && keys[t0 - 1] == key;
        const bool open_right = p == cnt - 1 && t0 + cnt < A.items && keys[t0 + cnt] == key;
        float *dst = nullptr;
        if (open_right) dst = V.part + ((int64_t)blockIdx.x * 2 + 1) * 8;
        else if (open_left) dst = V.part + ((int64_t)blockIdx.x * 2) * 8;
        else if (key < T.size[l]) dst = g_params + ((size_t)T.offset[l] + key) * F;
        if (dst) {
#pragma unroll
            for (int j = 0; j < F; ++j) dst[j] = acc[j];
        }
    }
}

// Runs that cross tile borders: one thread per (tile, feature); the thread of the tile in which a run starts adds the run's
// segment sums in tile order (the tail of its tile, then whole tiles' tails, then the head of the tile where the run ends).
__global__ __launch_bounds__(256) void hs_carry_kernel(const HashGridLevels T, const HashSortArgs A, int F,
                                                       float *__restrict__ g_params)
{
    const int l = A.first_level + (int)blockIdx.y;
    const HashSortView V = hs_view(A, (int)blockIdx.y);
    const uint32_t *keys = V.keys(hs_passes(T.size[l]) & 1);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = idx / F;
    const int j = (int)(idx - t * F);
    if (t >= A.n_tiles) return;
    const int64_t t0 = t * NFA_HS_TILE, end = t0 + NFA_HS_TILE;
    if (end >= A.items) return;                                        // the last tile: nothing follows
    const uint32_t k = keys[end - 1];
    if (keys[end] != k) return;                                        // its last run ends with the tile
    if (t0 > 0 && keys[t0] == k && keys[t0 - 1] == k) return;          // the run started in an earlier tile
    float acc = V.part[(t * 2 + 1) * 8 + j];
    for (int64_t t2 = t + 1; t2 < A.n_tiles; ++t2) {
        const int64_t e2 = t2 * NFA_HS_TILE + NFA_HS_TILE;
        const bool more = e2 < A.items && keys[e2 - 1] == k && keys[e2] == k;   // the whole tile, and the run goes on
        acc = acc + V.part[(t2 * 2 + (more ? 1 : 0)) * 8 + j];
        if (!more) break;
    }
    if (k < T.size[l]) g_params[((size_t)T.offset[l] + k) * F + j] = acc;
}

static int hashsort_check(const char *name, const GridArgs &G, const void *scratch, int64_t scratch_bytes)
{
    NFA_REQUIRE(G.n_points < ((int64_t)1 << (32 - G.n_dims)), "%s: %d * n_points must be below 2^32 (got n_points %lld)", name,
                1 << G.n_dims, (long long)G.n_points);
    const HashSortPlan p = hashsort_plan(G.n_points, G.n_levels, G.n_dims);
    NFA_REQUIRE(scratch, "%s: scratch is null (a table gradient needs nfa_hashgrid_sorted_scratch_bytes bytes)", name);
    NFA_REQUIRE(aligned16(scratch), "%s: scratch must be 16-byte aligned", name);
    NFA_REQUIRE(scratch_bytes >= p.scratch_bytes, "%s: scratch too small (%lld bytes, %lld needed)", name,
                (long long)scratch_bytes, (long long)p.scratch_bytes);
    return NFA_OK;
}

// the table gradient of either order (gg_x: second) into the zeroed grad_params
template <class E>
static int hashsort_table_grad(const char *name, int32_t interp, const float *x, const E *grad_y, const float *gg_x,
                               const GridArgs &G, const HashGridLevels &T, float *grad_params, void *scratch, hipStream_t s)
{
    const HashSortPlan p = hashsort_plan(G.n_points, T.n_levels, G.n_dims);
    HashSortArgs A = {static_cast<unsigned char *>(scratch), p.level_bytes, p.items, p.n_blocks, p.n_tiles, G.n_points, 0};
    const dim3 block(256);
    for (int first = 0; first < T.n_levels; first += p.group) {
        const unsigned g = (unsigned)(T.n_levels - first < p.group ? T.n_levels - first : p.group);
        A.first_level = first;
        int passes = 0;
        for (unsigned k = 0; k < g; ++k) passes = passes > hs_passes(T.size[first + k]) ? passes : hs_passes(T.size[first + k]);
        dispatch_int<2, 3, 4>(G.n_dims, [&](auto d) {
            hipLaunchKernelGGL(hs_keys_kernel<d()>, dim3(grid_1d(p.items, 256), g), block, 0, s, x, T, A);
        });
        for (int pass = 0; pass < passes; ++pass) {
            hipLaunchKernelGGL(hs_count_kernel, dim3((unsigned)p.n_blocks, g), block, 0, s, T, A, pass);
            hipLaunchKernelGGL(hs_scan_kernel, dim3(256, g), block, 0, s, T, A, pass);
            hipLaunchKernelGGL(hs_scatter_kernel, dim3((unsigned)p.n_blocks, g), block, 0, s, T, A, pass);
        }
        const dim3 tiles((unsigned)p.n_tiles, g);
        if (gg_x)
            dispatch_grid<3>(G, interp, [&](auto d, auto f, auto i) {
                hipLaunchKernelGGL((hs_sum_kernel<d(), f(), E, true, i()>), tiles, block, 0, s, x, grad_y, gg_x, T, A, grad_params);
            });
        else
            dispatch_grid<2, 3, 4>(G, interp, [&](auto d, auto f, auto i) {
                hipLaunchKernelGGL((hs_sum_kernel<d(), f(), E, false, i()>), tiles, block, 0, s, x, grad_y, gg_x, T, A, grad_params);
            });
        hipLaunchKernelGGL(hs_carry_kernel, dim3((unsigned)ceil_div64(p.n_tiles * G.n_features, 256), g), block, 0, s, T, A,
                           (int)G.n_features, grad_params);
    }
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

template <class E>
static int hashgrid_bwd_sorted(int32_t interp, const float *x, const float *params, const E *grad_y, const GridArgs &G,
                               float *grad_params, float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream)
{
    if (!grad_params) return hashgrid_bwd(interp, x, params, grad_y, G, grad_params, grad_x, stream);
    HashGridLevels T;
    int rc = hashgrid_table("hashgrid_bwd_sorted", G, T);
    if (rc != NFA_OK) return rc;
    if (G.n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && grad_y && (params || !grad_x), "hashgrid_bwd_sorted: null pointer");
    NFA_REQUIRE(G.n_dims == 3 || all_aligned16(x, grad_x),
                "hashgrid_bwd_sorted: x and grad_x must be 16-byte aligned at n_dims %d", G.n_dims);
    NFA_REQUIRE((std::is_same<E, float>::value) || aligned16(grad_y), "hashgrid_bwd_sorted: a half grad_y must be 16-byte aligned");
    rc = hashsort_check("hashgrid_bwd_sorted", G, scratch, scratch_bytes);
    if (rc != NFA_OK) return rc;
    hipStream_t s = as_stream(stream);
    if (grad_x) {
        rc = hashgrid_bwd_launch(interp, x, params, grad_y, G, T, (float *)nullptr, grad_x, s);
        if (rc != NFA_OK) return rc;
    }
    return hashsort_table_grad<E>("hashgrid_bwd_sorted", interp, x, grad_y, nullptr, G, T, grad_params, scratch, s);
}

template <class E>
static int hashgrid_bwd_bwd_sorted(int32_t interp, const float *x, const float *params, const E *grad_y,
                                   const float *grad_grad_x, const GridArgs &G, E *grad_grad_y, float *grad_params,
                                   float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream)
{
    if (!grad_params)
        return hashgrid_bwd_bwd(interp, x, params, grad_y, grad_grad_x, G, grad_grad_y, grad_params, grad_x, stream);
    HashGridLevels T;
    int rc = hashgrid_table("hashgrid_bwd_bwd_sorted", G, T);
    if (rc != NFA_OK) return rc;
    if (G.n_points == 0) return NFA_OK;
    NFA_REQUIRE(grad_grad_x, "hashgrid_bwd_bwd_sorted: grad_grad_x is null");
    NFA_REQUIRE(x && grad_y && (params || !(grad_grad_y || grad_x)), "hashgrid_bwd_bwd_sorted: null pointer");
    NFA_REQUIRE((std::is_same<E, float>::value) || (aligned16(grad_y) && aligned16(grad_grad_y)),
                "hashgrid_bwd_bwd_sorted: half grad_y and grad_grad_y must be 16-byte aligned");
    rc = hashsort_check("hashgrid_bwd_bwd_sorted", G, scratch, scratch_bytes);
    if (rc != NFA_OK) return rc;
    hipStream_t s = as_stream(stream);
    if (grad_grad_y || grad_x) {
        rc = hashgrid_bwd_bwd_launch(interp, x, params, grad_y, grad_grad_x, G, T, grad_grad_y, (float *)nullptr, grad_x, s);
        if (rc != NFA_OK) return rc;
    }
    return hashsort_table_grad<E>("hashgrid_bwd_bwd_sorted", interp, x, grad_y, grad_grad_x, G, T, grad_params, scratch, s);
}

}  // namespace nfa

using namespace nfa;

#define ELEM_DISPATCH(name, elem, call)                                                        \
    int rc = NFA_OK;                                                                           \
    if (!dispatch_elem(elem, [&](auto tag) { using E = typename decltype(tag)::type; rc = call; })) \
        NFA_REQUIRE(false, name ": elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", (int)(elem)); \
    return rc

int nfa_hashgrid_fwd_d(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const float *params, int64_t n_points,
                       int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, void *y,
                       nfa_stream_t stream)
{
    if (check_interp("hashgrid_fwd", interp) != NFA_OK) return NFA_EINVAL;
    const GridArgs G = {n_dims, n_points, n_levels, n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host,
                        n_params};
    ELEM_DISPATCH("hashgrid_fwd", elem, hashgrid_fwd(interp, x, params, G, static_cast<E *>(y), stream));
}

int nfa_hashgrid_fwd_i(int32_t interp, int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_levels,
                       int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, void *y,
                       nfa_stream_t stream)
{
    return nfa_hashgrid_fwd_d(3, interp, elem, x, params, n_points, n_levels, n_features, log2_hashmap_size, scales_host,
                              resolutions_host, sizes_host, n_params, y, stream);
}

int nfa_hashgrid_fwd_t(int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_levels,
                       int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, void *y,
                       nfa_stream_t stream)
{
    return nfa_hashgrid_fwd_i(NFA_INTERP_LINEAR, elem, x, params, n_points, n_levels, n_features, log2_hashmap_size,
                              scales_host, resolutions_host, sizes_host, n_params, y, stream);
}

int nfa_hashgrid_fwd(const float *x, const float *params, int64_t n_points, int32_t n_levels, int32_t n_features,
                     int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                     const int32_t *sizes_host, int64_t n_params, float *y, nfa_stream_t stream)
{
    return nfa_hashgrid_fwd_t(NFA_ELEM_F32, x, params, n_points, n_levels, n_features, log2_hashmap_size, scales_host,
                              resolutions_host, sizes_host, n_params, y, stream);
}

int nfa_hashgrid_bwd_d(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                       int64_t n_points, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                       const float *scales_host, const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params,
                       float *grad_params, float *grad_x, nfa_stream_t stream)
{
    if (check_interp("hashgrid_bwd", interp) != NFA_OK) return NFA_EINVAL;
    const GridArgs G = {n_dims, n_points, n_levels, n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host,
                        n_params};
    ELEM_DISPATCH("hashgrid_bwd", elem,
                  hashgrid_bwd(interp, x, params, static_cast<const E *>(grad_y), G, grad_params, grad_x, stream));
}

int nfa_hashgrid_bwd_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                       int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                       float *grad_x, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_d(3, interp, elem, x, params, grad_y, n_points, n_levels, n_features, log2_hashmap_size, scales_host,
                              resolutions_host, sizes_host, n_params, grad_params, grad_x, stream);
}

int nfa_hashgrid_bwd_t(int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                       int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                       float *grad_x, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_i(NFA_INTERP_LINEAR, elem, x, params, grad_y, n_points, n_levels, n_features, log2_hashmap_size,
                              scales_host, resolutions_host, sizes_host, n_params, grad_params, grad_x, stream);
}

int nfa_hashgrid_bwd(const float *x, const float *params, const float *grad_y, int64_t n_points, int32_t n_levels,
                     int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                     const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                     float *grad_x, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_t(NFA_ELEM_F32, x, params, grad_y, n_points, n_levels, n_features, log2_hashmap_size, scales_host,
                              resolutions_host, sizes_host, n_params, grad_params, grad_x, stream);
}

int nfa_hashgrid_bwd_bwd_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                           const float *grad_grad_x, int64_t n_points, int32_t n_levels, int32_t n_features,
                           int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                           const int32_t *sizes_host, int64_t n_params, void *grad_grad_y, float *grad_params, float *grad_x,
                           nfa_stream_t stream)
{
    if (check_interp("hashgrid_bwd_bwd", interp) != NFA_OK) return NFA_EINVAL;
    const GridArgs G = {3, n_points, n_levels, n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host, n_params};
    ELEM_DISPATCH("hashgrid_bwd_bwd", elem, hashgrid_bwd_bwd(interp, x, params, static_cast<const E *>(grad_y), grad_grad_x, G,
                                                             static_cast<E *>(grad_grad_y), grad_params, grad_x, stream));
}

int nfa_hashgrid_bwd_bwd_t(int32_t elem, const float *x, const float *params, const void *grad_y, const float *grad_grad_x,
                           int64_t n_points, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                           const float *scales_host, const int32_t *resolutions_host, const int32_t *sizes_host,
                           int64_t n_params, void *grad_grad_y, float *grad_params, float *grad_x, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_bwd_i(NFA_INTERP_LINEAR, elem, x, params, grad_y, grad_grad_x, n_points, n_levels, n_features,
                                  log2_hashmap_size, scales_host, resolutions_host, sizes_host, n_params, grad_grad_y,
                                  grad_params, grad_x, stream);
}

int nfa_hashgrid_bwd_bwd(const float *x, const float *params, const float *grad_y, const float *grad_grad_x, int64_t n_points,
                         int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                         const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_grad_y,
                         float *grad_params, float *grad_x, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_bwd_t(NFA_ELEM_F32, x, params, grad_y, grad_grad_x, n_points, n_levels, n_features,
                                  log2_hashmap_size, scales_host, resolutions_host, sizes_host, n_params, grad_grad_y,
                                  grad_params, grad_x, stream);
}

int nfa_sh_fwd_t(int32_t elem, const float *dirs, int64_t n_points, int32_t degree, void *out, nfa_stream_t stream)
{
    ELEM_DISPATCH("sh_fwd", elem, sh_fwd(dirs, n_points, degree, static_cast<E *>(out), stream));
}

int nfa_sh_fwd(const float *dirs, int64_t n_points, int32_t degree, float *out, nfa_stream_t stream)
{
    return nfa_sh_fwd_t(NFA_ELEM_F32, dirs, n_points, degree, out, stream);
}

int nfa_sh_bwd_t(int32_t elem, const float *dirs, const void *grad_out, int64_t n_points, int32_t degree, float *grad_dirs,
                 nfa_stream_t stream)
{
    ELEM_DISPATCH("sh_bwd", elem, sh_bwd(dirs, static_cast<const E *>(grad_out), n_points, degree, grad_dirs, stream));
}

int nfa_sh_bwd(const float *dirs, const float *grad_out, int64_t n_points, int32_t degree, float *grad_dirs,
               nfa_stream_t stream)
{
    return nfa_sh_bwd_t(NFA_ELEM_F32, dirs, grad_out, n_points, degree, grad_dirs, stream);
}

int64_t nfa_hashgrid_sorted_scratch_bytes_d(int32_t n_dims, int64_t n_points, int32_t n_levels, int32_t log2_hashmap_size)
{
    (void)log2_hashmap_size;   // every level sorts all 2^D n_points items, whatever its size
    if (n_dims < 2 || n_dims > NFA_HG_MAX_DIMS) {
        set_error("hashgrid_sorted_scratch_bytes: n_dims must be 2, 3 or 4 (got %d)", n_dims);
        return -1;
    }
    if (n_points <= 0 || n_levels < 1) return 0;
    const HashSortPlan p = hashsort_plan(n_points, n_levels > NFA_HG_MAX_LEVELS ? NFA_HG_MAX_LEVELS : n_levels, n_dims);
    return p.scratch_bytes;
}

int64_t nfa_hashgrid_sorted_scratch_bytes(int64_t n_points, int32_t n_levels, int32_t log2_hashmap_size)
{
    return nfa_hashgrid_sorted_scratch_bytes_d(3, n_points, n_levels, log2_hashmap_size);
}

int nfa_hashgrid_bwd_sorted_d(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const float *params,
                              const void *grad_y, int64_t n_points, int32_t n_levels, int32_t n_features,
                              int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                              const int32_t *sizes_host, int64_t n_params, float *grad_params, float *grad_x, void *scratch,
                              int64_t scratch_bytes, nfa_stream_t stream)
{
    if (check_interp("hashgrid_bwd_sorted", interp) != NFA_OK) return NFA_EINVAL;
    const GridArgs G = {n_dims, n_points, n_levels, n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host,
                        n_params};
    ELEM_DISPATCH("hashgrid_bwd_sorted", elem,
                  hashgrid_bwd_sorted(interp, x, params, static_cast<const E *>(grad_y), G, grad_params, grad_x, scratch,
                                      scratch_bytes, stream));
}

int nfa_hashgrid_bwd_sorted_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                              int64_t n_points, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                              const float *scales_host, const int32_t *resolutions_host, const int32_t *sizes_host,
                              int64_t n_params, float *grad_params, float *grad_x, void *scratch, int64_t scratch_bytes,
                              nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_sorted_d(3, interp, elem, x, params, grad_y, n_points, n_levels, n_features, log2_hashmap_size,
                                     scales_host, resolutions_host, sizes_host, n_params, grad_params, grad_x, scratch,
                                     scratch_bytes, stream);
}

int nfa_hashgrid_bwd_sorted(int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                            int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                            const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                            float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_sorted_i(NFA_INTERP_LINEAR, elem, x, params, grad_y, n_points, n_levels, n_features,
                                     log2_hashmap_size, scales_host, resolutions_host, sizes_host, n_params, grad_params,
                                     grad_x, scratch, scratch_bytes, stream);
}

int nfa_hashgrid_bwd_bwd_sorted_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                                  const float *grad_grad_x, int64_t n_points, int32_t n_levels, int32_t n_features,
                                  int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                                  const int32_t *sizes_host, int64_t n_params, void *grad_grad_y, float *grad_params,
                                  float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream)
{
    if (check_interp("hashgrid_bwd_bwd_sorted", interp) != NFA_OK) return NFA_EINVAL;
    const GridArgs G = {3, n_points, n_levels, n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host, n_params};
    ELEM_DISPATCH("hashgrid_bwd_bwd_sorted", elem,
                  hashgrid_bwd_bwd_sorted(interp, x, params, static_cast<const E *>(grad_y), grad_grad_x, G,
                                          static_cast<E *>(grad_grad_y), grad_params, grad_x, scratch, scratch_bytes, stream));
}

int nfa_hashgrid_bwd_bwd_sorted(int32_t elem, const float *x, const float *params, const void *grad_y,
                                const float *grad_grad_x, int64_t n_points, int32_t n_levels, int32_t n_features,
                                int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                                const int32_t *sizes_host, int64_t n_params, void *grad_grad_y, float *grad_params,
                                float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream)
{
    return nfa_hashgrid_bwd_bwd_sorted_i(NFA_INTERP_LINEAR, elem, x, params, grad_y, grad_grad_x, n_points, n_levels,
                                         n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host, n_params,
                                         grad_grad_y, grad_params, grad_x, scratch, scratch_bytes, stream);
}

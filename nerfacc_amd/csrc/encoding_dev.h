// encoding_dev.h -- the device functions of the hash grid and of the spherical harmonics that more than one file uses: the
// kernels of encoding.hip and the fused field query of ngp_field.hip, which interpolates a point's levels straight into MFMA
// operand registers.  One copy of each step, so that both produce the same bits.  The formulas are in encoding.hip's header.
#pragma once
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

// One corner's share of the table gradient: w_c * dL/dy added to entry e of a zeroed float32 table gradient with no-return
// float atomics, for the fused field's training backward (ngp_field.hip).  It is hashgrid_bwd_kernel's statement word for word;
// that kernel keeps its own copy, because calling this one swaps the operands of its commutative multiplies in the generated
// code, and encoding.hip's device code is to stay what it is.
template <int F>
__device__ __forceinline__ void scatter_corner(float *g_params, uint32_t e, const float wc, const FVec<F> g)
{
    float *dst = g_params + (size_t)e * F;
#pragma unroll
    for (int j = 0; j < F; ++j) unsafeAtomicAdd(dst + j, wc * g.v[j]);
}

// K consecutive halves (E = fp16 or bf16) at p as floats, K = 1, 2, 4 or a multiple of 8: pieces of 2, 4, 8 or 16 bytes; p is
// aligned to the piece.
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

// A point's F values of a level (piece = n * n_levels + l) as floats: float as one FVec<F>, halves as 2 F bytes
template <int F, class E>
__device__ __forceinline__ FVec<F> load_piece(const E *__restrict__ p, int64_t piece)
{
    FVec<F> v;
    if constexpr (std::is_same<E, float>::value) v = reinterpret_cast<const FVec<F> *>(p)[piece];
    else load_elems<F>(p + piece * F, v.v);
    return v;
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

// The body of an extern "C" entry that takes an element code: `call` with E the element type, or NFA_EINVAL under `name`
#define ELEM_DISPATCH(name, elem, call)                                                        \
    int rc = NFA_OK;                                                                           \
    if (!nfa::dispatch_elem(elem, [&](auto tag) { using E = typename decltype(tag)::type; rc = call; })) \
        NFA_REQUIRE(false, name ": elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", (int)(elem)); \
    return rc

}  // namespace nfa

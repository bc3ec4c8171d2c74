// sinenc.hip -- NeRF's sinusoidal (positional) encoding, the front end of the reference's MLP fields
// (ref: examples/radiance_fields/mlp.py, SinusoidalEncoder), forward, backward and the derivative of the backward.
//
// x [N, D], D in 1..4; L = n_freqs in 0..16 frequencies s_k = 2^(min_deg + k), k < L; K = (identity ? D : 0) + 2 L D columns:
//   out[n, d]                      = x[n, d]                       (identity; a copy: bitwise x)
//   out[n, id + k D + d]           = a_kd sin(xb),  xb = s_k x[n, d]                 (id = identity ? D : 0; xb is exact)
//   out[n, id + L D + k D + d]     = a_kd cos(xb)
//   a_kd = w_k * exp(-1/2 s_k^2 var[n, d])       (w = freq_weights or 1, the exp factor only with var: mip-NeRF's
//                                                 integrated encoding with a diagonal covariance)
// The reference forms its cosine block as sin(fl32(xb + pi/2)); here cos(xb) is evaluated itself, which differs from the
// reference by at most its rounding of that phase, 2^-22 max(1, |xb|) ("Sinusoidal encoding").
// All arithmetic is float32, every operation rounded on its own (-ffp-contract=off); sine and cosine are the device
// library's sincosf (one call per (n, k, d), shared by both blocks), exp its expf: no fast approximation anywhere.
//   a = w_k, then a = a * expf((-0.5f * (s_k * s_k)) * var);  out_sin = sin * a, out_cos = cos * a  (nothing is multiplied
//   when neither var nor freq_weights is given; w = 1 and var = 0 give the same bits as that).
//
// Backward (g = dL/dout; g_sin / g_cos the two columns of (k, d); out is recomputed, nothing but x is kept):
//   tx_kd = (s_k * a) * (g_sin * cos - g_cos * sin)        tv_kd = (s_k * s_k) * (g_sin * (a * sin) + g_cos * (a * cos))
//   grad_x[n, d]   = ((g_id + tx_0d) + tx_1d) + ...         (g_id: the identity column's gradient, 0 without identity)
//   grad_var[n, d] = -0.5f * (((0 + tv_0d) + tv_1d) + ...)
// Second order (no var): for v = gg_x[n, d], the derivative of grad_x towards g and towards x,
//   grad_grad_out: identity v;  sine (v * (s_k * w_k)) * cos;  cosine -((v * (s_k * w_k)) * sin)
//   grad_x[n, d] = -(((0 + q_0d) + q_1d) + ...),   q_kd = (v * (s_k * (s_k * w_k))) * (g_sin * sin + g_cos * cos)
// Every sum runs over k ascending in one lane: no atomics, the same bits on every run.
//
// Layout.  A row is K elements (63, 27, 18, 9, ..): not a multiple of 16 bytes, so a lane per point would store K scalars
// strided by the row.  Instead a workgroup of 256 lanes owns a tile of 64 consecutive points, whose K-element rows are one
// contiguous span of the flat [N K] stream that starts on a 16-byte boundary (64 K elements of 2 or 4 bytes).  The tile is
// staged in LDS as float32 [64, K]:
//   * streams (out, grad_out, grad_grad_out) move between LDS and memory as pieces of 4 elements, lane i of the workgroup
//     the piece i, i + 256, ..: 16-byte pieces (float32) or 8-byte pieces (fp16 / bf16), contiguous across the lanes of a
//     wave whatever K is; the at most 3 elements after the last whole piece of the LAST tile go one by one;
//   * the trigonometry runs one (point, k, d) item per lane, item i = p (L D) + k D + d, so consecutive lanes write
//     consecutive LDS words (no bank conflicts at any K) and every lane of the workgroup has work (64 L D items);
//   * the sums over k run one (point, d) per lane over the tile in LDS.
// Half element types are widened as a piece is loaded and rounded once as it is stored.
#include "common.hip.h"
#include "axis.h"   // store_elem / load_elem

namespace nfa {

#define NFA_SINENC_POINTS 64
#define NFA_SINENC_BLOCK 256

struct SinDesc {
    int32_t D, L, min_deg, id;   // id: the identity columns (D or 0)
    int32_t DL, K;               // L D and the row length id + 2 L D
    float rD, rDL;               // 1 / D, 1 / (L D): i / D = (int)((i + 0.5f) * rD) for i < 2^12 (the quotient's distance
                                 // from an integer is at least 1 / 128, the product's error below 2^-11)
};

extern __shared__ __attribute__((aligned(16))) float sin_tile[];

template <class E>
__device__ __forceinline__ void load_piece(const E *p, float (&v)[4])
{
    if constexpr (std::is_same<E, float>::value) {
        const nfa_v4f t = *reinterpret_cast<const nfa_v4f *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        const nfa_v2u w = *reinterpret_cast<const nfa_v2u *>(p);
        v[0] = unpack_half<E>(w.x, 0); v[1] = unpack_half<E>(w.x, 1); v[2] = unpack_half<E>(w.y, 0); v[3] = unpack_half<E>(w.y, 1);
    }
}
template <class E>
__device__ __forceinline__ void store_piece(E *p, const nfa_v4f v)
{
    if constexpr (std::is_same<E, float>::value) {
        *reinterpret_cast<nfa_v4f *>(p) = v;
    } else {
        const nfa_v2u w = {pack_halves<E>(v.x, v.y), pack_halves<E>(v.z, v.w)};
        *reinterpret_cast<nfa_v2u *>(p) = w;
    }
}
// `cnt` elements of a stream from g (on a 16-byte boundary) into the tile, and back
template <class E>
__device__ __forceinline__ void tile_load(const E *__restrict__ g, int cnt, float *tile)
{
    const int n_pieces = cnt >> 2;
    for (int i = (int)threadIdx.x; i < n_pieces; i += NFA_SINENC_BLOCK) {
        float v[4];
        load_piece(g + 4 * i, v);
        *reinterpret_cast<nfa_v4f *>(tile + 4 * i) = nfa_v4f{v[0], v[1], v[2], v[3]};
    }
    const int i = (n_pieces << 2) + (int)threadIdx.x;   // (at most 3 elements are left)
    if (i < cnt) tile[i] = load_elem(g + i);
}
template <class E>
__device__ __forceinline__ void tile_store(E *__restrict__ g, int cnt, const float *tile)
{
    const int n_pieces = cnt >> 2;
    for (int i = (int)threadIdx.x; i < n_pieces; i += NFA_SINENC_BLOCK)
        store_piece(g + 4 * i, *reinterpret_cast<const nfa_v4f *>(tile + 4 * i));
    const int i = (n_pieces << 2) + (int)threadIdx.x;   // (at most 3 elements are left)
    if (i < cnt) store_elem(g + i, tile[i]);
}

// item i of a tile -> (point p, column j = k D + d of a block, k, d)
struct SinItem { int p, j, k, d; };
__device__ __forceinline__ SinItem sin_item(const SinDesc &S, int i)
{
    SinItem it;
    it.p = (int)(((float)i + 0.5f) * S.rDL);
    it.j = i - it.p * S.DL;
    it.k = (int)(((float)it.j + 0.5f) * S.rD);
    it.d = it.j - it.k * S.D;
    return it;
}
__device__ __forceinline__ float sin_scale(const SinDesc &S, int k) { return ldexpf(1.0f, S.min_deg + k); }
// a_kd; e = the point's element n D + d
__device__ __forceinline__ float sin_amp(const float *__restrict__ var, const float *__restrict__ fw, int64_t e, int k, float sc)
{
    float a = fw != nullptr ? fw[k] : 1.0f;
    if (var != nullptr) a = a * expf((-0.5f * (sc * sc)) * var[e]);
    return a;
}

// A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ..; the tile at point n0 holds tile_points(..) points.
__device__ __forceinline__ int tile_points(int64_t n_points, int64_t n0)
{
    return n_points - n0 < NFA_SINENC_POINTS ? (int)(n_points - n0) : NFA_SINENC_POINTS;
}

template <class E, bool MOD>   // MOD: var or freq_weights is given
__global__ __launch_bounds__(NFA_SINENC_BLOCK) void sinenc_fwd_kernel(const float *__restrict__ x, const float *__restrict__ var,
                                                                      const float *__restrict__ fw, int64_t n_points,
                                                                      const SinDesc S, E *__restrict__ out)
{
    float *tile = sin_tile;
    for (int64_t n0 = (int64_t)blockIdx.x * NFA_SINENC_POINTS; n0 < n_points; n0 += (int64_t)gridDim.x * NFA_SINENC_POINTS) {
        const int np = tile_points(n_points, n0);
        const float *xt = x + n0 * S.D;
        if (S.id) {
            for (int i = (int)threadIdx.x; i < np * S.D; i += NFA_SINENC_BLOCK) {
                const int p = (int)(((float)i + 0.5f) * S.rD);
                tile[p * S.K + (i - p * S.D)] = xt[i];
            }
        }
        for (int i = (int)threadIdx.x; i < np * S.DL; i += NFA_SINENC_BLOCK) {
            const SinItem it = sin_item(S, i);
            const int e = it.p * S.D + it.d;
            const float sc = sin_scale(S, it.k);
            float s, c;
            sincosf(xt[e] * sc, &s, &c);
            if constexpr (MOD) {
                const float a = sin_amp(var, fw, n0 * S.D + e, it.k, sc);
                s = s * a;
                c = c * a;
            }
            float *row = tile + it.p * S.K + S.id + it.j;
            row[0] = s;
            row[S.DL] = c;
        }
        __syncthreads();
        tile_store(out + n0 * S.K, np * S.K, tile);
        __syncthreads();   // (the next tile overwrites this one)
    }
}

// grad_x and grad_var are each optional, at least one
template <class E, bool MOD>
__global__ __launch_bounds__(NFA_SINENC_BLOCK) void sinenc_bwd_kernel(const float *__restrict__ x, const float *__restrict__ var,
                                                                      const float *__restrict__ fw, const E *__restrict__ g,
                                                                      int64_t n_points, const SinDesc S, float *__restrict__ grad_x,
                                                                      float *__restrict__ grad_var)
{
    float *tile = sin_tile;
    for (int64_t n0 = (int64_t)blockIdx.x * NFA_SINENC_POINTS; n0 < n_points; n0 += (int64_t)gridDim.x * NFA_SINENC_POINTS) {
        const int np = tile_points(n_points, n0);
        const float *xt = x + n0 * S.D;
        tile_load(g + n0 * S.K, np * S.K, tile);
        __syncthreads();
        // the item's two gradients are replaced by its terms tx (sine slot) and tv (cosine slot)
        for (int i = (int)threadIdx.x; i < np * S.DL; i += NFA_SINENC_BLOCK) {
            const SinItem it = sin_item(S, i);
            const int e = it.p * S.D + it.d;
            const float sc = sin_scale(S, it.k);
            float s, c;
            sincosf(xt[e] * sc, &s, &c);
            float a = 1.0f;
            if constexpr (MOD) a = sin_amp(var, fw, n0 * S.D + e, it.k, sc);
            float *row = tile + it.p * S.K + S.id + it.j;
            const float gs = row[0], gc = row[S.DL];
            row[0] = (sc * a) * (gs * c - gc * s);
            if (grad_var != nullptr) row[S.DL] = (sc * sc) * (gs * (a * s) + gc * (a * c));
        }
        __syncthreads();
        for (int i = (int)threadIdx.x; i < np * S.D; i += NFA_SINENC_BLOCK) {
            const int p = (int)(((float)i + 0.5f) * S.rD), d = i - p * S.D;
            const float *row = tile + p * S.K;
            if (grad_x != nullptr) {
                float acc = S.id ? row[d] : 0.0f;
                for (int k = 0; k < S.L; ++k) acc = acc + row[S.id + k * S.D + d];
                grad_x[n0 * S.D + i] = acc;
            }
            if (grad_var != nullptr) {
                float acc = 0.0f;
                for (int k = 0; k < S.L; ++k) acc = acc + row[S.id + S.DL + k * S.D + d];
                grad_var[n0 * S.D + i] = -0.5f * acc;
            }
        }
        __syncthreads();
    }
}

// grad_grad_out and grad_x are each optional, at least one; g is read only for grad_x.  LDS: the tile, then the
// [64, L D] terms q.
template <class E>
__global__ __launch_bounds__(NFA_SINENC_BLOCK) void sinenc_bwd_bwd_kernel(const float *__restrict__ x, const float *__restrict__ fw,
                                                                          const E *__restrict__ g, const float *__restrict__ gg_x,
                                                                          int64_t n_points, const SinDesc S, E *__restrict__ gg_out,
                                                                          float *__restrict__ grad_x)
{
    float *tile = sin_tile, *terms = sin_tile + NFA_SINENC_POINTS * S.K;
    for (int64_t n0 = (int64_t)blockIdx.x * NFA_SINENC_POINTS; n0 < n_points; n0 += (int64_t)gridDim.x * NFA_SINENC_POINTS) {
        const int np = tile_points(n_points, n0);
        const float *xt = x + n0 * S.D, *vt = gg_x + n0 * S.D;
        if (grad_x != nullptr) {
            tile_load(g + n0 * S.K, np * S.K, tile);
            __syncthreads();
        }
        if (S.id) {
            for (int i = (int)threadIdx.x; i < np * S.D; i += NFA_SINENC_BLOCK) {
                const int p = (int)(((float)i + 0.5f) * S.rD);
                tile[p * S.K + (i - p * S.D)] = vt[i];
            }
        }
        for (int i = (int)threadIdx.x; i < np * S.DL; i += NFA_SINENC_BLOCK) {
            const SinItem it = sin_item(S, i);
            const int e = it.p * S.D + it.d;
            const float sc = sin_scale(S, it.k);
            float s, c;
            sincosf(xt[e] * sc, &s, &c);
            const float sw = sc * (fw != nullptr ? fw[it.k] : 1.0f), v = vt[e];
            float *row = tile + it.p * S.K + S.id + it.j;
            if (grad_x != nullptr) terms[i] = (v * (sc * sw)) * (row[0] * s + row[S.DL] * c);
            const float vs = v * sw;
            row[0] = vs * c;
            row[S.DL] = -(vs * s);
        }
        __syncthreads();
        if (gg_out != nullptr) tile_store(gg_out + n0 * S.K, np * S.K, tile);
        if (grad_x != nullptr) {
            for (int i = (int)threadIdx.x; i < np * S.D; i += NFA_SINENC_BLOCK) {
                const int p = (int)(((float)i + 0.5f) * S.rD), d = i - p * S.D;
                const float *q = terms + p * S.DL + d;
                float acc = 0.0f;
                for (int k = 0; k < S.L; ++k) acc = acc + q[k * S.D];
                grad_x[n0 * S.D + i] = -acc;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host side
struct SinArgs {
    int32_t elem;
    int64_t n_points;
    int32_t n_dims, min_deg, n_freqs, identity;
};
// The checks every entry shares, in this order: elem, n_dims, n_freqs, min_deg, n_points.
static int sin_desc(const char *name, const SinArgs &A, SinDesc &S)
{
    NFA_REQUIRE(A.elem == NFA_ELEM_F32 || A.elem == NFA_ELEM_F16 || A.elem == NFA_ELEM_BF16,
                "%s: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", name, A.elem);
    NFA_REQUIRE(A.n_dims >= 1 && A.n_dims <= 4, "%s: n_dims must be in 1..4 (got %d)", name, A.n_dims);
    NFA_REQUIRE(A.n_freqs >= 0 && A.n_freqs <= 16, "%s: n_freqs must be in 0..16 (got %d)", name, A.n_freqs);
    NFA_REQUIRE(A.min_deg >= -16 && A.min_deg + A.n_freqs <= 32, "%s: min_deg must be in -16..32 - n_freqs (got %d)", name, A.min_deg);
    NFA_REQUIRE(A.n_points >= 0, "%s: negative n_points", name);
    NFA_REQUIRE(A.n_points < ((int64_t)1 << 31), "%s: too many points (at most 2^31 - 1)", name);
    S.D = A.n_dims;
    S.L = A.n_freqs;
    S.min_deg = A.min_deg;
    S.id = A.identity ? A.n_dims : 0;
    S.DL = S.D * S.L;
    S.K = S.id + 2 * S.DL;
    S.rD = 1.0f / (float)S.D;
    S.rDL = S.DL ? 1.0f / (float)S.DL : 0.0f;
    return NFA_OK;
}
static unsigned sin_grid(int64_t n_points) { return grid_1d(n_points, NFA_SINENC_POINTS, 256 * 8); }

static int sinenc_fwd(const SinArgs &A, const float *x, const float *var, const float *fw, void *out, nfa_stream_t stream)
{
    const char *name = "sinenc_fwd";
    SinDesc S;
    const int rc = sin_desc(name, A, S);
    if (rc != NFA_OK) return rc;
    if (A.n_points == 0 || S.K == 0) return NFA_OK;
    NFA_REQUIRE(x && out, "%s: null pointer", name);
    NFA_REQUIRE(aligned16(out), "%s: out must be 16-byte aligned", name);
    const size_t lds = (size_t)NFA_SINENC_POINTS * S.K * sizeof(float);
    dispatch_elem(A.elem, [&](auto tag) {
        using E = typename decltype(tag)::type;
        dispatch_bool(var != nullptr || fw != nullptr, [&](auto mod) {
            hipLaunchKernelGGL((sinenc_fwd_kernel<E, mod()>), dim3(sin_grid(A.n_points)), dim3(NFA_SINENC_BLOCK), lds, as_stream(stream),
                               x, var, fw, A.n_points, S, static_cast<E *>(out));
        });
    });
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

static int sinenc_bwd(const SinArgs &A, const float *x, const float *var, const float *fw, const void *grad_out, float *grad_x,
                      float *grad_var, nfa_stream_t stream)
{
    const char *name = "sinenc_bwd";
    SinDesc S;
    const int rc = sin_desc(name, A, S);
    if (rc != NFA_OK) return rc;
    if (A.n_points == 0 || S.K == 0) return NFA_OK;
    NFA_REQUIRE(x && grad_out && (grad_x || grad_var), "%s: null pointer", name);
    NFA_REQUIRE(grad_var == nullptr || var != nullptr, "%s: grad_var without var", name);
    NFA_REQUIRE(aligned16(grad_out), "%s: grad_out must be 16-byte aligned", name);
    const size_t lds = (size_t)NFA_SINENC_POINTS * S.K * sizeof(float);
    dispatch_elem(A.elem, [&](auto tag) {
        using E = typename decltype(tag)::type;
        dispatch_bool(var != nullptr || fw != nullptr, [&](auto mod) {
            hipLaunchKernelGGL((sinenc_bwd_kernel<E, mod()>), dim3(sin_grid(A.n_points)), dim3(NFA_SINENC_BLOCK), lds, as_stream(stream),
                               x, var, fw, static_cast<const E *>(grad_out), A.n_points, S, grad_x, grad_var);
        });
    });
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

static int sinenc_bwd_bwd(const SinArgs &A, const float *x, const float *fw, const void *grad_out, const float *gg_x,
                          void *grad_grad_out, float *grad_x, nfa_stream_t stream)
{
    const char *name = "sinenc_bwd_bwd";
    SinDesc S;
    const int rc = sin_desc(name, A, S);
    if (rc != NFA_OK) return rc;
    if (A.n_points == 0 || S.K == 0) return NFA_OK;
    NFA_REQUIRE(x && grad_out && gg_x && (grad_grad_out || grad_x), "%s: null pointer", name);
    NFA_REQUIRE(aligned16(grad_out) && aligned16(grad_grad_out), "%s: grad_out and grad_grad_out must be 16-byte aligned", name);
    const size_t lds = (size_t)NFA_SINENC_POINTS * (S.K + S.DL) * sizeof(float);
    dispatch_elem(A.elem, [&](auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL((sinenc_bwd_bwd_kernel<E>), dim3(sin_grid(A.n_points)), dim3(NFA_SINENC_BLOCK), lds, as_stream(stream), x, fw,
                           static_cast<const E *>(grad_out), gg_x, A.n_points, S, static_cast<E *>(grad_grad_out), grad_x);
    });
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int nfa_sinenc_fwd(int32_t elem, const float *x, const float *var, const float *freq_weights, int64_t n_points, int32_t n_dims,
                   int32_t min_deg, int32_t n_freqs, int32_t identity, void *out, nfa_stream_t stream)
{
    return sinenc_fwd(SinArgs{elem, n_points, n_dims, min_deg, n_freqs, identity}, x, var, freq_weights, out, stream);
}

int nfa_sinenc_bwd(int32_t elem, const float *x, const float *var, const float *freq_weights, const void *grad_out, int64_t n_points,
                   int32_t n_dims, int32_t min_deg, int32_t n_freqs, int32_t identity, float *grad_x, float *grad_var,
                   nfa_stream_t stream)
{
    return sinenc_bwd(SinArgs{elem, n_points, n_dims, min_deg, n_freqs, identity}, x, var, freq_weights, grad_out, grad_x, grad_var,
                      stream);
}

int nfa_sinenc_bwd_bwd(int32_t elem, const float *x, const float *freq_weights, const void *grad_out, const float *gg_x,
                       int64_t n_points, int32_t n_dims, int32_t min_deg, int32_t n_freqs, int32_t identity, void *grad_grad_out,
                       float *grad_x, nfa_stream_t stream)
{
    return sinenc_bwd_bwd(SinArgs{elem, n_points, n_dims, min_deg, n_freqs, identity}, x, freq_weights, grad_out, gg_x, grad_grad_out,
                          grad_x, stream);
}

// mlp_tiles.h -- what the fused MLP passes share (mlp.hip: weights resident in the LDS; mlp_stream.hip: weights streamed through
// it): the shape arithmetic, the packed weight image and its pack kernel, the MFMA fragment conversions and the staged store.
// The image format, the k orders and the rounding points are described at the top of mlp.hip.
#pragma once
#include "common.hip.h"

namespace nfa {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int MLP_WAVES = 4;                              // waves per workgroup of the fused passes
constexpr int STAGE_LD = 33;                              // floats per row of a wave's 32 x 32 store staging tile (odd: no conflicts)
constexpr int64_t STAGE_BYTES = (int64_t)MLP_WAVES * 32 * STAGE_LD * 4;
constexpr int64_t LDS_BUDGET = 160 * 1024;

struct Shape {
    int32_t n_in, n_out, W, n_hidden;
    int32_t bias;        // every layer has a float32 bias, behind the matrices in the flat parameters
    int32_t skip_mask;   // bit l (2 <= l <= n_hidden): layer l is a cat layer, its input is [H_{l-1}, x]
    __host__ __device__ int layers() const { return n_hidden + 1; }
    __host__ __device__ bool cat(int l) const { return (skip_mask >> l) & 1; }
    __host__ __device__ int in_dim(int l) const { return l == 0 ? n_in : W + (cat(l) ? n_in : 0); }
    __host__ __device__ int out_dim(int l) const { return l == n_hidden ? n_out : W; }
    __host__ __device__ int64_t bias_off(int l) const   // of b_l in the flat parameters; bias_off(layers()) is their number with biases
    {
        int64_t o = master_off(layers());
        for (int i = 0; i < l; ++i) o += out_dim(i);
        return o;
    }
    __host__ __device__ int64_t n_params() const { return bias ? bias_off(layers()) : master_off(layers()); }
    // floats of the biases as a forward pass holds them in LDS: layer l at l W, the output layer padded to 32 rows with zeros
    __host__ __device__ int lds_bias_floats() const { return bias ? n_hidden * W + 32 : 0; }
    // the same for a streamed forward pass, whose output layer has up to nine row tiles
    __host__ __device__ int stream_bias_floats() const { return bias ? n_hidden * W + (n_out + 31) / 32 * 32 : 0; }
    __host__ __device__ int64_t master_off(int l) const
    {
        int64_t o = 0;
        for (int i = 0; i < l; ++i) o += (int64_t)out_dim(i) * in_dim(i);
        return o;
    }
    // forward image: A = W_l; backward image: A = W_l^T
    __host__ __device__ int fwd_mt(int l) const { return (out_dim(l) + 31) / 32; }
    __host__ __device__ int fwd_kq(int l) const { return cat(l) ? W / 16 + (n_in + 15) / 16 : (in_dim(l) + 15) / 16; }
    __host__ __device__ int bwd_mt(int l) const { return (in_dim(l) + 31) / 32; }
    __host__ __device__ int bwd_kq(int l) const { return (out_dim(l) + 15) / 16; }
    __host__ __device__ int64_t fwd_off(int l) const   // in elements; fwd_off(layers()) is the image's size
    {
        int64_t o = 0;
        for (int i = 0; i < l; ++i) o += (int64_t)fwd_mt(i) * fwd_kq(i) * 512;
        return o;
    }
    __host__ __device__ int64_t bwd_off(int l) const
    {
        int64_t o = 0;
        for (int i = 0; i < l; ++i) o += (int64_t)bwd_mt(i) * bwd_kq(i) * 512;
        return o;
    }
};

__host__ __device__ inline int kpos(bool permuted, int h, int j) { return permuted ? 8 * (j >> 2) + 4 * h + (j & 3) : 8 * h + j; }
// row of a 32 x 32 accumulator tile that register `reg` of lane half h holds (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <class E>
__device__ __forceinline__ f32x16 mfma(nfa_v4u a, nfa_v4u b, f32x16 c)
{
    if constexpr (std::is_same<E, nfa_f16>::value)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---------------------------------------------------------------- packing

template <class E>
__global__ __launch_bounds__(256) void mlp_pack_kernel(Shape S, const float *__restrict__ params, uint16_t *__restrict__ fwd,
                                                       uint16_t *__restrict__ bwd, int64_t fwd_elems, int64_t bwd_elems)
{
    const int L = S.layers();
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < fwd_elems + bwd_elems; idx += (int64_t)gridDim.x * 256) {
        const bool is_bwd = idx >= fwd_elems;
        const int64_t e = is_bwd ? idx - fwd_elems : idx;
        int l = 0;
        int64_t off = 0;
        for (;; ++l) {
            const int64_t sz = (is_bwd ? (int64_t)S.bwd_mt(l) * S.bwd_kq(l) : (int64_t)S.fwd_mt(l) * S.fwd_kq(l)) * 512;
            if (e < off + sz || l == L - 1) break;
            off += sz;
        }
        const int64_t local = e - off;
        const int j = (int)(local & 7), lane = (int)((local >> 3) & 63);
        const int64_t blk = local >> 9;
        const int KQ = is_bwd ? S.bwd_kq(l) : S.fwd_kq(l);
        const int q = (int)(blk % KQ), m = (int)(blk / KQ);
        const int row = 32 * m + (lane & 31);
        // the B operand of a chain's first product comes from memory in natural k order: layer 0 forward, the last layer backward
        // and the x part of a cat layer forward, which starts on a k-step boundary (W is a multiple of 16)
        const bool permuted = is_bwd ? (l != L - 1) : (l != 0);
        const bool x_part = !is_bwd && S.cat(l) && q >= S.W / 16;
        const int k = x_part ? S.W + 16 * (q - S.W / 16) + kpos(false, lane >> 5, j) : 16 * q + kpos(permuted, lane >> 5, j);
        const int in = S.in_dim(l), out = S.out_dim(l);
        float v = 0.f;
        if (!is_bwd) { if (row < out && k < in) v = params[S.master_off(l) + (int64_t)row * in + k]; }
        else         { if (row < in && k < out) v = params[S.master_off(l) + (int64_t)k * in + row]; }
        (is_bwd ? bwd : fwd)[e] = (uint16_t)half_bits<E>(v);
    }
}

// ---------------------------------------------------------------- pieces shared by the passes

// Elements k0 .. k0+7 of row `row` of a [*, ld] matrix as a B fragment of element type E; columns >= ld read as zero.  The
// matrix holds float32 (rounded here) or E.  `vec`: ld is a multiple of 8 and the base is 16-byte aligned.
template <class E>
__device__ __forceinline__ nfa_v4u load_row8(const void *base, bool is_f32, int64_t row, int ld, int k0, bool vec)
{
    nfa_v4u f = {0u, 0u, 0u, 0u};
    if (vec) {
        if (k0 < ld) {
            if (is_f32) {
                const nfa_v4f *p = reinterpret_cast<const nfa_v4f *>(static_cast<const float *>(base) + row * ld + k0);
                const nfa_v4f a = p[0], b = p[1];
                f[0] = pack_halves<E>(a[0], a[1]); f[1] = pack_halves<E>(a[2], a[3]);
                f[2] = pack_halves<E>(b[0], b[1]); f[3] = pack_halves<E>(b[2], b[3]);
            } else {
                f = *reinterpret_cast<const nfa_v4u *>(static_cast<const uint16_t *>(base) + row * ld + k0);
            }
        }
    } else {
        uint32_t b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            b[j] = 0u;
            if (k0 + j < ld)
                b[j] = is_f32 ? half_bits<E>(static_cast<const float *>(base)[row * ld + k0 + j])
                              : (uint32_t)static_cast<const uint16_t *>(base)[row * ld + k0 + j];
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) f[d] = b[2 * d] | (b[2 * d + 1] << 16);
    }
    return f;
}

// registers 8s .. 8s+7 of an accumulator tile, rounded pairwise to E: the B fragment of k-step s of the next product
template <class E>
__device__ __forceinline__ nfa_v4u acc_frag(const f32x16 &a, int s)
{
    nfa_v4u f;
#pragma unroll
    for (int d = 0; d < 4; ++d) f[d] = pack_halves<E>(a[8 * s + 2 * d], a[8 * s + 2 * d + 1]);
    return f;
}

// The two fragments of tile t of a [*, W] half matrix's row p: 8-byte pieces at columns 32t + 8g + 4h, g = 0..3, which are
// registers 4g .. 4g+3 of the accumulator tile the fragments came from.
template <int W>
__device__ __forceinline__ void store_tile_row(uint16_t *m, int64_t p, int t, int h, const nfa_v4u &f0, const nfa_v4u &f1)
{
    nfa_v2u *d = reinterpret_cast<nfa_v2u *>(m + p * W + 32 * t + 4 * h);
    d[0] = nfa_v2u{f0[0], f0[1]};
    d[2] = nfa_v2u{f0[2], f0[3]};
    d[4] = nfa_v2u{f1[0], f1[1]};
    d[6] = nfa_v2u{f1[2], f1[3]};
}

// acc *= (H > 0) for tile t of row p of a saved [*, W] activation matrix H: the pieces store_tile_row wrote, register for register.
template <class E, int W>
__device__ __forceinline__ void mask_tile_row(f32x16 &acc, const uint16_t *m, int64_t p, int t, int h)
{
    const nfa_v2u *hp = reinterpret_cast<const nfa_v2u *>(m + p * W + 32 * t + 4 * h);
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const nfa_v2u hv = hp[2 * gq];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a = unpack_half<E>(hv[i >> 1], i & 1);
            acc[4 * gq + i] = a > 0.f ? acc[4 * gq + i] : 0.f;
        }
    }
}

// The B fragment of k-step s read back from row p of a [*, W] half matrix that store_tile_row wrote: the lane's own two pieces.
template <int W>
__device__ __forceinline__ nfa_v4u load_tile_frag(const uint16_t *m, int64_t p, int s, int h)
{
    const nfa_v2u *d = reinterpret_cast<const nfa_v2u *>(m + p * W + 16 * s + 4 * h);
    const nfa_v2u a = d[0], b = d[2];
    return nfa_v4u{a[0], a[1], b[0], b[1]};
}

// ---------------------------------------------------------------- activations (nfa_mlp_act; the ACT instantiations of mlp.hip)

// What an ACT instantiation takes beside the operands of the plain pass.  The codes and beta are wave-uniform.
struct ActOps {
    int32_t hidden = 0, output = 0;
    float beta = 1.f;
    const void *y = nullptr;            // the output as the forward stored it (the derivatives of the output activation)
    int32_t y_f32 = 0;
    const uint16_t *dz = nullptr;       // tangent: dZ_0 .. dZ_{L-1} and dZ_L of the first backward
    const uint16_t *dz_out = nullptr;
    uint16_t *r = nullptr;              // tangent: R_0 .. R_{L-1} (laid out as `hidden`) and R_L [N, n_out]; both or neither
    uint16_t *r_out = nullptr;
    const uint16_t *inject = nullptr;   // curvature: R_l, added to dH_l f'(H_l) before the rounding
};

// f(integral_constant<code>) for a wave-uniform activation code: one switch, the element loops inside the cases
template <class F>
__device__ __forceinline__ void act_switch(int code, F &&f)
{
    switch (code) {
    case NFA_MLP_ACT_RELU: f(std::integral_constant<int, NFA_MLP_ACT_RELU>{}); break;
    case NFA_MLP_ACT_LEAKY_RELU: f(std::integral_constant<int, NFA_MLP_ACT_LEAKY_RELU>{}); break;
    case NFA_MLP_ACT_SIGMOID: f(std::integral_constant<int, NFA_MLP_ACT_SIGMOID>{}); break;
    case NFA_MLP_ACT_TANH: f(std::integral_constant<int, NFA_MLP_ACT_TANH>{}); break;
    case NFA_MLP_ACT_SOFTPLUS: f(std::integral_constant<int, NFA_MLP_ACT_SOFTPLUS>{}); break;
    case NFA_MLP_ACT_EXPONENTIAL: f(std::integral_constant<int, NFA_MLP_ACT_EXPONENTIAL>{}); break;
    default: f(std::integral_constant<int, NFA_MLP_ACT_NONE>{}); break;
    }
}

constexpr bool act_has_rho(int code)
{
    return code == NFA_MLP_ACT_SIGMOID || code == NFA_MLP_ACT_TANH || code == NFA_MLP_ACT_SOFTPLUS || code == NFA_MLP_ACT_EXPONENTIAL;
}

// y = f(z), float32, the accurate device functions; the caller rounds once
template <int CODE>
__device__ __forceinline__ float act_value(float z, float beta)
{
    if constexpr (CODE == NFA_MLP_ACT_RELU) return z < 0.f ? 0.f : z;
    else if constexpr (CODE == NFA_MLP_ACT_LEAKY_RELU) return z > 0.f ? z : 0.01f * z;
    else if constexpr (CODE == NFA_MLP_ACT_SIGMOID) return 1.f / (1.f + expf(-z));
    else if constexpr (CODE == NFA_MLP_ACT_TANH) return tanhf(z);
    else if constexpr (CODE == NFA_MLP_ACT_SOFTPLUS) return (z > 0.f ? z : 0.f) + log1pf(expf(-beta * fabsf(z))) / beta;   // NaN: the log term
    else if constexpr (CODE == NFA_MLP_ACT_EXPONENTIAL) return expf(z);
    else return z;
}

// d * f'(y) from the stored y.  ReLU and LeakyReLU select (y = NaN counts as not positive), the others multiply.
template <int CODE>
__device__ __forceinline__ float act_times_deriv(float d, float y, float beta)
{
    if constexpr (CODE == NFA_MLP_ACT_RELU) return y > 0.f ? d : 0.f;
    else if constexpr (CODE == NFA_MLP_ACT_LEAKY_RELU) return y > 0.f ? d : 0.01f * d;
    else if constexpr (CODE == NFA_MLP_ACT_SIGMOID) return d * (y * (1.f - y));
    else if constexpr (CODE == NFA_MLP_ACT_TANH) return d * (1.f - y * y);
    else if constexpr (CODE == NFA_MLP_ACT_SOFTPLUS) return d * (1.f - expf(-beta * y));
    else if constexpr (CODE == NFA_MLP_ACT_EXPONENTIAL) return d * y;
    else return d;
}

// rho = f'' / f' from the stored y (only for the codes of act_has_rho)
template <int CODE>
__device__ __forceinline__ float act_rho(float y, float beta)
{
    if constexpr (CODE == NFA_MLP_ACT_SIGMOID) return 1.f - 2.f * y;
    else if constexpr (CODE == NFA_MLP_ACT_TANH) return -2.f * y;
    else if constexpr (CODE == NFA_MLP_ACT_SOFTPLUS) return beta * expf(-beta * y);
    else if constexpr (CODE == NFA_MLP_ACT_EXPONENTIAL) return 1.f;
    else return 0.f;
}

// R = (rho(y) dZ) A, an exact zero where rho is identically zero (never a product with it)
template <int CODE>
__device__ __forceinline__ float act_curvature(float a, float y, float dz, float beta)
{
    if constexpr (act_has_rho(CODE)) return (act_rho<CODE>(y, beta) * dz) * a;
    else return 0.f;
}

// acc = acc * f'(H) (+ inject) for tile t of row p: mask_tile_row for any activation, the pieces store_tile_row wrote
template <class E, int W, int CODE>
__device__ __forceinline__ void deriv_tile_row(f32x16 &acc, const uint16_t *m, const uint16_t *inject, int64_t p, int t, int h, float beta)
{
    const nfa_v2u *hp = reinterpret_cast<const nfa_v2u *>(m + p * W + 32 * t + 4 * h);
    const nfa_v2u *ip = reinterpret_cast<const nfa_v2u *>(inject + p * W + 32 * t + 4 * h);
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const nfa_v2u hv = hp[2 * gq];
        nfa_v2u iv = {0u, 0u};
        if (inject) iv = ip[2 * gq];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = act_times_deriv<CODE>(acc[4 * gq + i], unpack_half<E>(hv[i >> 1], i & 1), beta);
            acc[4 * gq + i] = inject ? d + unpack_half<E>(iv[i >> 1], i & 1) : d;
        }
    }
}

// The tangent's step at a hidden layer: rr = (rho(H) dZ) A (zero without `dz`), then acc = A * f'(H)
template <class E, int W, int CODE>
__device__ __forceinline__ void tangent_tile_row(f32x16 &acc, f32x16 &rr, const uint16_t *m, const uint16_t *dz, int64_t p, int t, int h,
                                                 float beta)
{
    const nfa_v2u *hp = reinterpret_cast<const nfa_v2u *>(m + p * W + 32 * t + 4 * h);
    const nfa_v2u *dp = reinterpret_cast<const nfa_v2u *>(dz + p * W + 32 * t + 4 * h);
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const nfa_v2u hv = hp[2 * gq];
        nfa_v2u dv = {0u, 0u};
        if (act_has_rho(CODE) && dz) dv = dp[2 * gq];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float y = unpack_half<E>(hv[i >> 1], i & 1), a = acc[4 * gq + i];
            rr[4 * gq + i] = dz ? act_curvature<CODE>(a, y, unpack_half<E>(dv[i >> 1], i & 1), beta) : 0.f;
            acc[4 * gq + i] = act_times_deriv<CODE>(a, y, beta);
        }
    }
}

// element `i` of a float32 or E matrix as float32
template <class E>
__device__ __forceinline__ float load_elem(const void *base, bool is_f32, int64_t i)
{
    return is_f32 ? static_cast<const float *>(base)[i] : half_value<E>(static_cast<const uint16_t *>(base)[i]);
}

// load_row8 of g * f_out'(y): dZ_L of a network with an output activation, rounded once
template <class E, int CODE>
__device__ __forceinline__ nfa_v4u load_row8_deriv(const void *g, bool g_f32, const void *y, bool y_f32, int64_t row, int ld, int k0, float beta)
{
    uint32_t b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        b[j] = 0u;
        if (k0 + j < ld) b[j] = half_bits<E>(act_times_deriv<CODE>(load_elem<E>(g, g_f32, row * ld + k0 + j), load_elem<E>(y, y_f32, row * ld + k0 + j), beta));
    }
    nfa_v4u f;
#pragma unroll
    for (int d = 0; d < 4; ++d) f[d] = b[2 * d] | (b[2 * d + 1] << 16);
    return f;
}

// The tangent's step at the output layer, on the accumulator tile o = A_L (rows = outputs): ro = (rho(y) dZ_L) A_L, o = f_out'(y) A_L
template <class E, int CODE>
__device__ __forceinline__ void tangent_out_tile(f32x16 &o, f32x16 &ro, const ActOps &A, int64_t p, int n_out, int h)
{
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = acc_row(reg, h);
        float y = 0.f, d = 0.f;
        if (CODE != NFA_MLP_ACT_NONE && row < n_out) y = load_elem<E>(A.y, A.y_f32 != 0, p * n_out + row);
        if (act_has_rho(CODE) && A.r_out && row < n_out) d = load_elem<E>(A.dz_out, false, p * n_out + row);
        const float a = o[reg];
        ro[reg] = A.r_out ? act_curvature<CODE>(a, y, d, A.beta) : 0.f;
        o[reg] = act_times_deriv<CODE>(a, y, A.beta);
    }
}

// An accumulator tile's start: rows 32m .. 32m+31 of a layer's float32 bias (lb: that tile's 32 floats in LDS), or zero.
__device__ __forceinline__ void init_acc(f32x16 &a, bool has_bias, const float *lb, int h)
{
    if (has_bias) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const nfa_v4f v = *reinterpret_cast<const nfa_v4f *>(lb + 8 * gq + 4 * h);   // acc_row(4 gq + i, h) = 8 gq + 4 h + i
#pragma unroll
            for (int i = 0; i < 4; ++i) a[4 * gq + i] = v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = 0.f;
    }
}

// A wave's 32 x 32 accumulator tile (row = column of the output matrix, column = point) to memory through its LDS staging
// tile, so that stores run along the output rows: columns col0 .. col0+ncols-1 of rows row0 .. row0+nrows-1 of out [*, ld].
template <class E>
__device__ __forceinline__ void stage_store(const f32x16 &acc, float *st, void *out, bool out_f32, int64_t row0, int nrows, int ld,
                                            int col0, int ncols, int lane)
{
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) st[r * STAGE_LD + acc_row(reg, h)] = acc[reg];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int total = nrows * ncols;
    for (int i = lane; i < total; i += NFA_WAVE) {
        const int pr = i / ncols, c = i - pr * ncols;
        const float v = st[pr * STAGE_LD + c];
        const int64_t gi = (row0 + pr) * ld + col0 + c;
        if (out_f32) static_cast<float *>(out)[gi] = v;
        else static_cast<uint16_t *>(out)[gi] = (uint16_t)half_bits<E>(v);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grad[e] = ((partials[0][e] + partials[1][e]) + ...): one order, whatever the launch
__global__ __launch_bounds__(256) void mlp_wgrad_sum_kernel(const float *__restrict__ partials, int64_t n_slices, int64_t P,
                                                            float *__restrict__ grad)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= P) return;
    float s = partials[e];
    for (int64_t k = 1; k < n_slices; ++k) s += partials[k * P + e];
    grad[e] = s;
}

// ---------------------------------------------------------------- host side

bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool row8_vec(const void *p, int ld) { return ld % 8 == 0 && aligned_to(p, 16); }

template <class Kern>
int allow_lds(const char *who, Kern kern, int64_t lds_bytes)
{
    if (lds_bytes <= 64 * 1024) return NFA_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) {
        set_error("%s: %lld bytes of LDS refused: %s", who, (long long)lds_bytes, hipGetErrorString(e));
        return NFA_EHIP;
    }
    return NFA_OK;
}

}  // namespace
}  // namespace nfa

// mlp.hip -- the field's network as fused half-precision MFMA passes: tiny-cuda-nn's FullyFusedMLP (no biases, ReLU on the
// hidden layers, no output activation), n_hidden + 1 weight matrices W_l [out_l, in_l] (torch's Linear layout), width 64 or 128;
// and, described by nfa_mlp_desc, the reference's MLP class: float32 biases b_l and skip connections (a "cat layer" l takes
// [H_{l-1}, x], its matrix is [out_l, W + n_in]).  The lines below are the plain chain; with both features
//   z_l = b_l + W_l in_l, in_l = [H_{l-1}, x] at a cat layer;  dx += W_l[:, W:]^T dZ_l and dW_l = dZ_l^T [H_{l-1}, x] there;
//   db_l = sum_p dZ_l[p, :];  the tangent starts every accumulator at zero and sees [T_{l-1}, v] at a cat layer.
// A bias is never rounded: it is the float32 value an MFMA accumulator starts from.
//
//   forward     H_0 = relu(x W_0^T), H_l = relu(H_{l-1} W_l^T), y = H_last W_L^T          one launch (nfa_mlp_fwd)
//   data grad   dZ_L = g, dH_{l-1} = dZ_l W_l, dZ_{l-1} = dH_{l-1} * (H_{l-1} > 0), dx = dZ_0 W_0   one launch (nfa_mlp_bwd_data)
//   weight grad dW_l = dZ_l^T H_{l-1}, H_{-1} = x                                         split-K + ordered sum (nfa_mlp_bwd_weights)
//   tangent     T_{-1} = v, T_l = (T_{l-1} W_l^T) * (H_l > 0), u = T_last W_L^T           one launch (nfa_mlp_tangent)
//
// The tangent pass is the second order: with v the cotangent of dx and s = <v, dx>, u = ds/dg and ds/dW_l = dZ_l^T T_{l-1}, which is
// the weight gradient pass run on (v, T) in the place of (x, H).  The masks are the saved ones, never a ReLU of the tangent.
//
// Activations (nfa_mlp_act, the ACT instantiations: one per type, width and pass, the general form, the codes run-time values
// switched once per layer): one hidden activation f and one output activation f_out of None, ReLU, LeakyReLU (slope 0.01f), Sigmoid,
// Tanh, Softplus (beta) and Exponential.  With y = f(z) as STORED (rounded), f' and rho = f'' / f' are formed from y, never from z:
//   forward     H_l = f(z_l), y = f_out(z_L)                                   float32, accurate expf / log1pf / tanhf, rounded once
//   data grad   dZ_L = g * f_out'(y), dZ_l = dH_l * f'(H_l)                    a select for ReLU and LeakyReLU, a product otherwise
//   tangent     A_l = W_l [T_{l-1}(, v)], T_l = A_l * f'(H_l), u = f_out'(y) * A_L; and R_l = (rho(H_l) dZ_l) A_l, R_L = (rho_out(y) dZ_L) A_L
//   curvature   E_L = R_L, E_{l-1} = (W_l^T E_l)[:W] * f'(H_{l-1}) + R_{l-1}, ds/dx = W_0^T E_0 + sum_cat W_l[:, W:]^T E_l
// The curvature pass is the data gradient's chain (the same kernel) with R injected before the rounding: the second derivative of
// an activation puts a cotangent into every layer.  ds/dW_l = dZ_l^T [T_{l-1}(, v)] + E_l^T [H_{l-1}(, x)] and ds/db_l = sum_p E_l[p]
// are the weight gradient pass twice.  Where rho is identically zero R is an exact zero, never a product with it.
//
// Everything works TRANSPOSED, with the weights as the A operand of v_mfma_f32_32x32x16_{f16,bf16}: a wave owns 32 points, a point
// is a COLUMN of every tile and so stays on lane (point & 31) of both lane halves through all layers.  The 32x32 float32 result
// of one layer has its rows (neurons) in the 16 accumulator registers of a lane; converted pairwise to half, registers
// 8s .. 8s+7 are the B fragment of k-step s of the next layer, with no lane movement and no LDS.  The k order inside such a step
// is permuted (element j of lane half h is row 16s + 8(j>>2) + 4h + (j&3)); the packed weight images absorb the permutation, so
// a lane's A fragment is one 16-byte LDS read whatever the layer.  A cat layer appends ceil(n_in / 16) k-steps in natural order
// behind its W / 16 permuted ones (forward image: their B fragments are rows of x from memory, as layer 0's are) and n_in rows
// behind its W rows (backward image: they feed dL/dx only).
//
// Packed image of a matrix A [rows, k] (rows padded to 32, k to 16, padding zero): blocks of 1 KiB, block (m, q) = rows
// 32m .. 32m+31, k-step q, at element ((m KQ + q) 64 + lane) 8 + j, lane = 32h + r: A[32m + r][16q + kpos(h, j)], with
// kpos = 8h + j where the B operand is loaded from memory (first product of a chain) and the permuted order above elsewhere.
// The forward image holds W_l, the backward image W_l^T (rows = inputs of the layer, k = its outputs).
//
// Rounding points (all to nearest even, the compiler's conversion; never the pkrtz form): x and the masters to the half type
// on load / when packed, every hidden activation after its ReLU, every dZ_l and T_l after its mask, y, dx and u once as stored (float32
// outputs are the accumulators themselves).  Products are exact in float32 and summed by the MFMA in float32.
//
// Number-format edges (IEEE arithmetic and torch.autograd's semantics; tests/test_mlp_edges_{cpu,gpu}.py):
//   1. every rounding above is ONE round-to-nearest-even of the exact float32 value over the whole range: results among the fp16
//      subnormals are kept (gradual underflow, ties to even), a value at or above MAX + ulp/2 becomes +-inf and one float32 step
//      below it MAX (fp16: 65520 -> inf, 65519.996 -> 65504; bf16: (2 - 2^-8) 2^127 -> inf), never saturated (bf16: pinned by
//      the tests' hand-built rows; their scaled bf16 cases pass 2^128 with one product, inf in the float32 accumulator already);
//   2. fp16 subnormals reach the MFMA un-flushed on both sides: as packed weights (A) and as x, H_l, dZ_l fragments (B);
//   3. relu(NaN) = NaN, relu(-inf) = 0, relu(+inf) = +inf; the backward's and the tangent's mask is a SELECT (dZ = dH where
//      H > 0, else 0, whatever dH is; H = NaN counts as not positive), never a multiplication by 0 or 1;
//   4. a non-finite value in row p of x, g or v changes row p of y, H_l, dZ_l, T_l, dx and u and nothing else in them, also for
//      p = N - 1 of a partial tile, whose clamped loads put that row into lanes that do not store;
//   5. an element of dL/dparams is NaN, +inf, -inf or finite exactly where IEEE sums of the rounded operands are (inf * 0 = NaN:
//      a padded zero never hides an infinity of a real row), and the finite ones are the same bits;
//   6. so an overflow that is born inside the backward (g * scale finite, dZ_l past MAX) reaches dL/dparams as inf or NaN and
//      DeviceGradScaler skips the step.
// Not covered: bf16 subnormals, overflow of a float32 accumulator, non-finite biases.
//
// EXEC is all ones around every MFMA: a partial tile clamps the point index of its loads and masks only its stores.
#include "mlp_tiles.h"

namespace nfa {
namespace {

__device__ __forceinline__ void stage_image(nfa_v4u *dst, const nfa_v4u *src, int64_t n16)
{
    for (int64_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// The shape as an instantiation sees it: without EXT both features are compile-time zeros, so every in_dim / k-step count folds
// to the plain chain's and the plain kernels are the code they were before the features existed.
template <bool EXT>
__device__ __forceinline__ Shape shape_of(Shape S)
{
    if constexpr (!EXT) { S.bias = 0; S.skip_mask = 0; }
    return S;
}

// ---------------------------------------------------------------- forward and tangent forward

// The layer chain W_L act(... act(W_0 in)) over the workgroup's tiles, for both passes that run it.  Forward: act = ReLU, the
// rounded activations go to `save` (the backward's `hidden`, optional).  TANGENT: act = the mask (mask_l > 0) of the activations
// the forward saved, the rounded T_l go to `save` (optional): the derivative of the chain along `in`, which is linear in it.
// `bias` (forward only; the tangent of a bias is zero): b_0 .. b_L float32, staged once behind the image; every accumulator
// starts from its rows.  A cat layer runs kq0 more k-steps whose B fragments are rows of `in`, loaded again as layer 0 loads them.
// ACT (implies EXT): the hidden and the output activation are the run-time codes of `A`, switched once per layer outside the element
// loops; the forward applies f, the tangent multiplies by f' formed from the saved activations and, given A.r, also writes
// R_l = (rho(H_l) dZ_l) A_l and R_L, the cotangents the curvature pass injects.
template <class E, int W, bool TANGENT, bool EXT, bool ACT = false>
__device__ __forceinline__ void mlp_chain(const Shape &S, const void *__restrict__ in, int in_f32, int in_vec,
                                          const uint16_t *__restrict__ image, int64_t image_elems, const float *__restrict__ bias,
                                          int64_t N, void *__restrict__ out, int out_f32, const uint16_t *__restrict__ mask,
                                          uint16_t *__restrict__ save, const ActOps &A = ActOps{})
{
    static_assert(EXT || !ACT, "ACT is an instantiation of the general form");
    constexpr int MT = W / 32, KQ = W / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_lds[];
    nfa_v4u *wimg = reinterpret_cast<nfa_v4u *>(mlp_lds);
    const bool has_bias = EXT && !TANGENT && S.bias != 0;
    float *lb = reinterpret_cast<float *>(mlp_lds + image_elems * 2);
    const int n_lb = has_bias ? S.lds_bias_floats() : 0;
    for (int i = threadIdx.x; i < n_lb; i += blockDim.x) {
        const int i_out = i - S.n_hidden * W;   // >= 0: row of the output layer, zero beyond n_out
        lb[i] = i_out < 0 || i_out < S.n_out ? bias[i] : 0.f;
    }
    stage_image(wimg, reinterpret_cast<const nfa_v4u *>(image), image_elems / 8);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    float *st = lb + n_lb + wave * 32 * STAGE_LD;
    const int kq0 = S.fwd_kq(0);
    const int64_t n_tiles = (N + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * MLP_WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * MLP_WAVES) {
        const int64_t p = tile * 32 + r, pc = p < N ? p : N - 1;
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) init_acc(acc[m], has_bias, lb + 32 * m, h);
        for (int q = 0; q < kq0; ++q) {
            const nfa_v4u b = load_row8<E>(in, in_f32 != 0, pc, S.n_in, 16 * q + 8 * h, in_vec != 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma<E>(wimg[(m * kq0 + q) * 64 + lane], b, acc[m]);
        }
        int64_t off16 = (int64_t)MT * kq0 * 64;   // in 16-byte fragments
        nfa_v4u hf[KQ];
        for (int l = 1;; ++l) {
            // H_{l-1} = relu(acc) (T_{l-1} = acc * (H_{l-1} > 0)), rounded: the next product's B fragments, and what the
            // backward (the second weight gradient) reads
            if constexpr (ACT) {
                act_switch(A.hidden, [&](auto code) __attribute__((always_inline)) {
                    constexpr int CODE = decltype(code)::value;
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if constexpr (TANGENT) {
                            f32x16 rr;
                            tangent_tile_row<E, W, CODE>(acc[t], rr, mask + (int64_t)(l - 1) * N * W,
                                                         A.r ? A.dz + (int64_t)(l - 1) * N * W : nullptr, pc, t, h, A.beta);
                            if (A.r && p < N)
                                store_tile_row<W>(A.r + (int64_t)(l - 1) * N * W, p, t, h, acc_frag<E>(rr, 0), acc_frag<E>(rr, 1));
                        } else {
#pragma unroll
                            for (int i = 0; i < 16; ++i) acc[t][i] = act_value<CODE>(acc[t][i], A.beta);
                        }
                        hf[2 * t] = acc_frag<E>(acc[t], 0);
                        hf[2 * t + 1] = acc_frag<E>(acc[t], 1);
                        if (save && p < N) store_tile_row<W>(save + (int64_t)(l - 1) * N * W, p, t, h, hf[2 * t], hf[2 * t + 1]);
                    }
                });
            } else {
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    if constexpr (TANGENT) {
                        mask_tile_row<E, W>(acc[t], mask + (int64_t)(l - 1) * N * W, pc, t, h);
                    } else {
#pragma unroll
                        for (int i = 0; i < 16; ++i) acc[t][i] = acc[t][i] < 0.f ? 0.f : acc[t][i];
                    }
                    hf[2 * t] = acc_frag<E>(acc[t], 0);
                    hf[2 * t + 1] = acc_frag<E>(acc[t], 1);
                    if (save && p < N) store_tile_row<W>(save + (int64_t)(l - 1) * N * W, p, t, h, hf[2 * t], hf[2 * t + 1]);
                }
            }
            if (l == S.n_hidden) break;
            const bool cat = EXT && S.cat(l);
            const int kql = KQ + (cat ? kq0 : 0);   // k-steps of this layer's image
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                init_acc(acc[m], has_bias, lb + l * W + 32 * m, h);
#pragma unroll
                for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(wimg[off16 + (m * kql + q) * 64 + lane], hf[q], acc[m]);
            }
            if (cat) {
                for (int q = 0; q < kq0; ++q) {
                    const nfa_v4u b = load_row8<E>(in, in_f32 != 0, pc, S.n_in, 16 * q + 8 * h, in_vec != 0);
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m] = mfma<E>(wimg[off16 + (m * kql + KQ + q) * 64 + lane], b, acc[m]);
                }
            }
            off16 += (int64_t)MT * kql * 64;
        }
        f32x16 o;
        init_acc(o, has_bias, lb + S.n_hidden * W, h);
#pragma unroll
        for (int q = 0; q < KQ; ++q) o = mfma<E>(wimg[off16 + q * 64 + lane], hf[q], o);
        if (EXT && S.cat(S.n_hidden)) {
            for (int q = 0; q < kq0; ++q) {
                const nfa_v4u b = load_row8<E>(in, in_f32 != 0, pc, S.n_in, 16 * q + 8 * h, in_vec != 0);
                o = mfma<E>(wimg[off16 + (KQ + q) * 64 + lane], b, o);
            }
        }
        const int64_t row0 = tile * 32;
        const int nrows = (int)(N - row0 < 32 ? N - row0 : 32);
        if constexpr (ACT && TANGENT) {   // u = f_out'(y) A_L, R_L = (rho_out(y) dZ_L) A_L
            f32x16 ro;
            act_switch(A.output, [&](auto code) __attribute__((always_inline)) {
                tangent_out_tile<E, decltype(code)::value>(o, ro, A, pc, S.n_out, h);
            });
            if (A.r_out) stage_store<E>(ro, st, A.r_out, false, row0, nrows, S.n_out, 0, S.n_out, lane);
        } else if constexpr (ACT) {
            act_switch(A.output, [&](auto code) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] = act_value<decltype(code)::value>(o[i], A.beta);
            });
        }
        stage_store<E>(o, st, out, out_f32 != 0, row0, nrows, S.n_out, 0, S.n_out, lane);
    }
}

template <class E, int W, bool EXT>
__global__ __launch_bounds__(MLP_WAVES * NFA_WAVE) void mlp_fwd_kernel(Shape S, const void *__restrict__ x, int x_f32, int x_vec,
                                                                      const uint16_t *__restrict__ image, int64_t image_elems,
                                                                      const float *__restrict__ bias, int64_t N,
                                                                      void *__restrict__ y, int y_f32, uint16_t *__restrict__ hidden)
{
    mlp_chain<E, W, false, EXT>(shape_of<EXT>(S), x, x_f32, x_vec, image, image_elems, bias, N, y, y_f32, nullptr, hidden);
}

// T_{-1} = v, T_l = (W_l [T_{l-1}(, v)]) * (H_l > 0), u = W_L [T_{L-1}(, v)]: the forward's chain on the forward image, masks from
// `hidden`, no biases
template <class E, int W, bool EXT>
__global__ __launch_bounds__(MLP_WAVES * NFA_WAVE) void mlp_tangent_kernel(Shape S, const void *__restrict__ v, int v_f32, int v_vec,
                                                                          const uint16_t *__restrict__ hidden,
                                                                          const uint16_t *__restrict__ image, int64_t image_elems,
                                                                          int64_t N, uint16_t *__restrict__ tangent,
                                                                          void *__restrict__ u, int u_f32)
{
    mlp_chain<E, W, true, EXT>(shape_of<EXT>(S), v, v_f32, v_vec, image, image_elems, nullptr, N, u, u_f32, hidden, tangent);
}

// The ACT instantiations of both: one per (type, width), whatever the activations
template <class E, int W>
__global__ __launch_bounds__(MLP_WAVES * NFA_WAVE) void mlp_act_fwd_kernel(Shape S, ActOps A, const void *__restrict__ x, int x_f32,
                                                                          int x_vec, const uint16_t *__restrict__ image,
                                                                          int64_t image_elems, const float *__restrict__ bias, int64_t N,
                                                                          void *__restrict__ y, int y_f32, uint16_t *__restrict__ hidden)
{
    mlp_chain<E, W, false, true, true>(S, x, x_f32, x_vec, image, image_elems, bias, N, y, y_f32, nullptr, hidden, A);
}

template <class E, int W>
__global__ __launch_bounds__(MLP_WAVES * NFA_WAVE) void mlp_act_tangent_kernel(Shape S, ActOps A, const void *__restrict__ v, int v_f32,
                                                                              int v_vec, const uint16_t *__restrict__ hidden,
                                                                              const uint16_t *__restrict__ image, int64_t image_elems,
                                                                              int64_t N, uint16_t *__restrict__ tangent,
                                                                              void *__restrict__ u, int u_f32)
{
    mlp_chain<E, W, true, true, true>(S, v, v_f32, v_vec, image, image_elems, nullptr, N, u, u_f32, hidden, tangent, A);
}

// ---------------------------------------------------------------- data gradient

// The gradient chain dZ_L = g (* f_out'(y)), dZ_l = (W_{l+1}^T dZ_{l+1})[:W] * f'(H_l), dx over the workgroup's tiles.  ACT: the
// activations of `A`; with A.inject it is the curvature pass, E_l = (W_{l+1}^T E_{l+1})[:W] * f'(H_l) + R_l, started from g = R_L.
// One kernel template for both, so that the chain exists once; the instantiations without ACT never read `A`.
template <class E, int W, bool EXT, bool ACT = false>
__global__ __launch_bounds__(MLP_WAVES * NFA_WAVE) void mlp_bwd_data_kernel(Shape S_, const void *__restrict__ g, int g_f32, int g_vec,
                                                                           const uint16_t *__restrict__ hidden,
                                                                           const uint16_t *__restrict__ image, int64_t image_elems,
                                                                           int64_t N, uint16_t *__restrict__ dz,
                                                                           uint16_t *__restrict__ dz_out, void *__restrict__ dx,
                                                                           int dx_f32, ActOps A)
{
    static_assert(EXT || !ACT, "ACT is an instantiation of the general form");
    constexpr int MT = W / 32, KQ = W / 16;
    const Shape S = shape_of<EXT>(S_);
    const bool out_act = ACT && A.output != NFA_MLP_ACT_NONE;   // dZ_L = g * f_out'(y), which then lives in dz_out
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_lds[];
    nfa_v4u *wimg = reinterpret_cast<nfa_v4u *>(mlp_lds);
    stage_image(wimg, reinterpret_cast<const nfa_v4u *>(image), image_elems / 8);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    float *st = reinterpret_cast<float *>(mlp_lds + image_elems * 2) + wave * 32 * STAGE_LD;
    const int L = S.layers(), kqo = S.bwd_kq(L - 1), mt0 = S.bwd_mt(0);
    const int64_t n_tiles = (N + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * MLP_WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * MLP_WAVES) {
        const int64_t p = tile * 32 + r, pc = p < N ? p : N - 1;
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
        // dH_last = W_L^T dZ_L, dZ_L = g rounded
        int64_t off16 = S.bwd_off(L - 1) / 8;
        for (int q = 0; q < kqo; ++q) {
            nfa_v4u b;
            if (out_act) {
                act_switch(A.output, [&](auto code) __attribute__((always_inline)) {
                    b = load_row8_deriv<E, decltype(code)::value>(g, g_f32 != 0, A.y, A.y_f32 != 0, pc, S.n_out, 16 * q + 8 * h, A.beta);
                });
            } else {
                b = load_row8<E>(g, g_f32 != 0, pc, S.n_out, 16 * q + 8 * h, g_vec != 0);
            }
            if (dz_out && p < N) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * q + 8 * h + j;
                    if (k < S.n_out) dz_out[p * S.n_out + k] = (uint16_t)(b[j >> 1] >> (16 * (j & 1)));
                }
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma<E>(wimg[off16 + (m * kqo + q) * 64 + lane], b, acc[m]);
        }
        nfa_v4u df[KQ];
        for (int l = S.n_hidden - 1;; --l) {
            // dZ_l = dH_l * (H_l > 0), rounded
            const uint16_t *hl = hidden + (int64_t)l * N * W;
            if constexpr (ACT) {
                const uint16_t *inj = A.inject ? A.inject + (int64_t)l * N * W : nullptr;
                act_switch(A.hidden, [&](auto code) __attribute__((always_inline)) {
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        deriv_tile_row<E, W, decltype(code)::value>(acc[t], hl, inj, pc, t, h, A.beta);
                        df[2 * t] = acc_frag<E>(acc[t], 0);
                        df[2 * t + 1] = acc_frag<E>(acc[t], 1);
                        if (p < N) store_tile_row<W>(dz + (int64_t)l * N * W, p, t, h, df[2 * t], df[2 * t + 1]);
                    }
                });
            } else {
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    mask_tile_row<E, W>(acc[t], hl, pc, t, h);
                    df[2 * t] = acc_frag<E>(acc[t], 0);
                    df[2 * t + 1] = acc_frag<E>(acc[t], 1);
                    if (p < N) store_tile_row<W>(dz + (int64_t)l * N * W, p, t, h, df[2 * t], df[2 * t + 1]);
                }
            }
            if (l == 0) break;
            off16 = S.bwd_off(l) / 8;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
#pragma unroll
                for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(wimg[off16 + (m * KQ + q) * 64 + lane], df[q], acc[m]);
            }
        }
        if (dx) {   // dx = W_0^T dZ_0 + sum over the cat layers W_l[:, W:]^T dZ_l, 32 input features at a time
            const int64_t row0 = tile * 32;
            const int nrows = (int)(N - row0 < 32 ? N - row0 : 32);
            if (EXT && S.skip_mask) {
                // df[] holds dZ_0 by now, so a cat layer's dZ_l comes back from dz.  Each lane reads exactly the two 8-byte pieces
                // it stored itself (store_tile_row and load_tile_frag address the same columns for a lane), and the lanes of a
                // partial tile beyond N read row N - 1, which a lane of this same wave stored: nothing crosses waves, so making
                // the wave's own stores visible to the wave is enough.
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            for (int m = 0; m < mt0; ++m) {
                f32x16 o;
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
                for (int q = 0; q < KQ; ++q) o = mfma<E>(wimg[(m * KQ + q) * 64 + lane], df[q], o);
                for (int l = 2; EXT && l < L; ++l) {
                    if (!S.cat(l)) continue;
                    // rows W + 32m .. of the layer's image: row tile MT + m
                    const int64_t base = S.bwd_off(l) / 8;
                    if (l == L - 1) {   // dZ_L = g (with an output activation: what this lane's wave wrote to dz_out), natural k order
                        for (int q = 0; q < kqo; ++q) {
                            const nfa_v4u b = out_act ? load_row8<E>(dz_out, false, pc, S.n_out, 16 * q + 8 * h, false)
                                                      : load_row8<E>(g, g_f32 != 0, pc, S.n_out, 16 * q + 8 * h, g_vec != 0);
                            o = mfma<E>(wimg[base + ((MT + m) * kqo + q) * 64 + lane], b, o);
                        }
                    } else {
                        const uint16_t *dzl = dz + (int64_t)l * N * W;
#pragma unroll
                        for (int q = 0; q < KQ; ++q)
                            o = mfma<E>(wimg[base + ((MT + m) * KQ + q) * 64 + lane], load_tile_frag<W>(dzl, pc, q, h), o);
                    }
                }
                const int ncols = S.n_in - 32 * m < 32 ? S.n_in - 32 * m : 32;
                stage_store<E>(o, st, dx, dx_f32 != 0, row0, nrows, S.n_in, 32 * m, ncols, lane);
            }
        }
    }
}

// ---------------------------------------------------------------- weight gradient

constexpr int WG_CHUNK = 64;          // points staged per step
constexpr int WG_LD = WG_CHUNK + 8;   // halves per row of the transposed LDS images (16-byte aligned rows)

// Rows c0 .. c0+63 of src [*, ld] (float32 or E; rows >= n1 and columns >= ld read as zero), transposed into T [colsP][WG_LD].
template <class E>
__device__ __forceinline__ void stage_transposed(uint16_t *T, const void *src, bool is_f32, int ld, int colsP, int64_t c0, int64_t n1,
                                                 bool vec)
{
    const int units = (colsP / 8) * WG_CHUNK;
    for (int u = threadIdx.x; u < units; u += blockDim.x) {
        const int n = u & (WG_CHUNK - 1), cg = u >> 6;
        nfa_v4u f = {0u, 0u, 0u, 0u};
        if (c0 + n < n1) f = load_row8<E>(src, is_f32, c0 + n, ld, 8 * cg, vec);
#pragma unroll
        for (int j = 0; j < 8; ++j) T[(8 * cg + j) * WG_LD + n] = (uint16_t)(f[j >> 1] >> (16 * (j & 1)));
    }
}

// Workgroup (slice, layer): partial dW_l over the slice's points, the 32 x 32 tiles of [out_l, in_l] dealt round-robin to the waves.
// A cat layer's B operand [H_{l-1}, x] is staged from its two sources into the one Tb (W + n_in <= 256 rows).  With biases the
// workgroup also writes the slice's partial db_l = sum_p dZ_l[p, :]: thread c adds column c of the staged dZ in float32, the
// points in ascending order (eight at a time as a fixed tree), so the sum over the slices has one order whatever the launch;
// `zero_bias` writes zeros there instead (the second order: d/db of <v, dL/dx> is zero, the masks being piecewise constant).
template <class E, int W, bool EXT>
__global__ __launch_bounds__(256) void mlp_wgrad_kernel(Shape S_, const void *__restrict__ x, int x_f32, int x_vec,
                                                        const uint16_t *__restrict__ hidden, const uint16_t *__restrict__ dz,
                                                        const uint16_t *__restrict__ dz_out, int dzo_vec, int64_t N, int64_t slice_len,
                                                        float *__restrict__ partials, int64_t P, int zero_bias)
{
    constexpr int MAXT = (W / 32) * 8 / 4;   // tiles per wave at most: (W / 32) x (256 / 32) tiles over 4 waves
    const Shape S = shape_of<EXT>(S_);
    __shared__ __attribute__((aligned(16))) uint16_t Ta[128 * WG_LD];
    __shared__ __attribute__((aligned(16))) uint16_t Tb[256 * WG_LD];
    const int l = blockIdx.y, L = S.layers();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int M = S.out_dim(l), K = S.in_dim(l);
    const int mt = (M + 31) / 32, nt = (K + 31) / 32, n_tile = mt * nt;
    const void *a_src = l == L - 1 ? (const void *)dz_out : (const void *)(dz + (int64_t)l * N * W);
    const bool a_vec = l == L - 1 ? dzo_vec != 0 : true;
    const void *b_src = l == 0 ? x : (const void *)(hidden + (int64_t)(l - 1) * N * W);
    const bool b_f32 = l == 0 && x_f32 != 0, b_vec = l == 0 ? x_vec != 0 : true;
    const bool cat = EXT && S.cat(l), has_bias = EXT && S.bias != 0, col_sum = has_bias && !zero_bias && (int)threadIdx.x < M;
    float db = 0.f;
    f32x16 acc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
    const int64_t n0 = (int64_t)blockIdx.x * slice_len, n1 = n0 + slice_len < N ? n0 + slice_len : N;
    for (int64_t c0 = n0; c0 < n1; c0 += WG_CHUNK) {
        __syncthreads();
        stage_transposed<E>(Ta, a_src, false, M, mt * 32, c0, n1, a_vec);
        if (cat) {
            stage_transposed<E>(Tb, b_src, false, W, W, c0, n1, true);
            stage_transposed<E>(Tb + W * WG_LD, x, x_f32 != 0, S.n_in, nt * 32 - W, c0, n1, x_vec != 0);
        } else {
            stage_transposed<E>(Tb, b_src, b_f32, K, nt * 32, c0, n1, b_vec);
        }
        __syncthreads();
        if (col_sum) {   // points beyond the slice were staged as zeros
#pragma unroll
            for (int n8 = 0; n8 < WG_CHUNK / 8; ++n8) {
                const nfa_v4u f = *reinterpret_cast<const nfa_v4u *>(Ta + threadIdx.x * WG_LD + 8 * n8);
                const float s0 = unpack_half<E>(f[0], 0) + unpack_half<E>(f[0], 1), s1 = unpack_half<E>(f[1], 0) + unpack_half<E>(f[1], 1);
                const float s2 = unpack_half<E>(f[2], 0) + unpack_half<E>(f[2], 1), s3 = unpack_half<E>(f[3], 0) + unpack_half<E>(f[3], 1);
                db += (s0 + s1) + (s2 + s3);
            }
        }
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            const int tile = wave + 4 * i;
            if (tile < n_tile) {   // wave-uniform
                const int tm = tile / nt, tn = tile - tm * nt;
#pragma unroll
                for (int ks = 0; ks < WG_CHUNK / 16; ++ks) {
                    const nfa_v4u a = *reinterpret_cast<const nfa_v4u *>(Ta + (32 * tm + r) * WG_LD + 16 * ks + 8 * h);
                    const nfa_v4u b = *reinterpret_cast<const nfa_v4u *>(Tb + (32 * tn + r) * WG_LD + 16 * ks + 8 * h);
                    acc[i] = mfma<E>(a, b, acc[i]);
                }
            }
        }
    }
    if (has_bias && (int)threadIdx.x < M) partials[(int64_t)blockIdx.x * P + S.bias_off(l) + threadIdx.x] = db;
    float *out = partials + (int64_t)blockIdx.x * P + S.master_off(l);
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int tile = wave + 4 * i;
        if (tile < n_tile) {
            const int tm = tile / nt, tn = tile - tm * nt, col = 32 * tn + r;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = 32 * tm + acc_row(reg, h);
                if (row < M && col < K) out[(int64_t)row * K + col] = acc[i][reg];
            }
        }
    }
}

// ---------------------------------------------------------------- host side

int check_shape(const char *who, int32_t elem, const nfa_mlp_desc *net, int64_t n_points, Shape *S)
{
    NFA_REQUIRE(net, "%s: the network descriptor is null", who);
    const int32_t n_in = net->n_in, n_out = net->n_out, width = net->width, n_hidden = net->n_hidden;
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the network's type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    NFA_REQUIRE(width == 64 || width == 128, "%s: width %d: 64 or 128 neurons are supported", who, width);
    NFA_REQUIRE(n_hidden >= 1 && n_hidden <= 4, "%s: n_hidden %d: 1 to 4 hidden layers are supported", who, n_hidden);
    NFA_REQUIRE(n_in >= 1 && n_in <= 256, "%s: n_in %d: 1 to 256 input features are supported", who, n_in);
    NFA_REQUIRE(n_out >= 1 && n_out <= 32, "%s: n_out %d: 1 to 32 outputs are supported", who, n_out);
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    NFA_REQUIRE(net->bias == 0 || net->bias == 1, "%s: bias %d: 0 or 1", who, net->bias);
    NFA_REQUIRE((net->skip_mask & ~((2 << n_hidden) - 4)) == 0, "%s: skip_mask 0x%x: only bits 2 to n_hidden (%d) may be set: layer 0 "
                "takes x itself and layer 1 follows it", who, (unsigned)net->skip_mask, n_hidden);
    NFA_REQUIRE(net->skip_mask == 0 || n_in + width <= 256, "%s: n_in %d + width %d = %d: a layer that takes [H, x] holds at most 256 "
                "inputs", who, n_in, width, n_in + width);
    *S = Shape{n_in, n_out, width, n_hidden, net->bias, net->skip_mask};
    const int64_t f = S->fwd_off(S->layers()) * 2, b = S->bwd_off(S->layers()) * 2, fb = (int64_t)S->lds_bias_floats() * 4;
    NFA_REQUIRE(f + fb + STAGE_BYTES <= LDS_BUDGET && b + STAGE_BYTES <= LDS_BUDGET,
                "%s: the packed weights do not fit the LDS: forward image %lld B with %lld B of biases, backward image %lld B, each with "
                "%lld B of store staging, against %lld B per compute unit (n_in %d, n_out %d, width %d, n_hidden %d, bias %d, "
                "skip_mask 0x%x)", who, (long long)f, (long long)fb, (long long)b, (long long)STAGE_BYTES, (long long)LDS_BUDGET, n_in,
                n_out, width, n_hidden, net->bias, (unsigned)net->skip_mask);
    return NFA_OK;
}

nfa_mlp_desc plain_net(int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden)
{
    return nfa_mlp_desc{n_in, n_out, width, n_hidden, 0, 0};
}

// EXT: the network has biases or a skip.  The plain chain is an instantiation of its own, in which both are compiled out: with
// them as run-time conditions the forward kernel's register count cut its occupancy from 5 to 3 waves per SIMD (64 wide).
template <class F>
bool dispatch_mlp(int32_t elem, const Shape &S, F &&f)
{
    auto widths = [&](auto tag, auto ext) {
        if (S.W == 64) f(tag, std::integral_constant<int, 64>{}, ext);
        else f(tag, std::integral_constant<int, 128>{}, ext);
    };
    auto exts = [&](auto tag) {
        if (S.bias || S.skip_mask) widths(tag, std::true_type{});
        else widths(tag, std::false_type{});
    };
    if (elem == NFA_ELEM_F16) exts(ElemTag<nfa_f16>{});
    else if (elem == NFA_ELEM_BF16) exts(ElemTag<nfa_bf16>{});
    else return false;
    return true;
}

// The ACT instantiations: f(element tag, width).  One per (type, width, pass), the general (EXT) form whatever the network.
template <class F>
bool dispatch_mlp_act(int32_t elem, const Shape &S, F &&f)
{
    auto widths = [&](auto tag) {
        if (S.W == 64) f(tag, std::integral_constant<int, 64>{});
        else f(tag, std::integral_constant<int, 128>{});
    };
    if (elem == NFA_ELEM_F16) widths(ElemTag<nfa_f16>{});
    else if (elem == NFA_ELEM_BF16) widths(ElemTag<nfa_bf16>{});
    else return false;
    return true;
}

int check_act(const char *who, const nfa_mlp_act *act)
{
    NFA_REQUIRE(act, "%s: the activation descriptor is null", who);
    NFA_REQUIRE(act->hidden >= NFA_MLP_ACT_NONE && act->hidden <= NFA_MLP_ACT_EXPONENTIAL, "%s: hidden activation %d: an NFA_MLP_ACT_* code, %d to %d",
                who, act->hidden, NFA_MLP_ACT_NONE, NFA_MLP_ACT_EXPONENTIAL);
    NFA_REQUIRE(act->output >= NFA_MLP_ACT_NONE && act->output <= NFA_MLP_ACT_EXPONENTIAL, "%s: output activation %d: an NFA_MLP_ACT_* code, %d to %d",
                who, act->output, NFA_MLP_ACT_NONE, NFA_MLP_ACT_EXPONENTIAL);
    NFA_REQUIRE(act->beta > 0.f, "%s: beta %g: Softplus' beta must be positive", who, (double)act->beta);
    return NFA_OK;
}

// workgroups of a fused pass: as many as stay resident (LDS and the 8 that 32 waves allow), never more than there are tiles
unsigned fused_grid(int64_t n_points, int64_t lds_bytes)
{
    int64_t per_cu = LDS_BUDGET / lds_bytes;
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int64_t want = ceil_div64(ceil_div64(n_points, 32), MLP_WAVES);
    return (unsigned)(want < 256 * per_cu ? want : 256 * per_cu);
}

int64_t wgrad_slice_len(int64_t n_points)
{
    int64_t s = ceil_div64(n_points, NFA_MLP_WGRAD_MIN_SLICE);
    s = s > NFA_MLP_WGRAD_MAX_SLICES ? NFA_MLP_WGRAD_MAX_SLICES : (s < 1 ? 1 : s);
    return ceil_div64(ceil_div64(n_points, s), WG_CHUNK) * WG_CHUNK;
}

// The five passes behind both families of entries; `who` is the name of the entry that was called.

int pack_weights(const char *who, int32_t elem, const nfa_mlp_desc *net, const float *params, void *fwd_image, int64_t fwd_elems,
                 void *bwd_image, int64_t bwd_elems, nfa_stream_t stream)
{
    Shape S;
    if (int rc = check_shape(who, elem, net, 0, &S)) return rc;
    const int64_t fe = S.fwd_off(S.layers()), be = S.bwd_off(S.layers());
    NFA_REQUIRE(fwd_elems == fe && bwd_elems == be, "%s: the images hold %lld and %lld elements for this shape, got %lld and %lld", who,
                (long long)fe, (long long)be, (long long)fwd_elems, (long long)bwd_elems);
    NFA_REQUIRE(params && fwd_image && bwd_image, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(fwd_image, 16) && aligned_to(bwd_image, 16), "%s: the images must be 16-byte aligned", who);
    dispatch_elem(elem, [&](auto tag) {
        using E = typename decltype(tag)::type;
        if constexpr (sizeof(E) == 2)
            mlp_pack_kernel<E><<<grid_1d(fe + be, 256), 256, 0, as_stream(stream)>>>(S, params, static_cast<uint16_t *>(fwd_image),
                                                                                   static_cast<uint16_t *>(bwd_image), fe, be);
    });
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int fwd(const char *who, int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *fwd_image, const float *bias,
        int64_t n_points, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream,
        const nfa_mlp_act *act = nullptr, bool with_act = false)
{
    Shape S;
    if (int rc = check_shape(who, elem, net, n_points, &S)) return rc;
    if (with_act)
        if (int rc = check_act(who, act)) return rc;
    NFA_REQUIRE(x_elem == NFA_ELEM_F32 || x_elem == elem, "%s: x_elem %d: float32 or the network's type (%d)", who, x_elem, elem);
    NFA_REQUIRE(y_elem == NFA_ELEM_F32 || y_elem == elem, "%s: y_elem %d: float32 or the network's type (%d)", who, y_elem, elem);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && fwd_image && y && (!save_hidden || hidden) && (!S.bias || bias), "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(fwd_image, 16) && aligned_to(hidden, 8) && aligned_to(x, x_elem == NFA_ELEM_F32 ? 4 : 2) &&
                aligned_to(y, y_elem == NFA_ELEM_F32 ? 4 : 2) && aligned_to(bias, 4),
                "%s: misaligned pointer (image 16, hidden 8, x, y and bias their element)", who);
    const int64_t img = S.fwd_off(S.layers()), lds = img * 2 + (int64_t)S.lds_bias_floats() * 4 + STAGE_BYTES;
    int rc = NFA_OK;
    if (with_act) {
        ActOps A;
        A.hidden = act->hidden, A.output = act->output, A.beta = act->beta;
        dispatch_mlp_act(elem, S, [&](auto tag, auto w) {
            using E = typename decltype(tag)::type;
            auto kern = mlp_act_fwd_kernel<E, decltype(w)::value>;
            if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
            kern<<<fused_grid(n_points, lds), MLP_WAVES * NFA_WAVE, (size_t)lds, as_stream(stream)>>>(
                S, A, x, x_elem == NFA_ELEM_F32, row8_vec(x, S.n_in), static_cast<const uint16_t *>(fwd_image), img,
                S.bias ? bias : nullptr, n_points, y, y_elem == NFA_ELEM_F32, save_hidden ? static_cast<uint16_t *>(hidden) : nullptr);
        });
        if (rc != NFA_OK) return rc;
        NFA_CHECK_LAUNCH(who);
        return NFA_OK;
    }
    dispatch_mlp(elem, S, [&](auto tag, auto w, auto ext) {
        using E = typename decltype(tag)::type;
        auto kern = mlp_fwd_kernel<E, decltype(w)::value, decltype(ext)::value>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        kern<<<fused_grid(n_points, lds), MLP_WAVES * NFA_WAVE, (size_t)lds, as_stream(stream)>>>(
            S, x, x_elem == NFA_ELEM_F32, row8_vec(x, S.n_in), static_cast<const uint16_t *>(fwd_image), img, S.bias ? bias : nullptr,
            n_points, y, y_elem == NFA_ELEM_F32, save_hidden ? static_cast<uint16_t *>(hidden) : nullptr);
    });
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int bwd_data(const char *who, int32_t elem, const nfa_mlp_desc *net, const void *grad_y, int32_t g_elem, const void *hidden,
             const void *bwd_image, int64_t n_points, void *dz, void *dz_out, void *grad_x, int32_t x_elem, nfa_stream_t stream,
             const nfa_mlp_act *act = nullptr, bool with_act = false, const void *y = nullptr, int32_t y_elem = NFA_ELEM_F32,
             const void *inject = nullptr, bool curvature = false)
{
    Shape S;
    if (int rc = check_shape(who, elem, net, n_points, &S)) return rc;
    if (with_act) {
        if (int rc = check_act(who, act)) return rc;
        NFA_REQUIRE(y_elem == NFA_ELEM_F32 || y_elem == elem, "%s: y_elem %d: float32 or the network's type (%d)", who, y_elem, elem);
    }
    NFA_REQUIRE(g_elem == NFA_ELEM_F32 || g_elem == elem, "%s: g_elem %d: float32 or the network's type (%d)", who, g_elem, elem);
    NFA_REQUIRE(x_elem == NFA_ELEM_F32 || x_elem == elem, "%s: x_elem %d: float32 or the network's type (%d)", who, x_elem, elem);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(grad_y && hidden && bwd_image && dz, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(bwd_image, 16) && aligned_to(hidden, 8) && aligned_to(dz, 8) && aligned_to(dz_out, 2) &&
                aligned_to(grad_y, g_elem == NFA_ELEM_F32 ? 4 : 2) && aligned_to(grad_x, x_elem == NFA_ELEM_F32 ? 4 : 2),
                "%s: misaligned pointer (image 16, hidden and dz 8, the others their element)", who);
    const int64_t img = S.bwd_off(S.layers()), lds = img * 2 + STAGE_BYTES;
    int rc = NFA_OK;
    if (with_act) {
        ActOps A;
        A.hidden = act->hidden, A.beta = act->beta;
        if (curvature) {   // E_L = R_L as it is: no output derivative
            NFA_REQUIRE(inject, "%s: null pointer (inject)", who);
            NFA_REQUIRE(aligned_to(inject, 8), "%s: misaligned pointer (inject 8)", who);
            A.output = NFA_MLP_ACT_NONE, A.inject = static_cast<const uint16_t *>(inject);
        } else {
            A.output = act->output;
            if (A.output != NFA_MLP_ACT_NONE) {
                NFA_REQUIRE(y && dz_out, "%s: null pointer (an output activation needs y and dz_out)", who);
                NFA_REQUIRE(aligned_to(y, y_elem == NFA_ELEM_F32 ? 4 : 2), "%s: misaligned pointer (y its element)", who);
                A.y = y, A.y_f32 = y_elem == NFA_ELEM_F32;
            }
        }
        dispatch_mlp_act(elem, S, [&](auto tag, auto w) {
            using E = typename decltype(tag)::type;
            auto kern = mlp_bwd_data_kernel<E, decltype(w)::value, true, true>;
            if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
            kern<<<fused_grid(n_points, lds), MLP_WAVES * NFA_WAVE, (size_t)lds, as_stream(stream)>>>(
                S, grad_y, g_elem == NFA_ELEM_F32, row8_vec(grad_y, S.n_out), static_cast<const uint16_t *>(hidden),
                static_cast<const uint16_t *>(bwd_image), img, n_points, static_cast<uint16_t *>(dz), static_cast<uint16_t *>(dz_out),
                grad_x, x_elem == NFA_ELEM_F32, A);
        });
        if (rc != NFA_OK) return rc;
        NFA_CHECK_LAUNCH(who);
        return NFA_OK;
    }
    dispatch_mlp(elem, S, [&](auto tag, auto w, auto ext) {
        using E = typename decltype(tag)::type;
        auto kern = mlp_bwd_data_kernel<E, decltype(w)::value, decltype(ext)::value>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        kern<<<fused_grid(n_points, lds), MLP_WAVES * NFA_WAVE, (size_t)lds, as_stream(stream)>>>(
            S, grad_y, g_elem == NFA_ELEM_F32, row8_vec(grad_y, S.n_out), static_cast<const uint16_t *>(hidden),
            static_cast<const uint16_t *>(bwd_image), img, n_points, static_cast<uint16_t *>(dz), static_cast<uint16_t *>(dz_out),
            grad_x, x_elem == NFA_ELEM_F32, ActOps{});
    });
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int bwd_weights(const char *who, int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *hidden, const void *dz,
                const void *dz_out, int64_t n_points, float *partials, int64_t partial_floats, float *grad_params, int32_t zero_bias,
                nfa_stream_t stream)
{
    Shape S;
    if (int rc = check_shape(who, elem, net, n_points, &S)) return rc;
    NFA_REQUIRE(x_elem == NFA_ELEM_F32 || x_elem == elem, "%s: x_elem %d: float32 or the network's type (%d)", who, x_elem, elem);
    NFA_REQUIRE(partial_floats >= 0, "%s: partial_floats %lld is negative", who, (long long)partial_floats);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && hidden && dz && dz_out && partials && grad_params, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(hidden, 16) && aligned_to(dz, 16) && aligned_to(dz_out, 2) && aligned_to(x, x_elem == NFA_ELEM_F32 ? 4 : 2) &&
                aligned_to(partials, 4) && aligned_to(grad_params, 4),
                "%s: misaligned pointer (hidden and dz 16, the others their element)", who);
    const int64_t P = S.n_params(), slice_len = wgrad_slice_len(n_points), n_slices = ceil_div64(n_points, slice_len);
    NFA_REQUIRE(partial_floats >= n_slices * P, "%s: partials holds %lld floats, %lld slices of %lld parameters need %lld", who,
                (long long)partial_floats, (long long)n_slices, (long long)P, (long long)(n_slices * P));
    dispatch_mlp(elem, S, [&](auto tag, auto w, auto ext) {
        using E = typename decltype(tag)::type;
        mlp_wgrad_kernel<E, decltype(w)::value, decltype(ext)::value><<<dim3((unsigned)n_slices, (unsigned)S.layers()), 256, 0, as_stream(stream)>>>(
            S, x, x_elem == NFA_ELEM_F32, row8_vec(x, S.n_in), static_cast<const uint16_t *>(hidden), static_cast<const uint16_t *>(dz),
            static_cast<const uint16_t *>(dz_out), row8_vec(dz_out, S.n_out), n_points, slice_len, partials, P, zero_bias != 0);
    });
    NFA_CHECK_LAUNCH(who);
    mlp_wgrad_sum_kernel<<<(unsigned)ceil_div64(P, 256), 256, 0, as_stream(stream)>>>(partials, n_slices, P, grad_params);
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int tangent_pass(const char *who, int32_t elem, const nfa_mlp_desc *net, const void *v, int32_t v_elem, const void *hidden,
                 const void *fwd_image, int64_t n_points, void *tangent, void *u, int32_t u_elem, nfa_stream_t stream,
                 const nfa_mlp_act *act = nullptr, bool with_act = false, const void *y = nullptr, int32_t y_elem = NFA_ELEM_F32,
                 const void *dz = nullptr, const void *dz_out = nullptr, void *r = nullptr, void *r_out = nullptr)
{
    Shape S;
    if (int rc = check_shape(who, elem, net, n_points, &S)) return rc;
    if (with_act) {
        if (int rc = check_act(who, act)) return rc;
        NFA_REQUIRE(y_elem == NFA_ELEM_F32 || y_elem == elem, "%s: y_elem %d: float32 or the network's type (%d)", who, y_elem, elem);
    }
    NFA_REQUIRE(v_elem == NFA_ELEM_F32 || v_elem == elem, "%s: v_elem %d: float32 or the network's type (%d)", who, v_elem, elem);
    NFA_REQUIRE(u_elem == NFA_ELEM_F32 || u_elem == elem, "%s: u_elem %d: float32 or the network's type (%d)", who, u_elem, elem);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(v && hidden && fwd_image && u, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(fwd_image, 16) && aligned_to(hidden, 8) && aligned_to(tangent, 8) && aligned_to(v, v_elem == NFA_ELEM_F32 ? 4 : 2) &&
                aligned_to(u, u_elem == NFA_ELEM_F32 ? 4 : 2),
                "%s: misaligned pointer (image 16, hidden and tangent 8, v and u their element)", who);
    const int64_t img = S.fwd_off(S.layers()), lds = img * 2 + STAGE_BYTES;   // no biases: a bias has no tangent
    int rc = NFA_OK;
    if (with_act) {
        ActOps A;
        A.hidden = act->hidden, A.output = act->output, A.beta = act->beta;
        NFA_REQUIRE((r != nullptr) == (r_out != nullptr), "%s: r and r_out: both or neither", who);
        NFA_REQUIRE(!r || (dz && dz_out), "%s: null pointer (r and r_out need dz and dz_out)", who);
        NFA_REQUIRE(A.output == NFA_MLP_ACT_NONE || y, "%s: null pointer (an output activation needs y)", who);
        NFA_REQUIRE(aligned_to(y, y_elem == NFA_ELEM_F32 ? 4 : 2) && aligned_to(dz, 8) && aligned_to(dz_out, 2) && aligned_to(r, 8) &&
                    aligned_to(r_out, 2), "%s: misaligned pointer (dz and r 8, y, dz_out and r_out their element)", who);
        A.y = y, A.y_f32 = y_elem == NFA_ELEM_F32;
        A.dz = static_cast<const uint16_t *>(dz), A.dz_out = static_cast<const uint16_t *>(dz_out);
        A.r = static_cast<uint16_t *>(r), A.r_out = static_cast<uint16_t *>(r_out);
        dispatch_mlp_act(elem, S, [&](auto tag, auto w) {
            using E = typename decltype(tag)::type;
            auto kern = mlp_act_tangent_kernel<E, decltype(w)::value>;
            if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
            kern<<<fused_grid(n_points, lds), MLP_WAVES * NFA_WAVE, (size_t)lds, as_stream(stream)>>>(
                S, A, v, v_elem == NFA_ELEM_F32, row8_vec(v, S.n_in), static_cast<const uint16_t *>(hidden),
                static_cast<const uint16_t *>(fwd_image), img, n_points, static_cast<uint16_t *>(tangent), u, u_elem == NFA_ELEM_F32);
        });
        if (rc != NFA_OK) return rc;
        NFA_CHECK_LAUNCH(who);
        return NFA_OK;
    }
    dispatch_mlp(elem, S, [&](auto tag, auto w, auto ext) {
        using E = typename decltype(tag)::type;
        auto kern = mlp_tangent_kernel<E, decltype(w)::value, decltype(ext)::value>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        kern<<<fused_grid(n_points, lds), MLP_WAVES * NFA_WAVE, (size_t)lds, as_stream(stream)>>>(
            S, v, v_elem == NFA_ELEM_F32, row8_vec(v, S.n_in), static_cast<const uint16_t *>(hidden),
            static_cast<const uint16_t *>(fwd_image), img, n_points, static_cast<uint16_t *>(tangent), u, u_elem == NFA_ELEM_F32);
    });
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

}  // namespace
}  // namespace nfa

using namespace nfa;

int nfa_mlp_net_pack_weights(int32_t elem, const nfa_mlp_desc *net, const float *params, void *fwd_image, int64_t fwd_elems,
                             void *bwd_image, int64_t bwd_elems, nfa_stream_t stream)
{
    return pack_weights("nfa_mlp_net_pack_weights", elem, net, params, fwd_image, fwd_elems, bwd_image, bwd_elems, stream);
}

int nfa_mlp_net_fwd(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *fwd_image, const float *bias,
                    int64_t n_points, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream)
{
    return fwd("nfa_mlp_net_fwd", elem, net, x, x_elem, fwd_image, bias, n_points, y, y_elem, hidden, save_hidden, stream);
}

int nfa_mlp_net_bwd_data(int32_t elem, const nfa_mlp_desc *net, const void *grad_y, int32_t g_elem, const void *hidden,
                         const void *bwd_image, int64_t n_points, void *dz, void *dz_out, void *grad_x, int32_t x_elem,
                         nfa_stream_t stream)
{
    return bwd_data("nfa_mlp_net_bwd_data", elem, net, grad_y, g_elem, hidden, bwd_image, n_points, dz, dz_out, grad_x, x_elem, stream);
}

int nfa_mlp_net_bwd_weights(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *hidden, const void *dz,
                            const void *dz_out, int64_t n_points, float *partials, int64_t partial_floats, float *grad_params,
                            int32_t zero_bias, nfa_stream_t stream)
{
    return bwd_weights("nfa_mlp_net_bwd_weights", elem, net, x, x_elem, hidden, dz, dz_out, n_points, partials, partial_floats,
                       grad_params, zero_bias, stream);
}

int nfa_mlp_net_tangent(int32_t elem, const nfa_mlp_desc *net, const void *v, int32_t v_elem, const void *hidden, const void *fwd_image,
                        int64_t n_points, void *tangent, void *u, int32_t u_elem, nfa_stream_t stream)
{
    return tangent_pass("nfa_mlp_net_tangent", elem, net, v, v_elem, hidden, fwd_image, n_points, tangent, u, u_elem, stream);
}

// The entries with activations: the same passes in their ACT instantiations.

int nfa_mlp_act_fwd(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *x, int32_t x_elem,
                    const void *fwd_image, const float *bias, int64_t n_points, void *y, int32_t y_elem, void *hidden,
                    int32_t save_hidden, nfa_stream_t stream)
{
    return fwd("nfa_mlp_act_fwd", elem, net, x, x_elem, fwd_image, bias, n_points, y, y_elem, hidden, save_hidden, stream, act, true);
}

int nfa_mlp_act_bwd_data(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *grad_y, int32_t g_elem,
                         const void *y, int32_t y_elem, const void *hidden, const void *bwd_image, int64_t n_points, void *dz,
                         void *dz_out, void *grad_x, int32_t x_elem, nfa_stream_t stream)
{
    return bwd_data("nfa_mlp_act_bwd_data", elem, net, grad_y, g_elem, hidden, bwd_image, n_points, dz, dz_out, grad_x, x_elem, stream,
                    act, true, y, y_elem);
}

int nfa_mlp_act_tangent(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *v, int32_t v_elem,
                        const void *y, int32_t y_elem, const void *hidden, const void *dz, const void *dz_out,
                        const void *fwd_image, int64_t n_points, void *tangent, void *r, void *r_out, void *u, int32_t u_elem,
                        nfa_stream_t stream)
{
    return tangent_pass("nfa_mlp_act_tangent", elem, net, v, v_elem, hidden, fwd_image, n_points, tangent, u, u_elem, stream, act, true,
                        y, y_elem, dz, dz_out, r, r_out);
}

int nfa_mlp_act_curvature(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *r_out, const void *hidden,
                          const void *inject, const void *bwd_image, int64_t n_points, void *e, void *grad_x, int32_t x_elem,
                          nfa_stream_t stream)
{
    return bwd_data("nfa_mlp_act_curvature", elem, net, r_out, elem, hidden, bwd_image, n_points, e, nullptr, grad_x, x_elem, stream,
                    act, true, nullptr, NFA_ELEM_F32, inject, true);
}

// The tiny-cuda-nn entries: the same passes for a descriptor without biases and without skips.

int nfa_mlp_pack_weights(int32_t elem, const float *params, int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden,
                         void *fwd_image, int64_t fwd_elems, void *bwd_image, int64_t bwd_elems, nfa_stream_t stream)
{
    const nfa_mlp_desc net = plain_net(n_in, n_out, width, n_hidden);
    return pack_weights("nfa_mlp_pack_weights", elem, &net, params, fwd_image, fwd_elems, bwd_image, bwd_elems, stream);
}

int nfa_mlp_fwd(int32_t elem, const void *x, int32_t x_elem, const void *fwd_image, int64_t n_points, int32_t n_in, int32_t n_out,
                int32_t width, int32_t n_hidden, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream)
{
    const nfa_mlp_desc net = plain_net(n_in, n_out, width, n_hidden);
    return fwd("nfa_mlp_fwd", elem, &net, x, x_elem, fwd_image, nullptr, n_points, y, y_elem, hidden, save_hidden, stream);
}

int nfa_mlp_bwd_data(int32_t elem, const void *grad_y, int32_t g_elem, const void *hidden, const void *bwd_image, int64_t n_points,
                     int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, void *dz, void *dz_out, void *grad_x,
                     int32_t x_elem, nfa_stream_t stream)
{
    const nfa_mlp_desc net = plain_net(n_in, n_out, width, n_hidden);
    return bwd_data("nfa_mlp_bwd_data", elem, &net, grad_y, g_elem, hidden, bwd_image, n_points, dz, dz_out, grad_x, x_elem, stream);
}

int nfa_mlp_bwd_weights(int32_t elem, const void *x, int32_t x_elem, const void *hidden, const void *dz, const void *dz_out,
                        int64_t n_points, int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, float *partials,
                        int64_t partial_floats, float *grad_params, nfa_stream_t stream)
{
    const nfa_mlp_desc net = plain_net(n_in, n_out, width, n_hidden);
    return bwd_weights("nfa_mlp_bwd_weights", elem, &net, x, x_elem, hidden, dz, dz_out, n_points, partials, partial_floats, grad_params,
                       0, stream);
}

int nfa_mlp_tangent(int32_t elem, const void *v, int32_t v_elem, const void *hidden, const void *fwd_image, int64_t n_points,
                    int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, void *tangent, void *u, int32_t u_elem,
                    nfa_stream_t stream)
{
    const nfa_mlp_desc net = plain_net(n_in, n_out, width, n_hidden);
    return tangent_pass("nfa_mlp_tangent", elem, &net, v, v_elem, hidden, fwd_image, n_points, tangent, u, u_elem, stream);
}

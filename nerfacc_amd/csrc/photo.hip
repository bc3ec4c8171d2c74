// photo.hip -- the photometric loss: the target side of a training step, from the image stack to dL/drgb.
//
// Replaces what the reference's loaders and trainers run as torch every step (ref: examples/datasets/nerf_synthetic.py:153,195,
// dnerf_synthetic.py:155,197, nerf_360_v2.py:327, examples/train_ngp_nerf_occ.py:198-208,245 and its three siblings): the pixel gather
// from the uint8 stack, the division by 255, the blend with the background, smooth_l1_loss (or another loss), its backward,
// and mse_loss for the PSNR -- about a dozen gather, elementwise and reduction launches with [N, 4] and [N, 3] temporaries.
//
// Per ray i, float32, every operation rounded on its own (the library builds with -ffp-contract=off):
//   stack source:  (id, y, x) clamped into [n_images, H, W, C]; without x and y the pixel is number i of the stack (clamped);
//                  the byte offset ((id H + y) W + x) C is 64-bit; p_c = float(byte_c) / 255.0f, a = float(byte_3) / 255.0f
//   float source:  p_c = in[i, c], a = in[i, 3]
//   target_c = C == 4 and a background ? (p_c * a) + (b_c * (1.0f - a)) : p_c                  b: [3] or [N, 3]
//   d = rgb_c - target_c                                                                      rgb widened exactly from its type
//   term, dterm/dd by kind (P = param):
//     L1           |d|                                            s(d) = d > 0 ? 1 : d < 0 ? -1 : d     (0 at 0; NaN stays NaN)
//     L2           d * d                                          2 * d
//     SMOOTH_L1    |d| < P ? ((0.5 * d) * d) / P : |d| - 0.5 * P  |d| < P ? d / P : s(d)
//     HUBER        |d| <= P ? (0.5 * d) * d : P * (|d| - 0.5 * P) |d| <= P ? d : P * s(d)
//     RELATIVE_L2  (d * d) / (rgb * rgb + 0.01)                   (2 * d) / (rgb * rgb + 0.01)         (the denominator a constant)
//     CHARBONNIER  sqrt(d * d + P * P)                            d / sqrt(d * d + P * P)
//   loss = sum_i,c w_i * term / (3 N),  mse = sum_i,c d * d / (3 N),  per_ray_i = (w_i * ((t_0 + t_1) + t_2)) / 3.0f
//
// Forward, first launch, photo_fwd_kernel: flat over rays, 4 consecutive rays per lane as in rays.hip, so that the 12-byte
// rows of rgb, float pixels, an [N, 3] background and the pixels output move as three 16-byte accesses per lane (three
// 8-byte ones for half rgb), the indices and weights as one or two; a C = 4 stack pixel is one 4-byte load, a C = 3 one
// three bytes.  A quad that is not full, or any array whose base is not 16-byte aligned, sends the launch's quads (that
// quad) element by element: the same arithmetic, the same bits.  A workgroup of 256 lanes owns PHOTO_CHUNK = 1024 rays.  Each product w * term and d * d is widened
// to float64 and added: per lane over its rays and channels in order, the wave's 64 lanes by a butterfly, the 4 waves in wave
// order; partials[chunk] = (sum of w * term, sum of d * d).  Forward, second launch, photo_finish_kernel, one wave: lane t
// adds partials t, t + 64, .. in index order, lane 0 adds the 64 lanes' sums in lane order, and loss = float(sum / (3 N)),
// the one rounding to float32.  No atomics; the shape of the sum depends on N and PHOTO_CHUNK only, and in float64 its
// rounding errors are 2^-29 of a float32 ulp per addition: the float32 result does not depend on the chunk size at any
// N a device holds.
//
// Backward, photo_bwd_kernel, one launch of the same shape: g_rgb = ((g * w_i) * inv) * dterm/dd with g read from the device
// (the 0-dim gradient of the loss, e.g. the loss scale), inv = 1.0f / (float)(3 N) formed on the host, d formed again from
// rgb and the saved target; stored in rgb's type, rounded once.  per_ray gets no gradient.
//
// Nothing reads outside its array whatever the indices hold, nothing is read back to the host, and nothing is allocated.
#include "common.hip.h"

namespace nfa {

constexpr int PHOTO_LANES = 256;                 // lanes of a workgroup
constexpr int PHOTO_CHUNK = PHOTO_LANES * 4;     // rays a workgroup reduces into one partial pair
constexpr int PHOTO_FIN = NFA_WAVE;              // lanes of the finish kernel

enum { PHOTO_SRC_STACK = 0, PHOTO_SRC_FLOAT = 1 };
enum { PHOTO_BKGD_NONE = 0, PHOTO_BKGD_SHARED = 1, PHOTO_BKGD_PER_RAY = 2 };

struct PhotoArgs {
    const void *rgb;             // [n, 3] of the kernel's element type, or NULL: targets only
    int64_t n;
    const uint8_t *images;       // [n_images, H, W, C]
    int64_t n_images, H, W;
    const void *ids, *x, *y;     // [n] int32 or int64 (idx64), ids optional; x == NULL: pixel i of the stack
    int32_t idx64;
    const float *pix_in;         // [n, C] ready pixels (float source)
    const float *bkgd;           // [3] or [n, 3]
    int32_t bkgd_mode;
    const float *weights;        // [n] or NULL
    int32_t kind;
    float param;
    float *pixels;               // [n, 3]
    double *partials;            // [n_chunks, 2]
    float *per_ray;              // [n] or NULL
};

// 4 rows of K elements as one aligned block: 16-byte pieces where the block is a multiple of 16 bytes, else 8-byte ones
template <class T, int K>
struct alignas((sizeof(T) * K * 4) % 16 == 0 ? 16 : 8) RowQuad {
    T v[4 * K];
};
// rows e .. e + 3 of an [n, K] array; without `vec` (a partial quad, or a base that is not 16-byte aligned) element by
// element, a row past the end taking row e's values (in range)
template <class T, int K>
__device__ __forceinline__ void load_rows(const T *__restrict__ base, int64_t e, bool vec, int cnt, T out[4 * K])
{
    const T *b = base + e * K;
    if (vec) {
        const RowQuad<T, K> q = *reinterpret_cast<const RowQuad<T, K> *>(b);
#pragma unroll
        for (int j = 0; j < 4 * K; ++j) out[j] = q.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = j < cnt ? j : 0;
#pragma unroll
            for (int k = 0; k < K; ++k) out[K * j + k] = b[K * r + k];
        }
    }
}
template <class T, int K>
__device__ __forceinline__ void store_rows(T *__restrict__ base, int64_t e, bool vec, int cnt, const T v[4 * K])
{
    T *b = base + e * K;
    if (vec) {
        RowQuad<T, K> q;
#pragma unroll
        for (int j = 0; j < 4 * K; ++j) q.v[j] = v[j];
        *reinterpret_cast<RowQuad<T, K> *>(b) = q;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
#pragma unroll
                for (int k = 0; k < K; ++k) b[K * j + k] = v[K * j + k];
            }
        }
    }
}

// rows of the element type E as float32 (halves widen exactly)
template <class E>
__device__ __forceinline__ void load_rgb_rows(const void *base, int64_t e, bool vec, int cnt, float out[12])
{
    if constexpr (std::is_same<E, float>::value) {
        load_rows<float, 3>(static_cast<const float *>(base), e, vec, cnt, out);
    } else {
        uint16_t h[12];
        load_rows<uint16_t, 3>(static_cast<const uint16_t *>(base), e, vec, cnt, h);
#pragma unroll
        for (int j = 0; j < 12; ++j) out[j] = half_value<E>(h[j]);
    }
}

__device__ __forceinline__ void load_index4(const void *p, bool idx64, int64_t e, bool vec, int cnt, int64_t out[4])
{
    if (idx64) {
        load_rows<int64_t, 1>(static_cast<const int64_t *>(p), e, vec, cnt, out);
    } else {
        int32_t v[4];
        load_rows<int32_t, 1>(static_cast<const int32_t *>(p), e, vec, cnt, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = v[j];
    }
}

__device__ __forceinline__ int64_t clamp_index(int64_t v, int64_t size) { return v < 0 ? 0 : (v >= size ? size - 1 : v); }

__device__ __forceinline__ float sign0f(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : d); }

// the term of one element (GRAD: its derivative with respect to d); the table of the file's header
template <bool GRAD>
__device__ __forceinline__ float loss_term(int32_t kind, float P, float d, float rgb)
{
    const float ad = fabsf(d);
    switch (kind) {
    case NFA_PHOTO_L1:
        return GRAD ? sign0f(d) : ad;
    case NFA_PHOTO_L2:
        return GRAD ? 2.0f * d : d * d;
    case NFA_PHOTO_SMOOTH_L1:
        if (ad < P) return GRAD ? d / P : ((0.5f * d) * d) / P;
        return GRAD ? sign0f(d) : ad - 0.5f * P;
    case NFA_PHOTO_HUBER:
        if (ad <= P) return GRAD ? d : (0.5f * d) * d;
        return GRAD ? P * sign0f(d) : P * (ad - 0.5f * P);
    case NFA_PHOTO_RELATIVE_L2: {
        const float den = rgb * rgb + 0.01f;
        return GRAD ? (2.0f * d) / den : (d * d) / den;
    }
    default: {   // NFA_PHOTO_CHARBONNIER
        const float r = sqrtf(d * d + P * P);
        return GRAD ? d / r : r;
    }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, NFA_WAVE);
    return v;
}

template <class E, int SRC, int C>
__global__ __launch_bounds__(PHOTO_LANES) void photo_fwd_kernel(const PhotoArgs a, const bool aligned)
{
    __shared__ double wave_sums[PHOTO_LANES / NFA_WAVE][2];
    const int64_t e = ((int64_t)blockIdx.x * PHOTO_LANES + threadIdx.x) * 4;
    double s_loss = 0.0, s_mse = 0.0;
    if (e < a.n) {
        const int cnt = a.n - e >= 4 ? 4 : (int)(a.n - e);
        const bool vec = aligned && cnt == 4;
        // ---- the source's channels: p [4 rays][3], alpha [4 rays]
        float p[12], alpha[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if constexpr (SRC == PHOTO_SRC_STACK) {
            int64_t px[4];
            const int64_t n_pixels = a.n_images * a.H * a.W;
            if (a.x) {
                int64_t xs[4], ys[4], is[4] = {0, 0, 0, 0};
                load_index4(a.x, a.idx64, e, vec, cnt, xs);
                load_index4(a.y, a.idx64, e, vec, cnt, ys);
                if (a.ids) load_index4(a.ids, a.idx64, e, vec, cnt, is);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    px[j] = (clamp_index(is[j], a.n_images) * a.H + clamp_index(ys[j], a.H)) * a.W + clamp_index(xs[j], a.W);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) px[j] = clamp_index(e + (j < cnt ? j : 0), n_pixels);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t *at = a.images + px[j] * C;   // (64-bit: a full-resolution stack exceeds 4 GiB)
                uint32_t b0, b1, b2, b3 = 255u;
                if constexpr (C == 4) {
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(at);
                    b0 = w & 255u; b1 = (w >> 8) & 255u; b2 = (w >> 16) & 255u; b3 = w >> 24;
                } else {
                    b0 = at[0]; b1 = at[1]; b2 = at[2];
                }
                p[3 * j] = (float)b0 / 255.0f;
                p[3 * j + 1] = (float)b1 / 255.0f;
                p[3 * j + 2] = (float)b2 / 255.0f;
                alpha[j] = (float)b3 / 255.0f;
            }
        } else {
            float in[4 * C];
            load_rows<float, C>(a.pix_in, e, vec, cnt, in);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[3 * j] = in[C * j]; p[3 * j + 1] = in[C * j + 1]; p[3 * j + 2] = in[C * j + 2];
                if constexpr (C == 4) alpha[j] = in[C * j + 3];
            }
        }
        // ---- the blend
        float tgt[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) tgt[j] = p[j];
        if (C == 4 && a.bkgd_mode != PHOTO_BKGD_NONE) {
            float bk[12];
            if (a.bkgd_mode == PHOTO_BKGD_PER_RAY) {
                load_rows<float, 3>(a.bkgd, e, vec, cnt, bk);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) bk[j] = a.bkgd[j % 3];
            }
#pragma unroll
            for (int j = 0; j < 12; ++j) tgt[j] = (p[j] * alpha[j / 3]) + (bk[j] * (1.0f - alpha[j / 3]));
        }
        store_rows<float, 3>(a.pixels, e, vec, cnt, tgt);
        // ---- the loss terms
        if (a.rgb) {
            float rgb[12], w[4] = {1.0f, 1.0f, 1.0f, 1.0f}, ray[4];
            load_rgb_rows<E>(a.rgb, e, vec, cnt, rgb);
            if (a.weights) load_rows<float, 1>(a.weights, e, vec, cnt, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float d = rgb[3 * j + k] - tgt[3 * j + k];
                    t[k] = loss_term<false>(a.kind, a.param, d, rgb[3 * j + k]);
                    if (j < cnt) {
                        s_loss += (double)(a.weights ? w[j] * t[k] : t[k]);
                        s_mse += (double)(d * d);
                    }
                }
                const float s = (t[0] + t[1]) + t[2];
                ray[j] = (a.weights ? w[j] * s : s) / 3.0f;
            }
            if (a.per_ray) store_rows<float, 1>(a.per_ray, e, vec, cnt, ray);
        }
    }
    if (!a.rgb) return;   // (uniform)
    s_loss = wave_sum_f64(s_loss);
    s_mse = wave_sum_f64(s_mse);
    const int wave = threadIdx.x / NFA_WAVE;
    if ((threadIdx.x & (NFA_WAVE - 1)) == 0) { wave_sums[wave][0] = s_loss; wave_sums[wave][1] = s_mse; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = wave_sums[0][0], m = wave_sums[0][1];
#pragma unroll
        for (int k = 1; k < PHOTO_LANES / NFA_WAVE; ++k) { l += wave_sums[k][0]; m += wave_sums[k][1]; }
        a.partials[2 * (int64_t)blockIdx.x] = l;
        a.partials[2 * (int64_t)blockIdx.x + 1] = m;
    }
}

__global__ __launch_bounds__(PHOTO_FIN) void photo_finish_kernel(const double *__restrict__ partials, int64_t n_partials, double count,
                                                                 float *__restrict__ loss, float *__restrict__ mse)
{
    __shared__ double lane_sums[PHOTO_FIN][2];
    double l = 0.0, m = 0.0;
    // (unrolled so that the loads of 8 steps are in flight together; the additions stay in index order)
#pragma unroll 8
    for (int64_t k = threadIdx.x; k < n_partials; k += PHOTO_FIN) { l += partials[2 * k]; m += partials[2 * k + 1]; }
    lane_sums[threadIdx.x][0] = l;
    lane_sums[threadIdx.x][1] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < PHOTO_FIN; ++k) { l += lane_sums[k][0]; m += lane_sums[k][1]; }
        *loss = (float)(l / count);
        *mse = (float)(m / count);
    }
}

template <class E>
__global__ __launch_bounds__(PHOTO_LANES) void photo_bwd_kernel(const void *__restrict__ rgb_in, const float *__restrict__ pixels,
                                                                const float *__restrict__ weights, const float *__restrict__ g_loss,
                                                                int64_t n, int32_t kind, float param, float inv, void *__restrict__ g_rgb,
                                                                const bool aligned)
{
    const int64_t e = ((int64_t)blockIdx.x * PHOTO_LANES + threadIdx.x) * 4;
    if (e >= n) return;
    const int cnt = n - e >= 4 ? 4 : (int)(n - e);
    const bool vec = aligned && cnt == 4;
    const float g = *g_loss;
    float rgb[12], tgt[12], w[4], out[12];
    load_rgb_rows<E>(rgb_in, e, vec, cnt, rgb);
    load_rows<float, 3>(pixels, e, vec, cnt, tgt);
    if (weights) load_rows<float, 1>(weights, e, vec, cnt, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float coef = weights ? (g * w[j]) * inv : g * inv;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * j + k] = coef * loss_term<true>(kind, param, rgb[3 * j + k] - tgt[3 * j + k], rgb[3 * j + k]);
    }
    if constexpr (std::is_same<E, float>::value) {
        store_rows<float, 3>(static_cast<float *>(g_rgb), e, vec, cnt, out);
    } else {
        uint16_t h[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) h[j] = (uint16_t)half_bits<E>(out[j]);
        store_rows<uint16_t, 3>(static_cast<uint16_t *>(g_rgb), e, vec, cnt, h);
    }
}

static bool photo_kind_ok(int32_t kind) { return kind >= NFA_PHOTO_L1 && kind <= NFA_PHOTO_CHARBONNIER; }

}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_photometric_chunk(void) { return PHOTO_CHUNK; }

int nfa_photometric_fwd(const void *rgb, int32_t elem, int64_t n_rays, const uint8_t *images, int64_t n_images, int64_t height,
                        int64_t width, const void *image_ids, const void *x, const void *y, int32_t index_dtype,
                        const float *pixels_in, int32_t n_channels, const float *bkgd, int64_t bkgd_stride, const float *weights,
                        int32_t kind, float param, float *pixels, double *partials, int64_t n_partials, float *loss, float *mse,
                        float *per_ray, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rays >= 0, "photometric_fwd: negative size");
    NFA_REQUIRE(n_channels == 3 || n_channels == 4, "photometric_fwd: n_channels must be 3 or 4 (got %d)", n_channels);
    NFA_REQUIRE(elem == NFA_ELEM_F32 || elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "photometric_fwd: elem must be an NFA_ELEM_* code");
    NFA_REQUIRE(bkgd_stride == 0 || bkgd_stride == 3, "photometric_fwd: bkgd_stride must be 0 (one shared row) or 3");
    NFA_REQUIRE(!rgb || photo_kind_ok(kind), "photometric_fwd: kind must be an NFA_PHOTO_* code (got %d)", kind);
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE((images != nullptr) != (pixels_in != nullptr), "photometric_fwd: exactly one of images and pixels_in");
    NFA_REQUIRE(pixels, "photometric_fwd: null pointer");
    const int64_t n_chunks = ceil_div64(n_rays, PHOTO_CHUNK);
    NFA_REQUIRE(n_chunks < ((int64_t)1 << 31) - 1, "photometric_fwd: too many rays");
    if (images) {
        NFA_REQUIRE(n_images >= 1 && height >= 1 && width >= 1, "photometric_fwd: empty image stack");
        NFA_REQUIRE(n_images < ((int64_t)1 << 40) / height / width, "photometric_fwd: image stack too large");
        NFA_REQUIRE((x == nullptr) == (y == nullptr) && (x || !image_ids), "photometric_fwd: x and y go together, image_ids with them");
        NFA_REQUIRE(index_dtype == 1 || index_dtype == 2, "photometric_fwd: index_dtype must be 1 (int32) or 2 (int64)");
        const uintptr_t index_align = index_dtype == 2 ? 8 : 4;
        NFA_REQUIRE((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(image_ids)) % index_align == 0,
                    "photometric_fwd: x, y and image_ids must be aligned to their element size");
        NFA_REQUIRE(n_channels == 3 || reinterpret_cast<uintptr_t>(images) % 4 == 0, "photometric_fwd: a 4-channel stack must be 4-byte aligned");
    }
    if (rgb) {
        NFA_REQUIRE(partials && loss && mse, "photometric_fwd: null pointer");
        NFA_REQUIRE(n_partials >= n_chunks, "photometric_fwd: partials must hold ceil(n_rays / chunk) = %lld pairs (got %lld)",
                    (long long)n_chunks, (long long)n_partials);
        NFA_REQUIRE(reinterpret_cast<uintptr_t>(partials) % 8 == 0, "photometric_fwd: partials must be 8-byte aligned");
    }
    const uintptr_t elem_align = elem == NFA_ELEM_F32 ? 4 : 2;
    NFA_REQUIRE(reinterpret_cast<uintptr_t>(rgb) % elem_align == 0 &&
                    (reinterpret_cast<uintptr_t>(pixels_in) | reinterpret_cast<uintptr_t>(bkgd) | reinterpret_cast<uintptr_t>(weights) |
                     reinterpret_cast<uintptr_t>(pixels) | reinterpret_cast<uintptr_t>(per_ray)) % 4 == 0,
                "photometric_fwd: arrays must be aligned to their element size");
    PhotoArgs a{};
    a.rgb = rgb; a.n = n_rays;
    a.images = images; a.n_images = n_images; a.H = height; a.W = width;
    a.ids = image_ids; a.x = x; a.y = y; a.idx64 = index_dtype == 2;
    a.pix_in = pixels_in;
    a.bkgd = bkgd; a.bkgd_mode = !bkgd ? PHOTO_BKGD_NONE : (bkgd_stride == 0 ? PHOTO_BKGD_SHARED : PHOTO_BKGD_PER_RAY);
    a.weights = rgb ? weights : nullptr;
    a.kind = kind; a.param = param;
    a.pixels = pixels; a.partials = partials; a.per_ray = rgb ? per_ray : nullptr;
    // the quad form for every array or for none (one flag, as in rays.hip); the shared background row is read by element
    const bool aligned = all_aligned16(rgb, image_ids, x, y, pixels_in, bkgd_stride ? bkgd : nullptr, weights, pixels, per_ray);
    hipStream_t s = as_stream(stream);
    dispatch_elem(rgb ? elem : NFA_ELEM_F32, [&](auto tag) {
        using E = typename decltype(tag)::type;
        dispatch_bool(images != nullptr, [&](auto stack) {
            dispatch_bool(n_channels == 4, [&](auto four) {
                constexpr int SRC = decltype(stack)::value ? PHOTO_SRC_STACK : PHOTO_SRC_FLOAT;
                constexpr int C = decltype(four)::value ? 4 : 3;
                hipLaunchKernelGGL((photo_fwd_kernel<E, SRC, C>), dim3((unsigned)n_chunks), dim3(PHOTO_LANES), 0, s, a, aligned);
            });
        });
    });
    NFA_CHECK_LAUNCH("photometric_fwd");
    if (rgb) {
        hipLaunchKernelGGL(photo_finish_kernel, dim3(1), dim3(PHOTO_FIN), 0, s, partials, n_chunks, (double)n_rays * 3.0, loss, mse);
        NFA_CHECK_LAUNCH("photometric_fwd");
    }
    return NFA_OK;
}

int nfa_photometric_bwd(const void *rgb, int32_t elem, const float *pixels, const float *weights, const float *g_loss,
                        int64_t n_rays, int32_t kind, float param, void *g_rgb, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rays >= 0, "photometric_bwd: negative size");
    NFA_REQUIRE(elem == NFA_ELEM_F32 || elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "photometric_bwd: elem must be an NFA_ELEM_* code");
    NFA_REQUIRE(photo_kind_ok(kind), "photometric_bwd: kind must be an NFA_PHOTO_* code (got %d)", kind);
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(rgb && pixels && g_loss && g_rgb, "photometric_bwd: null pointer");
    const int64_t n_blocks = ceil_div64(n_rays, PHOTO_CHUNK);
    NFA_REQUIRE(n_blocks < ((int64_t)1 << 31) - 1, "photometric_bwd: too many rays");
    const uintptr_t elem_align = elem == NFA_ELEM_F32 ? 4 : 2;
    NFA_REQUIRE((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(g_rgb)) % elem_align == 0 &&
                    (reinterpret_cast<uintptr_t>(pixels) | reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(g_loss)) % 4 == 0,
                "photometric_bwd: arrays must be aligned to their element size");
    const float inv = 1.0f / (float)(3 * n_rays);
    const bool aligned = all_aligned16(rgb, pixels, weights, g_rgb);
    dispatch_elem(elem, [&](auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL(photo_bwd_kernel<E>, dim3((unsigned)n_blocks), dim3(PHOTO_LANES), 0, as_stream(stream), rgb, pixels, weights,
                           g_loss, n_rays, kind, param, inv, g_rgb, aligned);
    });
    NFA_CHECK_LAUNCH("photometric_bwd");
    return NFA_OK;
}

}  // extern "C"

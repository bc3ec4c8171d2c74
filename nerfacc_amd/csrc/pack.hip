// pack.hip -- data movement between the packed and the padded sample layouts (nerfacc 0.3's pack_data / unpack_data).
//
//   packed: (n_packed, row) plus packed_info (n_rays, 2) {start, count};  padded: (n_rays, S, row).
//
// A sample is `row_bytes` opaque bytes, so every dtype and feature width takes the same kernels.  Two ways to say which
// padded slot a packed sample belongs to:
//   by counts  ray r's samples are packed[start, start + count) in order; the first min(count, S) of them are slots
//              0 .. min(count, S) - 1 of row r (rows_kernel);
//   by a mask  ray r's samples are packed[start, start + count) in order and go to the slots of row r where mask[r, s]
//              is set, in order (masked_rows_kernel; count == popcount of the row).
// Both kernels run in either direction.  Nothing is accumulated: every output byte has one writer, so the results are
// deterministic and no atomics are used.
//
// Width: bytes move in chunks of W = the largest power of two <= 16 that divides row_bytes and every base address, so a
// row of 16-byte multiples at aligned addresses takes 16-byte loads and stores, and a view with an odd storage offset
// still runs (with narrower chunks).  The chunks of one wave are consecutive in the padded layout (rows_kernel) or
// consecutive samples of one row (masked_rows_kernel).
#include "common.hip.h"

namespace nfa {

typedef unsigned int nfa_v4u __attribute__((ext_vector_type(4)));

template <int W> struct ChunkT;
template <> struct ChunkT<16> { typedef nfa_v4u T; };
template <> struct ChunkT<8> { typedef uint64_t T; };
template <> struct ChunkT<4> { typedef uint32_t T; };
template <> struct ChunkT<2> { typedef uint16_t T; };
template <> struct ChunkT<1> { typedef uint8_t T; };

// The padding value repeated over 16 bytes (its byte size divides 16), read at a byte offset from the padded base: the
// pattern's phase is then that of the elements it fills.
struct PadPattern {
    uint32_t w[4];
};

template <int W>
__device__ __forceinline__ typename ChunkT<W>::T pad_chunk(const PadPattern &p, int64_t off)
{
    const uint32_t o = (uint32_t)off & 15u;
    if constexpr (W == 16) {
        nfa_v4u v = {p.w[0], p.w[1], p.w[2], p.w[3]};
        return v;
    } else if constexpr (W == 8) {
        return (o & 8u) ? ((uint64_t)p.w[3] << 32 | p.w[2]) : ((uint64_t)p.w[1] << 32 | p.w[0]);
    } else {
        const uint32_t i = o >> 2;
        const uint32_t word = i == 0 ? p.w[0] : i == 1 ? p.w[1] : i == 2 ? p.w[2] : p.w[3];
        return (typename ChunkT<W>::T)(word >> ((o & 3u) * 8u));
    }
}

template <int W>
__device__ __forceinline__ typename ChunkT<W>::T zero_chunk()
{
    return typename ChunkT<W>::T(0);
}

template <int W>
__device__ __forceinline__ typename ChunkT<W>::T ld(const uint8_t *p)
{
    return *reinterpret_cast<const typename ChunkT<W>::T *>(p);
}

template <int W>
__device__ __forceinline__ void st(uint8_t *p, typename ChunkT<W>::T v)
{
    *reinterpret_cast<typename ChunkT<W>::T *>(p) = v;
}

// By counts.  One lane per W-byte chunk of the padded layout, rays [ray0, ray0 + n_chunks / cpr) of this launch (the
// host splits larger inputs so that the chunk index and its division by cpr stay 32-bit).  Chunk t is byte o of row r,
// and that row's byte o comes from (or goes to) byte start_r * row_bytes + o of the packed layout if it is one of the
// ray's first min(count, S) samples.
//   TO_PADDED: the other chunks of the row get the padding.
//   !TO_PADDED: the ray's samples past S (dropped on the way to the padded layout) get zeros, so that the packed output
//              needs no zero fill when the chunks cover all of it; packed rows no chunk covers are not written.
template <int W, bool TO_PADDED>
__global__ __launch_bounds__(256) void rows_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                   const longlong2 *__restrict__ packed_info, int64_t ray0,
                                                   uint32_t n_chunks, uint32_t cpr, int64_t row_bytes, int64_t S,
                                                   int64_t packed_bytes, PadPattern pad)
{
    typedef typename ChunkT<W>::T T;
    const int64_t ray_bytes = S * row_bytes;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_chunks; t += stride) {
        const uint32_t rl = t / cpr;
        const int64_t o = (int64_t)(t - rl * cpr) * W;
        const int64_t r = ray0 + rl;
        const longlong2 p = packed_info[r];
        const int64_t cnt_bytes = p.y * row_bytes;
        const int64_t keep_bytes = cnt_bytes < ray_bytes ? cnt_bytes : ray_bytes;
        const int64_t po = p.x * row_bytes + o;     // packed byte
        const int64_t qo = r * ray_bytes + o;       // padded byte
        const bool in = o < keep_bytes && po >= 0 && po + W <= packed_bytes;
        if constexpr (TO_PADDED) {
            T v = in ? ld<W>(src + po) : pad_chunk<W>(pad, qo);
            st<W>(dst + qo, v);
        } else {
            if (in) st<W>(dst + po, ld<W>(src + qo));
            for (int64_t u = o + ray_bytes; u < cnt_bytes; u += ray_bytes) {   // only rays longer than S
                const int64_t pu = p.x * row_bytes + u;
                if (pu >= 0 && pu + W <= packed_bytes) st<W>(dst + pu, zero_chunk<W>());
            }
        }
    }
}

// By a mask.  One wave per row (grid-stride over rows), 64 slots at a time: a slot's rank among the row's set slots is
// the number of set slots before its group of 64 (wave-uniform, carried) plus mbcnt of the group's ballot, which is what
// data[mask] gives: row-major order, no atomics.  Each lane moves its slot's row_bytes in W-byte chunks.
//   TO_PADDED: unset slots get the padding.
//   !TO_PADDED: unset slots are skipped.
template <int W, bool TO_PADDED>
__global__ __launch_bounds__(256) void masked_rows_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          const uint8_t *__restrict__ mask,
                                                          const longlong2 *__restrict__ packed_info, int64_t n_rows,
                                                          int64_t S, int64_t row_bytes, int64_t n_packed, PadPattern pad)
{
    const int lane = lane_id();
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x / NFA_WAVE);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x / NFA_WAVE) + threadIdx.x / NFA_WAVE; r < n_rows; r += n_waves) {
        const int64_t start = packed_info[r].x;
        int64_t base = 0;
        for (int64_t c = 0; c < S; c += NFA_WAVE) {
            const int64_t s = c + lane;
            const bool live = s < S;
            const bool m = live && mask[r * S + s] != 0;
            const unsigned long long b = __ballot(m);
            const int64_t k = start + base + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            const bool in = m && k >= 0 && k < n_packed;
            const int64_t po = k * row_bytes;
            const int64_t qo = (r * S + s) * row_bytes;
            if (TO_PADDED && live) {
                for (int64_t j = 0; j < row_bytes; j += W)
                    st<W>(dst + qo + j, in ? ld<W>(src + po + j) : pad_chunk<W>(pad, qo + j));
            } else if (!TO_PADDED && in) {
                for (int64_t j = 0; j < row_bytes; j += W) st<W>(dst + po + j, ld<W>(src + qo + j));
            }
            base += __popcll(b);
        }
    }
}

// counts[r] = number of set bytes in mask row r (one wave per row).
__global__ __launch_bounds__(256) void mask_row_counts_kernel(const uint8_t *__restrict__ mask, int64_t n_rows, int64_t S,
                                                              int64_t *__restrict__ counts)
{
    const int lane = lane_id();
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x / NFA_WAVE);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x / NFA_WAVE) + threadIdx.x / NFA_WAVE; r < n_rows; r += n_waves) {
        int64_t n = 0;
        for (int64_t c = 0; c < S; c += NFA_WAVE) {
            const int64_t s = c + lane;
            n += __popcll(__ballot(s < S && mask[r * S + s] != 0));
        }
        if (lane == 0) counts[r] = n;
    }
}

static int chunk_width(int64_t row_bytes, const void *a, const void *b)
{
    const uintptr_t bits = (uintptr_t)row_bytes | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | 16u;
    return (int)(bits & (~bits + 1));   // lowest set bit, at most 16
}

template <int W>
static void launch_rows(bool to_padded, const void *src, void *dst, const int64_t *packed_info, const uint8_t *mask,
                        int64_t n_rays, int64_t S, int64_t n_packed, int64_t row_bytes, const PadPattern &pad,
                        hipStream_t s)
{
    const uint8_t *sp = static_cast<const uint8_t *>(src);
    uint8_t *dp = static_cast<uint8_t *>(dst);
    const longlong2 *pi = reinterpret_cast<const longlong2 *>(packed_info);
    if (mask) {
        const unsigned grid = grid_1d(n_rays * NFA_WAVE, 256, 1 << 14);
        if (to_padded)
            hipLaunchKernelGGL((masked_rows_kernel<W, true>), dim3(grid), dim3(256), 0, s, sp, dp, mask, pi, n_rays, S, row_bytes, n_packed, pad);
        else
            hipLaunchKernelGGL((masked_rows_kernel<W, false>), dim3(grid), dim3(256), 0, s, sp, dp, mask, pi, n_rays, S, row_bytes, n_packed, pad);
        return;
    }
    const int64_t cpr = S * row_bytes / W;
    const int64_t rays_per_launch = ((int64_t)1 << 31) / cpr;
    for (int64_t r0 = 0; r0 < n_rays; r0 += rays_per_launch) {
        const int64_t nr = n_rays - r0 < rays_per_launch ? n_rays - r0 : rays_per_launch;
        const uint32_t n_chunks = (uint32_t)(nr * cpr);
        const unsigned grid = grid_1d(n_chunks, 256);
        if (to_padded)
            hipLaunchKernelGGL((rows_kernel<W, true>), dim3(grid), dim3(256), 0, s, sp, dp, pi, r0, n_chunks, (uint32_t)cpr, row_bytes, S,
                               n_packed * row_bytes, pad);
        else
            hipLaunchKernelGGL((rows_kernel<W, false>), dim3(grid), dim3(256), 0, s, sp, dp, pi, r0, n_chunks, (uint32_t)cpr, row_bytes, S,
                               n_packed * row_bytes, pad);
    }
}

static int rows_entry(const char *name, bool to_padded, const void *src, void *dst, const int64_t *packed_info,
                      const uint8_t *mask, int64_t n_rays, int64_t S, int64_t n_packed, int64_t row_bytes,
                      const void *pad_host, int32_t pad_bytes, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rays >= 0 && S >= 0 && n_packed >= 0, "%s: negative size", name);
    NFA_REQUIRE(row_bytes >= 1, "%s: row_bytes must be >= 1", name);
    NFA_REQUIRE(pad_bytes == 0 || ((pad_bytes == 1 || pad_bytes == 2 || pad_bytes == 4 || pad_bytes == 8 || pad_bytes == 16) && pad_host),
                "%s: pad_bytes must be 0, or 1, 2, 4, 8 or 16 with pad_host set", name);
    const void *packed = to_padded ? src : dst, *padded = to_padded ? dst : src;
    if (n_rays == 0 || S == 0 || (!to_padded && n_packed == 0)) return NFA_OK;
    NFA_REQUIRE(packed_info && padded && (packed || n_packed == 0), "%s: null pointer", name);
    const int W = chunk_width(row_bytes, src, dst);
    NFA_REQUIRE(mask || S * row_bytes / W < ((int64_t)1 << 31), "%s: a padded row of 2^31 or more %d-byte chunks", name, W);
    PadPattern pad = {{0u, 0u, 0u, 0u}};
    if (pad_bytes) {
        uint8_t bytes[16];
        for (int i = 0; i < 16; ++i) bytes[i] = static_cast<const uint8_t *>(pad_host)[i % pad_bytes];
        memcpy(pad.w, bytes, 16);
    }
    const hipStream_t s = as_stream(stream);
    switch (W) {
    case 16: launch_rows<16>(to_padded, src, dst, packed_info, mask, n_rays, S, n_packed, row_bytes, pad, s); break;
    case 8: launch_rows<8>(to_padded, src, dst, packed_info, mask, n_rays, S, n_packed, row_bytes, pad, s); break;
    case 4: launch_rows<4>(to_padded, src, dst, packed_info, mask, n_rays, S, n_packed, row_bytes, pad, s); break;
    case 2: launch_rows<2>(to_padded, src, dst, packed_info, mask, n_rays, S, n_packed, row_bytes, pad, s); break;
    default: launch_rows<1>(to_padded, src, dst, packed_info, mask, n_rays, S, n_packed, row_bytes, pad, s); break;
    }
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_unpack_rows(const void *packed, const int64_t *packed_info, const uint8_t *mask, int64_t n_rays, int64_t n_per_ray,
                    int64_t n_packed, int64_t row_bytes, const void *pad_host, int32_t pad_bytes, void *padded,
                    nfa_stream_t stream)
{
    return rows_entry("unpack_rows", true, packed, padded, packed_info, mask, n_rays, n_per_ray, n_packed, row_bytes, pad_host,
                      pad_bytes, stream);
}

int nfa_pack_rows(const void *padded, const int64_t *packed_info, const uint8_t *mask, int64_t n_rays, int64_t n_per_ray,
                  int64_t n_packed, int64_t row_bytes, void *packed, nfa_stream_t stream)
{
    return rows_entry("pack_rows", false, padded, packed, packed_info, mask, n_rays, n_per_ray, n_packed, row_bytes, nullptr, 0,
                      stream);
}

int nfa_mask_row_counts(const uint8_t *mask, int64_t n_rows, int64_t n_cols, int64_t *counts, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rows >= 0 && n_cols >= 0, "mask_row_counts: negative size");
    if (n_rows == 0) return NFA_OK;
    NFA_REQUIRE(counts && (mask || n_cols == 0), "mask_row_counts: null pointer");
    const unsigned grid = grid_1d(n_rows * NFA_WAVE, 256, 1 << 14);
    hipLaunchKernelGGL(mask_row_counts_kernel, dim3(grid), dim3(256), 0, as_stream(stream), mask, n_rows, n_cols, counts);
    NFA_CHECK_LAUNCH("mask_row_counts");
    return NFA_OK;
}

}  // extern "C"

// nerf_field.h -- what the fused NeRF field's query (nerf_field.hip) and its training backward (nerf_train.hip) share: the limits,
// the ring over two packed images, the one statement of the shapes (the T-NeRF warp network's included), and the staged store of
// rows that are no 16-byte rows.
#pragma once
#include "mlp_tiles.h"

namespace nfa {
namespace {

constexpr int NF_WAVES = 4;
constexpr int NF_THREADS = NF_WAVES * NFA_WAVE;
constexpr int NF_POINTS = NF_WAVES * 32;   // points of a workgroup per pass of the images
constexpr int NF_SLOTS = 2;
constexpr int NF_MAX_PIECES = 160;         // 8 * 8 + 9 of the trunk and 4 * 4 + 1 of the head at most
constexpr int NF_MAX_HIDDEN = 8, NF_HEAD_MAX_HIDDEN = 4, NF_HEAD_W = 128;
constexpr int NF_POS_L = 10, NF_DIR_L = 4;                               // the reference's degrees (0, 10) and (0, 4)
constexpr int NF_POS_DIMS = 3 + 6 * NF_POS_L, NF_DIR_DIMS = 3 + 6 * NF_DIR_L;   // 63 and 27, with identity
static_assert(NF_POINTS == NFA_MLP_STREAM_POINTS, "the streamed passes' split");
constexpr int NF_WARP_L = 4, NF_WARP_W = 64, NF_WARP_MAX_HIDDEN = 4;   // the reference's warp: degrees (0, 4) of x and of t
constexpr int NF_WARP_DIMS = 3 + 6 * NF_WARP_L + 1 + 2 * NF_WARP_L;    // 36 = 27 + 9, with both identities
constexpr int NF_WARP_KQ0 = (NF_WARP_DIMS + 15) / 16;

struct Piece { int32_t off16, n16; };   // of its image, in 16-byte fragments

// mlp_stream.hip's ring over two images: pieces below n0 come from img0, the others from img1.  PRE (the NDR field): a third image
// in front of them, the pieces below n_pre; the ring without it has no such members.
template <bool PRE>
struct RingPre {};
template <>
struct RingPre<true> {
    const nfa_v4u *pre;
    int n_pre;
};

template <int MAXV, bool PRE = false>
struct FieldRing : RingPre<PRE> {
    const nfa_v4u *img0, *img1;
    nfa_v4u *slots;
    const Piece *tab;
    int slot16, n0, n_pieces, next, cur;
    nfa_v4u regs[MAXV];

    __device__ __forceinline__ const nfa_v4u *source(int i) const
    {
        if constexpr (PRE) {   // a select of three values, not of three members' addresses: the ring stays in registers
            const uintptr_t a = reinterpret_cast<uintptr_t>(img0), b = reinterpret_cast<uintptr_t>(img1), c = reinterpret_cast<uintptr_t>(this->pre);
            const uintptr_t s = i < n0 ? a : b;
            return reinterpret_cast<const nfa_v4u *>(i < this->n_pre ? c : s) + tab[i].off16;
        }
        return (i < n0 ? img0 : img1) + tab[i].off16;
    }
    // thread 0 has written the table; stages piece 0
    __device__ __forceinline__ void start()
    {
        __syncthreads();
        const nfa_v4u *src = source(0);
        const int n16 = tab[0].n16;
        for (int i = threadIdx.x; i < n16; i += NF_THREADS) slots[i] = src[i];
        __syncthreads();
        cur = 0;
        next = 1;   // every network has at least two pieces
    }
    __device__ __forceinline__ const nfa_v4u *piece() const { return slots + cur * slot16; }
    // issues the loads of the next piece; the current one is read between fetch() and hand_over()
    __device__ __forceinline__ void fetch()
    {
        const nfa_v4u *src = source(next);
        const int n16 = tab[next].n16;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int i = threadIdx.x + v * NF_THREADS;
            if (i < n16) regs[v] = src[i];
        }
    }
    __device__ __forceinline__ void hand_over()
    {
        const int n16 = tab[next].n16;
        nfa_v4u *d = slots + (cur ^ 1) * slot16;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int i = threadIdx.x + v * NF_THREADS;
            if (i < n16) d[i] = regs[v];
        }
        __syncthreads();
        cur ^= 1;
        next = next + 1 == n_pieces ? 0 : next + 1;
    }
};

// ---------------------------------------------------------------- rows that are no 16-byte rows (63, W + 1, W + 27 halves)
//
// A wave's 32 points are 32 consecutive rows of an [N, ld] half matrix, and 32 ld halves are a multiple of 16 bytes whatever ld
// is: the tile is ONE contiguous, 16-byte aligned span of memory.  The lanes write their fragments' elements into the wave's own
// LDS tile in row-major order (2-byte LDS writes: a row starts on any even byte), and the wave copies the tile out as 16-byte
// pieces, lane i piece i, i + 64, ..: full 1 KiB store instructions.  Only the last tile of a matrix, cut at N, can end with
// fewer than eight halves; those leave one by one.

// bytes of a wave's staging tile for rows of ld halves
__host__ __device__ constexpr int row_stage_bytes(int ld) { return (32 * ld * 2 + 15) / 16 * 16; }

// halves c0 .. c0 + 2 n - 1 of row r, columns >= ld dropped
template <int N2>
__device__ __forceinline__ void stage_put(uint16_t *st, int ld, int r, int c0, const uint32_t (&v)[N2])
{
#pragma unroll
    for (int j = 0; j < 2 * N2; ++j)
        if (c0 + j < ld) st[r * ld + c0 + j] = (uint16_t)(v[j >> 1] >> (16 * (j & 1)));
}
__device__ __forceinline__ void stage_put8(uint16_t *st, int ld, int r, int c0, const nfa_v4u &f)
{
    const uint32_t v[4] = {f[0], f[1], f[2], f[3]};
    stage_put<4>(st, ld, r, c0, v);
}
// an acc_frag fragment of row tile t, k-step s (its permuted k order): columns 32 t + 16 s + 4 h .. + 3 and those 8 further
__device__ __forceinline__ void stage_put_acc_frag(uint16_t *st, int ld, int r, int h, int t, int s, const nfa_v4u &f)
{
    const uint32_t lo[2] = {f[0], f[1]}, hi[2] = {f[2], f[3]};
    stage_put<2>(st, ld, r, 32 * t + 16 * s + 4 * h, lo);
    stage_put<2>(st, ld, r, 32 * t + 16 * s + 8 + 4 * h, hi);
}

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows row0 .. row0 + nrows - 1 of dst [N, ld] (row0 a multiple of 32, dst 16-byte aligned) from the wave's tile
__device__ __forceinline__ void stage_flush(const uint16_t *st, uint16_t *dst, int64_t row0, int nrows, int ld, int lane)
{
    wave_sync_lds();
    const int halves = nrows * ld, n16 = halves / 8;
    uint16_t *d = dst + row0 * ld;
    for (int i = lane; i < n16; i += NFA_WAVE) reinterpret_cast<nfa_v4u *>(d)[i] = reinterpret_cast<const nfa_v4u *>(st)[i];
    for (int i = 8 * n16 + lane; i < halves; i += NFA_WAVE) d[i] = st[i];
    wave_sync_lds();
}

// rows of the wave's tile that exist
__device__ __forceinline__ int tile_rows(int64_t row0, int64_t N)
{
    const int64_t left = N - row0;
    return (int)(left < 0 ? 0 : (left < 32 ? left : 32));
}

// ---------------------------------------------------------------- host side

// The one statement of the shapes the fused query holds (nerfacc_amd/fields.py: nerf_field_limits_error says the same words).
int check_field_shape(const char *who, int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, int32_t trunk_width,
                      int64_t n_points, Shape *T, Shape *H)
{
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the networks' type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    if (T) {
        NFA_REQUIRE(trunk, "%s: the network descriptor is null", who);
        const int w = trunk->width, d = trunk->n_hidden;
        NFA_REQUIRE(w == 128 || w == 256, "%s: trunk width %d: 128 or 256 neurons are supported", who, w);
        NFA_REQUIRE(d >= 1 && d <= NF_MAX_HIDDEN, "%s: trunk n_hidden %d: 1 to %d hidden layers are supported", who, d, NF_MAX_HIDDEN);
        NFA_REQUIRE(trunk->n_in == NF_POS_DIMS, "%s: trunk n_in %d: the encoded position has %d features", who, trunk->n_in, NF_POS_DIMS);
        NFA_REQUIRE(trunk->n_out == w + 1, "%s: trunk n_out %d: width + 1 = %d outputs (the bottleneck, then sigma)", who, trunk->n_out, w + 1);
        NFA_REQUIRE(trunk->bias == 1, "%s: trunk bias %d: the field's networks have biases (1)", who, trunk->bias);
        NFA_REQUIRE((trunk->skip_mask & ~((2 << d) - 4)) == 0, "%s: trunk skip_mask 0x%x: only bits 2 to n_hidden (%d) may be set: layer 0 "
                    "takes x itself and layer 1 follows it", who, (unsigned)trunk->skip_mask, d);
        *T = Shape{trunk->n_in, trunk->n_out, w, d, 1, trunk->skip_mask};
        trunk_width = w;
    }
    if (H) {
        NFA_REQUIRE(head, "%s: the network descriptor is null", who);
        NFA_REQUIRE(trunk_width == 128 || trunk_width == 256, "%s: trunk width %d: 128 or 256 neurons are supported", who, trunk_width);
        const int d = head->n_hidden;
        NFA_REQUIRE(head->width == NF_HEAD_W, "%s: head width %d: %d neurons are supported", who, head->width, NF_HEAD_W);
        NFA_REQUIRE(d >= 1 && d <= NF_HEAD_MAX_HIDDEN, "%s: head n_hidden %d: 1 to %d hidden layers are supported", who, d, NF_HEAD_MAX_HIDDEN);
        NFA_REQUIRE(head->n_in == trunk_width + NF_DIR_DIMS, "%s: head n_in %d: trunk width + %d = %d inputs (the bottleneck, then the encoded "
                    "direction)", who, head->n_in, NF_DIR_DIMS, trunk_width + NF_DIR_DIMS);
        NFA_REQUIRE(head->n_out == 3, "%s: head n_out %d: 3 outputs (the colour)", who, head->n_out);
        NFA_REQUIRE(head->bias == 1, "%s: head bias %d: the field's networks have biases (1)", who, head->bias);
        NFA_REQUIRE(head->skip_mask == 0, "%s: head skip_mask 0x%x: the head has no skip", who, (unsigned)head->skip_mask);
        *H = Shape{head->n_in, 3, NF_HEAD_W, d, 1, 0};
    }
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    return NFA_OK;
}

// The one statement of the warp networks the T-NeRF entries hold (nerfacc_amd/fields.py: tnerf_field_limits_error says the same
// words), checked after elem and before the trunk and the head.
int check_warp_shape(const char *who, int32_t elem, const nfa_mlp_desc *warp, Shape *S)
{
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the networks' type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    NFA_REQUIRE(warp, "%s: the network descriptor is null", who);
    const int d = warp->n_hidden;
    NFA_REQUIRE(warp->width == NF_WARP_W, "%s: warp width %d: %d neurons are supported", who, warp->width, NF_WARP_W);
    NFA_REQUIRE(d >= 1 && d <= NF_WARP_MAX_HIDDEN, "%s: warp n_hidden %d: 1 to %d hidden layers are supported", who, d, NF_WARP_MAX_HIDDEN);
    NFA_REQUIRE(warp->n_in == NF_WARP_DIMS, "%s: warp n_in %d: the encoded position and time have %d features", who, warp->n_in, NF_WARP_DIMS);
    NFA_REQUIRE(warp->n_out == 3, "%s: warp n_out %d: 3 outputs (the deformation)", who, warp->n_out);
    NFA_REQUIRE(warp->bias == 1, "%s: warp bias %d: the field's networks have biases (1)", who, warp->bias);
    NFA_REQUIRE((warp->skip_mask & ~((2 << d) - 4)) == 0, "%s: warp skip_mask 0x%x: only bits 2 to n_hidden (%d) may be set: layer 0 "
                "takes x itself and layer 1 follows it", who, (unsigned)warp->skip_mask, d);
    *S = Shape{NF_WARP_DIMS, 3, NF_WARP_W, d, 1, warp->skip_mask};
    return NFA_OK;
}

}  // namespace
}  // namespace nfa

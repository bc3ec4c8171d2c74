// segscan.hip -- packed-segment ("flattened ray") kernels: scans, fused transmittance /
// weights forward+backward, visibility + compaction, per-ray accumulation.
//
// Design (MI355X, wave64).  The reference scans one ray per 16 threads through a 32-element
// shared-memory Blelloch tile with ~10 __syncthreads per tile (include/utils_scan.cuh) and
// builds everything else out of ATen elementwise launches.  Here a single engine streams the
// flat sample arrays once:
//   * the flat element range is cut into tiles of NFA_SEG_TILE element offsets and at most SEG_TILE_ROWS rays; a
//     tile OWNS the rays whose chunk starts inside it (ownership table built once per packed_info), so every
//     ray is scanned start-to-end by exactly one wave: no cross-workgroup carry, no atomics,
//     deterministic results that do not depend on the tiling, load balance independent of the ray-length
//     distribution (empty rays included); the tiles that own many rays are taken by a launch's first waves;
//   * a wave walks its element range in 256-element steps, 16 B per lane per array (coalesced
//     1 KiB wave loads/stores); everything that is uniform over the wave (tile bounds, step base,
//     loop control) lives in scalar registers;
//   * segment heads are scattered into a 1 KiB per-wave LDS line from a register-cached window
//     of packed_info rows (16 B/ray read once); the ray id of every element is resolved ONCE per
//     step (lane-local + 6 DPP steps: row_shr 1/2/4/8, row_bcast 15/31), value scans reuse that
//     structure (one DPP add + one select per step and channel) and carry the open ray across
//     steps; waves never synchronise with each other;
//   * a step may run a second scan stage whose inputs are the first stage's results (per-ray
//     totals of w*rgb after the transmittance scan) and a pre-scan hook that sees the ray id
//     (gradient of a per-ray reduction), which is how `rendering()` becomes one pass each way.
// The op-specific arithmetic (exp, alpha, weights, gradients, masks, compaction, per-ray sums)
// is fused into the same pass through small functor structs.
//
// Reverse scans (the reference's reverse-iterator launches, scan.cu:41-51) are the same engine
// with the lane/element order mirrored (DIR = -1).
#include <stdlib.h>

#include "common.hip.h"
#include "samples.h"

namespace nfa {

// Elements per lane and step: 4 consecutive ones, one 16-byte quad per lane and array.  (8 halves the cross-lane part of
// a step per element -- head resolution, 6 DPP steps per scan channel, the window of packed_info rows -- but its registers
// lower the occupancy and it was measured slower: DESIGN.md, "What the profiles showed -- round 2" (2).)
constexpr int SE = 4;
constexpr int SQ = SE / 4;              // 16-byte quads per lane (see Pos)
constexpr int SEG_CHUNK = 64 * SE;      // elements per wave step
#ifndef NFA_SEG_TILE_ROWS
#define NFA_SEG_TILE_ROWS 256
#endif
constexpr int64_t SEG_TILE_ROWS = NFA_SEG_TILE_ROWS;
#ifndef NFA_VIS_EXP_FREE
#define NFA_VIS_EXP_FREE 1
#endif
#ifndef NFA_SEG_WAVES_PER_BLOCK
#define NFA_SEG_WAVES_PER_BLOCK 4
#endif
// waves never cooperate, so the workgroup size is only a dispatch granularity; measured on cfg 2 (fused bwd / fwd /
// visibility, us): 1 wave 333 / 271 / 135, 2 waves 335 / 273 / 137, 4 waves 343 / 275 / 138, 8 waves 369 / 288 / 144 --
// but the whole step (and the pipelined loop) is not faster with 1 than with 4, so 4 stays
constexpr int SEG_WAVES_PER_BLOCK = NFA_SEG_WAVES_PER_BLOCK;

// ------------------------------------------------------------------------------------------
// tile ownership table
// tiles[b] = {first ray owned by tile b, its first element}; tiles[n_tiles] is the end sentinel
// {n_rays, end of the last ray}.  Tile b covers element offsets [b*tile_elems, (b+1)*tile_elems).
// (Uniform tiles: cutting the last sixth of the range into quarter-size tiles, to shorten a launch's emptying last
// round of waves, was measured slower -- fused fwd / bwd 290 / 352 -> 304 / 373 us.)
// A tile boundary is also drawn every SEG_TILE_ROWS rays: tile(ray r) = start[r] / tile_elems + r / SEG_TILE_ROWS (monotone in
// r), so that a region of short and empty rays is cut into tiles of at most SEG_TILE_ROWS rows instead of one tile with
// thousands (SS4 (10)): n_tiles = n_elems / tile_elems + n_rays / SEG_TILE_ROWS + 1.
__global__ __launch_bounds__(256) void seg_build_tiles_kernel(const int64_t *__restrict__ packed_info, int64_t n_rays,
                                                              int64_t n_elems, int64_t tile_elems, int64_t n_tiles,
                                                              longlong2 *__restrict__ tiles, int32_t *__restrict__ flags)
{
    // thread r (0..n_rays): ray r is the first ray of every tile b with
    // floor(start[r-1]/T) < b <= floor(start[r]/T); r == n_rays is the sentinel.
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rays;
         r += (int64_t)blockDim.x * gridDim.x) {
        int64_t b_lo, b_hi, e_first;
        bool bad = false;
        if (r < n_rays) {
            const int64_t s = packed_info[2 * r], n = packed_info[2 * r + 1];
            int64_t s_prev = -1;
            if (r > 0) {
                const int64_t ps = packed_info[2 * r - 2], pn = packed_info[2 * r - 1];
                s_prev = ps;
                bad |= (ps + pn != s);
            }
            bad |= (n < 0) || (s < 0) || (s + n > n_elems);
            if (bad) { if (flags) atomicOr(flags, 1); continue; }
            b_lo = (s_prev < 0) ? 0 : s_prev / tile_elems + (r - 1) / SEG_TILE_ROWS + 1;
            b_hi = s / tile_elems + r / SEG_TILE_ROWS;
            e_first = s;
        } else {
            const int64_t s_prev = n_rays > 0 ? packed_info[2 * n_rays - 2] : -1;
            const int64_t n_prev = n_rays > 0 ? packed_info[2 * n_rays - 1] : 0;
            b_lo = (s_prev < 0) ? 0 : s_prev / tile_elems + (n_rays - 1) / SEG_TILE_ROWS + 1;
            b_hi = n_tiles;
            e_first = (s_prev < 0) ? 0 : s_prev + n_prev;
            if (s_prev > n_elems) { if (flags) atomicOr(flags, 1); continue; }
        }
        for (int64_t b = b_lo; b <= b_hi && b <= n_tiles; ++b) tiles[b] = make_longlong2(r, e_first);
    }
}

// (A list of the tiles that own many rays, taken by a launch's first waves so that none of them starts last, was the first
// remedy for row-heavy tiles -- fused fwd 264 -> 237 us on cfg 2 -- and became useless, slightly harmful, once a tile could
// not own more than SEG_TILE_ROWS rays; removed.)
__host__ __device__ inline int64_t seg_table_rows(int64_t n_tiles) { return n_tiles + 1; }

// ------------------------------------------------------------------------------------------
// 16-byte vector helpers (addresses are 16 B aligned when VEC is true)
// Loads are UNCONDITIONAL and RAW: a lane without valid elements reads the step's base address `ps`
// (always inside the array), and the validity selects are applied where the values are consumed
// (sel).  A load inside an `if`, or a select right behind it, makes the compiler wait for that one
// load on the spot, which serialises the 3-7 array loads of a step (one memory latency each) and
// defeats the one-step-ahead prefetch.
struct F4 { float v[SE]; };  // one lane's elements of a step

// Where a lane stands in the current step.  `c` (step base, multiple of 256) and `safe` are wave-uniform
// and live in scalar registers; only `off` is per lane, so element addresses are scalar base + 32-bit
// lane offset and the range checks are 32-bit compares against scalars.
struct Pos {
    int64_t c;      // first element offset of the step
    int32_t off;    // SE * (lane in address order)
    int32_t safe;   // offset from c of an in-range, 16 B aligned quad every lane may read
    bool valid[SE]; // element c + off + j belongs to the tile's element range
    bool any, all;  // over the lane's SE elements
    int32_t d_lo, d_hi;  // the step's valid element offsets [d_lo, d_hi) from c (wave-uniform)
    // Per 16-byte quad.  With SE = 4 there is one quad per lane and qany / qall equal any / all, but folding the quad
    // loops away changes the register allocation of most kernels (same instructions, different order), so they stay.
    bool qany[SQ], qall[SQ];
    __device__ __forceinline__ int64_t p0() const { return c + off; }
};

template <bool VEC>
__device__ __forceinline__ void ld4(const float *__restrict__ p, const Pos &q, F4 &out)
{
    const float *b = p + q.c;
    if (VEC) {
#pragma unroll
        for (int h = 0; h < SQ; ++h) {
            const nfa_v4f v = *reinterpret_cast<const nfa_v4f *>(b + (q.qany[h] ? q.off + 4 * h : q.safe));
            out.v[4 * h] = v.x; out.v[4 * h + 1] = v.y; out.v[4 * h + 2] = v.z; out.v[4 * h + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SE; ++j) out.v[j] = b[q.valid[j] ? q.off + j : q.safe];
    }
}
__device__ __forceinline__ float sel(const F4 &r, int j, const bool valid[SE], float fill) { return valid[j] ? r.v[j] : fill; }

// Full lanes store one 16-byte vector.  The per-element path (a lane straddling a range end) starts with an opaque asm
// statement: without it the compiler if-converts both paths into dwordx3 + dword stores for EVERY lane, which halves the
// store rate.  (It used to go through a volatile pointer instead -- which compiles to system-scope flat stores with an
// s_waitcnt vmcnt(0) after EACH of them: sixteen serial round trips to memory in the first and last step of every tile
// of the fused backward, 22 us of its 344.)
#define NFA_ELEMENTWISE_PATH() asm volatile("; element-wise path" ::: "memory")
template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ p, const Pos &q, const float v[SE])
{
    float *b = p + q.c;
#pragma unroll
    for (int h = 0; h < SQ; ++h) {
        if (VEC && q.qall[h]) {
            store_f4(b + q.off + 4 * h, v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]);
        } else {
            NFA_ELEMENTWISE_PATH();
#pragma unroll
            for (int j = 4 * h; j < 4 * h + 4; ++j)
                if (q.valid[j]) b[q.off + j] = v[j];
        }
    }
}

// ------------------------------------------------------------------------------------------
// Wave-level segmented scan primitives (256 elements per step: 4 per lane in scan order k).
struct StepHeads {
    int32_t lh[SE];       // most recent head ray id over the lane's elements 0..k (-1: none)
    uint32_t acc;         // bit s: at Hillis-Steele step s (offset 2^s) this lane still accumulates
    bool open_prefix;     // no head in any earlier lane of this step: the carry of previous steps applies
    bool carry_on_lane_end;  // (wave-uniform) the range's last element is that lane's last element
    int32_t carry_lane;   // (wave-uniform) last lane in scan order that holds an element of the tile's range: carries are read
                          // THERE -- a ray that ends at the range's end gets the same scan tree as a ray that ends anywhere else
    int32_t ph;           // ray id in front of the lane's first element (carry folded in)
    int32_t rid[SE], prev_rid[SE];
    bool is_head[SE];
};

template <int S>
__device__ __forceinline__ void heads_step(int32_t &ah, uint32_t &acc)
{
    const int32_t uh = dpp_step<S>(-1, ah);
    // (a lane without a source reads -1: it keeps ah < 0 and its acc bit combines with the identity)
    if (ah < 0) { acc |= 1u << S; ah = uh; }
}

template <int DIR>
__device__ __forceinline__ void resolve_heads(const int32_t hj[SE], const bool valid[SE], int32_t carry_rid, StepHeads &hd)
{
#pragma unroll
    for (int k = 0; k < SE; ++k) {
        const int j = DIR > 0 ? k : SE - 1 - k;
        const int32_t h = valid[j] ? hj[j] : -1;
        hd.is_head[k] = h >= 0;
        hd.lh[k] = (k == 0 || h >= 0) ? h : hd.lh[k - 1 < 0 ? 0 : k - 1];  // most recent head (ids fall in reverse scans)
    }
    int32_t ah = hd.lh[SE - 1];
    uint32_t acc = 0;
    heads_step<0>(ah, acc); heads_step<1>(ah, acc); heads_step<2>(ah, acc);
    heads_step<3>(ah, acc); heads_step<4>(ah, acc); heads_step<5>(ah, acc);
    // keep only the steps at which this lane has a source lane (so that x + identity is never formed:
    // -0.0 would come back as +0.0)
    const int lane = lane_id(), r = lane & 15;
    const uint32_t has_src = (r >= 1 ? 1u : 0u) | (r >= 2 ? 2u : 0u) | (r >= 4 ? 4u : 0u) | (r >= 8 ? 8u : 0u) |
                             ((lane & 16) ? 16u : 0u) | (lane >= 32 ? 32u : 0u);
    hd.acc = acc & has_src;
    int32_t ph = dpp_prev_lane(-1, ah);
    hd.open_prefix = ph < 0;
    if (ph < 0) ph = carry_rid;
    hd.ph = ph;
    int32_t pr = ph;
#pragma unroll
    for (int k = 0; k < SE; ++k) {
        hd.prev_rid[k] = pr;
        hd.rid[k] = hd.lh[k] >= 0 ? hd.lh[k] : ph;
        pr = hd.rid[k];
    }
}

template <int S, int N, class FI, class FC>
__device__ __forceinline__ void values_step(const StepHeads &hd, float av[N], FI identity, FC comb)
{
    const bool take = (hd.acc >> S) & 1u;
#pragma unroll
    for (int ch = 0; ch < N; ++ch) {
        const float uv = dpp_step<S>(identity(ch), av[ch]);
        if (take) av[ch] = comb(ch, uv, av[ch]);
    }
}

// Inclusive segmented scan of x (scan order) given the resolved heads; `prev[k]` is the inclusive
// value of the element before k (in that element's own ray).  `carry` is updated to the state after
// the step's last element.
template <int N, class FI, class FC>
__device__ __forceinline__ void scan_values(const StepHeads &hd, const float x[SE][N], float carry[N], float incl[SE][N],
                                            float prev[SE][N], FI identity, FC comb)
{
    float li[SE][N];
#pragma unroll
    for (int k = 0; k < SE; ++k)
#pragma unroll
        for (int ch = 0; ch < N; ++ch)
            li[k][ch] = (k == 0 || hd.is_head[k]) ? x[k][ch] : comb(ch, li[k - 1 < 0 ? 0 : k - 1][ch], x[k][ch]);
    float av[N];
#pragma unroll
    for (int ch = 0; ch < N; ++ch) av[ch] = li[SE - 1][ch];
    values_step<0, N>(hd, av, identity, comb); values_step<1, N>(hd, av, identity, comb);
    values_step<2, N>(hd, av, identity, comb); values_step<3, N>(hd, av, identity, comb);
    values_step<4, N>(hd, av, identity, comb); values_step<5, N>(hd, av, identity, comb);
    float pv[N];
#pragma unroll
    for (int ch = 0; ch < N; ++ch) {
        pv[ch] = dpp_prev_lane(identity(ch), av[ch]);
        if (hd.open_prefix) pv[ch] = comb(ch, carry[ch], pv[ch]);
    }
#pragma unroll
    for (int k = 0; k < SE; ++k)
#pragma unroll
        for (int ch = 0; ch < N; ++ch) {
            prev[k][ch] = (k == 0) ? pv[ch] : incl[k - 1 < 0 ? 0 : k - 1][ch];
            incl[k][ch] = hd.lh[k] >= 0 ? li[k][ch] : comb(ch, pv[ch], li[k][ch]);
        }
    // The state after the range's last element, formed exactly as the NEXT element would see it (so that a ray's total does
    // not depend on whether the ray ends inside a tile or at its end): behind a lane's last element that is the scanned lane
    // aggregate (what the next lane reads as `pv`), inside a lane the element's inclusive value.
    const bool open_next = hd.open_prefix && hd.lh[SE - 1] < 0;
#pragma unroll
    for (int ch = 0; ch < N; ++ch) {
        const float nxt = open_next ? comb(ch, carry[ch], av[ch]) : av[ch];
        carry[ch] = lane_value(hd.carry_on_lane_end ? nxt : incl[SE - 1][ch], hd.carry_lane);
    }
}

// Per-ray totals: a ray is finished where the next head appears; (prev_rid, prev) there is its id and
// its inclusive total.  A lane has at most 4 such heads and almost always at most one, so the first is
// handled in one predicated block and further ones behind a wave-uniform (rarely taken) branch.
template <int N, class F>
__device__ __forceinline__ void flush_totals(const StepHeads &hd, const float prev[SE][N], F &&done)
{
    bool f[SE];
    int nf = 0;
#pragma unroll
    for (int k = 0; k < SE; ++k) { f[k] = hd.is_head[k] && hd.prev_rid[k] >= 0; nf += f[k] ? 1 : 0; }
    if (nf > 0) {
        int32_t rid = hd.prev_rid[SE - 1];   // the FIRST finished ray of the lane (lowest k wins)
        float t[N];
#pragma unroll
        for (int ch = 0; ch < N; ++ch) t[ch] = prev[SE - 1][ch];
#pragma unroll
        for (int k = SE - 2; k >= 0; --k) {
            if (f[k]) rid = hd.prev_rid[k];
#pragma unroll
            for (int ch = 0; ch < N; ++ch) if (f[k]) t[ch] = prev[k][ch];
        }
        done(rid, t);
    }
    if (__ballot(nf > 1) != 0ull) {
        bool seen = false;
#pragma unroll
        for (int k = 0; k < SE; ++k) {
            if (f[k] && seen) done(hd.prev_rid[k], prev[k]);
            seen = seen || f[k];
        }
    }
}

// Stage-B flavour of scan_values + flush_totals: only the per-ray totals are wanted, so the scan runs
// channel by channel (about ten live registers per channel instead of N x 12) and every finished ray's
// value goes straight to done(rid, ch, total).  xb(k, ch) yields the input of element k (scan order).
template <int N, class FX, class FD>
__device__ __forceinline__ void scan_totals(const StepHeads &hd, FX &&xb, float carry[N], FD &&done)
{
    bool f[SE];
    int nf = 0;
#pragma unroll
    for (int k = 0; k < SE; ++k) { f[k] = hd.is_head[k] && hd.prev_rid[k] >= 0; nf += f[k] ? 1 : 0; }
    int32_t rid1 = hd.prev_rid[SE - 1];   // the first finished ray of the lane
#pragma unroll
    for (int k = SE - 2; k >= 0; --k) if (f[k]) rid1 = hd.prev_rid[k];
    const bool more = __ballot(nf > 1) != 0ull;  // wave-uniform, rare: a lane closing two or more rays
#pragma unroll
    for (int ch = 0; ch < N; ++ch) {
        float li[SE];
#pragma unroll
        for (int k = 0; k < SE; ++k) {
            const float x = xb(k, ch);
            li[k] = (k == 0 || hd.is_head[k]) ? x : li[k - 1 < 0 ? 0 : k - 1] + x;
        }
        float av[1] = {li[SE - 1]};
        auto ident = [](int) { return 0.0f; };
        auto add = [](int, float u, float v) { return u + v; };
        values_step<0, 1>(hd, av, ident, add); values_step<1, 1>(hd, av, ident, add);
        values_step<2, 1>(hd, av, ident, add); values_step<3, 1>(hd, av, ident, add);
        values_step<4, 1>(hd, av, ident, add); values_step<5, 1>(hd, av, ident, add);
        float pv = dpp_prev_lane(0.0f, av[0]);
        if (hd.open_prefix) pv = carry[ch] + pv;
        // prev[k]: inclusive value of the element before k
        float prev[SE], incl = pv;
#pragma unroll
        for (int k = 0; k < SE; ++k) {
            prev[k] = incl;
            incl = hd.lh[k] >= 0 ? li[k] : pv + li[k];
        }
        float t1 = prev[SE - 1];
#pragma unroll
        for (int k = SE - 2; k >= 0; --k) if (f[k]) t1 = prev[k];
        if (nf > 0) done(rid1, ch, t1);
        if (more) {
            bool seen = false;
#pragma unroll
            for (int k = 0; k < SE; ++k) {
                if (f[k] && seen) done(hd.prev_rid[k], ch, prev[k]);
                seen = seen || f[k];
            }
        }
        const float nxt = (hd.open_prefix && hd.lh[SE - 1] < 0) ? carry[ch] + av[0] : av[0];   // (see scan_values)
        carry[ch] = lane_value(hd.carry_on_lane_end ? nxt : incl, hd.carry_lane);
    }
}

// ------------------------------------------------------------------------------------------
// The engine.  Op interface (all __device__; OpBase below holds the defaults of the constants and of identity / comb /
// ray_done / empty_ray):
//   static constexpr int NCH;                       scan channels of stage A
//   static constexpr int NCHB;                      channels of the optional stage B (additive; 0 = none):
//                                                   per-ray totals of values derived from stage A's results
//   static constexpr bool NEEDS_RID;                op.pre(j, pos, valid, rid) is called before stage A's
//                                                   inputs are read (the ray id is known before any value scan)
//   static constexpr bool TOTALS;                   op.ray_done(rid, total[NCH]) for EVERY finished ray
//   static constexpr int MIN_WAVES_PER_EU;          occupancy floor for the register allocator (1 = none)
//   static constexpr int RAY_LDS_FLOATS;            > 0: op.tile_begin(r_lo, r_hi, lds) stages per-ray data
//   static constexpr bool PIPE;                     fetch the next step's inputs one step ahead (see seg_run_tile)
//   float identity(int ch); float comb(int ch, float a, float b);   a = earlier in scan order
//   struct Raw;                                      registers filled straight from memory
//   void  fetch(const Pos &q, Raw &r) const;         loads only (unconditional, raw)
//   void  load(const Raw &r, const Pos &q);          derive scan inputs
//   float x(int j, int ch);                          stage-A input of element j (address order)
//   void  emit(int j, int64_t pos, bool valid, bool is_head, int rid, int prev_rid,
//              const float incl[NCH], const float prev[NCH]);
//        incl = inclusive scan value at this element; prev = inclusive value of the previous
//        element in scan order (in that element's own ray; exclusive value = is_head ? identity : prev)
//   float xb(int j, int ch);  void ray_done_b(int rid, int ch, float total);          (stage B)
//   void  store(const Pos &q);
//   void  empty_ray(int rid);
// Everything that is the same for the whole wave (tile bounds, step base, loop control) is kept in
// scalar registers (the tile index is made uniform with readfirstlane).
template <int DIR, class Op>
__device__ __forceinline__ void seg_run_tile(Op &op, const int64_t *__restrict__ packed_info,
                                             const longlong2 *__restrict__ tiles, int64_t n_rays, int64_t tile,
                                             int32_t *__restrict__ hid /* LDS, SEG_CHUNK ints, wave private */,
                                             float *__restrict__ ray_lds /* LDS, Op::RAY_LDS_FLOATS floats, wave private */)
{
    constexpr int NCH = Op::NCH;
    const int lane = lane_id();
    const int alane = DIR > 0 ? lane : 63 - lane;  // lane in address order
    const longlong2 t_lo = tiles[tile], t_hi = tiles[tile + 1];
    const int32_t r_lo = __builtin_amdgcn_readfirstlane((int32_t)t_lo.x), r_hi = __builtin_amdgcn_readfirstlane((int32_t)t_hi.x);
    if (r_lo >= r_hi) return;
    const int32_t n_own = r_hi - r_lo;
    // every element this wave touches belongs to one of the rays r_lo .. r_hi - 1: an op may stage their per-ray data
    if constexpr (Op::RAY_LDS_FLOATS > 0) op.tile_begin(r_lo, r_hi, ray_lds);
    const int64_t e_lo = uniform64(t_lo.y), e_hi = uniform64(t_hi.y);  // chunks are contiguous: the last owned ray ends where the next tile begins

    // window of packed_info rows, in walk order v = 0..n_own-1: ray(v) = r_lo + v (fwd) / r_hi-1-v (rev)
    // Each window of 64 rows is a load the wave waits for when its walk reaches it; a tile owns at most SEG_TILE_ROWS rows,
    // i.e. a few windows.  (A tile of short and empty rays used to own hundreds of rows: the bench's 30 % empty rays then
    // cost the fused passes 8 %, at 256^3 20 %.  Requesting the following window as soon as the current one was in place
    // measured neutral on cfg 2 once the row-heavy tiles were dispatched first, and 10 % slower for compaction on cfg 5.)
    int32_t v_next = 0, win_base = 0;
    longlong2 win = make_longlong2(0, 0);   // the lane's row of the window: {start, count}
    auto load_window = [&]() {
        const int32_t v = win_base + lane;
        if (v < n_own) {
            const int64_t ray = DIR > 0 ? (int64_t)r_lo + v : (int64_t)r_hi - 1 - v;
            win = *reinterpret_cast<const longlong2 *>(packed_info + 2 * ray);
        }
    };
    load_window();

    float carry[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) carry[ch] = op.identity(ch);
    constexpr int NCB = Op::NCHB > 0 ? Op::NCHB : 1;
    float carry_b[NCB];
#pragma unroll
    for (int ch = 0; ch < NCB; ++ch) carry_b[ch] = 0.0f;
    int32_t carry_rid = -1;

    // Steps are anchored at multiples of the step size, so a ray is cut into the same steps whatever the tiling (a range
    // of ~1000 elements at an arbitrary offset then touches five 256-element chunks).  (Anchoring them at the tile's own
    // range rounded to 32 elements made visibility 4 % faster on cfg 2 and the fused passes no faster, but results would
    // depend on the tiling; rounded to 4, the fused passes were 5 % slower.)
    const int64_t c_first = DIR > 0 ? (e_lo / SEG_CHUNK) * SEG_CHUNK : ((e_hi - 1) / SEG_CHUNK) * SEG_CHUNK;
    const int64_t n_chunks = e_hi > e_lo ? ((e_hi - 1) / SEG_CHUNK - e_lo / SEG_CHUNK + 1) : 0;

    auto chunk_base = [&](int64_t ci) { return c_first + (DIR > 0 ? ci : -ci) * SEG_CHUNK; };
    auto make_pos = [&](int64_t c, Pos &q) {
        // range of the step in element offsets from c, clamped to [0, 256]: scalar
        const int64_t lo64 = e_lo - c, hi64 = e_hi - c;
        const int32_t d_lo = lo64 < 0 ? 0 : (lo64 > SEG_CHUNK ? SEG_CHUNK : (int32_t)lo64);
        const int32_t d_hi = hi64 < 0 ? 0 : (hi64 > SEG_CHUNK ? SEG_CHUNK : (int32_t)hi64);
        q.c = c;
        q.d_lo = d_lo; q.d_hi = d_hi;
        q.off = SE * alane;
        q.safe = (d_lo / 4) * 4;  // first in-range multiple of 4 (every step holds at least one element)
#pragma unroll
        for (int j = 0; j < SE; ++j) q.valid[j] = (q.off + j >= d_lo) && (q.off + j < d_hi);
        q.any = (q.off + SE - 1 >= d_lo) && (q.off < d_hi);
        q.all = (q.off >= d_lo) && (q.off + SE - 1 < d_hi);
#pragma unroll
        for (int h = 0; h < SQ; ++h) {
            q.qany[h] = (q.off + 4 * h + 3 >= d_lo) && (q.off + 4 * h < d_hi);
            q.qall[h] = (q.off + 4 * h >= d_lo) && (q.off + 4 * h + 3 < d_hi);
        }
    };
    // When a step's inputs are requested (Op::PIPE).  false: in the step itself, after its segment heads have gone through
    // LDS, just before op.load (the first step's before the loop; requesting them before the heads was neutral on cfg 2
    // and made compaction 10 % slower on cfg 5).  true: one step ahead, before the previous step is computed and stored
    // (vmcnt retires in order: loads issued BEFORE the stores can be waited for without them).
    typename Op::Raw raw_cur, raw_next;
    if (n_chunks > 0) {
        Pos q0;
        make_pos(chunk_base(0), q0);
        op.fetch(q0, raw_cur);
    }
    for (int64_t ci = 0; ci < n_chunks; ++ci) {
        const int64_t c = chunk_base(ci);
        if (Op::PIPE && ci + 1 < n_chunks) {
            Pos qn;
            make_pos(chunk_base(ci + 1), qn);
            op.fetch(qn, raw_next);
        }
        // ---- segment heads of this chunk -> LDS
#pragma unroll
        for (int h = 0; h < SQ; ++h) *reinterpret_cast<int4 *>(hid + 256 * h + 4 * lane) = make_int4(-1, -1, -1, -1);
        __builtin_amdgcn_wave_barrier();
        for (;;) {
            const int32_t v = win_base + lane;
            const bool live = v >= v_next && v < n_own;
            const int64_t key = DIR > 0 ? win.x : win.x + win.y - 1;
            const bool take = live && (DIR > 0 ? key < c + SEG_CHUNK : key >= c);
            const int32_t ray = DIR > 0 ? r_lo + v : r_hi - 1 - v;
            if (take) {
                if (win.y > 0) hid[(int)(key - c)] = ray;
                else op.empty_ray(ray);
            }
            const int cnt = __builtin_popcountll(__ballot(take));
            v_next += cnt;
            if (v_next == win_base + 64 && v_next < n_own) {
                // (A tile owns at most SEG_TILE_ROWS rows, i.e. a few windows: long runs of empty rays -- the background of an
                //  image, the finished rays of the test-mode loop -- are spread over many tiles and walked in parallel.  The
                //  64-ary search that used to skip such runs inside one tile is gone with the tiles that needed it.)
                win_base = v_next;
                load_window();
                continue;
            }
            break;
        }
        __builtin_amdgcn_wave_barrier();
        int32_t hj[SE];
#pragma unroll
        for (int h = 0; h < SQ; ++h) {
            const int4 h4 = *reinterpret_cast<const int4 *>(hid + SE * alane + 4 * h);
            hj[4 * h] = h4.x; hj[4 * h + 1] = h4.y; hj[4 * h + 2] = h4.z; hj[4 * h + 3] = h4.w;
        }
        __builtin_amdgcn_wave_barrier();

        // ---- this step's data
        Pos q;
        make_pos(c, q);
        if (!Op::PIPE && ci > 0) op.fetch(q, raw_cur);
        op.load(raw_cur, q);

        // ---- segment structure of this step: ray id of every element (scan order k, address j = DIR>0 ? k : 3-k)
        StepHeads hd;
        resolve_heads<DIR>(hj, q.valid, carry_rid, hd);
        hd.carry_lane = DIR > 0 ? (q.d_hi - 1) / SE : 63 - q.d_lo / SE;
        hd.carry_on_lane_end = DIR > 0 ? (q.d_hi % SE == 0) : (q.d_lo % SE == 0);
        if constexpr (Op::NEEDS_RID) {
#pragma unroll
            for (int k = 0; k < SE; ++k) {
                const int j = DIR > 0 ? k : SE - 1 - k;
                op.pre(j, q.p0() + j, q.valid[j], hd.rid[k]);
            }
            op.store_pre(q);
        }
        // ---- stage A: scan of op.x, results to op.emit
        {
            float xa[SE][NCH], incl[SE][NCH], prev[SE][NCH];
#pragma unroll
            for (int k = 0; k < SE; ++k) {
                const int j = DIR > 0 ? k : SE - 1 - k;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) xa[k][ch] = q.valid[j] ? op.x(j, ch) : op.identity(ch);
            }
            scan_values<NCH>(hd, xa, carry, incl, prev, [&](int ch) { return op.identity(ch); },
                             [&](int ch, float u, float v) { return op.comb(ch, u, v); });
#pragma unroll
            for (int k = 0; k < SE; ++k) {
                const int j = DIR > 0 ? k : SE - 1 - k;
                op.emit(j, q.p0() + j, q.valid[j], hd.is_head[k], hd.rid[k], hd.prev_rid[k], incl[k], prev[k]);
            }
            if constexpr (Op::TOTALS) flush_totals<NCH>(hd, prev, [&](int32_t rid, const float *t) { op.ray_done(rid, t); });
        }
        // ---- stage B (optional): per-ray totals of values derived from stage A's results.  The per-element
        //      outputs are complete after stage A: they are stored first (their registers are free for stage B
        //      and the stores are in flight while it runs).
        op.store(q);
        if constexpr (Op::NCHB > 0) {
            scan_totals<NCB>(hd,
                             [&](int k, int ch) { const int j = DIR > 0 ? k : SE - 1 - k; return q.valid[j] ? op.xb(j, ch) : 0.0f; },
                             carry_b, [&](int32_t rid, int ch, float t) { op.ray_done_b(rid, ch, t); });
        }
        carry_rid = lane_value(hd.rid[SE - 1], hd.carry_lane);
        if (Op::PIPE) raw_cur = raw_next;
    }
    // remaining owned rays are all empty (their start equals e_hi / e_lo)
    for (;;) {
        const int32_t v = win_base + lane;
        const bool live = v >= v_next && v < n_own;
        if (live && win.y <= 0) op.empty_ray(DIR > 0 ? r_lo + v : r_hi - 1 - v);
        v_next = min(win_base + 64, n_own);
        if (v_next < n_own) { win_base = v_next; load_window(); continue; }
        break;
    }
    if (carry_rid >= 0 && lane == 0) {
        if constexpr (Op::TOTALS) op.ray_done(carry_rid, carry);
        if constexpr (Op::NCHB > 0) {
#pragma unroll
            for (int ch = 0; ch < NCB; ++ch) op.ray_done_b(carry_rid, ch, carry_b[ch]);
        }
    }
}

template <int DIR, class Op>
__global__ __launch_bounds__(64 * SEG_WAVES_PER_BLOCK, Op::MIN_WAVES_PER_EU) void seg_kernel(Op op, const int64_t *__restrict__ packed_info,
                                                                       const longlong2 *__restrict__ tiles,
                                                                       int64_t n_rays, int64_t n_tiles)
{
    __shared__ __attribute__((aligned(16))) int32_t hid_all[SEG_WAVES_PER_BLOCK * SEG_CHUNK];
    constexpr int RL = Op::RAY_LDS_FLOATS > 0 ? Op::RAY_LDS_FLOATS : 4;
    __shared__ __attribute__((aligned(16))) float ray_all[SEG_WAVES_PER_BLOCK * RL];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t tile = (int64_t)blockIdx.x * SEG_WAVES_PER_BLOCK + wave;
    if (tile >= n_tiles) return;
    seg_run_tile<DIR>(op, packed_info, tiles, n_rays, tile, hid_all + wave * SEG_CHUNK, ray_all + wave * RL);
}

template <int DIR, class Op>
static void launch_seg(const Op &op, const int64_t *packed_info, const int64_t *tiles_raw, int64_t n_rays, int64_t n_tiles,
                       hipStream_t s)
{
    const longlong2 *tiles = reinterpret_cast<const longlong2 *>(tiles_raw);
    const unsigned grid = (unsigned)ceil_div64(n_tiles, SEG_WAVES_PER_BLOCK);
    hipLaunchKernelGGL((seg_kernel<DIR, Op>), dim3(grid), dim3(64 * SEG_WAVES_PER_BLOCK), 0, s, op, packed_info, tiles,
                       n_rays, n_tiles);
}

// ------------------------------------------------------------------------------------------
// Ops.  `Raw` holds what one step loads (op.fetch, issued by the engine in the step itself or, with PIPE, one step
// ahead); the per-step working registers are members (fully unrolled, register resident).  Every op takes its defaults
// from OpBase and restates only what differs.

struct OpBase {  // one additive channel
    static constexpr int NCH = 1;
    static constexpr int NCHB = 0;
    static constexpr bool NEEDS_RID = false;
    static constexpr bool TOTALS = false;
    static constexpr int MIN_WAVES_PER_EU = 1;  // occupancy floor asked of the register allocator (1 = none)
    static constexpr int RAY_LDS_FLOATS = 0;    // per-wave LDS floats for per-ray data staged at tile start (tile_begin)
    static constexpr bool PIPE = false;         // the next step's loads are requested one step ahead (seg_run_tile)
    __device__ __forceinline__ float identity(int) const { return 0.0f; }
    __device__ __forceinline__ float comb(int, float a, float b) const { return a + b; }
    __device__ __forceinline__ void ray_done(int, const float *) const {}
    __device__ __forceinline__ void empty_ray(int) const {}
};

// ---- plain scans: scan.cu:9-165 (sum), :127-165 / :217-257 (prod)
template <bool EXCL, bool PROD, bool VEC>
struct ScanOp : OpBase {
    struct Raw { F4 x; };
    const float *in;
    float *out;
    float xin[SE], res[SE];
    __device__ __forceinline__ float identity(int) const { return PROD ? 1.0f : 0.0f; }
    __device__ __forceinline__ float comb(int, float a, float b) const { return PROD ? a * b : a + b; }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const { ld4<VEC>(in, q, r.x); }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) xin[j] = sel(r.x, j, valid, identity(0));
    }
    __device__ __forceinline__ float x(int j, int) const { return xin[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float incl[1], const float prev[1])
    {
        res[j] = EXCL ? (is_head ? identity(0) : prev[0]) : incl[0];
    }
    __device__ __forceinline__ void store(const Pos &q) { store4<VEC>(out, q, res); }
};

// ---- prod backward: reverse {incl,excl} sum of g*out, divided by clamp_min(in, 1e-10)
//      scan.cu:169-214, :259-304
template <bool EXCL, bool VEC>
struct ProdBwdOp : OpBase {
    struct Raw { F4 o, g, in; };
    const float *in, *outv, *g;
    float *gin;
    float q[SE], den[SE], res[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(outv, q, r.o);
        ld4<VEC>(g, q, r.g);
        ld4<VEC>(in, q, r.in);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) { q[j] = sel(r.g, j, valid, 0.0f) * sel(r.o, j, valid, 0.0f); den[j] = sel(r.in, j, valid, 1.0f); }
    }
    __device__ __forceinline__ float x(int j, int) const { return q[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float incl[1], const float prev[1])
    {
        const float sres = EXCL ? (is_head ? 0.0f : prev[0]) : incl[0];
        res[j] = sres / fmaxf(den[j], 1e-10f);
    }
    __device__ __forceinline__ void store(const Pos &q) { store4<VEC>(gin, q, res); }
};

// ------------------------------------------------------------------------------------------
// The rendering family -- DensityFwd/BwdOp, RenderAccum/AccumBwdOp, RenderFusedFwd/BwdOp, RenderRawFwd/BwdOp, RenderSdfFwd/BwdOp,
// RenderStepOp (volrend.py:109-151, :256-264, :358-362) -- is assembled from the steps below, each written once.  They are plain
// functions of values and base structs with __forceinline__ members: an op is a kernel argument and its working arrays
// are members, so after inlining a step reads and writes the op's own registers.

// ---- the density stage: sigma * delta (0 outside the range) is what stage A sums along the ray; with S the sum in front
//      of a sample, T = exp(-S), alpha = 1 - exp(-sigma * delta), w = T * alpha
__device__ __forceinline__ float sigma_delta(bool valid, float sigma, float delta) { return valid ? sigma * delta : 0.0f; }
__device__ __forceinline__ float midpoint(float ts, float te) { return (ts + te) / 2.0f; }
__device__ __forceinline__ float alpha_of(float xs) { return 1.0f - expf(-xs); }
__device__ __forceinline__ void trans_alpha(bool is_head, const float prev[1], float xs, float &T, float &a)
{
    const float S = is_head ? 0.0f : prev[0];
    T = expf(-S);
    a = alpha_of(xs);
}
// ---- constant-step samples (CS): the sampler's own output with step_size > 0 and no cone angle has
//      t_ends[i] == t_starts[i] + step for every sample (one fp32 add: the marching recurrence t_next = t_last + dt,
//      ref grid.cu:213-215), so the t_ends stream carries nothing the pass does not have already: it is not loaded and
//      formed from t_starts.  The sum is used exactly where the loaded value was (sigma * (te - ts), (ts + te) / 2), so
//      every result is bit for bit the one of the form that loads it.  Without CS the base is empty and the op is laid out
//      as before.
template <bool CS> struct ConstStep {};
template <> struct ConstStep<true> { float step; };
struct NoQuad {};   // stands in Raw for the quad that is not loaded
template <bool CS, class Op, class QA, class QB>
__device__ __forceinline__ float t_end_of(const Op &op, const QA &a, const QB &b, int j)
{
    if constexpr (CS) return a.v[j] + op.step;
    else return b.v[j];
}

// the per-sample outputs of that stage (each may be null)
struct SampleOut {
    float *w, *tr, *al;
    template <bool VEC>
    __device__ __forceinline__ void store_wta(const Pos &q, const float rw[SE], const float rt[SE], const float ra[SE]) const
    {
        if (w) store4<VEC>(w, q, rw);
        if (tr) store4<VEC>(tr, q, rt);
        if (al) store4<VEC>(al, q, ra);
    }
};

// ---- the five channels stage B totals per ray: w * rgb, w, w * mid -> colours(3), opacity, un-normalised depth
__device__ __forceinline__ float render_channel(int ch, float w, const float *c3, float mid)
{
    return ch < 3 ? w * c3[ch] : (ch == 3 ? w : w * mid);
}
// the per-ray outputs those totals go to: stored, added in place (the test-mode step), zero for an empty ray
struct RayOut {
    float *colors, *opac, *depth;   // [R,3], [R], [R]
    template <bool ADD>
    static __device__ __forceinline__ void set(float *o, float t) { *o = ADD ? *o + t : t; }
    template <bool ADD>
    __device__ __forceinline__ void ray_put(int rid, int ch, float t) const
    {
        if (ch < 3) set<ADD>(colors + 3 * (int64_t)rid + ch, t);
        else if (ch == 3) set<ADD>(opac + rid, t);
        else set<ADD>(depth + rid, t);
    }
    __device__ __forceinline__ void ray_store(int rid, int ch, float t) const { ray_put<false>(rid, ch, t); }
    __device__ __forceinline__ void ray_add(int rid, int ch, float t) const { ray_put<true>(rid, ch, t); }
    __device__ __forceinline__ void ray_store(int rid, const float t[5]) const
    {
#pragma unroll
        for (int ch = 0; ch < 5; ++ch) ray_store(rid, ch, t[ch]);
    }
    __device__ __forceinline__ void ray_zero(int rid) const
    {
        const float z[5] = {0, 0, 0, 0, 0};
        ray_store(rid, z);
    }
};
// what the one-pass forward ops share: stage A scans sigma * delta, stage B totals the five channels of w
struct RenderFwdStage : OpBase, RayOut {
    static constexpr int NCHB = 5;
    float xs[SE], mid[SE], rw[SE], c[3 * SE];
    __device__ __forceinline__ void sample(int j, bool valid, float sigma, float ts, float te)
    {
        xs[j] = sigma_delta(valid, sigma, te - ts);
        mid[j] = midpoint(ts, te);
    }
    __device__ __forceinline__ float x(int j, int) const { return xs[j]; }
    __device__ __forceinline__ float xb(int j, int ch) const { return render_channel(ch, rw[j], c + 3 * j, mid[j]); }
};

// ---- backward: the per-ray output gradients {g_colour(3), g_opacity, g_depth} (each array may be null) ...
struct RayGrads {
    const float *gc, *go, *gd;
    __device__ __forceinline__ void get(int rid, float g[5]) const   // gathered from memory
    {
        g[0] = gc ? gc[3 * (int64_t)rid] : 0.0f; g[1] = gc ? gc[3 * (int64_t)rid + 1] : 0.0f; g[2] = gc ? gc[3 * (int64_t)rid + 2] : 0.0f;
        g[3] = go ? go[rid] : 0.0f; g[4] = gd ? gd[rid] : 0.0f;
    }
};
// ... staged in LDS.  They are needed per ELEMENT, after the ray id is known: as global gathers they were a second,
// dependent memory latency in every step (12 gather instructions per lane and step; SQ counters: the pass waits 80 % of
// its wave-cycles, VALU 36 % busy).  The rays of a tile are consecutive, so the wave stages their gradients in LDS with
// coalesced loads at tile start (up to RAY_CAP rays, the rest falls back to the gathers) and the per-element reads are LDS
// reads.
struct RayGradStage : RayGrads {
    static constexpr int RAY_CAP = 192;
    static constexpr int LDS_FLOATS = 8 * RAY_CAP;   // {g_r, g_g, g_b, g_opacity, g_depth, -, -, -} per ray
    const float *g_lds = nullptr;
    int32_t g_lo = 0, g_n = 0;
    __device__ __forceinline__ void tile_begin(int32_t r_lo, int32_t r_hi, float *lds)
    {
        // (the pass runs from the tile's last ray to its first: when the tile owns more than RAY_CAP rays the stage holds
        //  the LAST ones, which most of its elements belong to)
        g_lds = lds; g_n = min(r_hi - r_lo, RAY_CAP); g_lo = r_hi - g_n;
        __builtin_amdgcn_wave_barrier();
        for (int32_t i = lane_id(); i < g_n; i += 64) {
            const int64_t r = (int64_t)g_lo + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gc) { v.x = gc[3 * r]; v.y = gc[3 * r + 1]; v.z = gc[3 * r + 2]; }
            if (go) v.w = go[r];
            *reinterpret_cast<float4 *>(lds + 8 * i) = v;
            lds[8 * i + 4] = gd ? gd[r] : 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void get(int rid, float g[5]) const
    {
        const uint32_t slot = (uint32_t)(rid - g_lo);
        if (slot < (uint32_t)g_n) {   // staged (the usual case)
            const float4 v = *reinterpret_cast<const float4 *>(g_lds + 8 * slot);
            g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w; g[4] = g_lds[8 * slot + 4];
        } else {
            RayGrads::get(rid, g);
        }
    }
};
// ... and what they make of one sample: the gradient of the three accumulations w.r.t. its weight (returned) and its
// colour (g_rgb3), from the sample's colour c3, weight w and midpoint.  G is RayGrads or RayGradStage.
template <class G>
__device__ __forceinline__ float sample_grads(const G &rays, bool valid, int rid, const float *c3, float w, float mid, float *g_rgb3)
{
    float g_w = 0.0f;
    g_rgb3[0] = g_rgb3[1] = g_rgb3[2] = 0.0f;
    if (valid) {
        float g[5];
        rays.get(rid, g);
        if (rays.gc) {
            g_w += g[0] * c3[0] + g[1] * c3[1] + g[2] * c3[2];
            g_rgb3[0] = g[0] * w; g_rgb3[1] = g[1] * w; g_rgb3[2] = g[2] * w;
        }
        if (rays.go) g_w += g[3];
        if (rays.gd) g_w += g[4] * mid;
    }
    return g_w;
}

// ---- backward: the gradients arriving at the per-sample weights / trans / alphas (each may be null; EXTRA false: none is
//      looked at), fetched raw and selected under `valid`
template <bool EXTRA>
struct ExtraGrads {
    struct GRaw { F4 gw, gt, ga; };
    const float *gw, *gt, *ga;
    template <bool VEC>
    __device__ __forceinline__ void fetch_extra(const Pos &q, GRaw &r) const
    {
        if (EXTRA) {
            if (gw) ld4<VEC>(gw, q, r.gw);
            if (gt) ld4<VEC>(gt, q, r.gt);
            if (ga) ld4<VEC>(ga, q, r.ga);
        }
    }
    __device__ __forceinline__ void select_extra(const GRaw &r, int j, bool valid, float &GW, float &GT, float &GA) const
    {
        GW = (EXTRA && gw && valid) ? r.gw.v[j] : 0.0f;
        GT = (EXTRA && gt && valid) ? r.gt.v[j] : 0.0f;
        GA = (EXTRA && ga && valid) ? r.ga.v[j] : 0.0f;
    }
};

// ---- backward through the transmittance chain: the reverse scan sums q = GW w + GT T over the samples
//      behind a sample; with E that sum, the gradient w.r.t. sigma * delta is B
__device__ __forceinline__ float chain_input(float GW, float GT, float T, float w) { return GW * w + GT * T; }
__device__ __forceinline__ float chain_grad(bool is_head, const float prev[1], float GW, float GA, float T, float A)
{
    const float E = is_head ? 0.0f : prev[0];
    const float om = 1.0f - A;
    return GW * T * om + GA * om - E;
}

// ---- transmittance / alpha / weights from density, volrend.py:256-264, :358-362
template <bool VEC>
struct DensityFwdOp : OpBase, SampleOut {
    struct Raw { F4 a, b, s, pf; };
    const float *ts, *te, *sig, *prefix;
    // batched rows of row_len samples (PropNetEstimator): the resampler's CDF rows `1 - cat([T, 0])` (row_len + 1 entries,
    // ref estimators/prop_net.py:104-107) written by the same pass; element p of ray r lands at p + r
    float *cdf = nullptr;
    int32_t row_len = 0;
    int32_t crid[SE];
    float xs[SE], pf[SE], rw[SE], rt[SE], ra[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(sig, q, r.s);
        if (prefix) ld4<VEC>(prefix, q, r.pf);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            xs[j] = sigma_delta(valid[j], r.s.v[j], r.b.v[j] - r.a.v[j]);
            pf[j] = prefix ? r.pf.v[j] : 1.0f;
        }
    }
    __device__ __forceinline__ float x(int j, int) const { return xs[j]; }
    __device__ __forceinline__ void emit(int j, int64_t pos, bool valid, bool is_head, int rid, int, const float *, const float prev[1])
    {
        float T, a;
        trans_alpha(is_head, prev, xs[j], T, a);
        if (prefix) T *= pf[j];
        rt[j] = T; ra[j] = a; rw[j] = T * a;
        if (cdf) {
            crid[j] = rid;
            if (valid && is_head) cdf[pos + rid + row_len] = 1.0f;   // the row's last entry, 1 - 0
        }
    }
    __device__ __forceinline__ void store(const Pos &q)
    {
        (void)q.p0();   // (no effect, but without it the compiler allocates this op's registers differently)
        store_wta<VEC>(q, rw, rt, ra);
        if (cdf) {
            // a quad inside one row is one 16-byte store at a 4-byte aligned address (rows are shifted by their index)
            struct __attribute__((packed, aligned(4))) Q4 { float x, y, z, w; };
            float *b = cdf + q.c;
#pragma unroll
            for (int h = 0; h < SQ; ++h) {
                if (q.qall[h] && crid[4 * h] == crid[4 * h + 3]) {
                    Q4 v = {1.0f - rt[4 * h], 1.0f - rt[4 * h + 1], 1.0f - rt[4 * h + 2], 1.0f - rt[4 * h + 3]};
                    *reinterpret_cast<Q4 *>(b + q.off + 4 * h + crid[4 * h]) = v;
                } else {
                    NFA_ELEMENTWISE_PATH();
#pragma unroll
                    for (int j = 4 * h; j < 4 * h + 4; ++j)
                        if (q.valid[j]) b[q.off + j + crid[j]] = 1.0f - rt[j];
                }
            }
        }
    }
};

// ---- transmittance / weights from alpha, volrend.py:200-206, :305-309
template <bool VEC>
struct AlphaFwdOp : OpBase {
    struct Raw { F4 a, pf; };
    const float *al, *prefix;
    float *w, *tr;
    float a4[SE], pf[SE], rw[SE], rt[SE];
    __device__ __forceinline__ float identity(int) const { return 1.0f; }
    __device__ __forceinline__ float comb(int, float a, float b) const { return a * b; }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(al, q, r.a);
        if (prefix) ld4<VEC>(prefix, q, r.pf);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) { a4[j] = sel(r.a, j, valid, 0.0f); pf[j] = prefix ? r.pf.v[j] : 1.0f; }
    }
    __device__ __forceinline__ float x(int j, int) const { return 1.0f - a4[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        float T = is_head ? 1.0f : prev[0];
        if (prefix) T *= pf[j];
        rt[j] = T; rw[j] = T * a4[j];
    }
    __device__ __forceinline__ void store(const Pos &q)
    {
        if (w) store4<VEC>(w, q, rw);
        if (tr) store4<VEC>(tr, q, rt);
    }
};

// ---- backward of the fused density op (reverse scan), SURVEY App. A.7
template <bool VEC, bool CDF = false /* the gradient arrives at the CDF rows of DensityFwdOp::cdf: g_T[p] = -g_cdf[p + ray] */>
struct DensityBwdOp : OpBase, ExtraGrads<true> {
    static constexpr bool NEEDS_RID = CDF;
    struct Raw { F4 a, b, T, A; GRaw g; };
    const float *ts, *te, *tr, *al;
    const float *gcdf = nullptr;
    float *gsig, *gx;
    float T[SE], A[SE], GW[SE], GA[SE], dlt[SE], q[SE], rs[SE], rx[SE];
    int32_t crid[SE];
    __device__ __forceinline__ void pre(int j, int64_t, bool, int rid) { crid[j] = rid; }
    // (called after the ray ids of all the lane's elements are known: a quad inside one row is one 16-byte load)
    __device__ __forceinline__ void store_pre(const Pos &pq)
    {
        struct __attribute__((packed, aligned(4))) Q4 { float x, y, z, w; };
        const float *b = gcdf + pq.c;
#pragma unroll
        for (int h = 0; h < SQ; ++h) {
            float g4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (pq.qall[h] && crid[4 * h] == crid[4 * h + 3]) {
                const Q4 v = *reinterpret_cast<const Q4 *>(b + pq.off + 4 * h + crid[4 * h]);
                g4[0] = v.x; g4[1] = v.y; g4[2] = v.z; g4[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pq.valid[4 * h + j]) g4[j] = b[pq.off + 4 * h + j + crid[4 * h + j]];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                q[4 * h + j] = chain_input(GW[4 * h + j], -g4[j], T[4 * h + j], T[4 * h + j] * A[4 * h + j]);
            }
        }
    }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(tr, q, r.T);
        if (!CDF) ld4<VEC>(al, q, r.A);   // (with only g_T arriving alpha drops out: B = -E, q = g_T T)
        fetch_extra<VEC>(q, r.g);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            T[j] = sel(r.T, j, valid, 0.0f); A[j] = CDF ? 0.0f : sel(r.A, j, valid, 0.0f);
            float GT;
            select_extra(r.g, j, valid[j], GW[j], GT, GA[j]);
            dlt[j] = r.b.v[j] - r.a.v[j];
            q[j] = chain_input(GW[j], GT, T[j], T[j] * A[j]);
        }
    }
    __device__ __forceinline__ float x(int j, int) const { return q[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        const float B = chain_grad(is_head, prev, GW[j], GA[j], T[j], A[j]);
        rx[j] = B; rs[j] = dlt[j] * B;
    }
    __device__ __forceinline__ void store(const Pos &q)
    {
        (void)q.p0();   // (no effect, but without it the compiler allocates this op's registers differently)
        if (gsig) store4<VEC>(gsig, q, rs);
        if (gx) store4<VEC>(gx, q, rx);
    }
};

// ---- backward of the fused alpha op: g_a = g_w T - sum_{i>k}(g_w_i w_i + g_T_i T_i) / max(1-a, 1e-10)
template <bool VEC>
struct AlphaBwdOp : OpBase {
    struct Raw { F4 T, A, gw, gt; };
    const float *al, *tr, *gw, *gt;
    float *galpha;
    float T[SE], A[SE], GW[SE], q[SE], res[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(tr, q, r.T);
        ld4<VEC>(al, q, r.A);
        if (gw) ld4<VEC>(gw, q, r.gw);
        if (gt) ld4<VEC>(gt, q, r.gt);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            T[j] = sel(r.T, j, valid, 0.0f); A[j] = sel(r.A, j, valid, 0.0f);
            GW[j] = (gw && valid[j]) ? r.gw.v[j] : 0.0f;
            const float GT = (gt && valid[j]) ? r.gt.v[j] : 0.0f;
            q[j] = (GW[j] * A[j] + GT) * T[j];
        }
    }
    __device__ __forceinline__ float x(int j, int) const { return q[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        const float E = is_head ? 0.0f : prev[0];
        res[j] = GW[j] * T[j] - E / fmaxf(1.0f - A[j], 1e-10f);
    }
    __device__ __forceinline__ void store(const Pos &q) { store4<VEC>(galpha, q, res); }
};

// ---- visibility mask, volrend.py:412-418 / :474-480.  COUNT adds the per-ray number of visible
//      samples (what the sampler's compaction needs) as a stage-B scan of the mask just computed.
template <bool DENSITY, bool VEC, bool COUNT, bool CS = false>
struct VisibilityOp : OpBase, ConstStep<CS> {
    static constexpr int NCHB = COUNT ? 1 : 0;
    struct Raw { F4 s, pf, a; std::conditional_t<CS, NoQuad, F4> b; };
    const float *ts, *te, *val, *prefix;
    float eps, thre;
    // Density without a prefix: T = exp(-S) >= eps is decided on S (the scanned sum) wherever S is clearly on one side of
    // -ln(eps); only inside a band of a few ulps around it is exp evaluated (same result as evaluating it everywhere: exp
    // is computed with the library's own expf there).  s_lo / s_hi come from the host.
    float s_lo, s_hi;
    uint8_t *vis;
    int64_t *cnts;
    float x0[SE], a4[SE], pf[SE];
    uint8_t m[SE];
    __device__ __forceinline__ float identity(int) const { return DENSITY ? 0.0f : 1.0f; }
    __device__ __forceinline__ float comb(int, float a, float b) const { return DENSITY ? a + b : a * b; }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(val, q, r.s);
        if (prefix) ld4<VEC>(prefix, q, r.pf);
        if (DENSITY) {
            ld4<VEC>(ts, q, r.a);
            if constexpr (!CS) ld4<VEC>(te, q, r.b);
        }
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            pf[j] = prefix ? r.pf.v[j] : 1.0f;
            const float sv = sel(r.s, j, valid, 0.0f);
            if (DENSITY) { x0[j] = valid[j] ? sv * (t_end_of<CS>(*this, r.a, r.b, j) - r.a.v[j]) : 0.0f; a4[j] = (thre > 0.0f) ? 1.0f - expf(-x0[j]) : 1.0f; }  // alpha only when it is tested
            else { a4[j] = sv; x0[j] = 1.0f - sv; }
        }
    }
    __device__ __forceinline__ float x(int j, int) const { return x0[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool valid, bool is_head, int, int, const float *, const float prev[1])
    {
        bool v;
        if (DENSITY && NFA_VIS_EXP_FREE && !prefix) {
            const float S = is_head ? 0.0f : prev[0];
            v = S <= s_lo;
            const bool band = S > s_lo && S < s_hi;
            if (__ballot(band) != 0ull) {   // wave-uniform, rare
                asm volatile("; transmittance near the threshold" ::: "memory");
                if (band) v = expf(-S) >= eps;
            }
        } else {
            float T = DENSITY ? expf(-(is_head ? 0.0f : prev[0])) : (is_head ? 1.0f : prev[0]);
            if (prefix) T *= pf[j];
            v = T >= eps;
        }
        if (thre > 0.0f) v = v && (a4[j] >= thre);
        m[j] = (valid && v) ? 1 : 0;
    }
    __device__ __forceinline__ float xb(int j, int) const { return (float)m[j]; }
    __device__ __forceinline__ void ray_done_b(int rid, int, float tot) const { cnts[rid] = (int64_t)tot; }
    __device__ __forceinline__ void store(const Pos &q)
    {
        uint8_t *b = vis + q.c;
#pragma unroll
        for (int h = 0; h < SQ; ++h) {
            if (VEC && q.qall[h]) {
                *reinterpret_cast<uchar4 *>(b + q.off + 4 * h) = make_uchar4(m[4 * h], m[4 * h + 1], m[4 * h + 2], m[4 * h + 3]);
            } else {
                NFA_ELEMENTWISE_PATH();
#pragma unroll
                for (int j = 4 * h; j < 4 * h + 4; ++j)
                    if (q.valid[j]) b[q.off + j] = m[j];
            }
        }
    }
    __device__ __forceinline__ void empty_ray(int rid) const
    {
        if (COUNT) cnts[rid] = 0;
    }
};

struct U4 { uint32_t w[SQ]; };  // the lane's SE mask bytes, raw
__device__ __forceinline__ void load_mask4(const uint8_t *vis, bool vec, const Pos &q, U4 &m)
{
    const uint8_t *b = vis + q.c;
#pragma unroll
    for (int h = 0; h < SQ; ++h) {
        if (vec) {
            // (written as arithmetic: the plain select became a two-entry table in scratch memory)
            const int32_t o = q.safe + (q.qany[h] ? 1 : 0) * (q.off + 4 * h - q.safe);
            m.w[h] = *reinterpret_cast<const uint32_t *>(b + o);
        } else {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= (uint32_t)b[q.valid[4 * h + j] ? q.off + 4 * h + j : q.safe] << (8 * j);
            m.w[h] = w;
        }
    }
}
__device__ __forceinline__ float mask_sel(const U4 &m, int j, const bool valid[SE])
{
    return (valid[j] && ((m.w[j / 4] >> (8 * (j % 4))) & 0xFFu)) ? 1.0f : 0.0f;
}

// ---- compaction of the visible samples (per-ray output offsets = cumsum of VisibilityOp's counts)
template <bool VEC>
struct CompactOp : OpBase {
    // The kept samples of a step go to CONSECUTIVE output positions (out_starts is the running sum of the per-ray counts and
    // a ray's kept samples are numbered by the scan), so the wave packs them in LDS and writes them out as 16-byte vectors,
    // 4 outputs per lane, instead of three predicated 4/8-byte scatters per element.  A caller whose out_starts are not that
    // running sum still gets every sample written (element-wise fallback, decided per step).
    // The output offsets of the tile's rays (consecutive rays) are staged in LDS when the tile starts, like the fused
    // backward's per-ray gradients: per element they would be a gather that depends on the ray id.
    static constexpr int RAY_CAP = 192;
    static constexpr int RAY_LDS_FLOATS = 3 * SEG_CHUNK + 2 * RAY_CAP;
    struct Raw { U4 m; F4 a, b; };
    const uint8_t *vis;
    int vis_vec;
    const float *ts, *te;
    const int64_t *out_starts;
    int64_t *o_ri;
    float *o_ts, *o_te;
    int64_t cap = (int64_t)1 << 62;   // elements the output arrays hold (a caller that sized them before the total was known)
    float *stage = nullptr;
    const int64_t *s_start = nullptr;
    int32_t g_lo = 0, g_n = 0;
    float m[SE], a[SE], b[SE];
    int64_t dst[SE];
    int32_t er[SE];
    float rank[SE];
    __device__ __forceinline__ void tile_begin(int32_t r_lo, int32_t r_hi, float *lds)
    {
        stage = lds;
        int64_t *st = reinterpret_cast<int64_t *>(lds + 3 * SEG_CHUNK);   // (8-byte aligned: the per-wave block is 16-byte aligned)
        s_start = st; g_lo = r_lo; g_n = min(r_hi - r_lo, RAY_CAP);
        __builtin_amdgcn_wave_barrier();
        for (int32_t i = lane_id(); i < g_n; i += 64) st[i] = out_starts[(int64_t)r_lo + i];
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        load_mask4(vis, vis_vec != 0, q, r.m);
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) { m[j] = mask_sel(r.m, j, valid); a[j] = r.a.v[j]; b[j] = r.b.v[j]; }
    }
    __device__ __forceinline__ float x(int j, int) const { return m[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int rid, int, const float *, const float prev[1])
    {
        er[j] = rid;
        rank[j] = is_head ? 0.0f : prev[0];   // kept samples of the ray in front of this one
    }
    __device__ __forceinline__ void store(const Pos &)
    {
        struct __attribute__((packed, aligned(4))) Q4 { float x, y, z, w; };
        struct __attribute__((packed, aligned(8))) L2 { int64_t x, y; };
        bool keep[SE];
        bool any = false;
        int n_mine = 0;
#pragma unroll
        for (int j = 0; j < SE; ++j) { keep[j] = m[j] != 0.0f; any = any || keep[j]; n_mine += keep[j] ? 1 : 0; }
        const unsigned long long lanes = __ballot(any);
        if (lanes == 0ull) return;  // wave-uniform
        // output offsets of the elements' rays: the staged ones are four independent LDS reads; rays beyond the stage
        // (a tile owning more than RAY_CAP rays) read global memory behind a wave-uniform branch.  (Written as a plain
        // select of the two sources the compiler forms ONE flat load through a select of the two pointers.)
        bool far = false;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            const uint32_t slot = (uint32_t)(er[j] - g_lo);
            const bool staged = slot < (uint32_t)g_n;
            dst[j] = s_start[staged ? slot : 0u];
            far = far || (keep[j] && !staged);
        }
        if (__ballot(far) != 0ull) {
            asm volatile("; output offsets beyond the staged rays" ::: "memory");
#pragma unroll
            for (int j = 0; j < SE; ++j)
                if (keep[j] && (uint32_t)(er[j] - g_lo) >= (uint32_t)g_n) dst[j] = out_starts[er[j]];
        }
#pragma unroll
        for (int j = 0; j < SE; ++j) dst[j] = keep[j] ? dst[j] + (int64_t)rank[j] : 0;
        const int lane = lane_id();
        const int first = __builtin_ctzll(lanes), last = 63 - __builtin_clzll(lanes);
        int64_t my_first = dst[SE - 1], my_last = dst[0];
#pragma unroll
        for (int j = SE - 2; j >= 0; --j) if (keep[j]) my_first = dst[j];
#pragma unroll
        for (int j = 1; j < SE; ++j) if (keep[j]) my_last = dst[j];
        const int64_t base = uniform64(__shfl(my_first, first, 64));
        const int64_t span = uniform64(__shfl(my_last, last, 64)) - base + 1;
        // number kept in the step (sum over lanes): equals span exactly when the outputs are consecutive
        int cnt = n_mine;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (span == (int64_t)cnt && span <= SEG_CHUNK) {
            float *s_ts = stage, *s_te = stage + SEG_CHUNK;
            int32_t *s_ri = reinterpret_cast<int32_t *>(stage + 2 * SEG_CHUNK);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < SE; ++j)
                if (keep[j]) {
                    const uint32_t o = (uint32_t)(dst[j] - base);
                    if (o < (uint32_t)SEG_CHUNK) { s_ts[o] = a[j]; s_te[o] = b[j]; s_ri[o] = er[j]; }
                }
            __builtin_amdgcn_wave_barrier();
            const int n = (int)max((int64_t)0, min(span, cap - base));   // nothing at or beyond the capacity
            float *g_ts = o_ts + base, *g_te = o_te + base;
            int64_t *g_ri = o_ri + base;
            for (int o = 4 * lane; o < n; o += 256) {
                if (o + 3 < n) {
                    const Q4 vt = {s_ts[o], s_ts[o + 1], s_ts[o + 2], s_ts[o + 3]};
                    const Q4 ve = {s_te[o], s_te[o + 1], s_te[o + 2], s_te[o + 3]};
                    *reinterpret_cast<Q4 *>(g_ts + o) = vt;
                    *reinterpret_cast<Q4 *>(g_te + o) = ve;
                    const L2 r0 = {(int64_t)s_ri[o], (int64_t)s_ri[o + 1]}, r1 = {(int64_t)s_ri[o + 2], (int64_t)s_ri[o + 3]};
                    *reinterpret_cast<L2 *>(g_ri + o) = r0;
                    *reinterpret_cast<L2 *>(g_ri + o + 2) = r1;
                } else {
                    for (int i = o; i < n; ++i) { g_ts[i] = s_ts[i]; g_te[i] = s_te[i]; g_ri[i] = (int64_t)s_ri[i]; }
                }
            }
            __builtin_amdgcn_wave_barrier();
        } else {
#pragma unroll
            for (int j = 0; j < SE; ++j)
                if (keep[j] && dst[j] < cap) { o_ri[dst[j]] = er[j]; o_ts[dst[j]] = a[j]; o_te[dst[j]] = b[j]; }
        }
    }
};

// ---- per-ray accumulation of w * values[:, d0:d0+C], volrend.py:532-547
template <int C, bool VEC>
struct AccumOp : OpBase {
    static constexpr int NCH = C;
    static constexpr bool TOTALS = true;
    struct Raw { F4 w; float v[SE][C]; };
    const float *w, *vals;  // vals may be null (C == 1): accumulate w
    int32_t D, d0;
    float *out;
    int accumulate;
    float xv[SE][C];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(w, q, r.w);
        if (vals) {
#pragma unroll
            for (int j = 0; j < SE; ++j)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) r.v[j][ch] = vals[(q.c + (q.valid[j] ? q.off + j : q.safe)) * D + d0 + ch];
        }
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j)
#pragma unroll
            for (int ch = 0; ch < C; ++ch) xv[j][ch] = valid[j] ? (vals ? r.w.v[j] * r.v[j][ch] : r.w.v[j]) : 0.0f;
    }
    __device__ __forceinline__ float x(int j, int ch) const { return xv[j][ch]; }
    __device__ __forceinline__ void put(int rid, const float *tot) const
    {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            float *o = out + (int64_t)rid * D + d0 + ch;
            *o = accumulate ? *o + tot[ch] : tot[ch];
        }
    }
    __device__ __forceinline__ void emit(int, int64_t, bool, bool, int, int, const float *, const float *) const {}
    __device__ __forceinline__ void store(const Pos &) const {}
    __device__ __forceinline__ void ray_done(int rid, const float tot[C]) const { put(rid, tot); }
    __device__ __forceinline__ void empty_ray(int rid) const
    {
        if (!accumulate)
#pragma unroll
            for (int ch = 0; ch < C; ++ch) out[(int64_t)rid * D + d0 + ch] = 0.0f;
    }
};

template <int C, bool VEC>
struct AccumBwdOp : OpBase {
    struct Raw { F4 w, g; float v[SE][C]; };
    const float *w, *vals, *gout;
    int32_t D, d0;
    int first;  // first channel group: g_w is written, later groups add to it
    float *gw, *gv;
    float ww[SE], res[SE], vv[SE][C];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(w, q, r.w);
        if (gw && !first) ld4<VEC>(gw, q, r.g);
        if (vals) {
#pragma unroll
            for (int j = 0; j < SE; ++j)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) r.v[j][ch] = vals[(q.c + (q.valid[j] ? q.off + j : q.safe)) * D + d0 + ch];
        }
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &)
    {
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            ww[j] = r.w.v[j];
            res[j] = (gw && !first) ? r.g.v[j] : 0.0f;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) vv[j][ch] = vals ? r.v[j][ch] : 0.0f;
        }
    }
    __device__ __forceinline__ float x(int, int) const { return 0.0f; }
    __device__ __forceinline__ void emit(int j, int64_t pos, bool valid, bool, int rid, int, const float *, const float *)
    {
        if (!valid) return;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const float go = gout[(int64_t)rid * D + d0 + ch];
            if (vals) {
                res[j] += go * vv[j][ch];
                if (gv) gv[pos * D + d0 + ch] = go * ww[j];
            } else {
                res[j] += go;
            }
        }
    }
    __device__ __forceinline__ void store(const Pos &q)
    {
        if (gw) store4<VEC>(gw, q, res);
    }
};

// 4 x rgb (12 consecutive floats at 3*p), raw.  With VEC the 48 bytes are three aligned 16 B loads from
// p0 when all 4 elements are valid, else from the step's base (always inside the array); the few
// lanes that straddle a range end re-read their valid elements one by one in fix_rgb12.
__device__ __forceinline__ void load_rgb12(const float *rgb, bool vec, const Pos &q, float c[3 * SE])
{
    const float *b = rgb + 3 * q.c;
    if (vec) {
#pragma unroll
        for (int h = 0; h < SQ; ++h) {
            const float4 *v = reinterpret_cast<const float4 *>(b + 3 * (q.qall[h] ? q.off + 4 * h : q.safe));
            const float4 q0 = v[0], q1 = v[1], q2 = v[2];
            float *o = c + 12 * h;
            o[0] = q0.x; o[1] = q0.y; o[2] = q0.z; o[3] = q0.w; o[4] = q1.x; o[5] = q1.y;
            o[6] = q1.z; o[7] = q1.w; o[8] = q2.x; o[9] = q2.y; o[10] = q2.z; o[11] = q2.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SE; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[3 * j + k] = b[3 * (q.valid[j] ? q.off + j : q.safe) + k];
    }
}
__device__ __forceinline__ void fix_rgb12(const float *rgb, bool vec, const Pos &q, const float raw[3 * SE], float c[3 * SE])
{
#pragma unroll
    for (int k = 0; k < 3 * SE; ++k) c[k] = raw[k];
    if (vec && q.any && !q.all) {  // rare: first / last lane of a range
        const float *b = rgb + 3 * q.c;
#pragma unroll
        for (int j = 0; j < SE; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (!q.qall[j / 4]) c[3 * j + k] = q.valid[j] ? b[3 * (q.off + j) + k] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < SE; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[3 * j + k] = q.valid[j] ? c[3 * j + k] : 0.0f;
}

// SE x rgb out: three 16 B stores per full quad, element-wise (see store4) where a range ends
__device__ __forceinline__ void store_rgb12(float *rgb, bool vec, const Pos &q, const float g[3 * SE])
{
    float *b = rgb + 3 * q.c;
#pragma unroll
    for (int h = 0; h < SQ; ++h) {
        if (vec && q.qall[h]) {
            float *o = b + 3 * (q.off + 4 * h);
            const float *s = g + 12 * h;
            store_f4(o, s[0], s[1], s[2], s[3]);
            store_f4(o + 4, s[4], s[5], s[6], s[7]);
            store_f4(o + 8, s[8], s[9], s[10], s[11]);
        } else {
            NFA_ELEMENTWISE_PATH();
#pragma unroll
            for (int j = 4 * h; j < 4 * h + 4; ++j)
                if (q.valid[j]) {
                    b[3 * (q.off + j)] = g[3 * j]; b[3 * (q.off + j) + 1] = g[3 * j + 1]; b[3 * (q.off + j) + 2] = g[3 * j + 2];
                }
        }
    }
}

// Half twins of ld4 / store4 / load_rgb12 / fix_rgb12 / store_rgb12 for raw streams of E = fp16 or bf16 (common.hip.h).  A
// lane's 4 elements are 8 bytes, its 4 colours 24: with VEC (the stream 8-byte aligned) one and three 8-byte vectors, raw
// like the float loads -- the halves are widened where they are consumed (elem / fix_rgb12), not behind the load.
// Without VEC every element is a 2-byte access, packed into the same dwords.
static_assert(SE == 4, "the half twins move one 8-byte quad per lane");
template <class E> struct H4 { uint32_t w[2]; };    // one lane's elements of a step, raw
template <class E> struct H12 { uint32_t w[6]; };   // one lane's colours of a step, raw
__device__ __forceinline__ float elem(const F4 &r, int j) { return r.v[j]; }
template <class E>
__device__ __forceinline__ float elem(const H4<E> &r, int j) { return unpack_half<E>(r.w[j / 2], j % 2); }
__device__ __forceinline__ uint32_t raw_half(const void *b, int32_t i) { return reinterpret_cast<const uint16_t *>(b)[i]; }

template <bool VEC, class E>
__device__ __forceinline__ void ld4(const E *__restrict__ p, const Pos &q, H4<E> &out)
{
    const E *b = p + q.c;
    if (VEC) {
        const nfa_v2u v = *reinterpret_cast<const nfa_v2u *>(b + (q.qany[0] ? q.off : q.safe));
        out.w[0] = v.x; out.w[1] = v.y;
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h)
            out.w[h] = raw_half(b, q.valid[2 * h] ? q.off + 2 * h : q.safe) | (raw_half(b, q.valid[2 * h + 1] ? q.off + 2 * h + 1 : q.safe) << 16);
    }
}
template <bool VEC, class E>
__device__ __forceinline__ void store4(E *__restrict__ p, const Pos &q, const float v[SE])
{
    E *b = p + q.c;
    if (VEC && q.qall[0]) {
        const nfa_v2u w = {pack_halves<E>(v[0], v[1]), pack_halves<E>(v[2], v[3])};
        *reinterpret_cast<nfa_v2u *>(b + q.off) = w;
    } else {
        NFA_ELEMENTWISE_PATH();
#pragma unroll
        for (int j = 0; j < SE; ++j)
            if (q.valid[j]) reinterpret_cast<uint16_t *>(b)[q.off + j] = (uint16_t)half_bits<E>(v[j]);
    }
}
template <class E>
__device__ __forceinline__ void load_rgb12(const E *rgb, bool vec, const Pos &q, H12<E> &c)
{
    const E *b = rgb + 3 * q.c;
    if (vec) {
        const nfa_v2u *v = reinterpret_cast<const nfa_v2u *>(b + 3 * (q.qall[0] ? q.off : q.safe));
        const nfa_v2u q0 = v[0], q1 = v[1], q2 = v[2];
        c.w[0] = q0.x; c.w[1] = q0.y; c.w[2] = q1.x; c.w[3] = q1.y; c.w[4] = q2.x; c.w[5] = q2.y;
    } else {
#pragma unroll
        for (int j = 0; j < SE; j += 2) {   // two samples: six halves, three dwords
            const int32_t e0 = 3 * (q.valid[j] ? q.off + j : q.safe), e1 = 3 * (q.valid[j + 1] ? q.off + j + 1 : q.safe);
            c.w[3 * j / 2] = raw_half(b, e0) | (raw_half(b, e0 + 1) << 16);
            c.w[3 * j / 2 + 1] = raw_half(b, e0 + 2) | (raw_half(b, e1) << 16);
            c.w[3 * j / 2 + 2] = raw_half(b, e1 + 1) | (raw_half(b, e1 + 2) << 16);
        }
    }
}
template <class E>
__device__ __forceinline__ void fix_rgb12(const E *rgb, bool vec, const Pos &q, const H12<E> &raw, float c[3 * SE])
{
#pragma unroll
    for (int k = 0; k < 3 * SE; ++k) c[k] = unpack_half<E>(raw.w[k / 2], k % 2);
    if (vec && q.any && !q.all) {  // rare: first / last lane of a range
        const E *b = rgb + 3 * q.c;
#pragma unroll
        for (int j = 0; j < SE; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[3 * j + k] = q.valid[j] ? half_value<E>(raw_half(b, 3 * (q.off + j) + k)) : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < SE; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[3 * j + k] = q.valid[j] ? c[3 * j + k] : 0.0f;
}
template <class E>
__device__ __forceinline__ void store_rgb12(E *rgb, bool vec, const Pos &q, const float g[3 * SE])
{
    E *b = rgb + 3 * q.c;
    if (vec && q.qall[0]) {
        nfa_v2u *o = reinterpret_cast<nfa_v2u *>(b + 3 * q.off);
        const nfa_v2u w0 = {pack_halves<E>(g[0], g[1]), pack_halves<E>(g[2], g[3])};
        const nfa_v2u w1 = {pack_halves<E>(g[4], g[5]), pack_halves<E>(g[6], g[7])};
        const nfa_v2u w2 = {pack_halves<E>(g[8], g[9]), pack_halves<E>(g[10], g[11])};
        o[0] = w0; o[1] = w1; o[2] = w2;
    } else {
        NFA_ELEMENTWISE_PATH();
#pragma unroll
        for (int j = 0; j < SE; ++j)
            if (q.valid[j]) {
#pragma unroll
                for (int k = 0; k < 3; ++k) reinterpret_cast<uint16_t *>(b)[3 * (q.off + j) + k] = (uint16_t)half_bits<E>(g[3 * j + k]);
            }
    }
}
// what an op keeps of a step's raw loads from a stream of E
template <class E> struct RawStream { typedef H4<E> S4; typedef H12<E> C12; };
template <> struct RawStream<float> { typedef F4 S4; typedef float C12[3 * SE]; };
template <class E> using Quad = typename RawStream<E>::S4;    // a lane's 4 elements of a step
template <class E> using Rgb12 = typename RawStream<E>::C12;  // its 4 colours

// ---- the three accumulations of `rendering` fused: colours(3), opacity, depth  (volrend.py:140-151)
template <bool VEC>
struct RenderAccumOp : OpBase, RayOut {
    static constexpr int NCH = 5;
    static constexpr bool TOTALS = true;
    struct Raw { Quad<float> w, a, b; Rgb12<float> c; };
    const float *w, *rgb, *ts, *te;
    float xv[SE][5];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(w, q, r.w);
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
        float c[3 * SE];
        fix_rgb12(rgb, VEC, pos, r.c, c);
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            const float ww = sel(r.w, j, valid, 0.0f);
#pragma unroll
            for (int ch = 0; ch < 5; ++ch) xv[j][ch] = render_channel(ch, ww, c + 3 * j, midpoint(r.a.v[j], r.b.v[j]));
        }
    }
    __device__ __forceinline__ float x(int j, int ch) const { return xv[j][ch]; }
    __device__ __forceinline__ void emit(int, int64_t, bool, bool, int, int, const float *, const float *) const {}
    __device__ __forceinline__ void store(const Pos &) const {}
    __device__ __forceinline__ void ray_done(int rid, const float t[5]) const { ray_store(rid, t); }
    __device__ __forceinline__ void empty_ray(int rid) const { ray_zero(rid); }
};

template <bool VEC>
struct RenderAccumBwdOp : OpBase, RayGrads {
    struct Raw { Quad<float> w, a, b; Rgb12<float> c; };
    const float *w, *rgb, *ts, *te;
    float *gw, *grgb;
    float ww[SE], mid[SE], res[SE], c[3 * SE], gr[3 * SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(w, q, r.w);
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
#pragma unroll
        for (int j = 0; j < SE; ++j) { ww[j] = r.w.v[j]; mid[j] = midpoint(r.a.v[j], r.b.v[j]); }
        fix_rgb12(rgb, VEC, pos, r.c, c);
    }
    __device__ __forceinline__ float x(int, int) const { return 0.0f; }
    __device__ __forceinline__ void emit(int j, int64_t, bool valid, bool, int rid, int, const float *, const float *)
    {
        res[j] = sample_grads(*this, valid, rid, c + 3 * j, ww[j], mid[j], gr + 3 * j);
    }
    __device__ __forceinline__ void store(const Pos &q)
    {
        if (gw) store4<VEC>(gw, q, res);
        if (grgb) store_rgb12(grgb, VEC, q, gr);
    }
};

// ---- `rendering` with a density callback in ONE pass (volrend.py:109-151): stage A scans
//      sigma*delta into transmittance -> (w, T, alpha); stage B scans w*rgb, w, w*mid into the per-ray
//      colour / opacity / un-normalised depth.  Bit-identical to DensityFwdOp followed by
//      RenderAccumOp (same expressions, same scan tree), 12 B/sample less traffic.
template <bool VEC, bool CS = false>
struct RenderFusedFwdOp : RenderFwdStage, SampleOut, ConstStep<CS> {   // (81 VGPRs: one over the 6-wave budget; asking for 6 waves was within noise)
    struct Raw { Quad<float> a; std::conditional_t<CS, NoQuad, Quad<float>> b; Quad<float> s; Rgb12<float> c; };
    const float *ts, *te, *sig, *rgb;
    float rt[SE], ra[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        if constexpr (!CS) ld4<VEC>(te, q, r.b);
        ld4<VEC>(sig, q, r.s);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        fix_rgb12(rgb, VEC, pos, r.c, c);
#pragma unroll
        for (int j = 0; j < SE; ++j) sample(j, pos.valid[j], r.s.v[j], r.a.v[j], t_end_of<CS>(*this, r.a, r.b, j));
    }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        trans_alpha(is_head, prev, xs[j], rt[j], ra[j]);
        rw[j] = rt[j] * ra[j];
    }
    __device__ __forceinline__ void ray_done_b(int rid, int ch, float t) const { ray_store(rid, ch, t); }
    __device__ __forceinline__ void empty_ray(int rid) const { ray_zero(rid); }
    __device__ __forceinline__ void store(const Pos &q) { store_wta<VEC>(q, rw, rt, ra); }
};

// ---- one iteration of the test-mode marching loop (ref: examples/utils.py:370-405) in one pass: weights with
//      prefix_trans = 1 - opacity[ray] (the ray id is known before the scan), samples with alpha < alpha_thre dropped,
//      and rgb / opacity / depth accumulated IN PLACE into the per-ray image buffers.  Nothing per sample is written.
//      A ray is owned by one wave, which reads its old opacity for all the ray's samples before it adds the total.
template <bool VEC>
struct RenderStepOp : RenderFwdStage {
    static constexpr bool NEEDS_RID = true;
    struct Raw { Quad<float> a, b, s; Rgb12<float> c; };
    const float *ts, *te, *sig, *rgb;
    float thre;
    unsigned long long *n_visible;  // [NFA_VISIBLE_SLOTS] += samples that pass the alpha threshold (the loop's sample count), or null
    float pf[SE];
    bool keep[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(sig, q, r.s);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        fix_rgb12(rgb, VEC, pos, r.c, c);
#pragma unroll
        for (int j = 0; j < SE; ++j) sample(j, pos.valid[j], r.s.v[j], r.a.v[j], r.b.v[j]);
    }
    __device__ __forceinline__ void pre(int j, int64_t, bool valid, int rid) { pf[j] = valid ? 1.0f - opac[rid] : 1.0f; }
    __device__ __forceinline__ void store_pre(const Pos &) const {}
    __device__ __forceinline__ void emit(int j, int64_t, bool valid, bool is_head, int, int, const float *, const float prev[1])
    {
        float T, a;
        trans_alpha(is_head, prev, xs[j], T, a);
        T = T * pf[j];
        keep[j] = valid && !(thre > 0.0f && !(a >= thre));
        rw[j] = keep[j] ? T * a : 0.0f;
    }
    __device__ __forceinline__ void ray_done_b(int rid, int ch, float t) const { ray_add(rid, ch, t); }
    __device__ __forceinline__ void store(const Pos &) const
    {
        if (n_visible) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < SE; ++j) c += __builtin_popcountll(__ballot(keep[j]));
            // One counter per step was one ADDRESS for the whole launch: atomics on one address are served one after the
            // other by its L2 channel (~15 ns each), and 33 k steps (8 M samples) made that 0.5 ms -- the whole pass.  The count
            // is spread over NFA_VISIBLE_SLOTS counters by wave; the caller adds them up.
            if (c > 0 && lane_id() == 0)
                atomicAdd(n_visible + ((blockIdx.x * SEG_WAVES_PER_BLOCK + (threadIdx.x >> 6)) & (NFA_VISIBLE_SLOTS - 1)), (unsigned long long)c);
        }
    }
};

// ---- what the one-pass backward ops share (one reverse pass): the gradient of the three accumulations w.r.t. w is formed
//      from the per-ray output gradients (needs the ray id before the scan: NEEDS_RID), added to the gradients arriving at
//      extras' weights / trans / alphas, and pushed through the transmittance chain.  Same expressions as
//      RenderAccumBwdOp followed by DensityBwdOp.
template <bool EXTRA /* gradients arrive at weights / trans / alphas too */>
struct RenderBwdStage : OpBase, RayGradStage, ExtraGrads<EXTRA> {
    static constexpr bool NEEDS_RID = true;
    static constexpr int RAY_LDS_FLOATS = RayGradStage::LDS_FLOATS;
    static constexpr bool PIPE = true;   // measured per op: a full step ahead is 2-4 % faster here (313 -> 300 us), 2 % slower on the forward pass
    float T[SE], A[SE], GW[SE], GT[SE], GA[SE], dlt[SE], mid[SE], q[SE], rs[SE], c[3 * SE], gr[3 * SE];
    // T, A, c and the extra gradients of the step are in place
    __device__ __forceinline__ void sample(int j, float ts, float te) { dlt[j] = te - ts; mid[j] = midpoint(ts, te); }
    __device__ __forceinline__ void pre(int j, int64_t, bool valid, int rid)
    {
        const float wj = T[j] * A[j];
        GW[j] = sample_grads(*this, valid, rid, c + 3 * j, wj, mid[j], gr + 3 * j) + GW[j];
        q[j] = chain_input(GW[j], GT[j], T[j], wj);
    }
    __device__ __forceinline__ float x(int j, int) const { return q[j]; }
    __device__ __forceinline__ float chain(int j, bool is_head, const float prev[1]) const
    {
        return chain_grad(is_head, prev, GW[j], GA[j], T[j], A[j]);
    }
};

template <bool VEC, bool EXTRA, bool CS = false>
struct RenderFusedBwdOp : RenderBwdStage<EXTRA>, ConstStep<CS> {   // (98 VGPRs without EXTRA: two over the 5-wave budget; asking for 5 waves was within noise)
    typedef RenderBwdStage<EXTRA> S;
    struct Raw { Quad<float> a; std::conditional_t<CS, NoQuad, Quad<float>> b; Quad<float> T, A; typename S::GRaw g; Rgb12<float> c; };
    const float *ts, *te, *rgb, *tr, *al;
    float *gsig, *grgb;
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        if constexpr (!CS) ld4<VEC>(te, q, r.b);
        ld4<VEC>(tr, q, r.T);
        ld4<VEC>(al, q, r.A);
        this->template fetch_extra<VEC>(q, r.g);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
        fix_rgb12(rgb, VEC, pos, r.c, S::c);
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            S::T[j] = sel(r.T, j, valid, 0.0f); S::A[j] = sel(r.A, j, valid, 0.0f);
            this->select_extra(r.g, j, valid[j], S::GW[j], S::GT[j], S::GA[j]);
            S::sample(j, r.a.v[j], t_end_of<CS>(*this, r.a, r.b, j));
        }
    }
    // g_rgb is complete before the scan: stored first (frees its registers, stores in flight during the scan)
    __device__ __forceinline__ void store_pre(const Pos &pq)
    {
        if (grgb) store_rgb12(grgb, VEC, pq, S::gr);
    }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        S::rs[j] = S::dlt[j] * S::chain(j, is_head, prev);
    }
    __device__ __forceinline__ void store(const Pos &pq)
    {
        if (gsig) store4<VEC>(gsig, pq, S::rs);
    }
};

// ---- `rendering` from the field's RAW outputs: the two passes above with the field's last activations applied on load
//      (examples/radiance_fields/ngp.py:23-36,174-175,196: density = trunc_exp(x - 1) * selector, rgb = sigmoid(x)).
//      The activation kind is a member, so its branch is wave-uniform; with NFA_ACT_NONE, bias 0 and no mask both passes
//      compute what RenderFusedFwdOp / RenderFusedBwdOp compute, bit for bit: they are the same shared steps around another
//      load.  The backward keeps no activated value: it forms sigma, alpha and c again from the raw ones with the
//      forward's expressions.
//      Compiler's report (VEC forms, no scratch in any): forward 91 VGPRs against RenderFusedFwdOp's 81, both 5 waves per
//      SIMD; backward 117 against RenderFusedBwdOp's 117 (4 waves), with EXTRA 141 against 136 (3 waves).
struct RawAct {
    const uint8_t *mask;   // [n] bool, or null: where false the density is exactly 0 and so is its gradient
    int32_t mask_vec;      // mask is 4-byte aligned
    int32_t dens, col;     // NFA_ACT_* / NFA_RGB_ACT_*
    float bias;
    __device__ __forceinline__ float density(float z) const
    {
        switch (dens) {
        case NFA_ACT_TRUNC_EXP:
        case NFA_ACT_EXP: return expf(z);
        case NFA_ACT_RELU: return z < 0.0f ? 0.0f : z;
        case NFA_ACT_SOFTPLUS: return z > 20.0f ? z : log1pf(expf(z));   // torch's defaults: beta 1, threshold 20
        default: return z;
        }
    }
    // d density / d z, given the density itself
    __device__ __forceinline__ float density_grad(float z, float s) const
    {
        switch (dens) {
        case NFA_ACT_TRUNC_EXP: return expf(fminf(z, 15.0f));
        case NFA_ACT_EXP: return s;
        case NFA_ACT_RELU: return z > 0.0f ? 1.0f : 0.0f;
        case NFA_ACT_SOFTPLUS: return z > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-z));
        default: return 1.0f;
        }
    }
    __device__ __forceinline__ void colours(float c[3 * SE]) const
    {
        if (col == NFA_RGB_ACT_SIGMOID) {
#pragma unroll
            for (int k = 0; k < 3 * SE; ++k) c[k] = 1.0f / (1.0f + expf(-c[k]));
        }
    }
    __device__ __forceinline__ bool live(const U4 &m, int j) const { return !mask || ((m.w[j / 4] >> (8 * (j % 4))) & 0xFFu); }
};

template <bool VEC, class ET /* element type of sig / rgb / asig / argb */>
struct RenderRawFwdOp : RenderFwdStage, SampleOut {
    struct Raw { Quad<float> a, b; Quad<ET> s; U4 m; Rgb12<ET> c; };
    const float *ts, *te;
    const ET *sig, *rgb;
    RawAct act;
    ET *asig, *argb;
    float sg[SE], rt[SE], ra[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(sig, q, r.s);
        if (act.mask) load_mask4(act.mask, act.mask_vec != 0, q, r.m);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        fix_rgb12(rgb, VEC, pos, r.c, c);
        act.colours(c);
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            sg[j] = act.live(r.m, j) ? act.density(elem(r.s, j) + act.bias) : 0.0f;
            sample(j, pos.valid[j], sg[j], r.a.v[j], r.b.v[j]);
        }
    }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        trans_alpha(is_head, prev, xs[j], rt[j], ra[j]);
        rw[j] = rt[j] * ra[j];
    }
    __device__ __forceinline__ void ray_done_b(int rid, int ch, float t) const { ray_store(rid, ch, t); }
    __device__ __forceinline__ void empty_ray(int rid) const { ray_zero(rid); }
    __device__ __forceinline__ void store(const Pos &q)
    {
        store_wta<VEC>(q, rw, rt, ra);
        if (asig) store4<VEC>(asig, q, sg);
        if (argb) store_rgb12(argb, VEC, q, c);
    }
};

template <bool VEC, bool EXTRA, class ET /* of sig / rgb / gsig / grgb */>
struct RenderRawBwdOp : RenderBwdStage<EXTRA> {
    typedef RenderBwdStage<EXTRA> S;
    struct Raw { Quad<float> a, b, T; Quad<ET> s; typename S::GRaw g; U4 m; Rgb12<ET> c; };
    const float *ts, *te;
    const ET *sig, *rgb;
    const float *tr;
    RawAct act;
    ET *gsig, *grgb;
    float ds[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(tr, q, r.T);
        ld4<VEC>(sig, q, r.s);
        this->template fetch_extra<VEC>(q, r.g);
        if (act.mask) load_mask4(act.mask, act.mask_vec != 0, q, r.m);
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
        fix_rgb12(rgb, VEC, pos, r.c, S::c);
        act.colours(S::c);
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            // sigma and alpha as the forward pass formed them
            const bool on = act.live(r.m, j);
            const float z = elem(r.s, j) + act.bias;
            const float s = on ? act.density(z) : 0.0f;
            ds[j] = (on && valid[j]) ? act.density_grad(z, s) : 0.0f;
            S::sample(j, r.a.v[j], r.b.v[j]);
            S::T[j] = sel(r.T, j, valid, 0.0f); S::A[j] = valid[j] ? alpha_of(sigma_delta(valid[j], s, S::dlt[j])) : 0.0f;
            this->select_extra(r.g, j, valid[j], S::GW[j], S::GT[j], S::GA[j]);
        }
    }
    __device__ __forceinline__ void pre(int j, int64_t pos, bool valid, int rid)
    {
        S::pre(j, pos, valid, rid);
        if (valid && S::gc && act.col == NFA_RGB_ACT_SIGMOID) {   // d sigmoid = c (1 - c)
#pragma unroll
            for (int k = 0; k < 3; ++k) S::gr[3 * j + k] *= S::c[3 * j + k] * (1.0f - S::c[3 * j + k]);
        }
    }
    __device__ __forceinline__ void store_pre(const Pos &pq)
    {
        if (grgb) store_rgb12(grgb, VEC, pq, S::gr);
    }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        // (a select, not a product: where the derivative is 0 -- a masked sample -- the gradient is exactly 0)
        S::rs[j] = ds[j] != 0.0f ? S::dlt[j] * S::chain(j, is_head, prev) * ds[j] : 0.0f;
    }
    __device__ __forceinline__ void store(const Pos &pq)
    {
        if (gsig) store4<VEC>(gsig, pq, S::rs);
    }
};

// ---- `rendering` of a signed-distance field: the two passes above with the SDF-to-opacity conversion of NeuS (Wang et
//      al. 2021, the logistic CDF of the SDF at the two ends of a sample) or VolSDF (Yariv et al. 2021, the Laplace CDF of
//      the SDF times 1 / beta) applied on load.  What the conversion yields is x, the summand of stage A
//      (RenderFwdStage::xs): alpha = 1 - exp(-x), T = exp(-sum of x in front), so trans_alpha / chain_grad serve unchanged.
//      The model is a template parameter; the mask and the sigmoid colour step are RawAct's.  The backward keeps trans
//      only: it forms x, alpha and c again with the forward's expressions (the same function, so bit for bit) and
//      multiplies dL/dx into the derivatives of x.
//      Arithmetic: float32 throughout, no contraction (-ffp-contract=off), expf / log1pf of the device library.  With
//      d = t_end - t_start, r = cos_anneal_ratio, s = *param (inv_s / beta: ONE float read through its device pointer, the
//      same for every sample):
//        NeuS    ct = -(max(0.5 - 0.5 cos, 0) (1 - r) + max(-cos, 0) r)                          (<= 0)
//                h = ct (d 0.5);  n = sdf + h;  p = sdf - h                                      (next, previous: n <= p)
//                sp(y) = max(y, 0) + log1pf(expf(-|y|))
//                x = max(sp(-s n) - sp(-s p), 0)        = log Phi(s p) - log Phi(s n), Phi the logistic function: the
//                                                         published (Phi(p) - Phi(n) + 1e-5) / (Phi(p) + 1e-5) without its 1e-5
//                with sn = 1 / (1 + expf(s n)), sq = 1 / (1 + expf(s p)), and all three exactly 0 where x is 0:
//                dx/dsdf = s (sq - sn);  dx/dcos = -(s (d 0.5)) (sn + sq) (0.5 (1 - r) [cos < 1] + r [cos < 0]);
//                dx/ds = p sq - n sn
//        VolSDF  e = 0.5 expf(-|sdf| / s);  psi = sdf >= 0 ? e : 1 - e;  sigma = psi / s;  x = sigma d
//                dx/dsdf = d (-e / (s s));  dx/ds = d (-psi / (s s) + e sdf / (s s s))
//      Where the mask is false x and every derivative are exactly 0 (selects, not products).  The gradient towards s is
//      written per sample (dL/dx dx/ds); the caller sums the stream, so no float atomics and two runs give the same bits.
//      Compiler's report: DESIGN.md, "Rendering from SDF fields".
struct SdfParam {
    const float *value;   // [1] on the device: inv_s (NeuS) or beta (VolSDF)
    float ratio;          // cos_anneal_ratio (NeuS)
};
__device__ __forceinline__ float sdf_softplus(float y) { return fmaxf(y, 0.0f) + log1pf(expf(-fabsf(y))); }
__device__ __forceinline__ float sdf_logistic_neg(float y) { return 1.0f / (1.0f + expf(y)); }   // Phi(-y)

template <int MODEL> struct SdfModel;
template <>
struct SdfModel<NFA_SDF_NEUS> {
    static constexpr bool HAS_COS = true;
    // x of one sample; with D also its derivatives w.r.t. sdf, cos and s
    template <bool D>
    static __device__ __forceinline__ float x(float sdf, float cs, float d, float s, float r, float &dx_sdf, float &dx_cos, float &dx_s)
    {
        const float ct = -(fmaxf(0.5f - 0.5f * cs, 0.0f) * (1.0f - r) + fmaxf(-cs, 0.0f) * r);
        const float hd = d * 0.5f;
        const float h = ct * hd;
        const float n = sdf + h, p = sdf - h;
        const float diff = sdf_softplus(-s * n) - sdf_softplus(-s * p);
        const float xv = diff < 0.0f ? 0.0f : diff;
        if (D) {
            const bool on = xv > 0.0f;
            const float sn = sdf_logistic_neg(s * n), sq = sdf_logistic_neg(s * p);
            const float dct = 0.5f * (1.0f - r) * (cs < 1.0f ? 1.0f : 0.0f) + r * (cs < 0.0f ? 1.0f : 0.0f);
            dx_sdf = on ? s * (sq - sn) : 0.0f;
            dx_cos = on ? -(s * hd) * (sn + sq) * dct : 0.0f;
            dx_s = on ? p * sq - n * sn : 0.0f;
        }
        return xv;
    }
};
template <>
struct SdfModel<NFA_SDF_VOLSDF> {
    static constexpr bool HAS_COS = false;
    template <bool D>
    static __device__ __forceinline__ float x(float sdf, float, float d, float s, float, float &dx_sdf, float &dx_cos, float &dx_s)
    {
        const float e = 0.5f * expf(-fabsf(sdf) / s);
        const float psi = sdf >= 0.0f ? e : 1.0f - e;
        if (D) {
            const float s2 = s * s;
            dx_sdf = d * (-e / s2);
            dx_cos = 0.0f;
            dx_s = d * (-psi / s2 + e * sdf / (s2 * s));
        }
        return psi / s * d;
    }
};
// the cos quad of a step where the model has one
template <bool HAS> struct CosQuad { typedef Quad<float> type; };
template <> struct CosQuad<false> { typedef NoQuad type; };
template <class Q>
__device__ __forceinline__ float cos_elem(const Q &q, int j)
{
    if constexpr (std::is_same<Q, NoQuad>::value) return 0.0f;
    else return q.v[j];
}

template <bool VEC, int MODEL>
struct RenderSdfFwdOp : RenderFwdStage, SampleOut {
    typedef SdfModel<MODEL> M;
    struct Raw { Quad<float> a, b, s; typename CosQuad<M::HAS_COS>::type cs; U4 m; float prm; Rgb12<float> c; };
    const float *ts, *te, *sig /* sdfs */, *cosv, *rgb;
    RawAct act;   // the mask and the colour step
    SdfParam par;
    float rt[SE], ra[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(sig, q, r.s);
        if constexpr (M::HAS_COS) ld4<VEC>(cosv, q, r.cs);
        if (act.mask) load_mask4(act.mask, act.mask_vec != 0, q, r.m);
        r.prm = *par.value;
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        fix_rgb12(rgb, VEC, pos, r.c, c);
        act.colours(c);
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            float u0, u1, u2;
            const float xv = M::template x<false>(r.s.v[j], cos_elem(r.cs, j), r.b.v[j] - r.a.v[j], r.prm, par.ratio, u0, u1, u2);
            xs[j] = (pos.valid[j] && act.live(r.m, j)) ? xv : 0.0f;
            mid[j] = midpoint(r.a.v[j], r.b.v[j]);
        }
    }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        trans_alpha(is_head, prev, xs[j], rt[j], ra[j]);
        rw[j] = rt[j] * ra[j];
    }
    __device__ __forceinline__ void ray_done_b(int rid, int ch, float t) const { ray_store(rid, ch, t); }
    __device__ __forceinline__ void empty_ray(int rid) const { ray_zero(rid); }
    __device__ __forceinline__ void store(const Pos &q) { store_wta<VEC>(q, rw, rt, ra); }
};

template <bool VEC, bool EXTRA, int MODEL>
struct RenderSdfBwdOp : RenderBwdStage<EXTRA> {
    typedef RenderBwdStage<EXTRA> S;
    typedef SdfModel<MODEL> M;
    // NeuS with EXTRA holds one quad and three derivative factors more than RenderRawBwdOp<EXTRA> (141 VGPRs): with the next
    // step's loads in registers as well it is 181 VGPRs, 2 waves per SIMD, and held to the 3-wave budget it spills.  That
    // form fetches in the step itself instead.
    static constexpr bool PIPE = !(M::HAS_COS && EXTRA);
    struct Raw { Quad<float> a, b, T, s; typename CosQuad<M::HAS_COS>::type cs; typename S::GRaw g; U4 m; float prm; Rgb12<float> c; };
    const float *ts, *te, *sig /* sdfs */, *cosv, *rgb, *tr;
    RawAct act;
    SdfParam par;
    float *gsig /* g_sdfs */, *gcos, *gpar, *grgb;
    float d_sdf[SE], d_cos[SE], d_par[SE], rc[SE], rp[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(tr, q, r.T);
        ld4<VEC>(sig, q, r.s);
        if constexpr (M::HAS_COS) ld4<VEC>(cosv, q, r.cs);
        this->template fetch_extra<VEC>(q, r.g);
        if (act.mask) load_mask4(act.mask, act.mask_vec != 0, q, r.m);
        r.prm = *par.value;
        load_rgb12(rgb, VEC, q, r.c);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
        fix_rgb12(rgb, VEC, pos, r.c, S::c);
        act.colours(S::c);
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            // x and alpha as the forward pass formed them
            const bool on = valid[j] && act.live(r.m, j);
            S::sample(j, r.a.v[j], r.b.v[j]);
            float d0, d1, d2;
            const float xv = M::template x<true>(r.s.v[j], cos_elem(r.cs, j), S::dlt[j], r.prm, par.ratio, d0, d1, d2);
            d_sdf[j] = on ? d0 : 0.0f; d_cos[j] = on ? d1 : 0.0f; d_par[j] = on ? d2 : 0.0f;
            S::T[j] = sel(r.T, j, valid, 0.0f); S::A[j] = on ? alpha_of(xv) : 0.0f;
            this->select_extra(r.g, j, valid[j], S::GW[j], S::GT[j], S::GA[j]);
        }
    }
    __device__ __forceinline__ void pre(int j, int64_t pos, bool valid, int rid)
    {
        S::pre(j, pos, valid, rid);
        if (valid && S::gc && act.col == NFA_RGB_ACT_SIGMOID) {   // d sigmoid = c (1 - c)
#pragma unroll
            for (int k = 0; k < 3; ++k) S::gr[3 * j + k] *= S::c[3 * j + k] * (1.0f - S::c[3 * j + k]);
        }
    }
    __device__ __forceinline__ void store_pre(const Pos &pq)
    {
        if (grgb) store_rgb12(grgb, VEC, pq, S::gr);
    }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[1])
    {
        // (selects, not products: where a derivative is 0 -- a masked sample, x = 0 -- the gradient is exactly 0)
        const float gx = S::chain(j, is_head, prev);
        S::rs[j] = d_sdf[j] != 0.0f ? gx * d_sdf[j] : 0.0f;
        if constexpr (M::HAS_COS) rc[j] = d_cos[j] != 0.0f ? gx * d_cos[j] : 0.0f;
        rp[j] = d_par[j] != 0.0f ? gx * d_par[j] : 0.0f;
    }
    __device__ __forceinline__ void store(const Pos &pq)
    {
        if (gsig) store4<VEC>(gsig, pq, S::rs);
        if constexpr (M::HAS_COS) { if (gcos) store4<VEC>(gcos, pq, rc); }
        if (gpar) store4<VEC>(gpar, pq, rp);
    }
};

// ---- Mip-NeRF 360 distortion loss (Barron et al. 2022, eq. 15) over samples in non-decreasing midpoint order per ray:
//      L = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 s_i = sum_k [2 w_k (d_k W<k - S<k) + w_k^2 s_k / 3], with
//      W<k / S<k the exclusive prefix sums of w and w*d, d = m - m(first sample of the ray).  The loss is shift-invariant;
//      the shift keeps d W - S free of cancellation when t is large.  Input out of midpoint order gets
//      what this formula gives (not detected).
// The first midpoint of every ray a tile touches is read at tile start into LDS (a tile owns at most SEG_TILE_ROWS rays;
// more would fall back to gathers), so pre() knows d before stage A.
constexpr int DIST_RAY_CAP = SEG_TILE_ROWS < 256 ? (int)SEG_TILE_ROWS : 256;
__device__ __forceinline__ float dist_mid(float a, float b) { return (a + b) / 2.0f; }
__device__ __forceinline__ float dist_first_mid(const int64_t *packed_info, const float *ts, const float *te, int64_t r)
{
    const longlong2 pr = *reinterpret_cast<const longlong2 *>(packed_info + 2 * r);
    return pr.y > 0 ? dist_mid(ts[pr.x], te[pr.x]) : 0.0f;   // (an empty ray has no element to read)
}

// forward: stage A scans {w, w*d}; stage B totals the per-element term into loss[ray]; TOTALS write W_tot / S_tot
template <bool VEC>
struct DistortionFwdOp : OpBase {
    static constexpr int NCH = 2;
    static constexpr int NCHB = 1;
    static constexpr bool NEEDS_RID = true;
    static constexpr bool TOTALS = true;
    static constexpr int RAY_LDS_FLOATS = DIST_RAY_CAP;   // m_first per ray
    struct Raw { F4 a, b, w; };
    const int64_t *pinfo;
    const float *ts, *te, *w;
    float *loss, *wtot, *stot;
    const float *m_lds = nullptr;
    int32_t g_lo = 0, g_n = 0;
    float ww[SE], mid[SE], sw[SE], d[SE], term[SE];
    __device__ __forceinline__ void tile_begin(int32_t r_lo, int32_t r_hi, float *lds)
    {
        m_lds = lds; g_lo = r_lo; g_n = min(r_hi - r_lo, DIST_RAY_CAP);
        __builtin_amdgcn_wave_barrier();
        for (int32_t i = lane_id(); i < g_n; i += 64) lds[i] = dist_first_mid(pinfo, ts, te, (int64_t)g_lo + i);
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(w, q, r.w);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            ww[j] = sel(r.w, j, valid, 0.0f);
            mid[j] = dist_mid(r.a.v[j], r.b.v[j]);
            sw[j] = valid[j] ? r.b.v[j] - r.a.v[j] : 0.0f;
        }
    }
    __device__ __forceinline__ void pre(int j, int64_t, bool valid, int rid)
    {
        float m0 = 0.0f;
        if (valid) {
            const uint32_t slot = (uint32_t)(rid - g_lo);
            m0 = slot < (uint32_t)g_n ? m_lds[slot] : dist_first_mid(pinfo, ts, te, rid);
        }
        d[j] = valid ? mid[j] - m0 : 0.0f;
    }
    __device__ __forceinline__ void store_pre(const Pos &) const {}
    __device__ __forceinline__ float x(int j, int ch) const { return ch == 0 ? ww[j] : ww[j] * d[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[2])
    {
        const float Wl = is_head ? 0.0f : prev[0], Sl = is_head ? 0.0f : prev[1];
        term[j] = 2.0f * ww[j] * (d[j] * Wl - Sl) + ww[j] * ww[j] * sw[j] * (1.0f / 3.0f);
    }
    __device__ __forceinline__ float xb(int j, int) const { return term[j]; }
    __device__ __forceinline__ void ray_done(int rid, const float t[2]) const { wtot[rid] = t[0]; stot[rid] = t[1]; }
    __device__ __forceinline__ void ray_done_b(int rid, int, float t) const { loss[rid] = t; }
    __device__ __forceinline__ void empty_ray(int rid) const { loss[rid] = 0.0f; wtot[rid] = 0.0f; stot[rid] = 0.0f; }
    __device__ __forceinline__ void store(const Pos &) const {}
};

// backward: one reverse pass scans {w, w*d} into the exclusive suffix sums W>k / S>k; the prefix sums follow from the
// forward's totals (W<k = W_tot - W>k - w_k).  {g[ray], m_first, W_tot, S_tot} are staged in LDS at tile start.
//   dL/dw_k = 2 (d_k (W_tot - 2 W>k) + 2 S>k - S_tot) + 2/3 w_k s_k      (= 2 (A_k + B_k) + 2/3 w_k s_k)
//   dL/dm_k = 2 w_k (W<k - W>k),  dL/ds_k = w_k^2 / 3;  t_start = m - s/2, t_end = m + s/2
template <bool VEC>
struct DistortionBwdOp : OpBase {
    static constexpr int NCH = 2;
    static constexpr bool NEEDS_RID = true;
    static constexpr int RAY_LDS_FLOATS = 4 * DIST_RAY_CAP;   // {g, m_first, W_tot, S_tot} per ray
    struct Raw { F4 a, b, w; };
    const int64_t *pinfo;
    const float *ts, *te, *w, *wtot, *stot, *gl;
    float *gw, *gts, *gte;
    const float *r_lds = nullptr;
    int32_t g_lo = 0, g_n = 0;
    float ww[SE], mid[SE], sw[SE], d[SE], G[SE], WT[SE], ST[SE], rw[SE], rts[SE], rte[SE];
    __device__ __forceinline__ float4 ray_row(int64_t r) const
    {
        return make_float4(gl[r], dist_first_mid(pinfo, ts, te, r), wtot[r], stot[r]);
    }
    __device__ __forceinline__ void tile_begin(int32_t r_lo, int32_t r_hi, float *lds)
    {
        // (the pass runs from the tile's last ray to its first: a tile owning more than DIST_RAY_CAP rays stages the last ones)
        r_lds = lds; g_n = min(r_hi - r_lo, DIST_RAY_CAP); g_lo = r_hi - g_n;
        __builtin_amdgcn_wave_barrier();
        for (int32_t i = lane_id(); i < g_n; i += 64) *reinterpret_cast<float4 *>(lds + 4 * i) = ray_row((int64_t)g_lo + i);
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        ld4<VEC>(w, q, r.w);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
        const bool *valid = pos.valid;
#pragma unroll
        for (int j = 0; j < SE; ++j) {
            ww[j] = sel(r.w, j, valid, 0.0f);
            mid[j] = dist_mid(r.a.v[j], r.b.v[j]);
            sw[j] = valid[j] ? r.b.v[j] - r.a.v[j] : 0.0f;
        }
    }
    __device__ __forceinline__ void pre(int j, int64_t, bool valid, int rid)
    {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) {
            const uint32_t slot = (uint32_t)(rid - g_lo);
            v = slot < (uint32_t)g_n ? *reinterpret_cast<const float4 *>(r_lds + 4 * slot) : ray_row(rid);
        }
        G[j] = v.x; WT[j] = v.z; ST[j] = v.w;
        d[j] = valid ? mid[j] - v.y : 0.0f;
    }
    __device__ __forceinline__ void store_pre(const Pos &) const {}
    __device__ __forceinline__ float x(int j, int ch) const { return ch == 0 ? ww[j] : ww[j] * d[j]; }
    __device__ __forceinline__ void emit(int j, int64_t, bool, bool is_head, int, int, const float *, const float prev[2])
    {
        const float Wg = is_head ? 0.0f : prev[0], Sg = is_head ? 0.0f : prev[1];
        const float g = G[j], wj = ww[j];
        const float ab = d[j] * (WT[j] - 2.0f * Wg) + 2.0f * Sg - ST[j];
        const float gm = g * 2.0f * wj * (WT[j] - 2.0f * Wg - wj);
        const float gs = g * wj * wj * (1.0f / 3.0f);
        rw[j] = g * (2.0f * ab + (2.0f / 3.0f) * wj * sw[j]);
        rts[j] = 0.5f * gm - gs;
        rte[j] = 0.5f * gm + gs;
    }
    __device__ __forceinline__ void store(const Pos &q)
    {
        if (gw) store4<VEC>(gw, q, rw);
        if (gts) store4<VEC>(gts, q, rts);
        if (gte) store4<VEC>(gte, q, rte);
    }
};

// ---- backward of nfa_sample_positions_fwd (samples.h) in one pass: per sample g_p = J^T g_x at the recomputed point
//      (o[r], d[r] are known before the values: NEEDS_RID) and g_t_start = g_t_end = 1/2 d[r] . g_p; per ray the six sums
//      g_o[r] = sum g_p and g_d[r] = sum (m g_p + dscale g_dirs), m = (t_start + t_end) / 2, written by the wave that owns
//      the ray: no atomics (torch's index_add_ has them), the same bits every run, zeros for empty rays.
template <bool VEC, int MODE>
struct SamplePosBwdOp : OpBase {
    static constexpr int NCH = 6;
    static constexpr bool NEEDS_RID = true;
    static constexpr bool TOTALS = true;
    struct Raw { F4 a, b; float gx[3 * SE], gd[3 * SE]; };
    const float *o, *d, *ts, *te, *gx, *gdirs;   // gx / gdirs may be null (no gradient arrived there)
    SampleBox box;
    float dscale;                                // d dirs / d d[r]: 1 ("raw") or 1/2 ("unit")
    float *go, *gd, *gts, *gte;                  // each may be null
    float tsv[SE], tev[SE], gxv[3 * SE], gdv[3 * SE], xv[SE][6], rt[SE];
    __device__ __forceinline__ void fetch(const Pos &q, Raw &r) const
    {
        ld4<VEC>(ts, q, r.a);
        ld4<VEC>(te, q, r.b);
        if (gx) load_rgb12(gx, VEC, q, r.gx);
        if (gdirs) load_rgb12(gdirs, VEC, q, r.gd);
    }
    __device__ __forceinline__ void load(const Raw &r, const Pos &pos)
    {
#pragma unroll
        for (int j = 0; j < SE; ++j) { tsv[j] = r.a.v[j]; tev[j] = r.b.v[j]; }
#pragma unroll
        for (int k = 0; k < 3 * SE; ++k) gxv[k] = gdv[k] = 0.0f;
        if (gx) fix_rgb12(gx, VEC, pos, r.gx, gxv);
        if (gdirs) fix_rgb12(gdirs, VEC, pos, r.gd, gdv);
    }
    __device__ __forceinline__ void pre(int j, int64_t, bool valid, int rid)
    {
        rt[j] = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 6; ++ch) xv[j][ch] = 0.0f;
        if (!valid) return;
        float ro[3], rd[3], p[3] = {0.f, 0.f, 0.f}, g[3] = {gxv[3 * j], gxv[3 * j + 1], gxv[3 * j + 2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) { ro[k] = o[3 * (int64_t)rid + k]; rd[k] = d[3 * (int64_t)rid + k]; }
        if (MODE != SP_NONE) {
            float lo[3], ext[3];
            box_resolve(box, lo, ext);
            if (MODE == SP_SPHERE || MODE == SP_CUBE) sample_point(ro, rd, tsv[j], tev[j], p);
            sample_grad_point<MODE>(p, lo, ext, g);
        }
        const float m = (tsv[j] + tev[j]) / 2.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            xv[j][k] = g[k];
            xv[j][3 + k] = m * g[k] + dscale * gdv[3 * j + k];
        }
        rt[j] = 0.5f * (rd[0] * g[0] + rd[1] * g[1] + rd[2] * g[2]);
    }
    __device__ __forceinline__ void store_pre(const Pos &) const {}
    __device__ __forceinline__ float x(int j, int ch) const { return xv[j][ch]; }
    __device__ __forceinline__ void emit(int, int64_t, bool, bool, int, int, const float *, const float *) const {}
    __device__ __forceinline__ void store(const Pos &q)
    {
        if (gts) store4<VEC>(gts, q, rt);
        if (gte) store4<VEC>(gte, q, rt);
    }
    __device__ __forceinline__ void put(int rid, const float *t) const
    {
        if (go) { go[3 * (int64_t)rid] = t[0]; go[3 * (int64_t)rid + 1] = t[1]; go[3 * (int64_t)rid + 2] = t[2]; }
        if (gd) { gd[3 * (int64_t)rid] = t[3]; gd[3 * (int64_t)rid + 1] = t[4]; gd[3 * (int64_t)rid + 2] = t[5]; }
    }
    __device__ __forceinline__ void ray_done(int rid, const float t[6]) const { put(rid, t); }
    __device__ __forceinline__ void empty_ray(int rid) const
    {
        const float z[6] = {0, 0, 0, 0, 0, 0};
        put(rid, z);
    }
};

// ------------------------------------------------------------------------------------------
// Generic fallback: arbitrary (start, count) chunks, one wave per ray (semantics of
// include/utils_scan.cuh incl. `normalize`).
template <bool EXCL, bool PROD>
__global__ __launch_bounds__(256) void generic_scan_kernel(const int64_t *__restrict__ packed_info, int64_t n_rays,
                                                           const float *__restrict__ in, float *__restrict__ out,
                                                           int reverse, int normalize)
{
    const int lane = lane_id();
    const float init = PROD ? 1.0f : 0.0f;
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rays;
         r += ((int64_t)blockDim.x * gridDim.x) >> 6) {
        const int64_t s = packed_info[2 * r], n = packed_info[2 * r + 1];
        if (n <= 0) continue;
        float den = 1.0f;
        if (normalize) {  // utils_scan.cuh:102-110 / :229-237: divide by the row's inclusive total
            float tot = init;
            for (int64_t k = lane; k < n; k += 64) tot = PROD ? tot * in[s + k] : tot + in[s + k];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float u = __shfl_xor(tot, off, 64);
                tot = PROD ? tot * u : tot + u;
            }
            den = fmaxf(tot, 1e-10f);
        }
        float carry = init;
        for (int64_t c = 0; c < n; c += 64) {
            const int64_t k = c + lane;
            const int64_t pos = reverse ? s + n - 1 - k : s + k;
            float v = k < n ? in[pos] : init;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float u = __shfl_up(v, off, 64);
                if (lane >= off) v = PROD ? u * v : u + v;
            }
            v = PROD ? carry * v : carry + v;
            float prevv = __shfl_up(v, 1, 64);
            if (lane == 0) prevv = carry;
            if (k < n) {
                float o = EXCL ? prevv : v;
                if (normalize && !(EXCL && k == 0)) o /= den;
                out[pos] = o;
            }
            carry = __shfl(v, 63, 64);
        }
    }
}

__global__ __launch_bounds__(256) void accumulate_atomic_kernel(const float *__restrict__ w, const float *__restrict__ vals,
                                                                int32_t D, const int64_t *__restrict__ ri, int64_t n_rays,
                                                                int64_t n, float *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * D; i += (int64_t)blockDim.x * gridDim.x) {
        const int64_t e = i / D;
        const int32_t ch = (int32_t)(i - e * D);
        const int64_t r = ri[e];
        if (r < 0 || r >= n_rays) continue;
        const float v = vals ? w[e] * vals[i] : w[e];
        atomicAdd(out + r * D + ch, v);
    }
}

}  // namespace nfa

using namespace nfa;

#define SEG_COMMON_CHECKS(name)                                                                         \
    NFA_REQUIRE(n_rays >= 0 && n_elems >= 0, name ": negative size");                                   \
    NFA_REQUIRE(n_rays < ((int64_t)1 << 31) - 64, name ": too many rays");                              \
    if (n_elems == 0 && n_rays == 0) return NFA_OK;                                                      \
    NFA_REQUIRE(packed_info && tiles && n_tiles >= 1, name ": packed_info/tiles is null")

// A half stream takes the vector form when its quads are 8-byte aligned
static inline bool aligned_quads(const float *p) { return aligned16(p); }
static inline bool aligned_quads(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// The one-pass rendering ops, RenderFused*Op and RenderRaw*Op<E>, share most of their streams.  One launch helper per
// direction tests the alignment (own_aligned: that of the streams only the caller's op has), picks the op's compile-time
// form -- make(V) / make(V, X) returns the op with its own members filled -- fills the shared members and launches.
template <class E, class Make>
static int launch_render_fwd(const char *name, Make &&make, bool own_aligned, const float *t_starts, const float *t_ends, const E *sigmas,
                             const E *rgbs, float *weights, float *trans, float *alphas, float *colors, float *opacities,
                             float *depths, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                             nfa_stream_t stream)
{
    const bool vec = own_aligned && all_aligned16(t_starts, t_ends, weights, trans, alphas) && aligned_quads(sigmas) && aligned_quads(rgbs);
    dispatch_bool(vec, [&](auto V) {
        auto op = make(V);
        op.ts = t_starts; op.te = t_ends; op.sig = sigmas; op.rgb = rgbs; op.w = weights; op.tr = trans; op.al = alphas;
        op.colors = colors; op.opac = opacities; op.depth = depths;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, as_stream(stream));
    });
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

template <class E, class Make>
static int launch_render_bwd(const char *name, Make &&make, bool own_aligned, const float *t_starts, const float *t_ends, const E *rgbs,
                             const float *trans, const float *g_colors, const float *g_opacities, const float *g_depths,
                             const float *g_weights, const float *g_trans, const float *g_alphas, E *grad_sigmas, E *grad_rgbs,
                             const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, nfa_stream_t stream)
{
    const bool vec = own_aligned && all_aligned16(t_starts, t_ends, trans, g_weights, g_trans, g_alphas) && aligned_quads(rgbs) &&
                     aligned_quads(grad_sigmas) && aligned_quads(grad_rgbs);
    const bool extra = g_weights || g_trans || g_alphas;
    dispatch_bool(vec, [&](auto V) {
        dispatch_bool(extra, [&](auto X) {
            auto op = make(V, X);
            op.ts = t_starts; op.te = t_ends; op.rgb = rgbs; op.tr = trans;
            op.gc = g_colors; op.go = g_opacities; op.gd = g_depths; op.gw = g_weights; op.gt = g_trans; op.ga = g_alphas;
            op.gsig = grad_sigmas; op.grgb = grad_rgbs;
            launch_seg<-1>(op, packed_info, tiles, n_rays, n_tiles, as_stream(stream));
        });
    });
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

extern "C" {

void nfa_seg_plan(int64_t n_elems, int64_t n_rays, int64_t *tile_elems, int64_t *n_tiles)
{
    // One wave per tile.  Measured on MI355X (scripts/sweep_seg.sh, 32 M samples): 1024-element tiles
    // (4 steps per wave, ~120 waves per CU) are fastest; longer tiles lose to the tail of the last
    // wave round, shorter ones to the per-tile prologue.  A tile also ends after SEG_TILE_ROWS rays.
    const int64_t t_env = tuning_env("NFA_SEG_TILE") ? atoll(tuning_env("NFA_SEG_TILE")) : 0;  // tuning knob (multiple of 4), read once
    const int64_t t = t_env > 0 ? t_env : 1024;
    *tile_elems = t;
    *n_tiles = n_elems / t + (n_rays > 0 ? n_rays : 0) / SEG_TILE_ROWS + 1;
}

int64_t nfa_seg_table_rows(int64_t n_tiles) { return seg_table_rows(n_tiles); }

int nfa_seg_build_tiles(const int64_t *packed_info, int64_t n_rays, int64_t n_elems, int64_t tile_elems, int64_t n_tiles,
                        int64_t *tiles, int32_t *flags, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rays >= 0 && n_elems >= 0 && tiles, "seg_build_tiles: bad arguments");
    NFA_REQUIRE(n_rays == 0 || packed_info, "seg_build_tiles: packed_info is null");
    NFA_REQUIRE(n_rays < ((int64_t)1 << 31) - 64, "seg_build_tiles: too many rays");
    NFA_REQUIRE(tile_elems >= 64 && tile_elems % 4 == 0 && n_tiles == n_elems / tile_elems + n_rays / SEG_TILE_ROWS + 1,
                "seg_build_tiles: tile_elems must be a multiple of 4 (>= 64) and n_tiles what nfa_seg_plan returns for (n_elems, n_rays)");
    hipStream_t s = as_stream(stream);
    if (flags && hipMemsetAsync(flags, 0, sizeof(int32_t), s) != hipSuccess) { set_error("seg_build_tiles: memset failed"); return NFA_EHIP; }
    hipLaunchKernelGGL(seg_build_tiles_kernel, dim3(grid_1d(n_rays + 1, 256)), dim3(256), 0, s, packed_info, n_rays,
                       n_elems, tile_elems, n_tiles, reinterpret_cast<longlong2 *>(tiles), flags);
    NFA_CHECK_LAUNCH("seg_build_tiles");
    return NFA_OK;
}

int nfa_packed_scan(int kind, int reverse, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                    int64_t n_elems, const float *inputs, float *outputs, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("packed_scan");
    NFA_REQUIRE(kind >= 0 && kind <= 3, "packed_scan: kind must be 0..3");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(inputs && outputs, "packed_scan: null data pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(inputs, outputs);
    dispatch_bool(kind & 1, [&](auto EX) {
        dispatch_bool(kind >= 2, [&](auto PR) {
            dispatch_bool(vec, [&](auto V) {
                ScanOp<EX, PR, V> op;
                op.in = inputs; op.out = outputs;
                dispatch_bool(reverse != 0, [&](auto REV) { launch_seg<REV ? -1 : 1>(op, packed_info, tiles, n_rays, n_tiles, s); });
            });
        });
    });
    NFA_CHECK_LAUNCH("packed_scan");
    return NFA_OK;
}

int nfa_packed_scan_generic(int kind, int reverse, int normalize, const int64_t *packed_info, int64_t n_rays,
                            int64_t n_elems, const float *inputs, float *outputs, nfa_stream_t stream)
{
    NFA_REQUIRE(kind >= 0 && kind <= 3 && n_rays >= 0 && n_elems >= 0, "packed_scan_generic: bad arguments");
    if (n_elems == 0 || n_rays == 0) return NFA_OK;
    NFA_REQUIRE(packed_info && inputs && outputs, "packed_scan_generic: null pointer");
    hipStream_t s = as_stream(stream);
    const unsigned grid = grid_1d(n_rays * 64, 256, 1 << 16);
    dispatch_bool(kind & 1, [&](auto EX) {
        dispatch_bool(kind >= 2, [&](auto PR) {
            hipLaunchKernelGGL((generic_scan_kernel<EX, PR>), dim3(grid), dim3(256), 0, s, packed_info, n_rays, inputs, outputs, reverse, normalize);
        });
    });
    NFA_CHECK_LAUNCH("packed_scan_generic");
    return NFA_OK;
}

int nfa_packed_prod_backward(int kind, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                             int64_t n_elems, const float *inputs, const float *outputs, const float *grad_outputs,
                             float *grad_inputs, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("packed_prod_backward");
    NFA_REQUIRE(kind == 2 || kind == 3, "packed_prod_backward: kind must be 2 or 3");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(inputs && outputs && grad_outputs && grad_inputs, "packed_prod_backward: null data pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(inputs, outputs, grad_outputs, grad_inputs);
    dispatch_bool(kind == 3, [&](auto EX) {
        dispatch_bool(vec, [&](auto V) {
            ProdBwdOp<EX, V> op;
            op.in = inputs; op.outv = outputs; op.g = grad_outputs; op.gin = grad_inputs;
            launch_seg<-1>(op, packed_info, tiles, n_rays, n_tiles, s);
        });
    });
    NFA_CHECK_LAUNCH("packed_prod_backward");
    return NFA_OK;
}

int nfa_render_from_density_fwd(const float *t_starts, const float *t_ends, const float *sigmas,
                                const float *prefix_trans, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                                int64_t n_rays, int64_t n_elems, float *weights, float *trans, float *alphas,
                                nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_from_density_fwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && sigmas, "render_from_density_fwd: null input");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(t_starts, t_ends, sigmas, prefix_trans, weights, trans, alphas);
    dispatch_bool(vec, [&](auto V) {
        DensityFwdOp<V> op;
        op.ts = t_starts; op.te = t_ends; op.sig = sigmas; op.prefix = prefix_trans;
        op.w = weights; op.tr = trans; op.al = alphas;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_from_density_fwd");
    return NFA_OK;
}

int nfa_render_from_alpha_fwd(const float *alphas, const float *prefix_trans, const int64_t *packed_info,
                              const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *weights, float *trans,
                              nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_from_alpha_fwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(alphas, "render_from_alpha_fwd: null input");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(alphas, prefix_trans, weights, trans);
    dispatch_bool(vec, [&](auto V) {
        AlphaFwdOp<V> op;
        op.al = alphas; op.prefix = prefix_trans; op.w = weights; op.tr = trans;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_from_alpha_fwd");
    return NFA_OK;
}

int nfa_render_from_density_bwd(const float *t_starts, const float *t_ends, const float *trans, const float *alphas,
                                const float *g_weights, const float *g_trans, const float *g_alphas,
                                const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                                float *grad_sigmas, float *grad_x, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_from_density_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && trans && alphas && (grad_sigmas || grad_x), "render_from_density_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(t_starts, t_ends, trans, alphas, g_weights, g_trans, g_alphas, grad_sigmas, grad_x);
    dispatch_bool(vec, [&](auto V) {
        DensityBwdOp<V> op;
        op.ts = t_starts; op.te = t_ends; op.tr = trans; op.al = alphas;
        op.gw = g_weights; op.gt = g_trans; op.ga = g_alphas; op.gsig = grad_sigmas; op.gx = grad_x;
        launch_seg<-1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_from_density_bwd");
    return NFA_OK;
}

int nfa_density_cdf_rows_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *packed_info,
                             const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, int32_t row_len,
                             float *trans, float *alphas, float *cdfs, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("density_cdf_rows_fwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && sigmas && cdfs, "density_cdf_rows_fwd: null pointer");
    NFA_REQUIRE(row_len >= 1 && n_rays * (int64_t)row_len == n_elems, "density_cdf_rows_fwd: n_elems must be n_rays * row_len");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(t_starts, t_ends, sigmas, trans, alphas);
    dispatch_bool(vec, [&](auto V) {
        DensityFwdOp<V> op;
        op.ts = t_starts; op.te = t_ends; op.sig = sigmas; op.prefix = nullptr;
        op.w = nullptr; op.tr = trans; op.al = alphas; op.cdf = cdfs; op.row_len = row_len;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("density_cdf_rows_fwd");
    return NFA_OK;
}

int nfa_density_cdf_rows_bwd(const float *t_starts, const float *t_ends, const float *trans, const float *alphas,
                             const float *g_cdfs, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                             int64_t n_rays, int64_t n_elems, int32_t row_len, float *grad_sigmas, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("density_cdf_rows_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && trans && g_cdfs && grad_sigmas, "density_cdf_rows_bwd: null pointer");
    (void)alphas;  // not needed: only the transmittance carries a gradient
    NFA_REQUIRE(row_len >= 1 && n_rays * (int64_t)row_len == n_elems, "density_cdf_rows_bwd: n_elems must be n_rays * row_len");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(t_starts, t_ends, trans, alphas, grad_sigmas);
    dispatch_bool(vec, [&](auto V) {
        DensityBwdOp<V, true> op;
        op.ts = t_starts; op.te = t_ends; op.tr = trans; op.al = alphas;
        op.gw = nullptr; op.gt = nullptr; op.ga = nullptr; op.gcdf = g_cdfs; op.gsig = grad_sigmas; op.gx = nullptr;
        launch_seg<-1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("density_cdf_rows_bwd");
    return NFA_OK;
}

int nfa_render_from_alpha_bwd(const float *alphas, const float *trans, const float *g_weights, const float *g_trans,
                              const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                              float *grad_alphas, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_from_alpha_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(alphas && trans && grad_alphas, "render_from_alpha_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(alphas, trans, g_weights, g_trans, grad_alphas);
    dispatch_bool(vec, [&](auto V) {
        AlphaBwdOp<V> op;
        op.al = alphas; op.tr = trans; op.gw = g_weights; op.gt = g_trans; op.galpha = grad_alphas;
        launch_seg<-1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_from_alpha_bwd");
    return NFA_OK;
}

// VisibilityOp's band [s_lo, s_hi] around S = -ln(eps), where exp(-S) crosses eps; expf is good to a couple of ulps, the band
// is +-2e-5 relative (~20 ulps).  That reasoning needs a normal eps: below 2^-126 expf's result moves in steps of 2^-149, up
// to a seventh of eps itself, so it rounds up to eps for sums as far as 0.07 beyond -ln(eps) -- no band of a few ulps covers
// that, and the band is everything: expf is evaluated at every sample.
static void visibility_band(float early_stop_eps, float &s_lo, float &s_hi)
{
    if (early_stop_eps >= 0x1p-126f) {
        const double L = -log((double)early_stop_eps);
        const double w = 2e-5 * (L > 1.0 ? L : 1.0);
        s_lo = (float)(L - w); s_hi = (float)(L + w);
    } else if (early_stop_eps > 0.0f) {
        s_lo = -INFINITY; s_hi = INFINITY;
    } else {   // every transmittance >= eps (exp(-S) is never negative; a NaN sum stays invisible as before)
        s_lo = INFINITY; s_hi = INFINITY;
    }
}

int nfa_render_visibility(const float *t_starts, const float *t_ends, const float *sigmas_or_alphas,
                          const float *prefix_trans, float early_stop_eps, float alpha_thre,
                          const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                          uint8_t *vis, int64_t *vis_cnts, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_visibility");
    hipStream_t s = as_stream(stream);
    if (n_elems > 0) {
        NFA_REQUIRE(sigmas_or_alphas && vis, "render_visibility: null pointer");
        const bool density = t_starts != nullptr;
        NFA_REQUIRE(!density || t_ends, "render_visibility: t_ends is null");
        float s_lo, s_hi;
        visibility_band(early_stop_eps, s_lo, s_hi);
        // the uchar4 mask store needs 4-byte alignment of vis, the float loads 16
        const bool vec = all_aligned16(t_starts, t_ends, sigmas_or_alphas, prefix_trans) &&
                         (reinterpret_cast<uintptr_t>(vis) & 3) == 0;
        dispatch_bool(density, [&](auto DN) {
            dispatch_bool(vec, [&](auto V) {
                dispatch_bool(vis_cnts != nullptr, [&](auto CN) {
                    VisibilityOp<DN, V, CN> op;
                    op.ts = t_starts; op.te = t_ends; op.val = sigmas_or_alphas; op.prefix = prefix_trans;
                    op.eps = early_stop_eps; op.thre = alpha_thre; op.vis = vis; op.cnts = vis_cnts; op.s_lo = s_lo; op.s_hi = s_hi;
                    launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
                });
            });
        });
    } else if (vis_cnts && n_rays > 0) {
        if (hipMemsetAsync(vis_cnts, 0, sizeof(int64_t) * n_rays, s) != hipSuccess) { set_error("render_visibility: memset failed"); return NFA_EHIP; }
    }
    NFA_CHECK_LAUNCH("render_visibility");
    return NFA_OK;
}

// The constant-step (_cs) entries: their siblings with `t_ends` replaced by the step the samples were marched with
// (ConstStep above); densities only.
#define SEG_STEP_CHECK(name) NFA_REQUIRE(step > 0.0f && step < INFINITY, name ": step must be > 0")

int nfa_render_visibility_cs(const float *t_starts, float step, const float *sigmas, const float *prefix_trans,
                             float early_stop_eps, float alpha_thre, const int64_t *packed_info, const int64_t *tiles,
                             int64_t n_tiles, int64_t n_rays, int64_t n_elems, uint8_t *vis, int64_t *vis_cnts, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_visibility_cs");
    SEG_STEP_CHECK("render_visibility_cs");
    hipStream_t s = as_stream(stream);
    if (n_elems > 0) {
        NFA_REQUIRE(t_starts && sigmas && vis, "render_visibility_cs: null pointer");
        float s_lo, s_hi;
        visibility_band(early_stop_eps, s_lo, s_hi);
        const bool vec = all_aligned16(t_starts, sigmas, prefix_trans) && (reinterpret_cast<uintptr_t>(vis) & 3) == 0;
        dispatch_bool(vec, [&](auto V) {
            dispatch_bool(vis_cnts != nullptr, [&](auto CN) {
                VisibilityOp<true, V, CN, true> op;
                op.ts = t_starts; op.te = nullptr; op.step = step; op.val = sigmas; op.prefix = prefix_trans;
                op.eps = early_stop_eps; op.thre = alpha_thre; op.vis = vis; op.cnts = vis_cnts; op.s_lo = s_lo; op.s_hi = s_hi;
                launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
            });
        });
    } else if (vis_cnts && n_rays > 0) {
        if (hipMemsetAsync(vis_cnts, 0, sizeof(int64_t) * n_rays, s) != hipSuccess) { set_error("render_visibility_cs: memset failed"); return NFA_EHIP; }
    }
    NFA_CHECK_LAUNCH("render_visibility_cs");
    return NFA_OK;
}

int nfa_compact_samples(const uint8_t *vis, const float *t_starts, const float *t_ends, const int64_t *packed_info,
                        const int64_t *tiles, int64_t n_tiles, const int64_t *out_starts, int64_t n_rays, int64_t n_elems,
                        int64_t *out_ray_indices, float *out_t_starts, float *out_t_ends, int64_t capacity, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("compact_samples");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(vis && t_starts && t_ends && out_starts, "compact_samples: null input");
    NFA_REQUIRE(capacity >= 0, "compact_samples: negative capacity");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(t_starts, t_ends);
    dispatch_bool(vec, [&](auto V) {
        CompactOp<V> op;
        op.vis = vis; op.vis_vec = (reinterpret_cast<uintptr_t>(vis) & 3) == 0; op.ts = t_starts; op.te = t_ends;
        op.out_starts = out_starts; op.o_ri = out_ray_indices; op.o_ts = out_t_starts; op.o_te = out_t_ends; op.cap = capacity;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("compact_samples");
    return NFA_OK;
}

int nfa_accumulate_along_rays(const float *weights, const float *values, int32_t D, const int64_t *packed_info,
                              const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, int accumulate, float *out,
                              nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("accumulate_along_rays");
    NFA_REQUIRE(D >= 1 && (values || D == 1), "accumulate_along_rays: bad D");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(out && (n_elems == 0 || weights), "accumulate_along_rays: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(weights);
    for (int32_t d0 = 0; d0 < D;) {
        const int32_t c = (D - d0 >= 4) ? 4 : (D - d0);
        dispatch_channels(c, [&](auto C) {
            dispatch_bool(vec, [&](auto V) {
                AccumOp<C, V> op;
                op.w = weights; op.vals = values; op.D = D; op.d0 = d0; op.out = out; op.accumulate = accumulate;
                launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
            });
        });
        d0 += c;
    }
    NFA_CHECK_LAUNCH("accumulate_along_rays");
    return NFA_OK;
}

int nfa_accumulate_along_rays_atomic(const float *weights, const float *values, int32_t D, const int64_t *ray_indices,
                                     int64_t n_rays, int64_t n_elems, float *out, nfa_stream_t stream)
{
    NFA_REQUIRE(D >= 1 && (values || D == 1) && n_rays >= 0 && n_elems >= 0, "accumulate_along_rays_atomic: bad arguments");
    if (n_elems == 0 || n_rays == 0) return NFA_OK;
    NFA_REQUIRE(weights && ray_indices && out, "accumulate_along_rays_atomic: null pointer");
    hipLaunchKernelGGL(accumulate_atomic_kernel, dim3(grid_1d(n_elems * D, 256)), dim3(256), 0, as_stream(stream), weights,
                       values, D, ray_indices, n_rays, n_elems, out);
    NFA_CHECK_LAUNCH("accumulate_along_rays_atomic");
    return NFA_OK;
}

int nfa_accumulate_along_rays_bwd(const float *weights, const float *values, int32_t D, const float *g_out,
                                  const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                                  float *g_weights, float *g_values, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("accumulate_along_rays_bwd");
    NFA_REQUIRE(D >= 1 && (values || D == 1), "accumulate_along_rays_bwd: bad D");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(weights && g_out && (g_weights || g_values), "accumulate_along_rays_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(weights, g_weights);
    for (int32_t d0 = 0; d0 < D;) {
        const int32_t c = (D - d0 >= 4) ? 4 : (D - d0);
        dispatch_channels(c, [&](auto C) {
            dispatch_bool(vec, [&](auto V) {
                AccumBwdOp<C, V> op;
                op.w = weights; op.vals = values; op.gout = g_out; op.D = D; op.d0 = d0;
                op.first = (d0 == 0); op.gw = g_weights; op.gv = g_values;
                launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
            });
        });
        d0 += c;
    }
    NFA_CHECK_LAUNCH("accumulate_along_rays_bwd");
    return NFA_OK;
}

int nfa_render_accumulate_fwd(const float *weights, const float *rgbs, const float *t_starts, const float *t_ends,
                              const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                              float *colors, float *opacities, float *depths, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_accumulate_fwd");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(colors && opacities && depths && (n_elems == 0 || (weights && rgbs && t_starts && t_ends)),
                "render_accumulate_fwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(weights, rgbs, t_starts, t_ends);
    dispatch_bool(vec, [&](auto V) {
        RenderAccumOp<V> op;
        op.w = weights; op.rgb = rgbs; op.ts = t_starts; op.te = t_ends;
        op.colors = colors; op.opac = opacities; op.depth = depths;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_accumulate_fwd");
    return NFA_OK;
}

int nfa_render_accumulate_bwd(const float *weights, const float *rgbs, const float *t_starts, const float *t_ends,
                              const float *g_colors, const float *g_opacities, const float *g_depths,
                              const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                              float *g_weights, float *g_rgbs, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_accumulate_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(weights && rgbs && t_starts && t_ends && (g_weights || g_rgbs), "render_accumulate_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(weights, rgbs, t_starts, t_ends, g_weights, g_rgbs);
    dispatch_bool(vec, [&](auto V) {
        RenderAccumBwdOp<V> op;
        op.w = weights; op.rgb = rgbs; op.ts = t_starts; op.te = t_ends;
        op.gc = g_colors; op.go = g_opacities; op.gd = g_depths; op.gw = g_weights; op.grgb = g_rgbs;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_accumulate_bwd");
    return NFA_OK;
}

int nfa_render_fused_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgbs,
                         const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                         float *weights, float *trans, float *alphas, float *colors, float *opacities, float *depths,
                         nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_fused_fwd");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(colors && opacities && depths && (n_elems == 0 || (t_starts && t_ends && sigmas && rgbs)),
                "render_fused_fwd: null pointer");
    return launch_render_fwd("render_fused_fwd", [](auto V) { return RenderFusedFwdOp<V>(); }, true, t_starts, t_ends, sigmas, rgbs,
                             weights, trans, alphas, colors, opacities, depths, packed_info, tiles, n_tiles, n_rays, stream);
}

int nfa_render_fused_bwd(const float *t_starts, const float *t_ends, const float *rgbs, const float *trans, const float *alphas,
                         const float *g_colors, const float *g_opacities, const float *g_depths, const float *g_weights,
                         const float *g_trans, const float *g_alphas, const int64_t *packed_info, const int64_t *tiles,
                         int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *grad_sigmas, float *grad_rgbs,
                         nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_fused_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && rgbs && trans && alphas && (grad_sigmas || grad_rgbs), "render_fused_bwd: null pointer");
    return launch_render_bwd("render_fused_bwd", [&](auto V, auto X) { RenderFusedBwdOp<V, X> op; op.al = alphas; return op; },
                             aligned16(alphas), t_starts, t_ends, rgbs, trans, g_colors, g_opacities, g_depths, g_weights, g_trans,
                             g_alphas, grad_sigmas, grad_rgbs, packed_info, tiles, n_tiles, n_rays, stream);
}

int nfa_render_fused_fwd_cs(const float *t_starts, float step, const float *sigmas, const float *rgbs,
                            const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                            float *weights, float *trans, float *alphas, float *colors, float *opacities, float *depths,
                            nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_fused_fwd_cs");
    SEG_STEP_CHECK("render_fused_fwd_cs");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(colors && opacities && depths && (n_elems == 0 || (t_starts && sigmas && rgbs)), "render_fused_fwd_cs: null pointer");
    return launch_render_fwd("render_fused_fwd_cs", [&](auto V) { RenderFusedFwdOp<V, true> op; op.step = step; return op; }, true,
                             t_starts, nullptr, sigmas, rgbs, weights, trans, alphas, colors, opacities, depths, packed_info, tiles,
                             n_tiles, n_rays, stream);
}

int nfa_render_fused_bwd_cs(const float *t_starts, float step, const float *rgbs, const float *trans, const float *alphas,
                            const float *g_colors, const float *g_opacities, const float *g_depths, const float *g_weights,
                            const float *g_trans, const float *g_alphas, const int64_t *packed_info, const int64_t *tiles,
                            int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *grad_sigmas, float *grad_rgbs,
                            nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_fused_bwd_cs");
    SEG_STEP_CHECK("render_fused_bwd_cs");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && rgbs && trans && alphas && (grad_sigmas || grad_rgbs), "render_fused_bwd_cs: null pointer");
    return launch_render_bwd("render_fused_bwd_cs",
                             [&](auto V, auto X) { RenderFusedBwdOp<V, X, true> op; op.al = alphas; op.step = step; return op; },
                             aligned16(alphas), t_starts, nullptr, rgbs, trans, g_colors, g_opacities, g_depths, g_weights, g_trans,
                             g_alphas, grad_sigmas, grad_rgbs, packed_info, tiles, n_tiles, n_rays, stream);
}

static RawAct raw_act(const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act)
{
    RawAct a;
    a.mask = selector; a.mask_vec = (reinterpret_cast<uintptr_t>(selector) & 3) == 0;
    a.dens = density_act; a.col = rgb_act; a.bias = density_bias;
    return a;
}
#define RAW_ACT_CHECKS(name)                                                                                     \
    NFA_REQUIRE(density_act >= NFA_ACT_NONE && density_act <= NFA_ACT_SOFTPLUS,                                  \
                name ": density_act must be in 0..4 (got %d)", (int)density_act);                                \
    NFA_REQUIRE(rgb_act == NFA_RGB_ACT_NONE || rgb_act == NFA_RGB_ACT_SIGMOID, name ": rgb_act must be 0 or 1 (got %d)", (int)rgb_act)

extern "C++" {   // one implementation per element type

template <class E>
static int render_raw_fwd(const float *t_starts, const float *t_ends, const E *raw_sigmas, const E *raw_rgbs,
                          const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act,
                          const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                          float *weights, float *trans, float *alphas, E *act_sigmas, E *act_rgbs, float *colors,
                          float *opacities, float *depths, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_raw_fwd");
    RAW_ACT_CHECKS("render_raw_fwd");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(colors && opacities && depths && (n_elems == 0 || (t_starts && t_ends && raw_sigmas && raw_rgbs)),
                "render_raw_fwd: null pointer");
    const RawAct act = raw_act(selector, density_act, density_bias, rgb_act);
    auto make = [&](auto V) { RenderRawFwdOp<V, E> op; op.act = act; op.asig = act_sigmas; op.argb = act_rgbs; return op; };
    return launch_render_fwd("render_raw_fwd", make, aligned_quads(act_sigmas) && aligned_quads(act_rgbs), t_starts, t_ends, raw_sigmas,
                             raw_rgbs, weights, trans, alphas, colors, opacities, depths, packed_info, tiles, n_tiles, n_rays, stream);
}

template <class E>
static int render_raw_bwd(const float *t_starts, const float *t_ends, const E *raw_sigmas, const E *raw_rgbs,
                          const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act, const float *trans,
                          const float *g_colors, const float *g_opacities, const float *g_depths, const float *g_weights,
                          const float *g_trans, const float *g_alphas, const int64_t *packed_info, const int64_t *tiles,
                          int64_t n_tiles, int64_t n_rays, int64_t n_elems, E *grad_raw_sigmas, E *grad_raw_rgbs,
                          nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_raw_bwd");
    RAW_ACT_CHECKS("render_raw_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && raw_sigmas && raw_rgbs && trans && (grad_raw_sigmas || grad_raw_rgbs),
                "render_raw_bwd: null pointer");
    const RawAct act = raw_act(selector, density_act, density_bias, rgb_act);
    auto make = [&](auto V, auto X) { RenderRawBwdOp<V, X, E> op; op.sig = raw_sigmas; op.act = act; return op; };
    return launch_render_bwd("render_raw_bwd", make, aligned_quads(raw_sigmas), t_starts, t_ends, raw_rgbs, trans, g_colors, g_opacities,
                             g_depths, g_weights, g_trans, g_alphas, grad_raw_sigmas, grad_raw_rgbs, packed_info, tiles, n_tiles, n_rays,
                             stream);
}

}  // extern "C++"

#define RAW_ELEM_DISPATCH(name, call)                                                                                  \
    int rc = NFA_OK;                                                                                                   \
    if (!dispatch_elem(elem, [&](auto tag) { using E = typename decltype(tag)::type; rc = call; }))                     \
        NFA_REQUIRE(false, name ": elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", (int)elem);      \
    return rc

int nfa_render_raw_fwd_t(int32_t elem, const float *t_starts, const float *t_ends, const void *raw_sigmas,
                         const void *raw_rgbs, const uint8_t *selector, int32_t density_act, float density_bias,
                         int32_t rgb_act, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                         int64_t n_rays, int64_t n_elems, float *weights, float *trans, float *alphas, void *act_sigmas,
                         void *act_rgbs, float *colors, float *opacities, float *depths, nfa_stream_t stream)
{
    RAW_ELEM_DISPATCH("render_raw_fwd", render_raw_fwd(
        t_starts, t_ends, static_cast<const E *>(raw_sigmas), static_cast<const E *>(raw_rgbs), selector, density_act,
        density_bias, rgb_act, packed_info, tiles, n_tiles, n_rays, n_elems, weights, trans, alphas,
        static_cast<E *>(act_sigmas), static_cast<E *>(act_rgbs), colors, opacities, depths, stream));
}

int nfa_render_raw_fwd(const float *t_starts, const float *t_ends, const float *raw_sigmas, const float *raw_rgbs,
                       const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act,
                       const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                       float *weights, float *trans, float *alphas, float *act_sigmas, float *act_rgbs, float *colors,
                       float *opacities, float *depths, nfa_stream_t stream)
{
    return nfa_render_raw_fwd_t(NFA_ELEM_F32, t_starts, t_ends, raw_sigmas, raw_rgbs, selector, density_act, density_bias,
                                rgb_act, packed_info, tiles, n_tiles, n_rays, n_elems, weights, trans, alphas, act_sigmas,
                                act_rgbs, colors, opacities, depths, stream);
}

int nfa_render_raw_bwd_t(int32_t elem, const float *t_starts, const float *t_ends, const void *raw_sigmas,
                         const void *raw_rgbs, const uint8_t *selector, int32_t density_act, float density_bias,
                         int32_t rgb_act, const float *trans, const float *g_colors, const float *g_opacities,
                         const float *g_depths, const float *g_weights, const float *g_trans, const float *g_alphas,
                         const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                         int64_t n_elems, void *grad_raw_sigmas, void *grad_raw_rgbs, nfa_stream_t stream)
{
    RAW_ELEM_DISPATCH("render_raw_bwd", render_raw_bwd(
        t_starts, t_ends, static_cast<const E *>(raw_sigmas), static_cast<const E *>(raw_rgbs), selector, density_act,
        density_bias, rgb_act, trans, g_colors, g_opacities, g_depths, g_weights, g_trans, g_alphas, packed_info, tiles,
        n_tiles, n_rays, n_elems, static_cast<E *>(grad_raw_sigmas), static_cast<E *>(grad_raw_rgbs), stream));
}

int nfa_render_raw_bwd(const float *t_starts, const float *t_ends, const float *raw_sigmas, const float *raw_rgbs,
                       const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act, const float *trans,
                       const float *g_colors, const float *g_opacities, const float *g_depths, const float *g_weights,
                       const float *g_trans, const float *g_alphas, const int64_t *packed_info, const int64_t *tiles,
                       int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *grad_raw_sigmas, float *grad_raw_rgbs,
                       nfa_stream_t stream)
{
    return nfa_render_raw_bwd_t(NFA_ELEM_F32, t_starts, t_ends, raw_sigmas, raw_rgbs, selector, density_act, density_bias,
                                rgb_act, trans, g_colors, g_opacities, g_depths, g_weights, g_trans, g_alphas, packed_info,
                                tiles, n_tiles, n_rays, n_elems, grad_raw_sigmas, grad_raw_rgbs, stream);
}

#define SDF_MODEL_CHECKS(name)                                                                                     \
    NFA_REQUIRE(model == NFA_SDF_NEUS || model == NFA_SDF_VOLSDF, name ": model must be 0 or 1 (got %d)", (int)model); \
    NFA_REQUIRE(rgb_act == NFA_RGB_ACT_NONE || rgb_act == NFA_RGB_ACT_SIGMOID, name ": rgb_act must be 0 or 1 (got %d)", (int)rgb_act)

extern "C++" {
template <class F>
static void dispatch_sdf_model(int32_t model, F &&f)
{
    if (model == NFA_SDF_NEUS) f(std::integral_constant<int, NFA_SDF_NEUS>{});
    else f(std::integral_constant<int, NFA_SDF_VOLSDF>{});
}
}  // extern "C++"

int nfa_render_sdf_fwd(const float *t_starts, const float *t_ends, const float *sdfs, const float *cos, const float *raw_rgbs,
                       const uint8_t *selector, int32_t model, const float *param, float cos_anneal_ratio, int32_t rgb_act,
                       const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                       float *weights, float *trans, float *alphas, float *colors, float *opacities, float *depths,
                       nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_sdf_fwd");
    SDF_MODEL_CHECKS("render_sdf_fwd");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(colors && opacities && depths && (n_elems == 0 || (t_starts && t_ends && sdfs && raw_rgbs)),
                "render_sdf_fwd: null pointer");
    NFA_REQUIRE(n_elems == 0 || model != NFA_SDF_NEUS || cos, "render_sdf_fwd: cos is null (NFA_SDF_NEUS)");
    NFA_REQUIRE(param, "render_sdf_fwd: param is null");
    const RawAct act = raw_act(selector, NFA_ACT_NONE, 0.0f, rgb_act);
    const SdfParam par = {param, cos_anneal_ratio};
    int rc = NFA_OK;
    dispatch_sdf_model(model, [&](auto tag) {
        constexpr int MD = decltype(tag)::value;
        auto make = [&](auto V) { RenderSdfFwdOp<V, MD> op; op.cosv = cos; op.act = act; op.par = par; return op; };
        rc = launch_render_fwd("render_sdf_fwd", make, MD != NFA_SDF_NEUS || aligned16(cos), t_starts, t_ends, sdfs, raw_rgbs, weights,
                               trans, alphas, colors, opacities, depths, packed_info, tiles, n_tiles, n_rays, stream);
    });
    return rc;
}

int nfa_render_sdf_bwd(const float *t_starts, const float *t_ends, const float *sdfs, const float *cos, const float *raw_rgbs,
                       const uint8_t *selector, int32_t model, const float *param, float cos_anneal_ratio, int32_t rgb_act,
                       const float *trans, const float *g_colors, const float *g_opacities, const float *g_depths,
                       const float *g_weights, const float *g_trans, const float *g_alphas, const int64_t *packed_info,
                       const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *grad_sdfs, float *grad_cos,
                       float *grad_param, float *grad_raw_rgbs, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_sdf_bwd");
    SDF_MODEL_CHECKS("render_sdf_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && sdfs && raw_rgbs && trans && (grad_sdfs || grad_cos || grad_param || grad_raw_rgbs),
                "render_sdf_bwd: null pointer");
    NFA_REQUIRE(model != NFA_SDF_NEUS || cos, "render_sdf_bwd: cos is null (NFA_SDF_NEUS)");
    NFA_REQUIRE(model == NFA_SDF_NEUS || !grad_cos, "render_sdf_bwd: grad_cos given with NFA_SDF_VOLSDF");
    NFA_REQUIRE(param, "render_sdf_bwd: param is null");
    const RawAct act = raw_act(selector, NFA_ACT_NONE, 0.0f, rgb_act);
    const SdfParam par = {param, cos_anneal_ratio};
    int rc = NFA_OK;
    dispatch_sdf_model(model, [&](auto tag) {
        constexpr int MD = decltype(tag)::value;
        auto make = [&](auto V, auto X) {
            RenderSdfBwdOp<V, X, MD> op;
            op.sig = sdfs; op.cosv = cos; op.act = act; op.par = par; op.gcos = grad_cos; op.gpar = grad_param;
            return op;
        };
        rc = launch_render_bwd("render_sdf_bwd", make, all_aligned16(sdfs, grad_cos, grad_param) && (MD != NFA_SDF_NEUS || aligned16(cos)),
                               t_starts, t_ends, raw_rgbs, trans, g_colors, g_opacities, g_depths, g_weights, g_trans, g_alphas,
                               grad_sdfs, grad_raw_rgbs, packed_info, tiles, n_tiles, n_rays, stream);
    });
    return rc;
}

int nfa_distortion_fwd(const float *weights, const float *t_starts, const float *t_ends, const int64_t *packed_info,
                       const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *loss, float *w_tot,
                       float *s_tot, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("distortion_fwd");
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(loss && w_tot && s_tot && (n_elems == 0 || (weights && t_starts && t_ends)), "distortion_fwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(weights, t_starts, t_ends);
    dispatch_bool(vec, [&](auto V) {
        DistortionFwdOp<V> op;
        op.pinfo = packed_info; op.ts = t_starts; op.te = t_ends; op.w = weights;
        op.loss = loss; op.wtot = w_tot; op.stot = s_tot;
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("distortion_fwd");
    return NFA_OK;
}

int nfa_distortion_bwd(const float *weights, const float *t_starts, const float *t_ends, const float *w_tot, const float *s_tot,
                       const float *g_loss, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                       int64_t n_elems, float *grad_weights, float *grad_t_starts, float *grad_t_ends, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("distortion_bwd");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(weights && t_starts && t_ends && w_tot && s_tot && g_loss && (grad_weights || grad_t_starts || grad_t_ends),
                "distortion_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(weights, t_starts, t_ends, grad_weights, grad_t_starts, grad_t_ends);
    dispatch_bool(vec, [&](auto V) {
        DistortionBwdOp<V> op;
        op.pinfo = packed_info; op.ts = t_starts; op.te = t_ends; op.w = weights;
        op.wtot = w_tot; op.stot = s_tot; op.gl = g_loss;
        op.gw = grad_weights; op.gts = grad_t_starts; op.gte = grad_t_ends;
        launch_seg<-1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("distortion_bwd");
    return NFA_OK;
}

int nfa_render_step_accumulate(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgbs,
                               const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                               int64_t n_elems, float alpha_thre, float *colors, float *opacities, float *depths,
                               int64_t *n_visible, nfa_stream_t stream)
{
    SEG_COMMON_CHECKS("render_step_accumulate");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(t_starts && t_ends && sigmas && rgbs && colors && opacities && depths, "render_step_accumulate: null pointer");
    hipStream_t s = as_stream(stream);
    const bool vec = all_aligned16(t_starts, t_ends, sigmas, rgbs);
    dispatch_bool(vec, [&](auto V) {
        RenderStepOp<V> op;
        op.ts = t_starts; op.te = t_ends; op.sig = sigmas; op.rgb = rgbs; op.thre = alpha_thre;
        op.colors = colors; op.opac = opacities; op.depth = depths;
        op.n_visible = reinterpret_cast<unsigned long long *>(n_visible);
        launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
    });
    NFA_CHECK_LAUNCH("render_step_accumulate");
    return NFA_OK;
}

int nfa_sample_positions_bwd(const float *rays_o, const float *rays_d, const float *t_starts, const float *t_ends,
                             const int64_t *ray_indices, const float *g_positions, const float *g_dirs,
                             const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                             int64_t samples_per_ray, const float *aabb_host, const float *aabb, int32_t contraction,
                             int32_t dirs_mode, float *grad_rays_o, float *grad_rays_d, float *grad_t_starts,
                             float *grad_t_ends, float *grad_p, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rays >= 0 && n_elems >= 0 && samples_per_ray >= 0, "sample_positions_bwd: negative size");
    NFA_REQUIRE(n_rays < ((int64_t)1 << 31) - 64, "sample_positions_bwd: too many rays");
    NFA_REQUIRE(contraction >= 0 && contraction <= 2 && dirs_mode >= 0 && dirs_mode <= 2,
                "sample_positions_bwd: contraction and dirs_mode must be 0, 1 or 2");
    const bool has_box = aabb_host || aabb;
    NFA_REQUIRE(has_box || contraction == 0, "sample_positions_bwd: contraction needs an aabb");
    NFA_REQUIRE(!(aabb_host && aabb), "sample_positions_bwd: aabb given twice");
    const bool per_ray = grad_rays_o || grad_rays_d;
    if (n_elems == 0 && (n_rays == 0 || !per_ray)) return NFA_OK;
    NFA_REQUIRE(rays_o && rays_d && t_starts && t_ends, "sample_positions_bwd: null pointer");
    NFA_REQUIRE(!g_dirs || dirs_mode != 0, "sample_positions_bwd: g_dirs needs dirs_mode");
    SampleBox box;
    for (int k = 0; k < 3; ++k) { box.lo[k] = aabb_host ? aabb_host[k] : 0.0f; box.hi[k] = aabb_host ? aabb_host[3 + k] : 1.0f; }
    box.dev = aabb;
    const int mode = has_box ? SP_AABB + contraction : SP_NONE;
    hipStream_t s = as_stream(stream);
    if (!per_ray) {
        NFA_REQUIRE(g_positions && (grad_p || grad_t_starts || grad_t_ends), "sample_positions_bwd: null pointer");
        NFA_REQUIRE(ray_indices ? n_rays >= 1 : (samples_per_ray >= 1 && n_elems == n_rays * samples_per_ray),
                    "sample_positions_bwd: without ray_indices n_elems must be n_rays * samples_per_ray");
        launch_sample_positions_bwd_flat(mode, box, rays_o, rays_d, t_starts, t_ends, ray_indices, n_rays, n_elems, samples_per_ray,
                                         g_positions, grad_p, grad_t_starts, grad_t_ends, s);
        NFA_CHECK_LAUNCH("sample_positions_bwd");
        return NFA_OK;
    }
    NFA_REQUIRE(packed_info && tiles && n_tiles >= 1, "sample_positions_bwd: packed_info/tiles is null");
    NFA_REQUIRE((g_positions || g_dirs) && !grad_p, "sample_positions_bwd: per-ray sums need g_positions or g_dirs, and write no grad_p");
    const bool vec = all_aligned16(t_starts, t_ends, g_positions, g_dirs, grad_t_starts, grad_t_ends);
    dispatch_bool(vec, [&](auto V) {
        dispatch_sample_mode(mode, [&](auto M) {
            SamplePosBwdOp<decltype(V)::value, decltype(M)::value> op;
            op.o = rays_o; op.d = rays_d; op.ts = t_starts; op.te = t_ends; op.gx = g_positions; op.gdirs = g_dirs;
            op.box = box; op.dscale = dirs_mode == 2 ? 0.5f : 1.0f;
            op.go = grad_rays_o; op.gd = grad_rays_d; op.gts = grad_t_starts; op.gte = grad_t_ends;
            launch_seg<1>(op, packed_info, tiles, n_rays, n_tiles, s);
        });
    });
    NFA_CHECK_LAUNCH("sample_positions_bwd");
    return NFA_OK;
}

}  // extern "C"

// common.hip.h -- shared device/host helpers for libnerfacc_hip.so (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/nerfacc_hip.h"

#define NFA_WAVE 64

namespace nfa {

void set_error(const char *fmt, ...);

#define NFA_REQUIRE(cond, ...)                         \
    do {                                               \
        if (!(cond)) {                                 \
            nfa::set_error(__VA_ARGS__);               \
            return NFA_EINVAL;                         \
        }                                              \
    } while (0)

// Launch errors are not swallowed (the reference discards cudaGetLastError, scan.cu:64).
#define NFA_CHECK_LAUNCH(name)                                                       \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess) {                                                     \
            nfa::set_error("%s: launch failed: %s", name, hipGetErrorString(e__));   \
            return NFA_EHIP;                                                         \
        }                                                                            \
    } while (0)

// Knobs of the A/B tests and measurement scripts, set through nfa_set_tuning (grid.hip); the entry points do not read the
// environment.  NULL: not set.
const char *tuning_env(const char *name);

// The launch plan of the cone walk's two forms (grid.hip: nfa_traverse_cone_runs, walk.hip: nfa_traverse_cone_walk) for n_walk rays:
// the refilling kernel for limited walks (NFA_REFILL_ALL = "1": for unlimited ones too, for measurements), where a wave owns
// `chunk` entries of the ray list and leaves its cell loop when fewer than `min_busy` lanes are walking; one ray per lane
// otherwise, and always with NFA_REFILL = "0".  NFA_REFILL = "chunk,min_busy" sets the two numbers.
struct RefillPlan {
    bool refill;
    int64_t chunk;
    int32_t min_busy;
};
static inline RefillPlan refill_plan(int64_t n_walk, int32_t steps_limit)
{
    const char *refill_env = tuning_env("NFA_REFILL"), *refill_all = tuning_env("NFA_REFILL_ALL");
    if (!(steps_limit > 0 || (refill_all && refill_all[0] == '1')) || (refill_env && refill_env[0] == '0')) return RefillPlan{false, 64, 64};
    // entries per wave: enough of them that a lane is refilled several times, as long as the launch still fills the chip
    int64_t chunk = ((n_walk + 4095) / 4096 + 63) / 64 * 64;
    chunk = chunk < 64 ? 64 : (chunk > 1024 ? 1024 : chunk);
    int min_busy = 48;
    if (refill_env) { long c = 0; int m = 0; if (sscanf(refill_env, "%ld,%d", &c, &m) == 2 && c >= 64 && m >= 1 && m <= 64) { chunk = c / 64 * 64; min_busy = m; } }
    return RefillPlan{true, chunk, min_busy};
}

static inline hipStream_t as_stream(nfa_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

__host__ __device__ static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grid for 1-D grid-stride kernels: enough workgroups to fill 256 CUs x 8 blocks.
static inline unsigned grid_1d(int64_t n, int block, int64_t cap = 256 * 16)
{
    int64_t g = ceil_div64(n, block);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <typename... P>
static inline bool all_aligned16(P... p) { return (aligned16(p) && ...); }

// Host-side dispatch of a run-time value to a compile-time one: f(std::true_type / std::false_type), f(the channel
// count 1..4 as std::integral_constant<int, C>), and f(the lanes per ray, a power of two 2..64, as
// std::integral_constant<int, L>; anything else goes to 64).
template <class F>
static void dispatch_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
static void dispatch_channels(int c, F &&f)
{
    if (c == 4) f(std::integral_constant<int, 4>{});
    else if (c == 3) f(std::integral_constant<int, 3>{});
    else if (c == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}
template <class F>
static void dispatch_lanes(int l, F &&f)
{
    if (l == 2) f(std::integral_constant<int, 2>{});
    else if (l == 4) f(std::integral_constant<int, 4>{});
    else if (l == 8) f(std::integral_constant<int, 8>{});
    else if (l == 16) f(std::integral_constant<int, 16>{});
    else if (l == 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}
// f(std::integral_constant<int, v>) when v is one of V...; nothing otherwise
template <int... V, class Fn>
static void dispatch_value(int32_t v, Fn &&f)
{
    (void)((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}

// ---------------------------------------------------------------- wave64 primitives
__device__ __forceinline__ int lane_id() { return __lane_id(); }

template <typename T>
__device__ __forceinline__ T wave_shfl_up(T v, int delta) { return __shfl_up(v, delta, NFA_WAVE); }
template <typename T>
__device__ __forceinline__ T wave_shfl(T v, int src) { return __shfl(v, src, NFA_WAVE); }

__device__ __forceinline__ int64_t wave_incl_sum_i64(int64_t v)
{
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < NFA_WAVE; off <<= 1) {
        int64_t u = __shfl_up(v, off, NFA_WAVE);
        if (lane >= off) v += u;
    }
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, NFA_WAVE);
    return v;
}

// a wave-uniform 64-bit value into a scalar register pair
__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Cross-lane moves as DPP modifiers (one VALU instruction each, no LDS crossbar round trip):
// step s < 4 shifts by 2^s inside each row of 16 lanes, step 4 broadcasts lane 15 of rows 0 / 2 to rows 1 / 3,
// step 5 broadcasts lane 31 to rows 2 and 3.  Lanes without a source keep `old`.
template <int S>
__device__ __forceinline__ int32_t dpp_step(int32_t old, int32_t src)
{
    static_assert(S >= 0 && S < 6, "dpp_step");
    if constexpr (S == 0) return __builtin_amdgcn_update_dpp(old, src, 0x111, 0xf, 0xf, false);       // row_shr:1
    else if constexpr (S == 1) return __builtin_amdgcn_update_dpp(old, src, 0x112, 0xf, 0xf, false);  // row_shr:2
    else if constexpr (S == 2) return __builtin_amdgcn_update_dpp(old, src, 0x114, 0xf, 0xf, false);  // row_shr:4
    else if constexpr (S == 3) return __builtin_amdgcn_update_dpp(old, src, 0x118, 0xf, 0xf, false);  // row_shr:8
    else if constexpr (S == 4) return __builtin_amdgcn_update_dpp(old, src, 0x142, 0xa, 0xf, false);  // row_bcast:15
    else return __builtin_amdgcn_update_dpp(old, src, 0x143, 0xc, 0xf, false);                        // row_bcast:31
}
template <int S>
__device__ __forceinline__ float dpp_step(float old, float src)
{
    return __int_as_float(dpp_step<S>(__float_as_int(old), __float_as_int(src)));
}
// value of the previous lane (lane 0 keeps `old`)
__device__ __forceinline__ int32_t dpp_prev_lane(int32_t old, int32_t src)
{
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false);  // wave_shr:1
}
__device__ __forceinline__ float dpp_prev_lane(float old, float src)
{
    return __int_as_float(dpp_prev_lane(__float_as_int(old), __float_as_int(src)));
}
// a * b + c on 24-bit unsigned operands as ONE full-rate instruction (hipcc turns __umul24(a, b) + c into the
// quarter-rate 64-bit v_mad_u64_u32)
// Level of an event of a ray's sorted intersection list.  t_indices holds argsort indices in [0, 2G) (grid.py:158-162: entries
// below G enter level idx, the others leave level idx - G), so the reference's `idx % G` (grid.cu:127,137) is a conditional
// subtraction; as a 64-bit modulo by a run-time divisor it was ~200 instructions, twice per event -- a fifth of a limited
// walk's launch (the test-mode loop reads its list from the start in every iteration).  Out-of-range input: level >= G,
// which callers treat as "not hit".
__device__ __forceinline__ int32_t event_level(int64_t idx, int32_t G)
{
    const int32_t i = (int32_t)idx;
    return i >= G ? i - G : i;
}

__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// Workgroups are dealt round-robin over the 8 XCDs (block b runs on XCD b % 8: MI355X_MICROARCH.md), and an XCD only
// takes the blocks dealt to it.  A cost that is periodic in the block index with a period that divides 8 therefore lands
// on a few XCDs: the rays of a 1024-pixel image row are four 256-ray blocks, the two middle ones cross the most cells, and
// XCDs 1, 2, 5, 6 were still walking them while the other four had been idle for the last third of the launch (wave
// time stamps, DESIGN.md: 4096 busy waves, then 2000).  Within each group of 8 consecutive blocks the work
// items are rotated by the group's number, so every XCD sees every residue; a bijection on [0, n_blocks).
__device__ __forceinline__ int64_t xcd_fair_block(uint32_t b, uint32_t n_blocks)
{
    const uint32_t group = b >> 3;
    if (((group + 1u) << 3) > n_blocks) return b;   // (the last, partial group)
    return (int64_t)((b & ~7u) | ((b + group) & 7u));
}

// ---------------------------------------------------------------- issue rates (gfx950, scripts/valu_probe.hip)
// One SIMD issues a wave64 v_add / v_sub / v_mul / v_fma (f32), v_add / v_sub (u32), v_and / v_or / v_xor, v_lshrrev,
// v_ashrrev, v_mov, v_cndmask (VOP2 form, condition in vcc) and v_bitop3 every 2 cycles, and every 4 cycles: v_min / v_max
// (f32 and u32), v_min3 / v_med3, v_cmp, v_cndmask with the condition in another scalar pair (VOP3 form), v_bfi, v_bfe,
// v_lshlrev, v_mul_u32_u24, v_cvt and all three-operand integer instructions (v_lshl_add, v_and_or, v_mad_u32_u24, v_add3,
// v_perm, v_alignbit); v_pk_add_f32 too (profiles/r04_valu_probe.txt).  The issue-bound kernels are written against that
// table: a select whose condition is a lane MASK in a register ((k & x) | (~k & y)) is one v_bitop3 at the full rate where
// v_cndmask / v_bfi run at half of it, and "x is the minimum m of the values" is the sign of m - x (two full-rate
// instructions for a mask that serves any number of selects) instead of a compare plus a select each.
// (The compiler's builtin where there is one: between two `asm` statements it puts an s_nop whenever the second reads what the
// first wrote -- it cannot know that the first is no transcendental -- and an s_nop costs an issue slot like an instruction.)
__device__ __forceinline__ uint32_t sel_mask(uint32_t k, uint32_t x, uint32_t y)   // k ? x : y, bit by bit
{
    return __builtin_amdgcn_bitop3_b32(k, x, y, 0xca);
}
__device__ __forceinline__ float sel_mask(uint32_t k, float x, float y)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_bitop3_b32(k, __builtin_bit_cast(uint32_t, x), __builtin_bit_cast(uint32_t, y), 0xca));
}
// ~0 where a - b is negative (a < b for finite a, b; a == b gives +0: no bits), else 0
__device__ __forceinline__ uint32_t mask_less(float a, float b)
{
    return (uint32_t)(__builtin_bit_cast(int32_t, a - b) >> 31);   // v_sub_f32, v_ashrrev_i32 (checked in the generated code)
}
__device__ __forceinline__ float min3_f32(float a, float b, float c)
{
    float m;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}

__device__ __forceinline__ int32_t last_lane(int32_t v) { return __builtin_amdgcn_readlane(v, 63); }
__device__ __forceinline__ float last_lane(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
// value of lane `l` (wave-uniform index)
__device__ __forceinline__ int32_t lane_value(int32_t v, int32_t l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_value(float v, int32_t l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }


// 16-byte stores of streamed outputs.  NT marks them non-temporal: traverse2.hip's expansions do, the engine ops lose with it.
typedef float nfa_v4f __attribute__((ext_vector_type(4)));
typedef long long nfa_v2l __attribute__((ext_vector_type(2)));
typedef uint32_t nfa_v2u __attribute__((ext_vector_type(2)));
typedef uint32_t nfa_v4u __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- half-precision activation streams (NFA_ELEM_*)
// fp16 and bf16 are storage types only: every value is widened on load (exact) and arithmetic stays float32.  A store is
// the compiler's conversion of the float32 value the float32 kernels store: one rounding to nearest even, results in fp16's
// subnormal range kept (the f16 denormal mode is on by default), on gfx950 the packed bf16 convert.  Halves travel as the 16-bit halves of
// dwords, two to a dword, lower address in the low half.
typedef _Float16 nfa_f16;
typedef __bf16 nfa_bf16;
template <class E> struct ElemTag { using type = E; };

template <class E>
__device__ __forceinline__ uint32_t half_bits(float v)   // E(v) in the low 16 bits
{
    static_assert(sizeof(E) == 2, "half element types only");
    // The float32 value exists, rounded, before it is converted: left to itself the compiler folds the float32 multiply or
    // add that produced it into v_fma_mixlo_f16, which rounds the exact result to fp16 once -- in about one value of 2^13
    // not the fp16 nearest to the float32 value the float32 kernel stores.  (No instruction: a constraint on a register.)
    asm("" : "+v"(v));
    const E h = (E)v;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}
template <class E>
__device__ __forceinline__ float half_value(uint32_t bits16)
{
    if constexpr (std::is_same<E, nfa_bf16>::value) {
        return __uint_as_float(bits16 << 16);
    } else {
        const uint16_t b = (uint16_t)bits16;
        E h;
        __builtin_memcpy(&h, &b, 2);
        return (float)h;
    }
}
template <class E>
__device__ __forceinline__ uint32_t pack_halves(float lo, float hi) { return half_bits<E>(lo) | (half_bits<E>(hi) << 16); }
// half k (0 or 1) of a dword
template <class E>
__device__ __forceinline__ float unpack_half(uint32_t w, int k) { return half_value<E>(k ? w >> 16 : w & 0xFFFFu); }

// f(ElemTag<float / nfa_f16 / nfa_bf16>) for an NFA_ELEM_* code; false for any other code
template <class F>
static bool dispatch_elem(int32_t elem, F &&f)
{
    if (elem == NFA_ELEM_F32) f(ElemTag<float>{});
    else if (elem == NFA_ELEM_F16) f(ElemTag<nfa_f16>{});
    else if (elem == NFA_ELEM_BF16) f(ElemTag<nfa_bf16>{});
    else return false;
    return true;
}

template <bool NT = false>
__device__ __forceinline__ void store_f4(float *p, float a, float b, float c, float d)
{
    nfa_v4f v = {a, b, c, d};
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<nfa_v4f *>(p));
    else *reinterpret_cast<nfa_v4f *>(p) = v;
}
template <bool NT = false>
__device__ __forceinline__ void store_l2(int64_t *p, int64_t a, int64_t b)
{
    nfa_v2l v = {a, b};
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<nfa_v2l *>(p));
    else *reinterpret_cast<nfa_v2l *>(p) = v;
}

// Four consecutive xyz rows (48 B) of a streamed [n, 3] output from element e on: three 16-byte stores when `vec` (the base
// is 16-byte aligned and the quad is full), else the first `cnt` rows element by element (samples.hip, rays.hip).
__device__ __forceinline__ void store_rows12(float *__restrict__ out, int64_t e, bool vec, int cnt, const float v[12])
{
    float *b = out + 3 * e;
    if (vec) {
        store_f4(b, v[0], v[1], v[2], v[3]);
        store_f4(b + 4, v[4], v[5], v[6], v[7]);
        store_f4(b + 8, v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) { b[3 * j] = v[3 * j]; b[3 * j + 1] = v[3 * j + 1]; b[3 * j + 2] = v[3 * j + 2]; }
    }
}

// ---------------------------------------------------------------- what the traversal kernels of grid.hip and walk.hip share
// Slab test, grid.cu:284-313 / include/utils_grid.cuh:10-55; tmin / tmax mean something only for a hit.
__device__ __forceinline__ bool slab_test(const float o[3], const float inv[3], const float *bmin, const float *bmax, float near,
                                          float far, float &tmin, float &tmax)
{
    float lo, hi;
    if (inv[0] >= 0) { tmin = (bmin[0] - o[0]) * inv[0]; tmax = (bmax[0] - o[0]) * inv[0]; }
    else             { tmin = (bmax[0] - o[0]) * inv[0]; tmax = (bmin[0] - o[0]) * inv[0]; }
#pragma unroll
    for (int a = 1; a < 3; ++a) {
        if (inv[a] >= 0) { lo = (bmin[a] - o[a]) * inv[a]; hi = (bmax[a] - o[a]) * inv[a]; }
        else             { lo = (bmax[a] - o[a]) * inv[a]; hi = (bmin[a] - o[a]) * inv[a]; }
        if (tmin > hi || lo > tmax) return false;
        if (lo > tmin) tmin = lo;
        if (hi < tmax) tmax = hi;
    }
    if (tmax <= 0) return false;
    tmin = fmaxf(tmin, near);
    tmax = fminf(tmax, far);
    return true;
}

// The event walk, grid.cu:125-150: the ray's next span (level, [this_tmin, this_tmax)) from its sorted intersection list,
// `ev` the next event to look at (2 * G: none left).  EVENTS says where the list lives: index(i), t(i), hit(level).
struct EventsInMemory {   // the caller's t_indices / t_sorted / hits rows
    const int64_t *ti;
    const float *ts;
    const uint8_t *hits;
    __device__ __forceinline__ EventsInMemory(const nfa_traverse_args &a, int64_t tid)
        : ti(a.t_indices + tid * 2 * a.n_grids), ts(a.t_sorted + tid * 2 * a.n_grids), hits(a.hits + tid * a.n_grids) {}
    __device__ __forceinline__ int64_t index(int32_t i) const { return ti[i]; }
    __device__ __forceinline__ float t(int32_t i) const { return ts[i]; }
    __device__ __forceinline__ bool hit(int32_t level) const { return hits[level] != 0; }
};
template <class EVENTS>
__device__ __forceinline__ bool next_event_span(const EVENTS &e, int32_t G, float near_plane, float far_plane, int32_t &ev,
                                                int32_t &level, float &this_tmin, float &this_tmax)
{
    while (ev < 2 * G - 1) {
        const int32_t i = ev++;
        const auto idx = e.index(i);
        level = event_level(idx, G);
        bool ok = (uint32_t)level < (uint32_t)G && e.hit(level);
        if (ok && idx >= G) {  // leaving: inside the next grid?
            const auto nidx = e.index(i + 1);
            level = event_level(nidx, G);
            ok = nidx >= G && (uint32_t)level < (uint32_t)G && e.hit(level);
        }
        this_tmin = fmaxf(e.t(i), near_plane);
        this_tmax = fminf(e.t(i + 1), far_plane);
        if (ok && this_tmin < this_tmax) return true;
    }
    return false;
}
// Run records of the cone-angle count passes (nfa_traverse_cone_runs, nfa_traverse_cone_walk; same format as traverse2.hip's):
// {t_first : f32 | k_start : 31, continues_previous : 1}, slot-major.  With a cone angle a chain of samples is the recurrence
// t <- t + max(step, t * cone) from its first distance, so {t_first, k_start} determines every sample of it; chains are cut
// every CONE_RUN_CAP samples so that the expansion (expand_runs_kernel<EXP_CONE>) iterates the recurrence at most that often
// per output.  The second walk of the fill pass becomes a coalesced expansion.
constexpr int CONE_RUN_CAP = 64;
struct RunOut {
    int32_t *run_cnts;          // [n_rays]
    unsigned long long *runs;   // [max_runs, n_rays]
    int32_t max_runs;
    int32_t *overflow;          // [1]
    const int32_t *order;       // lane -> ray assignment (nfa_bin_rays / nfa_bin_rays_levels) or NULL
    int64_t n_order;            // its entries (< n_rays: only the listed rays are walked; the others keep their outputs)
};
__device__ __forceinline__ unsigned long long run_record(float t_first, int32_t k_start, int32_t continues)
{
    return (unsigned long long)__float_as_uint(t_first) | ((unsigned long long)((uint32_t)k_start | (continues ? 0x80000000u : 0u)) << 32);
}
// the end of a ray of a count pass that leaves run records
__device__ __forceinline__ void run_ray_close(const nfa_traverse_args &a, const RunOut &ro, int64_t tid, float t_last, int32_t n_samples,
                                              int32_t n_runs)
{
    if (a.terminate_planes) a.terminate_planes[tid] = t_last;
    a.sm_cnts[tid] = n_samples;
    // rays with > 2^21 samples go to the serial fill (the expansion packs a 27-bit batch offset)
    if (n_samples > (1 << 21) && n_runs <= ro.max_runs) n_runs = ro.max_runs + 1;
    ro.run_cnts[tid] = n_runs;
    if (n_runs > ro.max_runs) atomicAdd(ro.overflow, 1);
}
// a ray masked out by rays_mask (grid.cu:100; the reference leaves its outputs uninitialised, we define them)
__device__ __forceinline__ bool ray_masked(const nfa_traverse_args &a, const RunOut &ro, int64_t tid)
{
    if (!(a.mode == 2 && a.rays_mask != nullptr && !a.rays_mask[tid])) return false;
    if (a.terminate_planes) a.terminate_planes[tid] = a.near_planes[tid];
    if (a.iv_cnts) a.iv_cnts[tid] = 0;
    if (a.sm_cnts) a.sm_cnts[tid] = 0;
    if (ro.run_cnts) ro.run_cnts[tid] = 0;
    return true;
}
// The ray's planes, origin and direction; false for a ray without geometry.  A non-finite origin or direction: upstream its NaN
// planes survive fmaxf / fminf as [near, far] and the ray is sampled all the way to the far plane (1e10 by default).  Here it
// gets no samples.
__device__ __forceinline__ bool ray_load(const nfa_traverse_args &a, int64_t tid, float &near_plane, float &far_plane, float o[3], float d[3])
{
    near_plane = a.near_planes[tid]; far_plane = a.far_planes[tid];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { o[ax] = a.rays_o[3 * tid + ax]; d[ax] = a.rays_d[3 * tid + ax]; }
    return isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

// The refilling scheduler of the limited cone walks (traverse_steps_limit > 0: one iteration of the test-mode loop,
// examples/utils.py:252-425).  Such walks stop after a handful of samples, i.e. after a number of cells that is geometric in the
// local occupancy.  With one ray per lane from start to end a wave lasts as long as its unluckiest ray: on cfg 5 (2 % scattered
// occupancy) the mean is 50 cells to the first sample, the maximum over 64 lanes about 240, and the lanes are busy a fifth of
// the time (2.5 ms per call for 2 M rays where the cells themselves are worth 0.3 ms).  Here a wave (number `wave` of the
// launch) owns `chunk` consecutive slots of the ray list and a lane that has finished its ray is given the next one: the wave
// leaves its cell loop when fewer than `min_busy` lanes are still walking, sets up new rays (and the next spans of rays that
// crossed into another level) on the free lanes, and re-enters; when the chunk is handed out, it stays until a quarter of the
// walking lanes have left.  The WALKER holds a lane's ray and does the arithmetic -- the same functions as its one-ray-per-lane
// kernel, so results are identical --:
//     bool take(tid)      load ray tid; false: nothing to walk (masked: its outputs are written; or filtered out)
//     bool next_span()    set up the ray's next span; false: it has none left
//     int  cell()         visit one cell: RF_WALK (the span goes on), RF_SPAN (it is over), RF_FINISH (the sample budget is
//                         spent: nothing after it changes the ray)
//     void finish()       write the ray's outputs
enum { RF_IDLE = 0, RF_SPAN = 1, RF_WALK = 2, RF_FINISH = 3 };
template <class WALKER>
__device__ __forceinline__ void refill_schedule(WALKER &w, const int32_t *order, int64_t n_walk, int64_t wave, int32_t chunk, int32_t min_busy)
{
    const int lane = lane_id();
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    int64_t next = wave * chunk;  // (wave-uniform) first slot not handed out yet
    const int64_t end = next + chunk < n_walk ? next + chunk : n_walk;
    int32_t phase = RF_IDLE;
    for (;;) {
        // Two passes: rays that left a span in the cell loop (their next span, or their end), then the rays handed to
        // the lanes that are free after that.
#pragma nounroll
        for (int pass = 0; pass < 2; ++pass) {
            if (phase == RF_SPAN) phase = w.next_span() ? RF_WALK : RF_FINISH;
            if (phase == RF_FINISH) {
                w.finish();
                phase = RF_IDLE;
            }
            if (pass == 1) break;
            // ---- free lanes take the next rays of the wave's chunk
            const unsigned long long idle = __ballot(phase == RF_IDLE);
            if (idle != 0ull && next < end) {
                if (phase == RF_IDLE) {
                    const int64_t slot = next + __popcll(idle & lanes_below);
                    if (slot < end && w.take(order ? (int64_t)order[slot] : slot)) phase = RF_SPAN;
                }
                next += __popcll(idle);
            }
        }
        const unsigned long long walking = __ballot(phase == RF_WALK);
        if (walking == 0ull) {
            if (next >= end) break;  // (every lane is idle here: RF_SPAN and RF_FINISH were resolved above)
            continue;
        }
        // ---- cells, for as long as enough lanes have one to visit
        const int32_t n_walking = __popcll(walking);
        const int32_t need = next < end ? min_busy : (n_walking * 3 >> 2) > 1 ? (n_walking * 3 >> 2) : 1;
        do {
            if (phase == RF_WALK) phase = w.cell();
        } while (__popcll(__ballot(phase == RF_WALK)) >= need);
    }
}

}  // namespace nfa

// hashgrid_merged.hip -- the hash grid's table gradient with equal cells merged before the atomics (nfa_hashgrid_bwd_merged):
// a third way of forming dL/dparams, next to the atomic scatter of hashgrid_bwd_kernel and the sorted sum (encoding.hip).
//
// Why: hashgrid_bwd_kernel's lanes are (point, level) pairs with the level fastest, so a wave writes to 16 level slices and
// two neighbouring samples of a ray never share an instruction.  On a coarse level those samples sit in the same cell and
// send their 2^D F float atomics to the same 2^D entries, where they serialise.  Here a lane is a point and a workgroup row
// a level (the forward's layout), so a wave holds 64 consecutive points of one level, and equal cells meet twice before
// anything goes to memory: inside the wave, and in a copy of the level's gradient in LDS.
//
// The term of a (point, corner, feature) is the atomic path's, bit for bit: Corner<D>::first_order() * g[j] on the Cell that
// locate() gives (Smoothstep: after smoothstep()), added to the entry corner_index() names.  Only the order and grouping of
// the float32 additions differ, so the result is NOT bitwise reproducible (it still ends in float atomics) and agrees with
// the atomic path's within the rounding of a float32 sum.  params is not read and dL/dx is not formed: the caller gets dL/dx
// from nfa_hashgrid_bwd* with a null grad_params, as the sorted path does.
//
// Layout.  blockIdx.y is the level, a workgroup of 256 threads owns `span_l` consecutive points [blockIdx.x span_l,
// (blockIdx.x + 1) span_l) and walks them 256 at a time; thread t of a pass has point base + t.  Points are indexed in 64 bits.
//
// Stage 1, the run merge (registers).  A lane is a run head if it is lane 0, if its point is past n_points (such lanes stay in
// the instruction stream with zero terms and are runs of their own, so every cross-lane read has a defined source), or if its
// cell differs from the previous lane's in any of the D integer coordinates g_d.  Cells are compared, not entries: two
// cells that hash to one entry are two runs, and the atomics add them.  heads = ballot(head).
//   heads all ones (a fine level, unordered points): nothing to merge; every lane scatters its own terms.  The cost of
//   the stage is then the D compares and the ballot.
//   otherwise: dist = lane - (the nearest head at or below the lane), and the terms are summed over each run by a segmented
//   Hillis-Steele scan, t[lane] += t[lane - off] where dist >= off, for off = 1, 2, 4, .. while any lane still has
//   dist >= off (at most log2 64 = 6 steps of ds_bpermute moves, which pass through the LDS crossbar but no memory).  The
//   last lane of a run then holds the run's sum, and only it computes the 2^D indices and scatters.
// A lane holds merged_group<D, F>() corners x F terms at a time, at most 32 floats: D = 3 at F = 8 and D = 4 from F = 4 take
// the corners in groups, each group formed, scanned and scattered before the next (the order of the groups does not matter to
// the result; corner_group_bwd of encoding.hip is the precedent).
//
// Stage 2, a level's gradient in LDS.  Levels 0 .. n_lds - 1, the leading levels whose slice size_l F is at most
// NFA_HG_MERGED_LDS_FLOATS (include/nerfacc_hip.h; hashed levels count when the table is small), are one launch with
// max_l size_l F floats of dynamic LDS: the workgroup zeroes its copy, adds the run sums of stage 1 into it with ds_add_f32
// (atomicAdd on __shared__ floats), and at the end of its span adds the non-zero entries of the copy to grad_params with
// global float atomics, consecutive lanes over consecutive entries.  The other levels are a second launch without LDS, whose
// run sums go straight to memory with unsafeAtomicAdd.  The cap of 16,384 floats is 64 KiB, the most a workgroup gets without
// opting in to more and two workgroups in a CU's 160 KiB; the Instant-NGP grids (base resolution 16, F = 2: 8,192 floats on
// level 0) take 32 KiB and keep five.
//
// The span rule (host, merged_plan): a function of (n_points, size_l, F, D) alone.
//   LDS level:   span_l = 256 ceil(8 size_l / (2^D 256)): a span's flush issues at most size_l F atomics where the atomic
//                path issues span_l 2^D F, so the flush is at most one eighth of the adds it replaces.
//   other level: span_l = 1,024: four passes, and 256 workgroups per level at 2^18 points (3,840 for the 15 upper levels of
//                the NGP grid: the launch fills 256 CUs several times over).
//   both:        at least 256 ceil(n_points / 2^28) (at most 2^20 workgroups per level), at most n_points rounded up to 256.
// The launch depends on (n_points, the level table) alone, reads nothing back and needs no scratch, so it can be captured.
// Measurements, the resource table and the alternatives tried: DESIGN.md, "Hash grid: merged table gradient".
#include "encoding_dev.h"

namespace nfa {

#define NFA_HG_MERGED_FLUSH_RATIO 8     // an LDS level's span issues at least this many times the adds of its flush
#define NFA_HG_MERGED_SPAN 1024         // points per workgroup on a level without LDS
#define NFA_HG_MERGED_MAX_SPANS ((int64_t)1 << 20)

struct MergedPlan {
    uint32_t span[NFA_HG_MAX_LEVELS];   // points per workgroup on the level, a multiple of 256
    int32_t n_lds;                      // levels 0 .. n_lds - 1 keep their gradient in LDS
    uint32_t lds_floats;                // the largest slice among them
    int64_t min_span[2];                // the shortest span of the LDS levels / of the others
};

// NFA_HG_MERGED_PLAN = "ratio,span,cap" (nfa_set_tuning) replaces the three constants for measurements; cap <= the header's.
static MergedPlan merged_plan(const GridArgs &G, const HashGridLevels &T)
{
    int64_t ratio = NFA_HG_MERGED_FLUSH_RATIO, span_global = NFA_HG_MERGED_SPAN, cap = NFA_HG_MERGED_LDS_FLOATS;
    if (const char *env = tuning_env("NFA_HG_MERGED_PLAN")) {
        long r = 0, s = 0, c = 0;
        if (sscanf(env, "%ld,%ld,%ld", &r, &s, &c) == 3 && r >= 1 && s >= 256 && s % 256 == 0 && c >= 0 && c <= NFA_HG_MERGED_LDS_FLOATS) {
            ratio = r; span_global = s; cap = c;
        }
    }
    MergedPlan P = {};
    const int64_t all = ceil_div64(G.n_points, 256) * 256;
    const int64_t least = ceil_div64(G.n_points, 256 * NFA_HG_MERGED_MAX_SPANS) * 256;
    P.min_span[0] = P.min_span[1] = all;
    bool lds = true;   // the LDS levels are a prefix: the first level over the cap ends it
    for (int l = 0; l < T.n_levels; ++l) {
        const int64_t floats = (int64_t)T.size[l] * G.n_features;
        lds = lds && floats <= cap;
        int64_t span = lds ? ceil_div64(ratio * T.size[l], (int64_t)256 << G.n_dims) * 256 : span_global;
        span = span < least ? least : span;
        span = span > all ? all : span;
        P.span[l] = (uint32_t)span;
        if (lds) {
            P.n_lds = l + 1;
            P.lds_floats = floats > P.lds_floats ? (uint32_t)floats : P.lds_floats;
        }
        P.min_span[lds ? 0 : 1] = span < P.min_span[lds ? 0 : 1] ? span : P.min_span[lds ? 0 : 1];
    }
    return P;
}

// corners whose terms a lane holds at a time: all 2^D up to 32 terms, else 32 / F
template <int D, int F>
__host__ __device__ constexpr int merged_group() { return (1 << D) * F <= 32 ? 1 << D : 32 / F; }

// The G corners from `first` of the run that ends in this lane: t[k F + j] added to feature j of corner first + k's entry, in
// the workgroup's LDS copy of the level (dst = the copy) or in grad_params (dst = the level's slice)
template <bool LDS, int D, int F, int G>
__device__ __forceinline__ void merged_scatter(float *dst, const Cell<D> &c, int first, const LevelRef &L, const float *t)
{
#pragma unroll
    for (int k = 0; k < G; ++k) {
        float *e = dst + (size_t)corner_index(c, first + k, L) * F;
#pragma unroll
        for (int j = 0; j < F; ++j) {
            if constexpr (LDS) atomicAdd(e + j, t[k * F + j]);
            else unsafeAtomicAdd(e + j, t[k * F + j]);
        }
    }
}

template <int D, int F, class E, int I>
__global__ __launch_bounds__(256) void hashgrid_bwd_merged_kernel(const float *__restrict__ x, const E *__restrict__ g_y,
                                                                  int64_t n_points, const HashGridLevels T, const MergedPlan P,
                                                                  int first_level, int use_lds, float *__restrict__ g_params)
{
    extern __shared__ float copy[];   // use_lds: the level's gradient, size_l F floats
    constexpr int G = merged_group<D, F>();
    const int l = first_level + (int)blockIdx.y;
    const LevelRef L(T, l);
    const int64_t begin = (int64_t)blockIdx.x * P.span[l];
    if (begin >= n_points) return;   // (the whole workgroup: the grid is sized by the shortest span of the launch)
    const int64_t end = begin + P.span[l] < n_points ? begin + P.span[l] : n_points;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t floats = L.size * F;
    float *slice = g_params + (size_t)L.offset * F;
    if (use_lds) {
        for (uint32_t i = tid; i < floats; i += 256) copy[i] = 0.0f;
        __syncthreads();
    }
    for (int64_t base = begin; base < end; base += 256) {   // (uniform: every lane of the workgroup makes every pass)
        const int64_t n = base + tid;
        const bool active = n < end;
        Cell<D> c = {};
        FVec<F> g = {};
        if (active) {
            c = locate<D>(x + n * D, L.scale);
            if constexpr (I == NFA_INTERP_SMOOTHSTEP) {
                float d1[D], d2[D];
                smoothstep(c, d1, d2);
            }
            g = load_piece<F>(g_y, n * T.n_levels + l);
        }
        bool head = lane == 0 || !active;
#pragma unroll
        for (int d = 0; d < D; ++d) {   // (every lane makes every move: no `||`, whose right side lanes that are heads would skip)
            const uint32_t before = __shfl_up(c.g[d], 1, NFA_WAVE);
            head = head | (before != c.g[d]);
        }
        const unsigned long long heads = __ballot(head);
        const int dist = lane - (63 - __clzll((long long)(heads & ((2ull << lane) - 1ull))));   // (bit 0 is set: lane 0 is a head)
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#pragma nounroll
        for (int first = 0; first < (1 << D); first += G) {
            float t[G * F];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const float wc = Corner<D>(c, first + k).first_order();
#pragma unroll
                for (int j = 0; j < F; ++j) t[k * F + j] = wc * g.v[j];
            }
            if (heads != ~0ull) {
                for (int off = 1; off < NFA_WAVE; off <<= 1) {
                    const bool take = dist >= off;
                    if (!__any(take)) break;   // (no run is longer than off: none will be at 2 off)
#pragma unroll
                    for (int i = 0; i < G * F; ++i) {
                        const float u = __shfl_up(t[i], off, NFA_WAVE);
                        t[i] = take ? t[i] + u : t[i];
                    }
                }
            }
            if (tail && active) {
                if (use_lds) merged_scatter<true, D, F, G>(copy, c, first, L, t);
                else merged_scatter<false, D, F, G>(slice, c, first, L, t);
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t i = tid; i < floats; i += 256) {
            const float v = copy[i];
            if (v != 0.0f) unsafeAtomicAdd(slice + i, v);
        }
    }
}

template <class E>
static int hashgrid_bwd_merged(int32_t interp, const float *x, const E *grad_y, const GridArgs &G, float *grad_params,
                               nfa_stream_t stream)
{
    HashGridLevels T;
    const int rc = hashgrid_table("hashgrid_bwd_merged", G, T);
    if (rc != NFA_OK) return rc;
    if (G.n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && grad_y && grad_params, "hashgrid_bwd_merged: null pointer");
    NFA_REQUIRE(G.n_dims == 3 || aligned16(x), "hashgrid_bwd_merged: x must be 16-byte aligned at n_dims %d", G.n_dims);
    NFA_REQUIRE((std::is_same<E, float>::value) || aligned16(grad_y), "hashgrid_bwd_merged: a half grad_y must be 16-byte aligned");
    const MergedPlan P = merged_plan(G, T);
    hipStream_t s = as_stream(stream);
    const dim3 block(256);
    dispatch_grid<2, 3, 4>(G, interp, [&](auto d, auto f, auto i) {
        auto kernel = hashgrid_bwd_merged_kernel<d(), f(), E, i()>;
        if (P.n_lds > 0)
            hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(G.n_points, P.min_span[0]), P.n_lds), block,
                               P.lds_floats * sizeof(float), s, x, grad_y, G.n_points, T, P, 0, 1, grad_params);
        if (P.n_lds < T.n_levels)
            hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(G.n_points, P.min_span[1]), T.n_levels - P.n_lds), block, 0, s,
                               x, grad_y, G.n_points, T, P, P.n_lds, 0, grad_params);
    });
    NFA_CHECK_LAUNCH("hashgrid_bwd_merged");
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int nfa_hashgrid_bwd_merged(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const void *grad_y, int64_t n_points,
                            int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                            const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                            nfa_stream_t stream)
{
    if (check_interp("hashgrid_bwd_merged", interp) != NFA_OK) return NFA_EINVAL;
    const GridArgs G = {n_dims, n_points, n_levels, n_features, log2_hashmap_size, scales_host, resolutions_host, sizes_host,
                        n_params};
    ELEM_DISPATCH("hashgrid_bwd_merged", elem, hashgrid_bwd_merged(interp, x, static_cast<const E *>(grad_y), G, grad_params, stream));
}

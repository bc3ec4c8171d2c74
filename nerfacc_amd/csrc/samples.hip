// samples.hip -- the glue between sampling() and a field: sample positions from ray samples, normalised to a box or
// contracted, the per-sample directions and the inside-the-box selector, in one streaming pass (samples.h has the
// formulas and what they replace).
//
// The torch composition (gather rays_o / rays_d rows, add, multiply, divide, add, then subtract, divide, compare, reduce)
// is about ten launches that move ~160-260 B per sample; the floor is 16 B in (ray index, t_start, t_end; the 24 B ray rows
// stay in cache, samples of a ray being consecutive) and 12 B out, plus 12 B for the directions and 1 B for the selector.
//
// Forward: flat over samples, no segment structure needed, so ray indices may come in any order.  A lane takes 4
// consecutive samples: one 16-byte load each of t_starts / t_ends, two of the indices, and the 48 B of four xyz rows as
// three 16-byte stores (VEC); bases that are not 16-byte aligned take the same kernel with element-wise accesses, and so
// does the quad that holds the tail.  Batched input (ray_indices NULL) derives the ray from the element index.
// Nothing is kept in LDS and the register count is low, so the launch runs at full occupancy: a pure streaming kernel.
//
// Backward towards the rays is a per-ray sum: SamplePosBwdOp of the segmented engine (segscan.hip).  The flat kernel here
// is its form without the sums, for ray indices that are not sorted (the caller reduces g_p) and for callers that only
// want the gradients of t_starts / t_ends.
#include "samples.h"

namespace nfa {

struct SampleFwdArgs {
    const float *o, *d, *ts, *te;
    const int64_t *ri;   // NULL: batched, ray = element / S
    int64_t n_rays, n, S;
    SampleBox box;
    int dirs_mode;       // 0 none, 1 raw d[r], 2 (d[r] + 1) / 2
    float *pos, *dirs;
    uint8_t *sel;
};

// o[r], d[r]; an index outside [0, n_rays) reads row 0 and yields NaN rows (never an address outside the arrays)
__device__ __forceinline__ void ray_rows(const float *__restrict__ o, const float *__restrict__ d, int64_t r, int64_t n_rays,
                                         float ro[3], float rd[3])
{
    const bool ok = (uint64_t)r < (uint64_t)n_rays;
    const int64_t b = ok ? 3 * r : 0;
    const float bad = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float vo = o[b + k], vd = d[b + k];
        ro[k] = ok ? vo : bad;
        rd[k] = ok ? vd : bad;
    }
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void sample_positions_kernel(SampleFwdArgs a)
{
    float lo[3] = {0.f, 0.f, 0.f}, ext[3] = {1.f, 1.f, 1.f};
    if (MODE != SP_NONE) box_resolve(a.box, lo, ext);
    const int64_t n_quads = (a.n + 3) / 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += stride) {
        const int64_t e = 4 * q;
        const int cnt = a.n - e >= 4 ? 4 : (int)(a.n - e);
        const bool vec = VEC && cnt == 4;   // (the tail quad of an aligned input goes element by element)
        float ts[4], te[4];
        int64_t r[4];
        if (vec) {
            const nfa_v4f s4 = *reinterpret_cast<const nfa_v4f *>(a.ts + e), e4 = *reinterpret_cast<const nfa_v4f *>(a.te + e);
            ts[0] = s4.x; ts[1] = s4.y; ts[2] = s4.z; ts[3] = s4.w;
            te[0] = e4.x; te[1] = e4.y; te[2] = e4.z; te[3] = e4.w;
            if (a.ri) {
                const nfa_v2l r01 = *reinterpret_cast<const nfa_v2l *>(a.ri + e), r23 = *reinterpret_cast<const nfa_v2l *>(a.ri + e + 2);
                r[0] = r01.x; r[1] = r01.y; r[2] = r23.x; r[3] = r23.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t i = j < cnt ? e + j : e;   // (in range: cnt >= 1)
                ts[j] = a.ts[i]; te[j] = a.te[i];
                if (a.ri) r[j] = a.ri[i];
            }
        }
        if (!a.ri) {
            int64_t r0 = e / a.S, rem = e - r0 * a.S;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = r0;
                if (++rem == a.S) { rem = 0; ++r0; }
            }
        }
        float pos[12], dirs[12];
        uint32_t inside = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float ro[3], rd[3], p[3];
            ray_rows(a.o, a.d, r[j], a.n_rays, ro, rd);
            sample_point(ro, rd, ts[j], te[j], p);
            if (MODE != SP_NONE) sample_normalise<MODE>(p, lo, ext);
            if (MODE != SP_NONE && sample_inside(p)) inside |= 1u << (8 * j);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pos[3 * j + k] = p[k];
                dirs[3 * j + k] = a.dirs_mode == 2 ? (rd[k] + 1.0f) / 2.0f : rd[k];
            }
        }
        if (a.pos) store_rows12(a.pos, e, vec, cnt, pos);
        if (a.dirs) store_rows12(a.dirs, e, vec, cnt, dirs);
        if (MODE != SP_NONE && a.sel) {
            if (vec) {
                *reinterpret_cast<uint32_t *>(a.sel + e) = inside;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) a.sel[e + j] = (uint8_t)((inside >> (8 * j)) & 1u);
            }
        }
    }
}

// One sample per lane: g_p = J^T g_x, g_t_start = g_t_end = 1/2 d[r] . g_p.
template <int MODE>
__global__ __launch_bounds__(256) void sample_positions_bwd_flat_kernel(SampleBox box, const float *__restrict__ o,
                                                                        const float *__restrict__ d, const float *__restrict__ ts,
                                                                        const float *__restrict__ te, const int64_t *__restrict__ ri,
                                                                        int64_t n_rays, int64_t n, int64_t S,
                                                                        const float *__restrict__ gx, float *__restrict__ gp,
                                                                        float *__restrict__ gts, float *__restrict__ gte)
{
    float lo[3] = {0.f, 0.f, 0.f}, ext[3] = {1.f, 1.f, 1.f};
    if (MODE != SP_NONE) box_resolve(box, lo, ext);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float ro[3], rd[3], p[3] = {0.f, 0.f, 0.f}, g[3];
        ray_rows(o, d, ri ? ri[i] : i / S, n_rays, ro, rd);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = gx[3 * i + k];
        if (MODE == SP_SPHERE || MODE == SP_CUBE) sample_point(ro, rd, ts[i], te[i], p);
        sample_grad_point<MODE>(p, lo, ext, g);
        if (gp) { gp[3 * i] = g[0]; gp[3 * i + 1] = g[1]; gp[3 * i + 2] = g[2]; }
        const float gt = 0.5f * (rd[0] * g[0] + rd[1] * g[1] + rd[2] * g[2]);
        if (gts) gts[i] = gt;
        if (gte) gte[i] = gt;
    }
}

void launch_sample_positions_bwd_flat(int mode, const SampleBox &box, const float *rays_o, const float *rays_d,
                                      const float *t_starts, const float *t_ends, const int64_t *ray_indices,
                                      int64_t n_rays, int64_t n, int64_t samples_per_ray, const float *g_positions,
                                      float *grad_p, float *grad_t_starts, float *grad_t_ends, hipStream_t s)
{
    dispatch_sample_mode(mode, [&](auto M) {
        hipLaunchKernelGGL((sample_positions_bwd_flat_kernel<decltype(M)::value>), dim3(grid_1d(n, 256)), dim3(256), 0, s, box,
                           rays_o, rays_d, t_starts, t_ends, ray_indices, n_rays, n, samples_per_ray, g_positions, grad_p,
                           grad_t_starts, grad_t_ends);
    });
}

static inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_sample_positions_fwd(const float *rays_o, const float *rays_d, const float *t_starts, const float *t_ends,
                             const int64_t *ray_indices, int64_t n_rays, int64_t n_elems, int64_t samples_per_ray,
                             const float *aabb_host, const float *aabb, int32_t contraction, int32_t dirs_mode,
                             float *positions, float *dirs, uint8_t *selector, nfa_stream_t stream)
{
    NFA_REQUIRE(n_rays >= 0 && n_elems >= 0 && samples_per_ray >= 0, "sample_positions_fwd: negative size");
    NFA_REQUIRE(n_rays < ((int64_t)1 << 31) - 64, "sample_positions_fwd: too many rays");
    NFA_REQUIRE(contraction >= 0 && contraction <= 2 && dirs_mode >= 0 && dirs_mode <= 2,
                "sample_positions_fwd: contraction and dirs_mode must be 0, 1 or 2");
    const bool has_box = aabb_host || aabb;
    NFA_REQUIRE(has_box || contraction == 0, "sample_positions_fwd: contraction needs an aabb");
    NFA_REQUIRE(has_box || !selector, "sample_positions_fwd: the selector needs an aabb");
    NFA_REQUIRE(!(aabb_host && aabb), "sample_positions_fwd: aabb given twice");
    if (n_elems == 0) return NFA_OK;
    NFA_REQUIRE(rays_o && rays_d && t_starts && t_ends && (positions || dirs || selector), "sample_positions_fwd: null pointer");
    NFA_REQUIRE((dirs != nullptr) == (dirs_mode != 0), "sample_positions_fwd: dirs and dirs_mode must be given together");
    NFA_REQUIRE(ray_indices ? n_rays >= 1 : (samples_per_ray >= 1 && n_elems == n_rays * samples_per_ray),
                "sample_positions_fwd: without ray_indices n_elems must be n_rays * samples_per_ray");
    SampleFwdArgs a;
    a.o = rays_o; a.d = rays_d; a.ts = t_starts; a.te = t_ends; a.ri = ray_indices;
    a.n_rays = n_rays; a.n = n_elems; a.S = samples_per_ray;
    for (int k = 0; k < 3; ++k) { a.box.lo[k] = aabb_host ? aabb_host[k] : 0.0f; a.box.hi[k] = aabb_host ? aabb_host[3 + k] : 1.0f; }
    a.box.dev = aabb;
    a.dirs_mode = dirs_mode; a.pos = positions; a.dirs = dirs; a.sel = selector;
    const int mode = has_box ? SP_AABB + contraction : SP_NONE;
    const bool vec = aligned_to(t_starts, 16) && aligned_to(t_ends, 16) && aligned_to(ray_indices, 16) && aligned_to(positions, 16) &&
                     aligned_to(dirs, 16) && aligned_to(selector, 4);
    const unsigned grid = grid_1d((n_elems + 3) / 4, 256);
    hipStream_t s = as_stream(stream);
    dispatch_sample_mode(mode, [&](auto M) {
        constexpr int MODE = decltype(M)::value;
        if (vec) hipLaunchKernelGGL((sample_positions_kernel<true, MODE>), dim3(grid), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((sample_positions_kernel<false, MODE>), dim3(grid), dim3(256), 0, s, a);
    });
    NFA_CHECK_LAUNCH("sample_positions_fwd");
    return NFA_OK;
}

}  // extern "C"

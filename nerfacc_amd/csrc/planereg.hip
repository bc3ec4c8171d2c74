// planereg.hip -- the regularisers K-Planes (Fridovich-Keil et al. 2023) puts on its plane tables, over the plane grid of
// planes.hip (layout: plane_layout.h): per plane (s, k), seen as p[j, i, f] with j < H = R_b rows, i < W = R_a and f < F,
//   tv_h   = sum (p[j+1,i,f] - p[j,i,f])^2 / (F (H-1) W)
//   tv_w   = sum (p[j,i+1,f] - p[j,i,f])^2 / (F H (W-1))
//   smooth = sum ((p[j+2,i,f] - p[j+1,i,f]) - (p[j+1,i,f] - p[j,i,f]))^2 / (F (H-2) W)      (0 when H = 2)
//   l1     = sum |1 - p[j,i,f]| / (F H W)
// smooth and l1 exist on the time planes only (b == 3: k = 2, 4, 5 at D = 4; the rows are the time axis); on a spatial plane
// they are 0 and their incoming gradients are not looked at.  terms[s, k, :] = (tv_h, tv_w, smooth, l1).
//
// The planes are tiled, walked and summed by plane_tiles.h, which states the tiling, the row walks and the order of every
// sum: a spatial plane with the policy (no second difference, no L1 term), a time plane with (second difference,
// |1 - p|).  planereg_fwd_kernel stores a tile's 4 sums as partials[tile] (4 waves: 6 + 3 additions after the walk's 64);
// planereg_finish_kernel, one workgroup of NFA_PR_FIN = 256 lanes per plane, adds the plane's partial rows in runs of
// NFA_PR_RUN = 256 (at most 256 + 261 additions, a plane having at most 2^24 + 2^18 tiles), then the butterfly and the 4
// waves (9), and divides by the counts: the longest chain of float32 additions a term passes through is 64 + 9 + 517 + 9 =
// 599 <= 1024; every summand is non-negative, so a term's relative error is below 600 * 2^-24 + a few ulp of its summands.
//
// Backward, planereg_bwd_kernel: plane_tiles.h's gather walk with c_t = grad_terms[s, k, t] * (float)(1 / count_t) (c_s = 0
// when H = 2), so
//   grad_params = (2 c_h) gh + (2 c_w) gw                                          on a spatial plane
//   grad_params = (((2 c_h) gh + (2 c_w) gw) + (2 c_s) gs) + c_l sg,  sg = sign(p - 1)   on a time plane
// nerfacc_amd/losses.py (_plane_terms_grad_torch) restates this in torch, bit for bit.
//
// params, partials, terms and grad_params must be 16-byte aligned (every access is a quad).
#include "common.hip.h"
#include "plane_layout.h"
#include "plane_tiles.h"

namespace nfa {

#define NFA_PR_FIN 256     // lanes of a workgroup of the finish kernel
#define NFA_PR_RUN 256     // partial rows a lane of the finish kernel adds before it starts a new run
#define NFA_PR_MAX (NFA_PG_MAX_SCALES * NFA_PG_MAX_PLANES)

struct RegPlan {
    TilePlane pl[NFA_PR_MAX];  // in table order
    uint32_t time[NFA_PR_MAX]; // rows are the time axis
    uint32_t n, F4, n_tiles;   // planes, quads per node, tiles in all
};
struct RegScale {
    float v[NFA_PR_MAX][4];    // per plane and term: the count (forward), its reciprocal (backward)
};

__global__ __launch_bounds__(NFA_PT_QUADS) void planereg_fwd_kernel(const float *__restrict__ params, const RegPlan R,
                                                                    float *__restrict__ partials)
{
    __shared__ float lds[NFA_PT_QUADS / NFA_WAVE * 4];
    const TileAt t = locate_tile(R.pl, R.n, blockIdx.x);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t.c4 < t.pl.L4) {
        const float *col = params + t.pl.offset + t.c4 * 4u;
        const bool right = t.c4 + R.F4 < t.pl.L4;
        const uint32_t L = t.pl.L4 * 4u, F = R.F4 * 4u;
        if (R.time[t.plane]) fwd_rows<true, L1Form::one_minus>(col, L, t.pl.H, t.j0, t.j1, right, F, acc[0], acc[1], acc[2], acc[3]);
        else fwd_rows<false, L1Form::none>(col, L, t.pl.H, t.j0, t.j1, right, F, acc[0], acc[1], acc[2], acc[3]);
    }
    block_sum<4, NFA_PT_QUADS / NFA_WAVE>(acc, lds);
    if (threadIdx.x == 0) store_f4(partials + (size_t)blockIdx.x * 4, acc[0], acc[1], acc[2], acc[3]);
}

__global__ __launch_bounds__(NFA_PR_FIN) void planereg_finish_kernel(const float *__restrict__ partials, const RegPlan R,
                                                                     const RegScale count, float *__restrict__ terms)
{
    __shared__ float lds[NFA_PR_FIN / NFA_WAVE * 4];
    const uint32_t p = blockIdx.x, end = p + 1 < R.n ? R.pl[p + 1].tile_first : R.n_tiles;
    const nfa_v4f s = sum_partials<NFA_PR_FIN, NFA_PR_RUN>(partials, R.pl[p].tile_first, end);
    float acc[4] = {s[0], s[1], s[2], s[3]};
    block_sum<4, NFA_PR_FIN / NFA_WAVE>(acc, lds);
    if (threadIdx.x == 0) store_f4(terms + (size_t)p * 4, acc[0] / count.v[p][0], acc[1] / count.v[p][1], acc[2] / count.v[p][2],
                                   acc[3] / count.v[p][3]);
}

__global__ __launch_bounds__(NFA_PT_QUADS) void planereg_bwd_kernel(const float *__restrict__ params, const RegPlan R,
                                                                    const RegScale inv_count, const float *__restrict__ grad_terms,
                                                                    float *__restrict__ grad_params)
{
    const TileAt t = locate_tile(R.pl, R.n, blockIdx.x);
    if (t.c4 >= t.pl.L4) return;
    float c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = grad_terms[t.plane * 4u + q] * inv_count.v[t.plane][q];
    const uint32_t at = t.pl.offset + t.c4 * 4u;
    const bool left = t.c4 >= R.F4, right = t.c4 + R.F4 < t.pl.L4;
    if (R.time[t.plane])
        bwd_rows<true, L1Form::one_minus>(params + at, grad_params + at, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, left, right, R.F4 * 4u, c);
    else bwd_rows<false, L1Form::none>(params + at, grad_params + at, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, left, right, R.F4 * 4u, c);
}

// ---------------------------------------------------------------- host side
struct RegHost {
    RegPlan plan;
    RegScale count, inv_count;
};

// The checks every entry makes, in this order: n_dims, n_features, n_scales, res_host (null; a resolution below 2; the
// size limit); then the tiling and the counts of the checked shape.
static int planereg_plan(const char *name, int32_t n_dims, int32_t n_scales, int32_t n_features, const int32_t *res_host, RegHost &h)
{
    NFA_REQUIRE(n_dims == 3 || n_dims == 4, "%s: n_dims must be 3 or 4 (got %d)", name, n_dims);
    NFA_REQUIRE(n_features == 4 || n_features == 8 || n_features == 16 || n_features == 32,
                "%s: n_features must be 4, 8, 16 or 32 (got %d)", name, n_features);
    NFA_REQUIRE(n_scales >= 1 && n_scales <= NFA_PG_MAX_SCALES, "%s: n_scales must be in 1..8 (got %d)", name, n_scales);
    PlaneGridDesc P;
    const int rc = plane_layout(name, n_dims, n_features, n_scales, res_host, P);
    if (rc != NFA_OK) return rc;
    h = {};
    const int K = n_dims == 3 ? n_planes<3>() : n_planes<4>();
    int64_t tiles = 0;   // (a plane has fewer than 2^25 tiles, a table fewer than 48 * 2^25)
    for (int s = 0; s < n_scales; ++s)
        for (int k = 0; k < K; ++k) {
            const int a = n_dims == 3 ? plane_a<3>(k) : plane_a<4>(k), b = n_dims == 3 ? plane_b<3>(k) : plane_b<4>(k);
            const int p = s * K + k;
            h.plan.pl[p] = tile_plane(P.offset[s][k], P.res[s][b], P.res[s][a], n_features, tiles);
            h.plan.time[p] = b == 3;
            double cnt[4];
            plane_counts(P.res[s][b], P.res[s][a], n_features, b == 3, b == 3, cnt);
            for (int t = 0; t < 4; ++t) term_scale(cnt[t], h.count.v[p][t], h.inv_count.v[p][t]);
        }
    h.plan.n = (uint32_t)(n_scales * K);
    h.plan.F4 = (uint32_t)n_features / 4;
    h.plan.n_tiles = (uint32_t)tiles;
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int64_t nfa_planereg_partials(int32_t n_dims, int32_t n_scales, int32_t n_features, const int32_t *res_host)
{
    RegHost h;
    if (planereg_plan("planereg_partials", n_dims, n_scales, n_features, res_host, h) != NFA_OK) return -1;
    return (int64_t)h.plan.n_tiles;
}

int nfa_planereg_fwd(int32_t n_dims, const float *params, int32_t n_scales, int32_t n_features, const int32_t *res_host,
                     float *partials, int64_t n_partials, float *terms, nfa_stream_t stream)
{
    RegHost h;
    const int rc = planereg_plan("planereg_fwd", n_dims, n_scales, n_features, res_host, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && partials && terms, "planereg_fwd: null pointer");
    NFA_REQUIRE(all_aligned16(params, partials, terms), "planereg_fwd: params, partials and terms must be 16-byte aligned");
    NFA_REQUIRE(n_partials >= (int64_t)h.plan.n_tiles, "planereg_fwd: n_partials is below nfa_planereg_partials (%lld < %lld)",
                (long long)n_partials, (long long)h.plan.n_tiles);
    hipLaunchKernelGGL(planereg_fwd_kernel, dim3(h.plan.n_tiles), dim3(NFA_PT_QUADS), 0, as_stream(stream), params, h.plan, partials);
    hipLaunchKernelGGL(planereg_finish_kernel, dim3(h.plan.n), dim3(NFA_PR_FIN), 0, as_stream(stream), partials, h.plan, h.count,
                       terms);
    NFA_CHECK_LAUNCH("planereg_fwd");
    return NFA_OK;
}

int nfa_planereg_bwd(int32_t n_dims, const float *params, int32_t n_scales, int32_t n_features, const int32_t *res_host,
                     const float *grad_terms, float *grad_params, nfa_stream_t stream)
{
    RegHost h;
    const int rc = planereg_plan("planereg_bwd", n_dims, n_scales, n_features, res_host, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && grad_terms && grad_params, "planereg_bwd: null pointer");
    NFA_REQUIRE(all_aligned16(params, grad_params), "planereg_bwd: params and grad_params must be 16-byte aligned");
    hipLaunchKernelGGL(planereg_bwd_kernel, dim3(h.plan.n_tiles), dim3(NFA_PT_QUADS), 0, as_stream(stream), params, h.plan,
                       h.inv_count, grad_terms, grad_params);
    NFA_CHECK_LAUNCH("planereg_bwd");
    return NFA_OK;
}

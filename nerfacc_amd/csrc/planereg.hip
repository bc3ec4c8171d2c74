// planereg.hip -- the regularisers K-Planes (Fridovich-Keil et al. 2023) puts on its plane tables, over the plane grid of
// planes.hip (layout: plane_layout.h): per plane (s, k), seen as p[j, i, f] with j < H = R_b rows, i < W = R_a and f < F,
//   tv_h   = sum (p[j+1,i,f] - p[j,i,f])^2 / (F (H-1) W)
//   tv_w   = sum (p[j,i+1,f] - p[j,i,f])^2 / (F H (W-1))
//   smooth = sum ((p[j+2,i,f] - p[j+1,i,f]) - (p[j+1,i,f] - p[j,i,f]))^2 / (F (H-2) W)      (0 when H = 2)
//   l1     = sum |1 - p[j,i,f]| / (F H W)
// smooth and l1 exist on the time planes only (b == 3: k = 2, 4, 5 at D = 4; the rows are the time axis); on a spatial plane
// they are 0 and their incoming gradients are not looked at.  terms[s, k, :] = (tv_h, tv_w, smooth, l1).
//
// All arithmetic is float32, every operation rounded on its own (the library builds with -ffp-contract=off).  A row of a
// plane is L = W F floats = L4 = L / 4 quads (16-byte pieces; F is a multiple of 4, so a quad never crosses a node and every
// plane starts on a quad).  A TILE is NFA_PR_ROWS = 16 consecutive rows by NFA_PR_QUADS = 256 consecutive quads of one plane
// (fewer at the plane's lower and right border); plane (s, k) has ceil(H / 16) row blocks of ceil(L4 / 256) segments, tiles
// numbered row block first, planes in table order: the tiling follows from the shape alone.  One workgroup of 256 lanes per
// tile, lane t at quad 256 seg + t of every row, so a wave-instruction loads 1 KiB of one row.
//
// Forward, planereg_fwd_kernel: a lane walks down the tile's rows j0 .. j1 - 1 with rows j, j + 1 (and j + 2 on a time
// plane) in registers: each row of the tile is loaded once, plus the halo rows j1 (and j1 + 1) and the quad F floats to the
// right (the neighbour node; the same bytes another lane loads: served by a cache).  Per row, in row order, and per float
// of the quad, in address order, each sum takes its term where the neighbour exists:
//   sum_h = sum_h + dh dh,  dh = p[j+1] - p[j]                       sum_w = sum_w + dw dw,  dw = p[i+1] - p[i]
//   sum_s = sum_s + d2 d2,  d2 = (p[j+2] - p[j+1]) - (p[j+1] - p[j]) sum_l = sum_l + |1 - p|
// (at most 64 additions per lane and sum, from 0).  The lanes' sums are added by an xor butterfly over the wave (distances
// 32, 16, .. 1: 6 additions, the same bits in every lane), the 4 waves' in wave order from the first (3 additions), and
// the tile's 4 sums are stored as partials[tile].  planereg_finish_kernel, one workgroup of 256 lanes per plane: lane t adds
// the plane's partial rows t, t + 256, .. in that order in runs of 256 (a run's sum from its first row, the runs' sums
// in run order from the first run's: at most 256 + 261 additions, a plane having at most 2^24 + 2^18 tiles), then the
// butterfly and the 4 waves as above (9), and terms = sum / (float)count, the count formed on the host in double and rounded
// once (a term without summands: 0 / 1).  No atomics: the same bits on every run, and the longest chain of float32
// additions a term passes through is 64 + 9 + 517 + 9 = 599 <= 1024; every summand is non-negative, so a term's relative
// error is below 600 * 2^-24 + a few ulp of its summands.
//
// Backward, planereg_bwd_kernel, the same tiling in gather form: element (j, i, f) reads its own value, rows j-2 .. j+2 of
// its column and the nodes i-1, i+1 of its row.  With c_t = grad_terms[s, k, t] * (float)(1 / count_t) (the reciprocal
// formed on the host in double and rounded once; c_s = 0 when H = 2), each of A, B, C below replaced by the literal 0 where a
// row or node it names does not exist:
//   gh = A - B,             A = p[j] - p[j-1],  B = p[j+1] - p[j]
//   gw = A - B,             A = p[i] - p[i-1],  B = p[i+1] - p[i]
//   gs = (A - 2 B) + C,     A = d2[j-2], B = d2[j-1], C = d2[j],  d2[m] = (p[m+2] - p[m+1]) - (p[m+1] - p[m]), 0 <= m <= H-3
//   sg = d > 0 ? 1 : d < 0 ? -1 : d,  d = p - 1                     (0 at p == 1; NaN stays NaN)
//   grad_params = (2 c_h) gh + (2 c_w) gw                                          on a spatial plane
//   grad_params = (((2 c_h) gh + (2 c_w) gw) + (2 c_s) gs) + c_l sg                on a time plane
// Every element is written with a plain 16-byte store.  nerfacc_amd/losses.py (_plane_terms_grad_torch) restates this in
// torch, bit for bit.
//
// Indices are uint32: a table holds fewer than 2^31 floats, so every float index and every tile number fits; no index
// depends on data.  params and grad_params must be 16-byte aligned (every access is a quad).
#include "common.hip.h"
#include "plane_layout.h"

namespace nfa {

#define NFA_PR_ROWS 16     // rows of a tile
#define NFA_PR_QUADS 256   // quads of a tile's row segment = lanes of a workgroup
#define NFA_PR_RUN 256     // partial rows a lane of the finish kernel adds before it starts a new run
#define NFA_PR_MAX (NFA_PG_MAX_SCALES * NFA_PG_MAX_PLANES)

struct RegPlane {
    uint32_t offset;       // first float
    uint32_t H, L4;        // rows, quads per row
    uint32_t tile_first;   // the plane's first tile
    uint32_t segs;         // tiles per row block
    uint32_t time;         // rows are the time axis
};
struct RegPlan {
    RegPlane pl[NFA_PR_MAX];   // in table order
    uint32_t n, F4, n_tiles;   // planes, quads per node, tiles in all
};
struct RegScale {
    float v[NFA_PR_MAX][4];    // per plane and term: the count (forward), its reciprocal (backward)
};

__device__ __forceinline__ nfa_v4f load_quad(const float *p) { return *reinterpret_cast<const nfa_v4f *>(p); }

// The plane of a tile, and the tile's rows [j0, j1) and quad c4 of this lane.
struct TileAt {
    RegPlane pl;
    uint32_t plane, j0, j1, c4;
};
__device__ __forceinline__ TileAt locate_tile(const RegPlan &R)
{
    TileAt t;
    const uint32_t tile = blockIdx.x;
    t.plane = 0;
    for (uint32_t q = 1; q < R.n; ++q) t.plane = tile >= R.pl[q].tile_first ? q : t.plane;
    t.pl = R.pl[t.plane];
    const uint32_t local = tile - t.pl.tile_first, rb = local / t.pl.segs, seg = local - rb * t.pl.segs;
    t.j0 = rb * NFA_PR_ROWS;
    t.j1 = min(t.j0 + NFA_PR_ROWS, t.pl.H);
    t.c4 = seg * NFA_PR_QUADS + threadIdx.x;
    return t;
}

// the 256 lanes' values, added in the fixed order of the header; valid in lane 0 of wave 0
__device__ __forceinline__ void block_sum4(float v[4], float (*lds)[4])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = v[t] + __shfl_xor(v[t], off, NFA_WAVE);
    }
    const int wave = (int)threadIdx.x / NFA_WAVE;
    if (lane_id() == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) lds[wave][t] = v[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = ((lds[0][t] + lds[1][t]) + lds[2][t]) + lds[3][t];
    }
}

template <bool TIME>
__device__ __forceinline__ void fwd_rows(const float *__restrict__ col, uint32_t L, uint32_t H, uint32_t j0, uint32_t j1, bool right,
                                         uint32_t F, float acc[4])
{
    nfa_v4f cur = load_quad(col + j0 * L);
    nfa_v4f nxt = j0 + 1 < H ? load_quad(col + (j0 + 1) * L) : cur;
#pragma unroll 4
    for (uint32_t j = j0; j < j1; ++j) {
        nfa_v4f nn = nxt;   // row j + 2: the halo of a time plane reaches one row further
        if (j + 2 < H && j + 2 <= j1 + (TIME ? 1u : 0u)) nn = load_quad(col + (j + 2) * L);
        if (right) {
            const nfa_v4f r = load_quad(col + j * L + F);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dw = r[e] - cur[e];
                acc[1] = acc[1] + dw * dw;
            }
        }
        if (j + 1 < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dh = nxt[e] - cur[e];
                acc[0] = acc[0] + dh * dh;
            }
        }
        if constexpr (TIME) {
            if (j + 2 < H) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d2 = (nn[e] - nxt[e]) - (nxt[e] - cur[e]);
                    acc[2] = acc[2] + d2 * d2;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[3] = acc[3] + fabsf(1.0f - cur[e]);
        }
        cur = nxt;
        nxt = nn;
    }
}

__global__ __launch_bounds__(NFA_PR_QUADS) void planereg_fwd_kernel(const float *__restrict__ params, const RegPlan R,
                                                                    float *__restrict__ partials)
{
    __shared__ float lds[NFA_PR_QUADS / NFA_WAVE][4];
    const TileAt t = locate_tile(R);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t.c4 < t.pl.L4) {
        const float *col = params + t.pl.offset + t.c4 * 4u;
        const bool right = t.c4 + R.F4 < t.pl.L4;
        if (t.pl.time) fwd_rows<true>(col, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, right, R.F4 * 4u, acc);
        else fwd_rows<false>(col, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, right, R.F4 * 4u, acc);
    }
    block_sum4(acc, lds);
    if (threadIdx.x == 0) store_f4(partials + (size_t)blockIdx.x * 4, acc[0], acc[1], acc[2], acc[3]);
}

__global__ __launch_bounds__(NFA_PR_QUADS) void planereg_finish_kernel(const float *__restrict__ partials, const RegPlan R,
                                                                       const RegScale count, float *__restrict__ terms)
{
    __shared__ float lds[NFA_PR_QUADS / NFA_WAVE][4];
    const uint32_t p = blockIdx.x;
    const uint32_t first = R.pl[p].tile_first, end = p + 1 < R.n ? R.pl[p + 1].tile_first : R.n_tiles;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool any = false;
    for (uint32_t run = first + threadIdx.x; run < end; run += NFA_PR_QUADS * NFA_PR_RUN) {   // (< 2^31 + 2^16: no wrap)
        const uint32_t run_end = min(end, run + NFA_PR_QUADS * NFA_PR_RUN);
        nfa_v4f s = load_quad(partials + (size_t)run * 4);
        for (uint32_t i = run + NFA_PR_QUADS; i < run_end; i += NFA_PR_QUADS) {
            const nfa_v4f v = load_quad(partials + (size_t)i * 4);
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = s[t] + v[t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = any ? acc[t] + s[t] : s[t];
        any = true;
    }
    block_sum4(acc, lds);
    if (threadIdx.x == 0) store_f4(terms + (size_t)p * 4, acc[0] / count.v[p][0], acc[1] / count.v[p][1], acc[2] / count.v[p][2],
                                   acc[3] / count.v[p][3]);
}

template <bool TIME>
__device__ __forceinline__ void bwd_rows(const float *__restrict__ col, float *__restrict__ out, uint32_t L, uint32_t H, uint32_t j0,
                                         uint32_t j1, bool left, bool right, uint32_t F, const float c[4])
{
    const float ch2 = 2.0f * c[0], cw2 = 2.0f * c[1], cs2 = 2.0f * c[2], cl = c[3];
    nfa_v4f cur = load_quad(col + j0 * L);
    nfa_v4f m1 = j0 >= 1 ? load_quad(col + (j0 - 1) * L) : cur;
    nfa_v4f m2 = TIME && j0 >= 2 ? load_quad(col + (j0 - 2) * L) : cur;
    nfa_v4f p1 = j0 + 1 < H ? load_quad(col + (j0 + 1) * L) : cur;
#pragma unroll 4
    for (uint32_t j = j0; j < j1; ++j) {
        // the row that enters the window: j + 2 on a time plane (p2), j + 2 as the next p1 on a spatial one
        nfa_v4f p2 = p1;
        if (j + 2 < H && (TIME || j + 2 <= j1)) p2 = load_quad(col + (j + 2) * L);
        const nfa_v4f lq = left ? load_quad(col + j * L - F) : cur;
        const nfa_v4f rq = right ? load_quad(col + j * L + F) : cur;
        const bool up = j >= 1, up2 = j >= 2, dn = j + 1 < H, dn2 = j + 2 < H;
        nfa_v4f g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d_m1 = cur[e] - m1[e], d_0 = p1[e] - cur[e];
            const float gh = (up ? d_m1 : 0.0f) - (dn ? d_0 : 0.0f);
            const float gw = (left ? cur[e] - lq[e] : 0.0f) - (right ? rq[e] - cur[e] : 0.0f);
            float v = ch2 * gh + cw2 * gw;
            if constexpr (TIME) {
                const float d_m2 = m1[e] - m2[e], d_p1 = p2[e] - p1[e];
                const float A = up2 ? d_m1 - d_m2 : 0.0f;
                const float B = up && dn ? d_0 - d_m1 : 0.0f;
                const float C = dn2 ? d_p1 - d_0 : 0.0f;
                const float gs = (A - 2.0f * B) + C;
                const float d = cur[e] - 1.0f;
                const float sg = d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d;
                v = (v + cs2 * gs) + cl * sg;
            }
            g[e] = v;
        }
        *reinterpret_cast<nfa_v4f *>(out + j * L) = g;
        m2 = m1;
        m1 = cur;
        cur = p1;
        p1 = p2;
    }
}

__global__ __launch_bounds__(NFA_PR_QUADS) void planereg_bwd_kernel(const float *__restrict__ params, const RegPlan R,
                                                                    const RegScale inv_count, const float *__restrict__ grad_terms,
                                                                    float *__restrict__ grad_params)
{
    const TileAt t = locate_tile(R);
    if (t.c4 >= t.pl.L4) return;
    float c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = grad_terms[t.plane * 4u + q] * inv_count.v[t.plane][q];
    const uint32_t at = t.pl.offset + t.c4 * 4u;
    const bool left = t.c4 >= R.F4, right = t.c4 + R.F4 < t.pl.L4;
    if (t.pl.time) bwd_rows<true>(params + at, grad_params + at, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, left, right, R.F4 * 4u, c);
    else bwd_rows<false>(params + at, grad_params + at, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, left, right, R.F4 * 4u, c);
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
            const int64_t H = P.res[s][b], W = P.res[s][a], L4 = W * n_features / 4;
            const int p = s * K + k;
            RegPlane &pl = h.plan.pl[p];
            pl.offset = P.offset[s][k];
            pl.H = (uint32_t)H;
            pl.L4 = (uint32_t)L4;
            pl.tile_first = (uint32_t)tiles;
            pl.segs = (uint32_t)ceil_div64(L4, NFA_PR_QUADS);
            pl.time = b == 3;
            tiles += ceil_div64(H, NFA_PR_ROWS) * pl.segs;
            const double F = n_features;
            const double cnt[4] = {F * (double)(H - 1) * (double)W, F * (double)H * (double)(W - 1),
                                   pl.time && H > 2 ? F * (double)(H - 2) * (double)W : 0.0, pl.time ? F * (double)H * (double)W : 0.0};
            for (int t = 0; t < 4; ++t) {
                h.count.v[p][t] = cnt[t] > 0.0 ? (float)cnt[t] : 1.0f;
                h.inv_count.v[p][t] = cnt[t] > 0.0 ? (float)(1.0 / cnt[t]) : 0.0f;
            }
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
    hipLaunchKernelGGL(planereg_fwd_kernel, dim3(h.plan.n_tiles), dim3(NFA_PR_QUADS), 0, as_stream(stream), params, h.plan, partials);
    hipLaunchKernelGGL(planereg_finish_kernel, dim3(h.plan.n), dim3(NFA_PR_QUADS), 0, as_stream(stream), partials, h.plan, h.count,
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
    hipLaunchKernelGGL(planereg_bwd_kernel, dim3(h.plan.n_tiles), dim3(NFA_PR_QUADS), 0, as_stream(stream), params, h.plan,
                       h.inv_count, grad_terms, grad_params);
    NFA_CHECK_LAUNCH("planereg_bwd");
    return NFA_OK;
}

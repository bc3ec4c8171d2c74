// vmreg.hip -- the regularisers TensoRF (Chen et al. 2022, `TensorVMSplit`) puts on its tables, over the VM grid of
// vmgrid.hip (layout: vm_layout.h).  Per mode, with the plane seen as p[j, i, k] (j < H = R_b rows, i < W = R_a, k < C) and
// the line as l[r, k] (r < R = R_c):
//   tv_h     = sum (p[j+1,i,k] - p[j,i,k])^2 / (C (H-1) W)          tv_line = sum (l[r+1,k] - l[r,k])^2 / (C (R-1))
//   tv_w     = sum (p[j,i+1,k] - p[j,i,k])^2 / (C H (W-1))          l1_line = sum |l[r,k]| / (C R)
//   l1_plane = sum |p[j,i,k]| / (C H W)                             ortho   = sum_{i<j} |G_ij| / (C (C-1) / 2)
//   G_ij = sum_r l[r,i] l[r,j]
// terms[m, :] = (tv_h, tv_w, l1_plane, tv_line, l1_line, ortho).  Every resolution is >= 2 and C >= 4: every count is positive.
//
// All arithmetic is float32, every operation rounded on its own (the library builds with -ffp-contract=off).  C is a
// multiple of 4, so a 16-byte quad never crosses a node and every block of the table starts on one.  The three planes are
// tiled, walked and summed by plane_tiles.h, which states the tiling, the row walks and the order of every sum, with the
// policy (no second difference, |p|).
//
// Forward, first launch, vmreg_fwd_kernel: the walk, then the tile's sums through the butterfly and the 4 waves (6 + 3
// additions after the walk's 64) are stored as partials[tile] = (sum_h, sum_w, sum_l, 0).
//
// Forward, second launch, vmreg_finish_kernel: one workgroup of NFA_VR_FIN = 512 lanes per mode.
//   Planes.  The mode's partial rows in runs of NFA_VR_RUN = 128 (a plane has at most 2^24 + 1 tiles, so at most 127 +
//     256 additions).
//   Line sums.  With the line as R C / 4 quads in address order, lane t takes the quads t, t + 512, .. in runs of 128 quads:
//     per quad and float in address order s_t = s_t + d d, d = l[r+1] - l[r] (where row r + 1 exists) and s_a = s_a + |l|,
//     a run's sums from 0, the runs' sums in run order from the first run's: 4 min(n, 128) + ceil(n / 128) - 1 additions for
//     the n = ceil(R C / 2048) quads of a lane.
//   Gram matrix, by 2 x 2 blocks: block (bi, bj), bi <= bj < C / 2, holds G_ij for i = 2 bi + u, j = 2 bj + v.  The blocks
//     are numbered row by row over the upper triangle ((0,0) (0,1) .. (0,C/2-1) (1,1) ..: 300 at C = 48, at most 1,176); lane
//     t takes the blocks t, t + 512, .. (one block up to C = 60, three at C = 96).  The 4 sums of a block stay in that lane:
//     from 0, G_ij = G_ij + l[r,i] l[r,j] for r = 0 .. R - 1 ascending (two 8-byte loads per r).  Then for (u, v) in row-major
//     order, where i < j: s_ij = G_ij > 0 ? 1 : G_ij < 0 ? -1 : G_ij (0 at 0; NaN stays NaN) is stored to signs[m, i, j] and
//     signs[m, j, i], and s_o = s_o + |G_ij| (from 0, over the lane's blocks in order: at most 12 additions); the diagonal
//     signs[m, i, i] is stored as 0 and never read.  Work is divided by pair only, never by r.
//   The line is read from an LDS copy where 4 max(R) C + 256 <= NFA_VR_LDS_BYTES = 64 KiB (the size a launch may ask for;
//     300 nodes x 48 components is 57,600 bytes; the 256 bytes hold the waves' sums; the longest of the three lines decides
//     for the launch, as in vmgrid.hip); a longer line takes the same arithmetic from global memory.
//   The six sums of the 512 lanes are added by the butterfly (6) and the 8 waves' in wave order from the first (7), and
//   terms = sum / (float)count, the count formed on the host in double and rounded once.
// No atomics anywhere: the same bits on every run.  The longest chain of float32 additions a plane term passes through is
// 64 + 9 + 383 + 13 = 469; tv_line and l1_line pass through 4 min(n, 128) + ceil(n / 128) + 12 (below 1024 for lines of up to
// 2^18 quads, 2^20 floats); ortho's sum of |G_ij| through at most 12 + 13 = 25, each G_ij itself a chain of R.
//
// Backward, vmreg_bwd_kernel, one launch in gather form: the plane tiles (plane_tiles.h's gather walk), then per mode
// ceil(R C / 1024) workgroups of 256 lanes, one line quad per lane.  With c_t = grad_terms[m, t] * (float)(1 / count_t) (the
// reciprocal formed on the host in double and rounded once), each of A, B replaced by the literal 0 where a row it names does
// not exist, and sg = plane_tiles.h's sign0:
//   plane element: grad_params = ((2 c_h) gh + (2 c_w) gw) + c_l1 sg(p)                       (gh, gw: plane_tiles.h)
//   gt = A - B,  A = l[r] - l[r-1],  B = l[r+1] - l[r]
//   go[r, i] = sum_{j != i} signs[m, i, j] l[r, j], from 0, j ascending (the term j == i is skipped, not multiplied by 0)
//   line element:  grad_params = ((2 c_tv) gt + c_l1 sg(l)) + c_o go
// Every float of grad_params is written, with plain 16-byte stores.  nerfacc_amd/losses.py (_vm_terms_grad_torch) restates
// this in torch, bit for bit.
//
// Indices are uint32: a table holds fewer than 2^31 floats, so every float index, tile and workgroup number fits; no index
// depends on data.  params, partials, signs and grad_params must be 16-byte aligned (they are accessed by quads).
#include <algorithm>

#include "common.hip.h"
#include "plane_tiles.h"
#include "vm_layout.h"

namespace nfa {

#define NFA_VR_FIN 512          // lanes of a workgroup of the finish kernel
#define NFA_VR_RUN 128          // partial rows (line quads) a lane of the finish kernel adds before it starts a new run
#define NFA_VR_LDS_BYTES 65536 // what a launch of the finish kernel may ask for: the waves' sums and the line copy
#define NFA_VR_SCRATCH 256      // bytes of the waves' sums: 8 waves x 6 floats, padded

struct VRLine {
    uint32_t offset, R;        // first float, rows
    uint32_t first;            // backward: the line's first workgroup
};
struct VRPlan {
    TilePlane pl[3];
    VRLine ln[3];
    uint32_t C4, n_tiles, n_blocks;   // quads per node, plane tiles in all, workgroups of the backward
};
struct VRScale {
    float v[3][6];   // per mode and term: the count (forward), its reciprocal (backward)
};

typedef float vr_v2f __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(NFA_PT_QUADS) void vmreg_fwd_kernel(const float *__restrict__ params, const VRPlan P,
                                                                 float *__restrict__ partials)
{
    __shared__ float lds[NFA_PT_QUADS / NFA_WAVE * 3];
    const TileAt t = locate_tile(P.pl, 3, blockIdx.x);
    float sum[3] = {0.0f, 0.0f, 0.0f}, none = 0.0f;   // (tv_h, tv_w, l1); no second difference
    if (t.c4 < t.pl.L4)
        fwd_rows<false, L1Form::abs>(params + t.pl.offset + t.c4 * 4u, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, t.c4 + P.C4 < t.pl.L4,
                                     P.C4 * 4u, sum[0], sum[1], none, sum[2]);
    block_sum<3, NFA_PT_QUADS / NFA_WAVE>(sum, lds);
    if (threadIdx.x == 0) store_f4(partials + (size_t)blockIdx.x * 4, sum[0], sum[1], sum[2], 0.0f);
}

// block `blk` of the upper triangle of an n x n block matrix, numbered row by row
__device__ __forceinline__ void vr_gram_block(uint32_t blk, uint32_t n, uint32_t &bi, uint32_t &bj)
{
    bi = 0;
    while (blk >= n - bi) {
        blk -= n - bi;
        ++bi;
    }
    bj = bi + blk;
}

template <bool LDS>
__global__ __launch_bounds__(NFA_VR_FIN) void vmreg_finish_kernel(const float *__restrict__ params, const float *__restrict__ partials,
                                                                  const VRPlan P, const VRScale count, float *__restrict__ signs,
                                                                  float *__restrict__ terms)
{
    extern __shared__ __attribute__((aligned(16))) float vr_lds[];   // the waves' sums, then (LDS) the line
    const uint32_t m = blockIdx.x, t = threadIdx.x;
    const VRLine ln_m = P.ln[m];
    const uint32_t C4 = P.C4, C = C4 * 4u, n4 = ln_m.R * C4;   // quads of the line

    // ---- the plane's partial rows
    const uint32_t tiles_end = m + 1 < 3 ? P.pl[m + 1].tile_first : P.n_tiles;
    const nfa_v4f ps = sum_partials<NFA_VR_FIN, NFA_VR_RUN>(partials, P.pl[m].tile_first, tiles_end);
    float acc[6] = {ps[0], ps[1], ps[2], 0.0f, 0.0f, 0.0f};

    // ---- the line: its copy, then every read below through `ln`
    const float *gline = params + ln_m.offset;
    float *copy = vr_lds + NFA_VR_SCRATCH / 4;
    if constexpr (LDS) {
        for (uint32_t q = t; q < n4; q += NFA_VR_FIN) *reinterpret_cast<nfa_v4f *>(copy + q * 4u) = load_quad(gline + q * 4u);
        __syncthreads();
    }
    const float *ln = LDS ? copy : gline;

    // ---- tv_line and l1_line
    {
        bool any = false;
        for (uint32_t run = t; run < n4; run += NFA_VR_FIN * NFA_VR_RUN) {   // (< 2^29 + 2^16: no wrap)
            const uint32_t run_end = min(n4, run + NFA_VR_FIN * NFA_VR_RUN);
            float st = 0.0f, sa = 0.0f;
            for (uint32_t q = run; q < run_end; q += NFA_VR_FIN) {
                const nfa_v4f v = load_quad(ln + q * 4u);
                if (q + C4 < n4) {
                    const nfa_v4f w = load_quad(ln + (q + C4) * 4u);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = w[e] - v[e];
                        st = st + d * d;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) sa = sa + fabsf(v[e]);
            }
            acc[3] = any ? acc[3] + st : st;
            acc[4] = any ? acc[4] + sa : sa;
            any = true;
        }
    }

    // ---- the Gram matrix by 2 x 2 blocks, its signs and the sum of its upper triangle
    {
        const uint32_t C2 = C4 * 2u, n_blk = C2 * (C2 + 1u) / 2u;
        float *sg = signs + m * C * C;
        for (uint32_t blk = t; blk < n_blk; blk += NFA_VR_FIN) {
            uint32_t bi, bj;
            vr_gram_block(blk, C2, bi, bj);
            float G[2][2] = {};
            const float *li = ln + bi * 2u, *lj = ln + bj * 2u;
#pragma unroll 8
            for (uint32_t r = 0; r < ln_m.R; ++r) {
                const vr_v2f a = *reinterpret_cast<const vr_v2f *>(li + r * C), b = *reinterpret_cast<const vr_v2f *>(lj + r * C);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int v = 0; v < 2; ++v) G[u][v] = G[u][v] + a[u] * b[v];
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const uint32_t i = bi * 2u + u, j = bj * 2u + v;
                    if (i < j) {
                        const float s = sign0(G[u][v]);
                        sg[i * C + j] = s;
                        sg[j * C + i] = s;
                        acc[5] = acc[5] + fabsf(G[u][v]);
                    } else if (i == j) {
                        sg[i * C + i] = 0.0f;
                    }
                }
            }
        }
    }

    block_sum<6, NFA_VR_FIN / NFA_WAVE>(acc, vr_lds);
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) terms[m * 6u + q] = acc[q] / count.v[m][q];
    }
}

__global__ __launch_bounds__(NFA_PT_QUADS) void vmreg_bwd_kernel(const float *__restrict__ params, const VRPlan P, const VRScale inv_count,
                                                                 const float *__restrict__ grad_terms, const float *__restrict__ signs,
                                                                 float *__restrict__ grad_params)
{
    const uint32_t C4 = P.C4, C = C4 * 4u;
    if (blockIdx.x < P.n_tiles) {   // ---- a plane tile
        const TileAt t = locate_tile(P.pl, 3, blockIdx.x);
        if (t.c4 >= t.pl.L4) return;
        const float *gm = grad_terms + t.plane * 6u, *ic = inv_count.v[t.plane];
        const float c[4] = {gm[0] * ic[0], gm[1] * ic[1], 0.0f, gm[2] * ic[2]};   // (c_h, c_w, none, c_l1)
        const uint32_t at = t.pl.offset + t.c4 * 4u;
        bwd_rows<false, L1Form::abs>(params + at, grad_params + at, t.pl.L4 * 4u, t.pl.H, t.j0, t.j1, t.c4 >= C4, t.c4 + C4 < t.pl.L4,
                                     C, c);
        return;
    }
    // ---- a line quad
    uint32_t m = 0;
    for (uint32_t q = 1; q < 3; ++q) m = blockIdx.x >= P.ln[q].first ? q : m;
    const VRLine ln = P.ln[m];
    const uint32_t q = (blockIdx.x - ln.first) * NFA_PT_QUADS + threadIdx.x;
    if (q >= ln.R * C4) return;
    const uint32_t r = q / C4, c4 = q - r * C4;
    const float ct = grad_terms[m * 6u + 3] * inv_count.v[m][3], cl = grad_terms[m * 6u + 4] * inv_count.v[m][4],
                co = grad_terms[m * 6u + 5] * inv_count.v[m][5];
    const float ct2 = 2.0f * ct;
    const float *row = params + ln.offset + r * C;
    const nfa_v4f cur = load_quad(row + c4 * 4u);
    const bool up = r >= 1, dn = r + 1 < ln.R;
    const nfa_v4f m1 = up ? load_quad(row + c4 * 4u - C) : cur, p1 = dn ? load_quad(row + c4 * 4u + C) : cur;
    const float *sg = signs + (m * C + c4 * 4u) * C;   // rows i = 4 c4 .. 4 c4 + 3 of the mode's signs
    float go[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t j4 = 0; j4 < C4; ++j4) {
        const nfa_v4f lj = load_quad(row + j4 * 4u);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const nfa_v4f s = load_quad(sg + e * C + j4 * 4u);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (j4 != c4 || v != e) go[e] = go[e] + s[v] * lj[v];
            }
        }
    }
    nfa_v4f g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gt = (up ? cur[e] - m1[e] : 0.0f) - (dn ? p1[e] - cur[e] : 0.0f);
        g[e] = (ct2 * gt + cl * sign0(cur[e])) + co * go[e];
    }
    *reinterpret_cast<nfa_v4f *>(grad_params + ln.offset + q * 4u) = g;
}

// ---------------------------------------------------------------- host side
struct VRHost {
    VRPlan plan;
    VRScale count, inv_count;
};

// The checks every entry makes, in this order: n_components; res_host (null; an axis below 2; the size limit); then the
// tiling and the counts of the checked shape.
static int vmreg_plan(const char *name, int32_t C, const int32_t *res_host, VRHost &h)
{
    int rc = vm_check_c(name, C);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(res_host != nullptr, "%s: null resolution table", name);
    VMDesc V;
    int64_t total;
    if ((rc = vm_layout(name, "", C, res_host, V, total)) != NFA_OK) return rc;
    h = {};
    int64_t tiles = 0;
    for (int m = 0; m < 3; ++m) {
        const int64_t W = V.res[vm_a(m)], H = V.res[vm_b(m)], R = V.res[vm_c(m)];
        h.plan.pl[m] = tile_plane(V.plane[m], H, W, C, tiles);   // (a plane has at most 2^24 + 1 tiles)
        h.plan.ln[m].offset = V.line[m];
        h.plan.ln[m].R = (uint32_t)R;
        double pc[4];
        plane_counts(H, W, C, false, true, pc);
        const double c = C, cnt[6] = {pc[0], pc[1], pc[3], c * (double)(R - 1), c * (double)R, c * (c - 1.0) / 2.0};
        for (int t = 0; t < 6; ++t) term_scale(cnt[t], h.count.v[m][t], h.inv_count.v[m][t]);
    }
    h.plan.C4 = (uint32_t)C / 4;
    h.plan.n_tiles = (uint32_t)tiles;
    int64_t blocks = tiles;
    for (int m = 0; m < 3; ++m) {
        h.plan.ln[m].first = (uint32_t)blocks;
        blocks += ceil_div64((int64_t)h.plan.ln[m].R * (C / 4), NFA_PT_QUADS);   // (at most 2^21 per line)
    }
    h.plan.n_blocks = (uint32_t)blocks;
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int64_t nfa_vmreg_partials(int32_t n_components, const int32_t *res_host)
{
    VRHost h;
    if (vmreg_plan("vmreg_partials", n_components, res_host, h) != NFA_OK) return -1;
    return (int64_t)h.plan.n_tiles;
}

int nfa_vmreg_fwd(const float *params, int32_t n_components, const int32_t *res_host, float *partials, int64_t n_partials,
                  float *signs, float *terms, nfa_stream_t stream)
{
    VRHost h;
    const int rc = vmreg_plan("vmreg_fwd", n_components, res_host, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && partials && signs && terms, "vmreg_fwd: null pointer");
    NFA_REQUIRE(all_aligned16(params, partials, signs), "vmreg_fwd: params, partials and signs must be 16-byte aligned");
    NFA_REQUIRE(n_partials >= (int64_t)h.plan.n_tiles, "vmreg_fwd: n_partials is below nfa_vmreg_partials (%lld < %lld)",
                (long long)n_partials, (long long)h.plan.n_tiles);
    hipLaunchKernelGGL(vmreg_fwd_kernel, dim3(h.plan.n_tiles), dim3(NFA_PT_QUADS), 0, as_stream(stream), params, h.plan, partials);
    // one launch for the three modes: the line copy only if every mode's line fits
    int64_t line_bytes = 0;
    for (int m = 0; m < 3; ++m) line_bytes = std::max<int64_t>(line_bytes, (int64_t)h.plan.ln[m].R * n_components * 4);
    const bool lds = line_bytes + NFA_VR_SCRATCH <= NFA_VR_LDS_BYTES;
    dispatch_bool(lds, [&](auto use_lds) {
        hipLaunchKernelGGL((vmreg_finish_kernel<use_lds()>), dim3(3), dim3(NFA_VR_FIN), (size_t)(NFA_VR_SCRATCH + (lds ? line_bytes : 0)),
                           as_stream(stream), params, partials, h.plan, h.count, signs, terms);
    });
    NFA_CHECK_LAUNCH("vmreg_fwd");
    return NFA_OK;
}

int nfa_vmreg_bwd(const float *params, int32_t n_components, const int32_t *res_host, const float *grad_terms, const float *signs,
                  float *grad_params, nfa_stream_t stream)
{
    VRHost h;
    const int rc = vmreg_plan("vmreg_bwd", n_components, res_host, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && grad_terms && signs && grad_params, "vmreg_bwd: null pointer");
    NFA_REQUIRE(all_aligned16(params, signs, grad_params), "vmreg_bwd: params, signs and grad_params must be 16-byte aligned");
    hipLaunchKernelGGL(vmreg_bwd_kernel, dim3(h.plan.n_blocks), dim3(NFA_PT_QUADS), 0, as_stream(stream), params, h.plan, h.inv_count,
                       grad_terms, signs, grad_params);
    NFA_CHECK_LAUNCH("vmreg_bwd");
    return NFA_OK;
}

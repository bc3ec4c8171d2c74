// vmreg.hip -- the regularisers TensoRF (Chen et al. 2022, `TensorVMSplit`) puts on its tables, over the VM grid of
// vmgrid.hip (the same layout: for mode m = 0, 1, 2 with axes (a, b, c) = (0,1,2) (0,2,1) (1,2,0) the plane, a row-major
// [R_b, R_a, C] block, then the line, a [R_c, C] block, without gaps).  Per mode, with the plane seen as p[j, i, k] (j < H =
// R_b rows, i < W = R_a, k < C) and the line as l[r, k] (r < R = R_c):
//   tv_h     = sum (p[j+1,i,k] - p[j,i,k])^2 / (C (H-1) W)          tv_line = sum (l[r+1,k] - l[r,k])^2 / (C (R-1))
//   tv_w     = sum (p[j,i+1,k] - p[j,i,k])^2 / (C H (W-1))          l1_line = sum |l[r,k]| / (C R)
//   l1_plane = sum |p[j,i,k]| / (C H W)                             ortho   = sum_{i<j} |G_ij| / (C (C-1) / 2)
//   G_ij = sum_r l[r,i] l[r,j]
// terms[m, :] = (tv_h, tv_w, l1_plane, tv_line, l1_line, ortho).  Every resolution is >= 2 and C >= 4: every count is positive.
//
// All arithmetic is float32, every operation rounded on its own (the library builds with -ffp-contract=off).  C is a
// multiple of 4, so a 16-byte quad never crosses a node and every block of the table starts on one; a row of a plane is
// L4 = W C / 4 quads.  The planes are tiled as planereg.hip tiles its planes: a TILE is NFA_VR_ROWS = 16 consecutive rows by
// NFA_VR_QUADS = 256 consecutive quads (fewer at the lower and right border); mode m's plane has ceil(H / 16) row blocks of
// ceil(L4 / 256) segments, tiles numbered row block first, modes in order.  One workgroup of 256 lanes per tile, lane t at
// quad 256 seg + t of every row, so a wave-instruction loads 1 KiB of one row.
//
// Forward, first launch, vmreg_fwd_kernel: a lane walks down the tile's rows j0 .. j1 - 1 with rows j and j + 1 in registers:
// each row of the tile is loaded once, plus the halo row j1 and the quad C floats to the right (the neighbour node; the same
// bytes another lane loads: served by a cache).  Per row, in row order, and per float of the quad, in address order:
//   sum_w = sum_w + dw dw, dw = p[i+1] - p[i]   (where node i + 1 exists)
//   sum_h = sum_h + dh dh, dh = p[j+1] - p[j]   (where row j + 1 exists)
//   sum_l = sum_l + |p|
// (at most 64 additions per lane and sum, from 0).  The lanes' sums are added by an xor butterfly over the wave (distances
// 32, 16, .. 1: 6 additions, the same bits in every lane), the waves' sums in wave order from the first (3 additions), and the
// tile's sums are stored as partials[tile] = (sum_h, sum_w, sum_l, 0).
//
// Forward, second launch, vmreg_finish_kernel: one workgroup of NFA_VR_FIN = 512 lanes per mode.
//   Planes.  Lane t adds the mode's partial rows t, t + 512, .. in that order in runs of NFA_VR_RUN = 128 (a run's sum from
//     its first row, the runs' sums in run order from the first run's: a plane has at most 2^24 + 1 tiles, so at most 127 +
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
// Backward, vmreg_bwd_kernel, one launch in gather form: the plane tiles as above, then per mode ceil(R C / 1024) workgroups
// of 256 lanes, one line quad per lane.  With c_t = grad_terms[m, t] * (float)(1 / count_t) (the reciprocal formed on the
// host in double and rounded once), each of A, B replaced by the literal 0 where a row or node it names does not exist, and
// sg(v) = v > 0 ? 1 : v < 0 ? -1 : v:
//   gh = A - B,  A = p[j] - p[j-1],  B = p[j+1] - p[j]              gw = A - B,  A = p[i] - p[i-1],  B = p[i+1] - p[i]
//   plane element: grad_params = ((2 c_h) gh + (2 c_w) gw) + c_l1 sg(p)
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

namespace nfa {

#define NFA_VR_ROWS 16         // rows of a tile
#define NFA_VR_QUADS 256        // quads of a tile's row segment = lanes of a workgroup of the plane and backward kernels
#define NFA_VR_FIN 512          // lanes of a workgroup of the finish kernel
#define NFA_VR_RUN 128          // partial rows (line quads) a lane of the finish kernel adds before it starts a new run
#define NFA_VR_LDS_BYTES 65536 // what a launch of the finish kernel may ask for: the waves' sums and the line copy
#define NFA_VR_SCRATCH 256      // bytes of the waves' sums: 8 waves x 6 floats, padded

struct VRMode {
    uint32_t plane, line;      // first float of the plane and of the line
    uint32_t H, L4, R;         // plane rows, quads per plane row, line rows
    uint32_t tile_first, segs; // the plane's first tile, tiles per row block
    uint32_t line_first;       // backward: the line's first workgroup
};
struct VRPlan {
    VRMode md[3];
    uint32_t C4, n_tiles, n_blocks;   // quads per node, plane tiles in all, workgroups of the backward
};
struct VRScale {
    float v[3][6];   // per mode and term: the count (forward), its reciprocal (backward)
};

typedef float vr_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ nfa_v4f vr_load(const float *p) { return *reinterpret_cast<const nfa_v4f *>(p); }
__device__ __forceinline__ float vr_sign(float v) { return v > 0.0f ? 1.0f : v < 0.0f ? -1.0f : v; }

// The mode of a plane tile, and the tile's rows [j0, j1) and quad c4 of this lane.
struct VRTile {
    VRMode md;
    uint32_t mode, j0, j1, c4;
};
__device__ __forceinline__ VRTile vr_locate_tile(const VRPlan &P, uint32_t tile)
{
    VRTile t;
    t.mode = 0;
    for (uint32_t q = 1; q < 3; ++q) t.mode = tile >= P.md[q].tile_first ? q : t.mode;
    t.md = P.md[t.mode];
    const uint32_t local = tile - t.md.tile_first, rb = local / t.md.segs, seg = local - rb * t.md.segs;
    t.j0 = rb * NFA_VR_ROWS;
    t.j1 = min(t.j0 + NFA_VR_ROWS, t.md.H);
    t.c4 = seg * NFA_VR_QUADS + threadIdx.x;
    return t;
}

// the N values of every lane of a workgroup of WAVES waves, added in the fixed order of the header; valid in lane 0 of wave 0
template <int N, int WAVES>
__device__ __forceinline__ void vr_block_sum(float (&v)[N], float *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int t = 0; t < N; ++t) v[t] = v[t] + __shfl_xor(v[t], off, NFA_WAVE);
    }
    const int wave = (int)threadIdx.x / NFA_WAVE;
    if (lane_id() == 0) {
#pragma unroll
        for (int t = 0; t < N; ++t) lds[wave * N + t] = v[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < N; ++t) {
            float s = lds[t];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s = s + lds[w * N + t];
            v[t] = s;
        }
    }
}

__global__ __launch_bounds__(NFA_VR_QUADS) void vmreg_fwd_kernel(const float *__restrict__ params, const VRPlan P,
                                                                 float *__restrict__ partials)
{
    __shared__ float lds[NFA_VR_QUADS / NFA_WAVE * 3];
    const VRTile t = vr_locate_tile(P, blockIdx.x);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (t.c4 < t.md.L4) {
        const uint32_t L = t.md.L4 * 4u, C = P.C4 * 4u, H = t.md.H;
        const float *col = params + t.md.plane + t.c4 * 4u;
        const bool right = t.c4 + P.C4 < t.md.L4;
        nfa_v4f cur = vr_load(col + t.j0 * L);
#pragma unroll 4
        for (uint32_t j = t.j0; j < t.j1; ++j) {
            const nfa_v4f nxt = j + 1 < H ? vr_load(col + (j + 1) * L) : cur;
            if (right) {
                const nfa_v4f r = vr_load(col + j * L + C);
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
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[2] = acc[2] + fabsf(cur[e]);
            cur = nxt;
        }
    }
    vr_block_sum<3, NFA_VR_QUADS / NFA_WAVE>(acc, lds);
    if (threadIdx.x == 0) store_f4(partials + (size_t)blockIdx.x * 4, acc[0], acc[1], acc[2], 0.0f);
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
    const VRMode md = P.md[m];
    const uint32_t C4 = P.C4, C = C4 * 4u, n4 = md.R * C4;   // quads of the line
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

    // ---- the plane's partial rows
    {
        const uint32_t first = md.tile_first, end = m + 1 < 3 ? P.md[m + 1].tile_first : P.n_tiles;
        bool any = false;
        for (uint32_t run = first + t; run < end; run += NFA_VR_FIN * NFA_VR_RUN) {   // (< 2^25 + 2^16: no wrap)
            const uint32_t run_end = min(end, run + NFA_VR_FIN * NFA_VR_RUN);
            nfa_v4f s = vr_load(partials + (size_t)run * 4);
            for (uint32_t i = run + NFA_VR_FIN; i < run_end; i += NFA_VR_FIN) {
                const nfa_v4f v = vr_load(partials + (size_t)i * 4);
#pragma unroll
                for (int q = 0; q < 3; ++q) s[q] = s[q] + v[q];
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = any ? acc[q] + s[q] : s[q];
            any = true;
        }
    }

    // ---- the line: its copy, then every read below through `ln`
    const float *gline = params + md.line;
    float *copy = vr_lds + NFA_VR_SCRATCH / 4;
    if constexpr (LDS) {
        for (uint32_t q = t; q < n4; q += NFA_VR_FIN) *reinterpret_cast<nfa_v4f *>(copy + q * 4u) = vr_load(gline + q * 4u);
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
                const nfa_v4f v = vr_load(ln + q * 4u);
                if (q + C4 < n4) {
                    const nfa_v4f w = vr_load(ln + (q + C4) * 4u);
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
            for (uint32_t r = 0; r < md.R; ++r) {
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
                        const float s = vr_sign(G[u][v]);
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

    vr_block_sum<6, NFA_VR_FIN / NFA_WAVE>(acc, vr_lds);
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) terms[m * 6u + q] = acc[q] / count.v[m][q];
    }
}

__device__ __forceinline__ void vr_bwd_plane(const float *__restrict__ col, float *__restrict__ out, uint32_t L, uint32_t H, uint32_t j0,
                                             uint32_t j1, bool left, bool right, uint32_t C, float ch2, float cw2, float cl)
{
    nfa_v4f cur = vr_load(col + j0 * L);
    nfa_v4f m1 = j0 >= 1 ? vr_load(col + (j0 - 1) * L) : cur;
#pragma unroll 4
    for (uint32_t j = j0; j < j1; ++j) {
        const bool up = j >= 1, dn = j + 1 < H;
        const nfa_v4f p1 = dn ? vr_load(col + (j + 1) * L) : cur;
        const nfa_v4f lq = left ? vr_load(col + j * L - C) : cur;
        const nfa_v4f rq = right ? vr_load(col + j * L + C) : cur;
        nfa_v4f g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gh = (up ? cur[e] - m1[e] : 0.0f) - (dn ? p1[e] - cur[e] : 0.0f);
            const float gw = (left ? cur[e] - lq[e] : 0.0f) - (right ? rq[e] - cur[e] : 0.0f);
            g[e] = (ch2 * gh + cw2 * gw) + cl * vr_sign(cur[e]);
        }
        *reinterpret_cast<nfa_v4f *>(out + j * L) = g;
        m1 = cur;
        cur = p1;
    }
}

__global__ __launch_bounds__(NFA_VR_QUADS) void vmreg_bwd_kernel(const float *__restrict__ params, const VRPlan P, const VRScale inv_count,
                                                                 const float *__restrict__ grad_terms, const float *__restrict__ signs,
                                                                 float *__restrict__ grad_params)
{
    const uint32_t C4 = P.C4, C = C4 * 4u;
    if (blockIdx.x < P.n_tiles) {   // ---- a plane tile
        const VRTile t = vr_locate_tile(P, blockIdx.x);
        if (t.c4 >= t.md.L4) return;
        const float ch = grad_terms[t.mode * 6u + 0] * inv_count.v[t.mode][0], cw = grad_terms[t.mode * 6u + 1] * inv_count.v[t.mode][1],
                    cl = grad_terms[t.mode * 6u + 2] * inv_count.v[t.mode][2];
        const uint32_t at = t.md.plane + t.c4 * 4u;
        vr_bwd_plane(params + at, grad_params + at, t.md.L4 * 4u, t.md.H, t.j0, t.j1, t.c4 >= C4, t.c4 + C4 < t.md.L4, C, 2.0f * ch,
                     2.0f * cw, cl);
        return;
    }
    // ---- a line quad
    uint32_t m = 0;
    for (uint32_t q = 1; q < 3; ++q) m = blockIdx.x >= P.md[q].line_first ? q : m;
    const VRMode md = P.md[m];
    const uint32_t q = (blockIdx.x - md.line_first) * NFA_VR_QUADS + threadIdx.x;
    if (q >= md.R * C4) return;
    const uint32_t r = q / C4, c4 = q - r * C4;
    const float ct = grad_terms[m * 6u + 3] * inv_count.v[m][3], cl = grad_terms[m * 6u + 4] * inv_count.v[m][4],
                co = grad_terms[m * 6u + 5] * inv_count.v[m][5];
    const float ct2 = 2.0f * ct;
    const float *row = params + md.line + r * C;
    const nfa_v4f cur = vr_load(row + c4 * 4u);
    const bool up = r >= 1, dn = r + 1 < md.R;
    const nfa_v4f m1 = up ? vr_load(row + c4 * 4u - C) : cur, p1 = dn ? vr_load(row + c4 * 4u + C) : cur;
    const float *sg = signs + (m * C + c4 * 4u) * C;   // rows i = 4 c4 .. 4 c4 + 3 of the mode's signs
    float go[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t j4 = 0; j4 < C4; ++j4) {
        const nfa_v4f lj = vr_load(row + j4 * 4u);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const nfa_v4f s = vr_load(sg + e * C + j4 * 4u);
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
        g[e] = (ct2 * gt + cl * vr_sign(cur[e])) + co * go[e];
    }
    *reinterpret_cast<nfa_v4f *>(grad_params + md.line + q * 4u) = g;
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
    NFA_REQUIRE(C >= 4 && C <= 96 && C % 4 == 0, "%s: n_components must be a multiple of 4 in 4..96 (got %d)", name, C);
    NFA_REQUIRE(res_host != nullptr, "%s: null resolution table", name);
    for (int d = 0; d < 3; ++d) NFA_REQUIRE(res_host[d] >= 2, "%s: axis %d resolution %d is below 2", name, d, res_host[d]);
    h = {};
    const int64_t limit = (int64_t)1 << 31;
    const int axes[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};   // (a, b, c) per mode, as vmgrid.hip
    int64_t total = 0, tiles = 0;
    for (int m = 0; m < 3; ++m) {
        const int64_t W = res_host[axes[m][0]], H = res_host[axes[m][1]], R = res_host[axes[m][2]];
        const int64_t cells = W * H + R;   // (< 2^62 + 2^31)
        NFA_REQUIRE(cells < limit && total + cells * C < limit, "%s: too many parameters (at most 2^31 - 1 floats)", name);
        VRMode &md = h.plan.md[m];
        md.plane = (uint32_t)total;
        md.line = (uint32_t)(total + W * H * C);
        total += cells * C;
        const int64_t L4 = W * C / 4;
        md.H = (uint32_t)H;
        md.L4 = (uint32_t)L4;
        md.R = (uint32_t)R;
        md.tile_first = (uint32_t)tiles;
        md.segs = (uint32_t)ceil_div64(L4, NFA_VR_QUADS);
        tiles += ceil_div64(H, NFA_VR_ROWS) * md.segs;   // (a plane has at most 2^24 + 1 tiles)
        const double c = C;
        const double cnt[6] = {c * (double)(H - 1) * (double)W, c * (double)H * (double)(W - 1), c * (double)H * (double)W,
                               c * (double)(R - 1),             c * (double)R,                   c * (c - 1.0) / 2.0};
        for (int t = 0; t < 6; ++t) {
            h.count.v[m][t] = (float)cnt[t];
            h.inv_count.v[m][t] = (float)(1.0 / cnt[t]);
        }
    }
    h.plan.C4 = (uint32_t)C / 4;
    h.plan.n_tiles = (uint32_t)tiles;
    int64_t blocks = tiles;
    for (int m = 0; m < 3; ++m) {
        h.plan.md[m].line_first = (uint32_t)blocks;
        blocks += ceil_div64((int64_t)h.plan.md[m].R * (C / 4), NFA_VR_QUADS);   // (at most 2^21 per line)
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
    hipLaunchKernelGGL(vmreg_fwd_kernel, dim3(h.plan.n_tiles), dim3(NFA_VR_QUADS), 0, as_stream(stream), params, h.plan, partials);
    // one launch for the three modes: the line copy only if every mode's line fits
    int64_t line_bytes = 0;
    for (int m = 0; m < 3; ++m) line_bytes = std::max<int64_t>(line_bytes, (int64_t)h.plan.md[m].R * n_components * 4);
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
    hipLaunchKernelGGL(vmreg_bwd_kernel, dim3(h.plan.n_blocks), dim3(NFA_VR_QUADS), 0, as_stream(stream), params, h.plan, h.inv_count,
                       grad_terms, signs, grad_params);
    NFA_CHECK_LAUNCH("vmreg_bwd");
    return NFA_OK;
}

// plane_tiles.h -- the tile engine of the plane regularisers: planereg.hip (K-Planes' plane grid) and vmreg.hip (the planes of
// TensoRF's VM grid) tile their planes, walk a tile's rows and add the tiles' sums with this one copy.  Each file's header
// states its own terms; the tiling, the two row walks and the order of every sum are stated here.
//
// A plane is p[j, i, f], j < H rows, i < W nodes, f < F floats per node (F a multiple of 4), row-major at `offset` of one
// flat float32 table.  All arithmetic is float32, every operation rounded on its own (the library builds with
// -ffp-contract=off).  A row is L = W F floats = L4 = L / 4 quads (16-byte pieces: a quad never crosses a node and every
// plane starts on a quad).  A TILE is NFA_PT_ROWS = 16 consecutive rows by NFA_PT_QUADS = 256 consecutive quads of one plane
// (fewer at the plane's lower and right border); a plane has ceil(H / 16) row blocks of ceil(L4 / 256) segments, tiles
// numbered row block first, planes in table order: the tiling follows from the shape alone.  One workgroup of 256 lanes per
// tile, lane t at quad 256 seg + t of every row, so a wave-instruction loads 1 KiB of one row.
//
// A walk is compiled per POLICY, two switches:
//   SECOND  the second difference along the rows (K-Planes' time planes only);
//   L1Form  none (a K-Planes spatial plane), one_minus: |1 - p| with sign(p - 1) (a K-Planes time plane), abs: |p| with
//           sign(p) (VM), where sign(d) = d > 0 ? 1 : d < 0 ? -1 : d (0 at 0; NaN stays NaN).
//
// Forward, fwd_rows: a lane walks down the tile's rows j0 .. j1 - 1 with rows j, j + 1 (and j + 2 with SECOND) in registers:
// each row of the tile is loaded once, plus the halo rows j1 (and j1 + 1) and the quad F floats to the right (the neighbour
// node; the same bytes another lane loads: served by a cache).  Per row, in row order, and per float of the quad, in address
// order, each sum takes its term where the neighbour exists:
//   sh = sh + dh dh,  dh = p[j+1] - p[j]                        sw = sw + dw dw,  dw = p[i+1] - p[i]
//   ss = ss + d2 d2,  d2 = (p[j+2] - p[j+1]) - (p[j+1] - p[j])  sl = sl + |1 - p|  or  + |p|
// (at most 64 additions per lane and sum, from the caller's 0; a sum the policy leaves out is not touched).  block_sum<N, WAVES> adds the lanes'
// sums by an xor butterfly over the wave (distances 32, 16, .. 1: 6 additions, the same bits in every lane), then the waves'
// in wave order from the first (WAVES - 1 additions); the caller stores the tile's sums as one quad, partials[tile].
// sum_partials<LANES, RUN>, in a finish kernel of LANES lanes per plane: lane t adds the plane's partial rows t, t + LANES,
// .. in that order in runs of RUN (a run's sum from its first row, the runs' sums in run order from the first run's), then
// block_sum again, and terms = sum / (float)count.  term_scale forms a count on the host in double and rounds it once (a
// term without summands: 0 / 1).  No atomics: the same bits on every run; every summand is non-negative.
//
// Backward, bwd_rows, the same tiling in gather form: element (j, i, f) reads its own value, rows j-1, j+1 (j-2 .. j+2 with
// SECOND) of its column and the nodes i-1, i+1 of its row.  With c = (c_h, c_w, c_s, c_l), c_t = grad_terms[.., t] *
// (float)(1 / count_t) (term_scale's reciprocal, formed in double and rounded once; 0 for a term without summands), each of
// A, B, C below replaced by the literal 0 where a row or node it names does not exist:
//   gh = A - B,             A = p[j] - p[j-1],  B = p[j+1] - p[j]
//   gw = A - B,             A = p[i] - p[i-1],  B = p[i+1] - p[i]
//   gs = (A - 2 B) + C,     A = d2[j-2], B = d2[j-1], C = d2[j],  d2[m] = (p[m+2] - p[m+1]) - (p[m+1] - p[m]), 0 <= m <= H-3
//   g  = (2 c_h) gh + (2 c_w) gw,  then with SECOND  g = g + (2 c_s) gs,  then with an L1 form  g = g + c_l sign(p - 1 or p)
// Every element is written with a plain 16-byte store.
//
// Indices are uint32: a table holds fewer than 2^31 floats, so every float index and every tile number fits; no index
// depends on data.  The tables must be 16-byte aligned (every access is a quad).
#pragma once
#include "common.hip.h"

namespace nfa {

#define NFA_PT_ROWS 16     // rows of a tile
#define NFA_PT_QUADS 256   // quads of a tile's row segment = lanes of a workgroup of the walks

struct TilePlane {
    uint32_t offset;       // first float
    uint32_t H, L4;        // rows, quads per row
    uint32_t tile_first;   // the plane's first tile
    uint32_t segs;         // tiles per row block
};

enum class L1Form { none, one_minus, abs };

__device__ __forceinline__ nfa_v4f load_quad(const float *p) { return *reinterpret_cast<const nfa_v4f *>(p); }
__device__ __forceinline__ float sign0(float v) { return v > 0.0f ? 1.0f : v < 0.0f ? -1.0f : v; }

// The plane of a tile among the n planes of a table, and the tile's rows [j0, j1) and quad c4 of this lane.
struct TileAt {
    TilePlane pl;
    uint32_t plane, j0, j1, c4;
};
template <int MAX>
__device__ __forceinline__ TileAt locate_tile(const TilePlane (&pl)[MAX], uint32_t n, uint32_t tile)
{
    TileAt t;
    t.plane = 0;
    for (uint32_t q = 1; q < n; ++q) t.plane = tile >= pl[q].tile_first ? q : t.plane;
    t.pl = pl[t.plane];
    const uint32_t local = tile - t.pl.tile_first, rb = local / t.pl.segs, seg = local - rb * t.pl.segs;
    t.j0 = rb * NFA_PT_ROWS;
    t.j1 = min(t.j0 + NFA_PT_ROWS, t.pl.H);
    t.c4 = seg * NFA_PT_QUADS + threadIdx.x;
    return t;
}

// the N values of every lane of a workgroup of WAVES waves, added in the fixed order of the header; valid in lane 0 of wave 0
template <int N, int WAVES>
__device__ __forceinline__ void block_sum(float (&v)[N], float *lds)
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

// this lane's share of the partial rows [first, end): rows first + t, first + t + LANES, .. in runs of RUN
template <int LANES, int RUN>
__device__ __forceinline__ nfa_v4f sum_partials(const float *__restrict__ partials, uint32_t first, uint32_t end)
{
    nfa_v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    bool any = false;
    for (uint32_t run = first + threadIdx.x; run < end; run += LANES * RUN) {   // (< 2^31 + 2^16: no wrap)
        const uint32_t run_end = min(end, run + LANES * RUN);
        nfa_v4f s = load_quad(partials + (size_t)run * 4);
        for (uint32_t i = run + LANES; i < run_end; i += LANES) s = s + load_quad(partials + (size_t)i * 4);
        acc = any ? acc + s : s;
        any = true;
    }
    return acc;
}

// adds this lane's column over the rows [j0, j1) to the sums of tv_h, tv_w, smooth and l1 (the policy's terms only)
template <bool SECOND, L1Form L1>
__device__ __forceinline__ void fwd_rows(const float *__restrict__ col, uint32_t L, uint32_t H, uint32_t j0, uint32_t j1, bool right,
                                         uint32_t F, float &sh, float &sw, float &ss, float &sl)
{
    // the row that enters the window in a step: j + 2 with SECOND (row j + 1 was loaded a step ahead), j + 1 without
    constexpr uint32_t A = SECOND ? 2 : 1;
    nfa_v4f cur = load_quad(col + j0 * L), ahead = cur;
    if constexpr (SECOND) ahead = j0 + 1 < H ? load_quad(col + (j0 + 1) * L) : cur;
#pragma unroll 4
    for (uint32_t j = j0; j < j1; ++j) {
        const nfa_v4f in = j + A < H ? load_quad(col + (j + A) * L) : SECOND ? ahead : cur;
        const nfa_v4f nxt = SECOND ? ahead : in, nn = in;   // rows j + 1 and (SECOND) j + 2
        if (right) {
            const nfa_v4f r = load_quad(col + j * L + F);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dw = r[e] - cur[e];
                sw = sw + dw * dw;
            }
        }
        if (j + 1 < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dh = nxt[e] - cur[e];
                sh = sh + dh * dh;
            }
        }
        if constexpr (SECOND) {
            if (j + 2 < H) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d2 = (nn[e] - nxt[e]) - (nxt[e] - cur[e]);
                    ss = ss + d2 * d2;
                }
            }
        }
        if constexpr (L1 != L1Form::none) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sl = sl + fabsf(L1 == L1Form::one_minus ? 1.0f - cur[e] : cur[e]);
        }
        cur = nxt;
        ahead = in;
    }
}

template <bool SECOND, L1Form L1>
__device__ __forceinline__ void bwd_rows(const float *__restrict__ col, float *__restrict__ out, uint32_t L, uint32_t H, uint32_t j0,
                                         uint32_t j1, bool left, bool right, uint32_t F, const float (&c)[4])
{
    const float ch2 = 2.0f * c[0], cw2 = 2.0f * c[1], cs2 = 2.0f * c[2], cl = c[3];
    // the row that enters the window in a step: j + 2 with SECOND (row j + 1 is loaded ahead), j + 1 without
    nfa_v4f cur = load_quad(col + j0 * L), m2 = cur, p1 = cur, p2 = cur;
    nfa_v4f m1 = j0 >= 1 ? load_quad(col + (j0 - 1) * L) : cur;
    if constexpr (SECOND) {
        m2 = j0 >= 2 ? load_quad(col + (j0 - 2) * L) : cur;
        p1 = j0 + 1 < H ? load_quad(col + (j0 + 1) * L) : cur;
    }
#pragma unroll 4
    for (uint32_t j = j0; j < j1; ++j) {
        const bool up = j >= 1, up2 = j >= 2, dn = j + 1 < H, dn2 = j + 2 < H;
        if constexpr (SECOND) p2 = dn2 ? load_quad(col + (j + 2) * L) : p1;
        else p1 = dn ? load_quad(col + (j + 1) * L) : cur;
        const nfa_v4f lq = left ? load_quad(col + j * L - F) : cur;
        const nfa_v4f rq = right ? load_quad(col + j * L + F) : cur;
        nfa_v4f g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d_m1 = cur[e] - m1[e], d_0 = p1[e] - cur[e];
            const float gh = (up ? d_m1 : 0.0f) - (dn ? d_0 : 0.0f);
            const float gw = (left ? cur[e] - lq[e] : 0.0f) - (right ? rq[e] - cur[e] : 0.0f);
            float v = ch2 * gh + cw2 * gw;
            if constexpr (SECOND) {
                const float d_m2 = m1[e] - m2[e], d_p1 = p2[e] - p1[e];
                const float A = up2 ? d_m1 - d_m2 : 0.0f;
                const float B = up && dn ? d_0 - d_m1 : 0.0f;
                const float C = dn2 ? d_p1 - d_0 : 0.0f;
                v = v + cs2 * ((A - 2.0f * B) + C);
            }
            if constexpr (L1 != L1Form::none) v = v + cl * sign0(L1 == L1Form::one_minus ? cur[e] - 1.0f : cur[e]);
            g[e] = v;
        }
        *reinterpret_cast<nfa_v4f *>(out + j * L) = g;
        if constexpr (SECOND) m2 = m1;
        m1 = cur;
        cur = p1;
        if constexpr (SECOND) p1 = p2;
    }
}

// ---------------------------------------------------------------- host side
// The tiling of an [H, W, F] plane at `offset` whose tiles follow the `tiles` of the planes before it (a plane has fewer
// than 2^25 tiles).
static TilePlane tile_plane(uint32_t offset, int64_t H, int64_t W, int64_t F, int64_t &tiles)
{
    TilePlane pl;
    pl.offset = offset;
    pl.H = (uint32_t)H;
    pl.L4 = (uint32_t)(W * F / 4);
    pl.tile_first = (uint32_t)tiles;
    pl.segs = (uint32_t)ceil_div64(W * F / 4, NFA_PT_QUADS);
    tiles += ceil_div64(H, NFA_PT_ROWS) * pl.segs;
    return pl;
}

// the summands of (tv_h, tv_w, smooth, l1) on an [H, W, F] plane; 0: the policy leaves the term out, or H = 2
static void plane_counts(int64_t H, int64_t W, int64_t F, bool second, bool l1, double cnt[4])
{
    const double f = (double)F, h = (double)H, w = (double)W;
    cnt[0] = f * (double)(H - 1) * w;
    cnt[1] = f * h * (double)(W - 1);
    cnt[2] = second && H > 2 ? f * (double)(H - 2) * w : 0.0;
    cnt[3] = l1 ? f * h * w : 0.0;
}

// the divisor of a term of `cnt` summands (forward) and the factor of its gradient (backward)
static void term_scale(double cnt, float &count, float &inv_count)
{
    count = cnt > 0.0 ? (float)cnt : 1.0f;
    inv_count = cnt > 0.0 ? (float)(1.0 / cnt) : 0.0f;
}

}  // namespace nfa

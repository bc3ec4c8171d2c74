// plane_layout.h -- the parameter layout of the plane grid, shared by planes.hip (the encoding) and planereg.hip (its
// regularisers): the axis pairs of the planes, the description the kernels take, and the host routine that checks a
// resolution table and lays the planes out.
//
// Planes: the axis pairs (a, b), a < b, in lexicographic order -- (0,1) (0,2) (1,2) at D = 3, (0,1) (0,2) (0,3) (1,2) (1,3)
// (2,3) at D = 4.  Scale s has the resolution R_{s,d} per axis (res[s * D + d], every one >= 2); plane (s, k) is a dense
// row-major [R_b, R_a, F] block of one flat float32 table, the blocks in scale-major, then plane order without gaps.  At
// most 8 scales; fewer than 2^31 floats in all.
#pragma once
#include "common.hip.h"

namespace nfa {

#define NFA_PG_MAX_SCALES 8
#define NFA_PG_MAX_PLANES 6

struct PlaneGridDesc {
    int32_t res[NFA_PG_MAX_SCALES][4];                      // R_{s,d}
    uint32_t offset[NFA_PG_MAX_SCALES][NFA_PG_MAX_PLANES];  // first float of plane (s, k)
    int32_t n_scales;
};

template <int D> __host__ __device__ constexpr int n_planes() { return D * (D - 1) / 2; }
// the axes (a, b) of plane k
template <int D> __host__ __device__ constexpr int plane_a(int k) { return D == 3 ? (k < 2 ? 0 : 1) : (k < 3 ? 0 : k < 5 ? 1 : 2); }
template <int D> __host__ __device__ constexpr int plane_b(int k) { return D == 3 ? (k == 0 ? 1 : 2) : (k < 3 ? k + 1 : k < 5 ? k - 1 : 3); }

// The checks of a resolution table, in this order (null; a resolution below 2; the size limit), and the planes' offsets.
// D (3 or 4), F and n_scales (1..8) have been checked by the caller.
static int plane_layout(const char *name, int D, int32_t n_features, int32_t n_scales, const int32_t *res_host, PlaneGridDesc &P)
{
    NFA_REQUIRE(res_host != nullptr, "%s: null resolution table", name);
    P = {};
    const int64_t limit = (int64_t)1 << 31;
    int64_t total = 0;
    for (int s = 0; s < n_scales; ++s) {
        for (int d = 0; d < D; ++d) {
            const int32_t r = res_host[s * D + d];
            NFA_REQUIRE(r >= 2, "%s: scale %d axis %d resolution %d is below 2", name, s, d, r);
            P.res[s][d] = r;
        }
        int k = 0;
        for (int a = 0; a < D; ++a)
            for (int b = a + 1; b < D; ++b, ++k) {
                const int64_t cells = (int64_t)P.res[s][a] * P.res[s][b];   // (< 2^62)
                NFA_REQUIRE(cells < limit && total + cells * n_features < limit,
                            "%s: too many parameters (at most 2^31 - 1 floats)", name);
                P.offset[s][k] = (uint32_t)total;
                total += cells * n_features;
            }
    }
    P.n_scales = n_scales;
    return NFA_OK;
}

}  // namespace nfa

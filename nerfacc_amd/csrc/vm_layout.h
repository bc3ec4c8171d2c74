// vm_layout.h -- the parameter layout of the VM grid, shared by vmgrid.hip (the encoding) and vmreg.hip (its regularisers):
// the axes of the modes, the description the kernels take, and the host routines that check a component count and a
// resolution table and lay the blocks out.
//
// Modes m = 0, 1, 2: plane axes (a, b) = (0,1) (0,2) (1,2) (TensoRF's matMode), line axis c = 2, 1, 0 (vecMode).  The
// resolution (R_0, R_1, R_2), every one >= 2, is shared by the modes, and so is the component count C, a multiple of 4 in
// 4..96.  One flat float32 table without gaps of fewer than 2^31 floats: for m in order the plane, a row-major [R_b, R_a, C]
// block, then the line, a [R_c, C] block.
#pragma once
#include "common.hip.h"

namespace nfa {

__host__ __device__ constexpr int vm_a(int m) { return m < 2 ? 0 : 1; }
__host__ __device__ constexpr int vm_b(int m) { return m == 0 ? 1 : 2; }
__host__ __device__ constexpr int vm_c(int m) { return 2 - m; }

struct VMDesc {
    int32_t res[3];
    uint32_t plane[3], line[3];   // first float of mode m's plane and line
    int32_t C;
};

// The checks of a component count and a resolution table, in this order (C; null, which the caller checks; a resolution
// below 2; the size limit), and the blocks' offsets.  `what` names the table in the messages ("" for the one table of the forward and backward).
static int vm_check_c(const char *name, int32_t C)
{
    NFA_REQUIRE(C >= 4 && C <= 96 && C % 4 == 0, "%s: n_components must be a multiple of 4 in 4..96 (got %d)", name, C);
    return NFA_OK;
}
static int vm_layout(const char *name, const char *what, int32_t C, const int32_t *res_host, VMDesc &V, int64_t &total)
{
    V = {};
    V.C = C;
    for (int d = 0; d < 3; ++d) {
        NFA_REQUIRE(res_host[d] >= 2, "%s: %saxis %d resolution %d is below 2", name, what, d, res_host[d]);
        V.res[d] = res_host[d];
    }
    const int64_t limit = (int64_t)1 << 31;
    total = 0;
    for (int m = 0; m < 3; ++m) {
        const int64_t cells = (int64_t)V.res[vm_a(m)] * V.res[vm_b(m)] + V.res[vm_c(m)];   // (< 2^62 + 2^31)
        NFA_REQUIRE(cells < limit && total + cells * C < limit, "%s: too many %sparameters (at most 2^31 - 1 floats)", name, what);
        V.plane[m] = (uint32_t)total;
        V.line[m] = (uint32_t)(total + (int64_t)V.res[vm_a(m)] * V.res[vm_b(m)] * C);
        total += cells * C;
    }
    return NFA_OK;
}

}  // namespace nfa

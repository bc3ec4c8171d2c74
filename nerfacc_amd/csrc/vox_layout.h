// vox_layout.h -- the host checks of the dense voxel grid's shape, shared by voxgrid.hip (the encoding) and voxreg.hip (its
// regularisers).  The table is one flat float32 block, row-major [R_z, R_y, R_x, C], of fewer than 2^31 floats; every R_d >= 2;
// C is 1, 2 or a multiple of 4 up to 64.
#pragma once
#include "common.hip.h"

namespace nfa {

// The checks of a feature count and a resolution table, in this order (C; null; a resolution below 2; the size limit).
// `what` names the table in the messages ("" for the one table of the forward and backward).
static int vox_check_c(const char *name, int32_t C)
{
    NFA_REQUIRE(C == 1 || C == 2 || (C >= 4 && C <= 64 && C % 4 == 0), "%s: n_features must be 1, 2 or a multiple of 4 up to 64 (got %d)",
                name, C);
    return NFA_OK;
}
static int vox_check_res(const char *name, const char *what, int32_t C, const int32_t *res_host, int32_t (&res)[3], int64_t &total)
{
    NFA_REQUIRE(res_host != nullptr, "%s: null %sresolution table", name, what);
    total = C;
    const int64_t limit = (int64_t)1 << 31;
    for (int d = 0; d < 3; ++d) {
        NFA_REQUIRE(res_host[d] >= 2, "%s: %saxis %d resolution %d is below 2", name, what, d, res_host[d]);
        res[d] = res_host[d];
    }
    for (int d = 0; d < 3; ++d) {
        total *= res[d];   // (< 2^31 * 2^31)
        NFA_REQUIRE(total < limit, "%s: too many %sparameters (at most 2^31 - 1 floats)", name, what);
    }
    return NFA_OK;
}

}  // namespace nfa

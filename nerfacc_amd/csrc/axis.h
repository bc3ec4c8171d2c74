// axis.h -- the per-axis locate step of the dense grids sampled as grid_sample(padding_mode="border", align_corners=True)
// samples them, and the element load / store of their activation streams; shared by planes.hip (the K-Planes plane grid)
// and vmgrid.hip (the TensoRF vector-matrix grid), so both use one copy.
//
// An axis of R >= 2 nodes, all arithmetic float32, every operation rounded on its own:
//   p = x * (float)(R - 1)                                                  (locate_axis; locate_pos is given p itself)
//   in = (p >= 0 && p <= R - 1)
//   q = p >= 0 ? p : 0 (NaN gives 0), then q = q <= R - 1 ? q : R - 1      (fminf(fmaxf(p, 0), R - 1), -0 kept as it is)
//   i = min((int)floorf(q), R - 2),   f = q - (float)i                     (f in [0, 1]; 1 only at the upper border)
// i and i + 1 lie in [0, R - 1] for every input, NaN and +-inf included.
#pragma once
#include "common.hip.h"

namespace nfa {

struct Axis {
    uint32_t i;   // the lower node, in [0, R - 2]
    float f;      // the fraction, in [0, 1]
    float rm1;    // (float)(R - 1)
    bool in;      // the coordinate is inside [0, 1]
};
// the node coordinate p = x (R - 1) located among R nodes
__device__ __forceinline__ Axis locate_pos(float p, int32_t R)
{
    Axis a;
    a.rm1 = (float)(R - 1);
    a.in = p >= 0.0f && p <= a.rm1;
    float q = p >= 0.0f ? p : 0.0f;
    q = q <= a.rm1 ? q : a.rm1;
    const int i = min((int)floorf(q), R - 2);
    a.i = (uint32_t)i;
    a.f = q - (float)i;
    return a;
}
__device__ __forceinline__ Axis locate_axis(float x, int32_t R) { return locate_pos(x * (float)(R - 1), R); }

template <class E>
__device__ __forceinline__ void store_elem(E *p, float v)
{
    if constexpr (std::is_same<E, float>::value) *p = v;
    else *reinterpret_cast<uint16_t *>(p) = (uint16_t)half_bits<E>(v);
}
template <class E>
__device__ __forceinline__ float load_elem(const E *p)
{
    if constexpr (std::is_same<E, float>::value) return *p;
    else return half_value<E>(*reinterpret_cast<const uint16_t *>(p));
}

}  // namespace nfa

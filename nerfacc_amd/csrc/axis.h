// axis.h -- the per-axis locate step of the dense grids sampled as grid_sample(padding_mode="border", align_corners=True)
// samples them, the bilinear taps of a plane and the linear ones of a line, and the element load / store of their activation
// streams; shared by planes.hip (the K-Planes plane grid), vmgrid.hip (the TensoRF vector-matrix grid) and voxgrid.hip (the
// dense voxel grid, with the trilinear taps of a volume), so all use one copy.
//
// An axis of R >= 2 nodes, all arithmetic float32, every operation rounded on its own:
//   p = x * (float)(R - 1)                                                  (locate_axis; locate_pos is given p itself)
//   in = (p >= 0 && p <= R - 1)
//   q = p >= 0 ? p : 0 (NaN gives 0), then q = q <= R - 1 ? q : R - 1      (fminf(fmaxf(p, 0), R - 1), -0 kept as it is)
//   i = min((int)floorf(q), R - 2),   f = q - (float)i                     (f in [0, 1]; 1 only at the upper border)
// i and i + 1 lie in [0, R - 1] for every input, NaN and +-inf included.
//
// A plane over the axes (a, b), a row-major [R_b, R_a] block of nodes of `stride` floats, and a line of such nodes; per
// component j, corners k = k_a + 2 k_b in the order 0..3:
//   w_k = (k_a ? f_a : 1 - f_a) * (k_b ? f_b : 1 - f_b),   T_k = table[((i_b + k_b) R_a + i_a + k_a) stride + j]
//   plane_value  = sum_k w_k * T_k, summed from 0 in corner order
//   line_value   = (0 + (1 - f) * l_0) + f * l_1
//   plane_slopes: dv_a = (((0 - (1 - f_b) * T_0) + (1 - f_b) * T_1) - f_b * T_2) + f_b * T_3        (d plane_value / d f_a)
//                 dv_b = (((0 - (1 - f_a) * T_0) - f_a * T_1) + (1 - f_a) * T_2) + f_a * T_3        (d plane_value / d f_b)
//
// A volume over the axes (a, b, c), a row-major [R_c, R_b, R_a] block of nodes (voxgrid.hip, the dense voxel grid); per
// component j, corners k = k_a + 2 k_b + 4 k_c in the order 0..7, e_k the first float of corner k's node:
//   w_k = ((k_a ? f_a : 1 - f_a) * (k_b ? f_b : 1 - f_b)) * (k_c ? f_c : 1 - f_c)      (the plane's product first),  T_k = table[e_k + j]
//   volume_value  = sum_k w_k * T_k, summed from 0 in corner order
//   volume_slopes: dv_a = sum_k (k_a ? + : -) u_k * T_k,  u_k = (k_b ? f_b : 1 - f_b) * (k_c ? f_c : 1 - f_c)   (d value / d f_a)
//                  dv_b = sum_k (k_b ? + : -) u_k * T_k,  u_k = (k_a ? f_a : 1 - f_a) * (k_c ? f_c : 1 - f_c)   (d value / d f_b)
//                  dv_c = sum_k (k_c ? + : -) u_k * T_k,  u_k = (k_a ? f_a : 1 - f_a) * (k_b ? f_b : 1 - f_b)   (d value / d f_c)
//   each from 0 in corner order, a term added or subtracted as its sign says.
// Index arithmetic is uint32 (a table holds fewer than 2^31 floats).
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

// The 4 corners of a plane at float `base` around a point: the first float of each corner's node (component 0; planes.hip
// folds its lane's component into `base` and loads component 0) and the corner weights.
struct Taps {
    uint32_t e[4];
    float w[4];
};
__device__ __forceinline__ Taps plane_taps(uint32_t base, const Axis &a, const Axis &b, uint32_t Ra, uint32_t stride)
{
    Taps t;
    const uint32_t e0 = base + (b.i * Ra + a.i) * stride;
    t.e[0] = e0; t.e[1] = e0 + stride; t.e[2] = e0 + Ra * stride; t.e[3] = e0 + Ra * stride + stride;
    const float wa0 = 1.0f - a.f, wb0 = 1.0f - b.f;
    t.w[0] = wa0 * wb0; t.w[1] = a.f * wb0; t.w[2] = wa0 * b.f; t.w[3] = a.f * b.f;
    return t;
}
// the corners' values of component j
__device__ __forceinline__ void load_taps(const float *__restrict__ table, const Taps &t, uint32_t j, float (&T)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) T[k] = table[t.e[k] + j];
}
__device__ __forceinline__ float plane_value(const float (&w)[4], const float (&T)[4])
{
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) v = v + w[k] * T[k];
    return v;
}
__device__ __forceinline__ float line_value(float f, float l0, float l1) { return (0.0f + (1.0f - f) * l0) + f * l1; }
__device__ __forceinline__ void plane_slopes(float fa, float fb, const float (&T)[4], float &dva, float &dvb)
{
    const float wa0 = 1.0f - fa, wb0 = 1.0f - fb;
    dva = (((0.0f - wb0 * T[0]) + wb0 * T[1]) - fb * T[2]) + fb * T[3];
    dvb = (((0.0f - wa0 * T[0]) - fa * T[1]) + wa0 * T[2]) + fa * T[3];
}

// The 8 corners of a volume cell: e0 is the first float of the lower corner's node, (da, db, dc) the floats from a node to its
// upper neighbour along each axis.
struct VolumeTaps {
    uint32_t e[8];
    float w[8];
};
__device__ __forceinline__ VolumeTaps volume_taps(uint32_t e0, const Axis &a, const Axis &b, const Axis &c, uint32_t da, uint32_t db,
                                                  uint32_t dc)
{
    VolumeTaps t;
    const float wa0 = 1.0f - a.f, wb0 = 1.0f - b.f, wc0 = 1.0f - c.f;
    const float wab[4] = {wa0 * wb0, a.f * wb0, wa0 * b.f, a.f * b.f};   // plane_taps' weights
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        t.e[k] = e0 + ((k & 1) ? da : 0u) + ((k & 2) ? db : 0u) + ((k & 4) ? dc : 0u);
        t.w[k] = wab[k & 3] * ((k & 4) ? c.f : wc0);
    }
    return t;
}
__device__ __forceinline__ float volume_value(const float (&w)[8], const float (&T)[8])
{
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v = v + w[k] * T[k];
    return v;
}
__device__ __forceinline__ void volume_slopes(float fa, float fb, float fc, const float (&T)[8], float &dva, float &dvb, float &dvc)
{
    const float wa0 = 1.0f - fa, wb0 = 1.0f - fb, wc0 = 1.0f - fc;
    const float wbc[4] = {wb0 * wc0, fb * wc0, wb0 * fc, fb * fc};   // index k_b + 2 k_c
    const float wac[4] = {wa0 * wc0, fa * wc0, wa0 * fc, fa * fc};   // index k_a + 2 k_c
    const float wab[4] = {wa0 * wb0, fa * wb0, wa0 * fb, fa * fb};   // index k_a + 2 k_b
    dva = dvb = dvc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float ta = wbc[k >> 1] * T[k], tb = wac[(k & 1) + ((k >> 2) << 1)] * T[k], tc = wab[k & 3] * T[k];
        dva = (k & 1) ? dva + ta : dva - ta;
        dvb = (k & 2) ? dvb + tb : dvb - tb;
        dvc = (k & 4) ? dvc + tc : dvc - tc;
    }
}

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

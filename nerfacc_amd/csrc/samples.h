// samples.h -- per-sample arithmetic of nfa_sample_positions_{fwd,bwd}, shared by the flat kernels (samples.hip) and the
// segmented-engine op of the backward (segscan.hip: SamplePosBwdOp), so that both forms of the backward compute g_p with
// the same expressions.
//
//   p  = o[r] + (d[r] * (t_start + t_end)) / 2                    ref: examples/utils.py:83-85
//   x  = (p - lo) / (hi - lo)                                     ref: examples/radiance_fields/ngp.py:162-163
//   u  = 2 x - 1;  m = |u|_2 (sphere) or |u|_inf (cube);  m > 1: u <- (2 - 1/m) (u / m);  x = u / 4 + 0.5
//                                                                 ref: ngp.py:42-66 (contract_to_unisphere)
// Every operation is rounded on its own (the library is built with -ffp-contract=off), in the reference's order.
#pragma once
#include <type_traits>

#include "common.hip.h"

namespace nfa {

enum { SP_NONE = 0, SP_AABB = 1, SP_SPHERE = 2, SP_CUBE = 3 };   // what happens to p: nothing, normalise, normalise + contract

// The box, by value in the kernel arguments (or read from `dev`, 6 floats, when the caller's box lives on the device).
struct SampleBox {
    float lo[3], hi[3];
    const float *dev;
};

__device__ __forceinline__ void box_resolve(const SampleBox &b, float lo[3], float ext[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = b.dev ? b.dev[k] : b.lo[k];
        ext[k] = (b.dev ? b.dev[3 + k] : b.hi[k]) - lo[k];
    }
}

__device__ __forceinline__ void sample_point(const float o[3], const float d[3], float ts, float te, float p[3])
{
    const float s = ts + te;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = o[k] + (d[k] * s) / 2.0f;
}

// index of the largest |u_k| (the first one at ties) and that magnitude
__device__ __forceinline__ int cube_argmax(const float u[3], float &m)
{
    const float a0 = fabsf(u[0]), a1 = fabsf(u[1]), a2 = fabsf(u[2]);
    int k = 0;
    m = a0;
    if (a1 > m) { m = a1; k = 1; }
    if (a2 > m) { m = a2; k = 2; }
    return k;
}

template <int MODE>
__device__ __forceinline__ float contraction_mag(const float u[3])
{
    if (MODE == SP_SPHERE) return sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    float m;
    cube_argmax(u, m);
    return m;
}

// p -> x (in place); MODE != SP_NONE
template <int MODE>
__device__ __forceinline__ void sample_normalise(float x[3], const float lo[3], const float ext[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (x[k] - lo[k]) / ext[k];
    if (MODE == SP_SPHERE || MODE == SP_CUBE) {
        float u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = x[k] * 2.0f - 1.0f;
        const float m = contraction_mag<MODE>(u);
        if (m > 1.0f) {
            const float f = 2.0f - 1.0f / m;
#pragma unroll
            for (int k = 0; k < 3; ++k) u[k] = f * (u[k] / m);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = u[k] / 4.0f + 0.5f;
    }
}

__device__ __forceinline__ bool sample_inside(const float x[3])
{
    return x[0] > 0.0f && x[0] < 1.0f && x[1] > 0.0f && x[1] < 1.0f && x[2] > 0.0f && x[2] < 1.0f;
}

// g_x -> g_p = J^T g_x at the point p (in place on g).  For m > 1 the Jacobian of u -> u' = (2/m - 1/m^2) u is
//   a I + c u (dm/du)^T,  a = (2m - 1) / m^2,  c = 2 (1 - m) / m^3,  dm/du = u / m (sphere) or sign(u_k) e_k (cube, k = argmax)
template <int MODE>
__device__ __forceinline__ void sample_grad_point(const float p[3], const float lo[3], const float ext[3], float g[3])
{
    if (MODE == SP_NONE) return;
    if (MODE == SP_SPHERE || MODE == SP_CUBE) {
        float u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u[k] = ((p[k] - lo[k]) / ext[k]) * 2.0f - 1.0f;
            g[k] = g[k] / 4.0f;
        }
        float m;
        const int kmax = cube_argmax(u, m);
        if (MODE == SP_SPHERE) m = contraction_mag<MODE>(u);
        if (m > 1.0f) {
            const float a = (2.0f * m - 1.0f) / (m * m);
            const float c = 2.0f * (1.0f - m) / (m * m * m);
            const float ug = c * (u[0] * g[0] + u[1] * g[1] + u[2] * g[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float dm = MODE == SP_SPHERE ? u[k] / m : (k == kmax ? (u[k] < 0.0f ? -1.0f : 1.0f) : 0.0f);
                g[k] = a * g[k] + ug * dm;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = g[k] * 2.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = g[k] / ext[k];
}

template <class F>
static void dispatch_sample_mode(int mode, F &&f)
{
    if (mode == SP_CUBE) f(std::integral_constant<int, SP_CUBE>{});
    else if (mode == SP_SPHERE) f(std::integral_constant<int, SP_SPHERE>{});
    else if (mode == SP_AABB) f(std::integral_constant<int, SP_AABB>{});
    else f(std::integral_constant<int, SP_NONE>{});
}

// The backward without per-ray sums (samples.hip): g_p[n, 3] (optional) and g_t_starts / g_t_ends (optional) per sample,
// for ray indices in any order.
void launch_sample_positions_bwd_flat(int mode, const SampleBox &box, const float *rays_o, const float *rays_d,
                                      const float *t_starts, const float *t_ends, const int64_t *ray_indices,
                                      int64_t n_rays, int64_t n, int64_t samples_per_ray, const float *g_positions,
                                      float *grad_p, float *grad_t_starts, float *grad_t_ends, hipStream_t s);

}  // namespace nfa

// camera.h -- the per-point lens solvers of camera.hip (its header has the models and the reference lines), shared with
// rays.hip: nfa_generate_rays_{fwd,bwd} undistort inside their own pass with the same functions, so a ray's (u, v) has the
// bits nfa_opencv_lens_undistortion[_fisheye] gives the same point.
#pragma once
#include "common.hip.h"

namespace nfa {

struct LensParams {
    float k1, k2, k3, k4, k5, k6, p1, p2, s1, s2, s3, s4;
};

// The C ABI's parameter layouts (include/nerfacc_hip.h): 5 {k1,k2,p1,p2,k3}, 8 {k1,k2,p1,p2,k3,k4,k5,k6},
// 12 {k1..k6,p1,p2,s1..s4}, fisheye 4 {k1,k2,k3,k4}.  Unused coefficients are 0.
template <int NP>
__device__ __forceinline__ LensParams load_params(const float *__restrict__ q)
{
    LensParams L = {};
    if constexpr (NP == 5 || NP == 8) {
        L.k1 = q[0]; L.k2 = q[1]; L.p1 = q[2]; L.p2 = q[3]; L.k3 = q[4];
        if constexpr (NP == 8) { L.k4 = q[5]; L.k5 = q[6]; L.k6 = q[7]; }
    } else if constexpr (NP == 12) {
        L.k1 = q[0]; L.k2 = q[1]; L.k3 = q[2]; L.k4 = q[3]; L.k5 = q[4]; L.k6 = q[5];
        L.p1 = q[6]; L.p2 = q[7]; L.s1 = q[8]; L.s2 = q[9]; L.s3 = q[10]; L.s4 = q[11];
    } else {
        static_assert(NP == 4, "parameter layout");
        L.k1 = q[0]; L.k2 = q[1]; L.k3 = q[2]; L.k4 = q[3];
    }
    return L;
}

// Residual f(x, y) - (xd, yd) of the radial-tangential model at (x, y) and its symmetric Jacobian; the Newton step below
// and the backward of nfa_generate_rays (which needs J^-1 at the solution) share it.
struct NewtonTerms {
    float ex, ey, jxx, jxy, jyy;
};
__device__ __forceinline__ NewtonTerms newton_terms(float x, float y, float2 pd, const LensParams &L)
{
    const float r = x * x + y * y;
    const float num = 1.0f + r * (L.k1 + r * (L.k2 + r * L.k3));
    const float den = 1.0f + r * (L.k4 + r * (L.k5 + r * L.k6));
    const float d = num / den;
    const float xy2 = 2.0f * x * y;
    NewtonTerms t;
    t.ex = d * x + L.p1 * xy2 + L.p2 * (r + 2.0f * x * x) - pd.x;
    t.ey = d * y + L.p2 * xy2 + L.p1 * (r + 2.0f * y * y) - pd.y;
    // d'(r), and the Jacobian through dr/dx = 2x, dr/dy = 2y
    const float num_r = L.k1 + r * (2.0f * L.k2 + r * (3.0f * L.k3));
    const float den_r = L.k4 + r * (2.0f * L.k5 + r * (3.0f * L.k6));
    const float d_r = (num_r * den - num * den_r) / (den * den);
    t.jxx = d + 2.0f * x * x * d_r + 2.0f * L.p1 * y + 6.0f * L.p2 * x;
    t.jxy = xy2 * d_r + 2.0f * L.p1 * x + 2.0f * L.p2 * y;   // = jyx
    t.jyy = d + 2.0f * y * y * d_r + 2.0f * L.p2 * x + 6.0f * L.p1 * y;
    return t;
}

__device__ __forceinline__ float2 undistort_newton(float2 pd, const LensParams &L, float eps, int iters)
{
    float x = pd.x, y = pd.y;
    for (int it = 0; it < iters; ++it) {
        const NewtonTerms t = newton_terms(x, y, pd, L);
        const float det = t.jxx * t.jyy - t.jxy * t.jxy;
        if (fabsf(det) < eps) break;
        // (dx, dy) = -J^-1 (ex, ey)
        const float dx = (t.jxy * t.ey - t.jyy * t.ex) / det;
        const float dy = (t.jxy * t.ex - t.jxx * t.ey) / det;
        x += dx;
        y += dy;
        if (fabsf(dx) < eps && fabsf(dy) < eps) break;
    }
    return make_float2(x, y);
}

__device__ __forceinline__ float2 undistort_thin_prism(float2 pd, const LensParams &L, int iters)
{
    float x = pd.x, y = pd.y;
    for (int it = 0; it < iters; ++it) {
        const float r = x * x + y * y;
        const float inv_d = (1.0f + r * (L.k4 + r * (L.k5 + r * L.k6))) / (1.0f + r * (L.k1 + r * (L.k2 + r * L.k3)));
        if (inv_d < 0.0f) return pd;
        const float xy2 = 2.0f * x * y;
        const float tx = L.p1 * xy2 + L.p2 * (r + 2.0f * x * x) + r * (L.s1 + r * L.s2);
        const float ty = L.p2 * xy2 + L.p1 * (r + 2.0f * y * y) + r * (L.s3 + r * L.s4);
        x = (pd.x - tx) * inv_d;
        y = (pd.y - ty) * inv_d;
    }
    return make_float2(x, y);
}

__device__ __forceinline__ float2 undistort_fisheye(float2 pd, const LensParams &L, float eps, int iters)
{
    const float half_pi = 1.57079632679489662f;
    const float theta_d = fminf(sqrtf(pd.x * pd.x + pd.y * pd.y), half_pi);   // >= 0, so only the upper clamp acts
    if (!(theta_d > eps)) return pd;                                           // scale 1 at the centre (and NaN input)
    const double td = (double)theta_d;
    const double k1 = L.k1, k2 = L.k2, k3 = L.k3, k4 = L.k4;
    double theta = td;
    bool converged = false;
    for (int it = 0; it < iters; ++it) {
        const double t2 = theta * theta;
        const double g = theta * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td;
        const double g_t = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))));
        const double step = g / g_t;
        theta -= step;
        if (fabs(step) < (double)eps) { converged = true; break; }
    }
    if (!converged || !(theta >= 0.0)) return pd;   // theta flipped sign (or NaN)
    const float scale = tanf((float)theta) / theta_d;
    return make_float2(pd.x * scale, pd.y * scale);
}

}  // namespace nfa

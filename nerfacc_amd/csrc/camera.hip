// camera.hip -- OpenCV lens undistortion (pinhole radial-tangential, thin prism, fisheye).
//
// Semantics (ref = the reference nerfacc): ref cuda/csrc/camera.cu:9-107 (kernels and their parameter layouts) and
// include/utils_camera.cuh (the per-point solvers).  The math is the OpenCV camera model restated here:
//
//   radial-tangential (5 / 8 parameters): the distorted point of (x, y) is
//       xd = x d(r) + 2 p1 x y + p2 (r + 2 x^2),   yd = y d(r) + 2 p2 x y + p1 (r + 2 y^2),
//       d(r) = (1 + k1 r + k2 r^2 + k3 r^3) / (1 + k4 r + k5 r^2 + k6 r^3),   r = x^2 + y^2.
//     Undistortion starts at (xd, yd) and takes at most `iters` Newton steps on (xd, yd) - f(x, y) with the analytic 2x2
//     Jacobian; it stops before a step when |det J| < eps and after a step when both |dx| and |dy| are below eps.
//   thin prism (12 parameters {k1..k6, p1, p2, s1..s4}): exactly `iters` fixed-point steps
//       x <- (xd - dx(x, y)) / d(r),  y <- (yd - dy(x, y)) / d(r)
//     with dx, dy the tangential terms plus s1 r + s2 r^2 (x) and s3 r + s4 r^2 (y), as OpenCV's undistortPoints does; eps
//     is unused.  A point whose 1 / d(r) turns negative is written back unchanged.
//   fisheye ({k1..k4}): theta_d = |(u, v)| clamped to [-pi/2, pi/2]; Newton on theta (1 + k1 theta^2 + k2 theta^4 +
//     k3 theta^6 + k4 theta^8) = theta_d in fp64 for at most `iters` steps, stopping when |step| < eps; the output is
//     (u, v) tan(theta) / theta_d.
//
// Defined where the reference is not (DESIGN.md "Lens undistortion"):
//   - a fisheye point that does not converge, or whose theta ends with the opposite sign of theta_d, is written back
//     unchanged (the reference leaves that element of its empty_like output unwritten);
//   - a fisheye point with |theta_d| <= eps is written back unchanged, i.e. scale 1, the limit of tan(theta) / theta_d
//     at 0 (the reference writes 0; the two differ by at most eps).
//
// Layout: uv / uv_out are interleaved float2 (one 8-byte load and one 8-byte store per lane, coalesced).  Parameters
// are either one set shared by every point -- read once per lane from a wave-uniform address, so they land in scalar
// registers (s_load) and the loop body reads no parameter memory -- or one set per point at a stride of n_params floats.
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

__device__ __forceinline__ float2 undistort_newton(float2 pd, const LensParams &L, float eps, int iters)
{
    float x = pd.x, y = pd.y;
    for (int it = 0; it < iters; ++it) {
        const float r = x * x + y * y;
        const float num = 1.0f + r * (L.k1 + r * (L.k2 + r * L.k3));
        const float den = 1.0f + r * (L.k4 + r * (L.k5 + r * L.k6));
        const float d = num / den;
        const float xy2 = 2.0f * x * y;
        // residual f(x, y) - (xd, yd)
        const float ex = d * x + L.p1 * xy2 + L.p2 * (r + 2.0f * x * x) - pd.x;
        const float ey = d * y + L.p2 * xy2 + L.p1 * (r + 2.0f * y * y) - pd.y;
        // d'(r), and the Jacobian through dr/dx = 2x, dr/dy = 2y
        const float num_r = L.k1 + r * (2.0f * L.k2 + r * (3.0f * L.k3));
        const float den_r = L.k4 + r * (2.0f * L.k5 + r * (3.0f * L.k6));
        const float d_r = (num_r * den - num * den_r) / (den * den);
        const float jxx = d + 2.0f * x * x * d_r + 2.0f * L.p1 * y + 6.0f * L.p2 * x;
        const float jxy = xy2 * d_r + 2.0f * L.p1 * x + 2.0f * L.p2 * y;   // = jyx
        const float jyy = d + 2.0f * y * y * d_r + 2.0f * L.p2 * x + 6.0f * L.p1 * y;
        const float det = jxx * jyy - jxy * jxy;
        if (fabsf(det) < eps) break;
        // (dx, dy) = -J^-1 (ex, ey)
        const float dx = (jxy * ey - jyy * ex) / det;
        const float dy = (jxy * ex - jxx * ey) / det;
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

// MODE 0: Newton (5 / 8 parameters), 1: thin prism (12), 2: fisheye (4).  SHARED: one parameter set for every point.
template <int MODE, int NP, bool SHARED>
__global__ __launch_bounds__(256) void lens_undistort_kernel(const float2 *__restrict__ uv, const float *__restrict__ params,
                                                             int64_t n, float eps, int iters, float2 *__restrict__ uv_out)
{
    LensParams shared_L = {};
    if constexpr (SHARED) shared_L = load_params<NP>(params);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float2 pd = uv[i];
        LensParams L;
        if constexpr (SHARED) L = shared_L;
        else L = load_params<NP>(params + i * NP);
        float2 o;
        if constexpr (MODE == 0) o = undistort_newton(pd, L, eps, iters);
        else if constexpr (MODE == 1) o = undistort_thin_prism(pd, L, iters);
        else o = undistort_fisheye(pd, L, eps, iters);
        uv_out[i] = o;
    }
}

template <int MODE, int NP>
static void launch_lens(const float *uv, const float *params, int64_t n, bool shared, float eps, int iters, float *uv_out,
                        hipStream_t s)
{
    const dim3 grid(grid_1d(n, 256)), block(256);
    const float2 *in = reinterpret_cast<const float2 *>(uv);
    float2 *out = reinterpret_cast<float2 *>(uv_out);
    if (shared) hipLaunchKernelGGL((lens_undistort_kernel<MODE, NP, true>), grid, block, 0, s, in, params, n, eps, iters, out);
    else hipLaunchKernelGGL((lens_undistort_kernel<MODE, NP, false>), grid, block, 0, s, in, params, n, eps, iters, out);
}

static int check_lens_args(const char *name, const float *uv, const float *params, int64_t n_points, int32_t n_params,
                           int64_t param_stride, int32_t iters, const float *uv_out)
{
    NFA_REQUIRE(n_points >= 0, "%s: negative n_points", name);
    NFA_REQUIRE(iters >= 0, "%s: iters must be >= 0 (got %d)", name, iters);
    NFA_REQUIRE(param_stride == 0 || param_stride == n_params,
                "%s: param_stride must be 0 (shared) or n_params = %d (per point), got %lld", name, n_params,
                (long long)param_stride);
    NFA_REQUIRE(n_points == 0 || (uv && params && uv_out), "%s: null pointer", name);
    NFA_REQUIRE((reinterpret_cast<uintptr_t>(uv) | reinterpret_cast<uintptr_t>(uv_out)) % 8 == 0,
                "%s: uv and uv_out must be 8-byte aligned", name);
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int nfa_opencv_lens_undistortion(const float *uv, const float *params, int64_t n_points, int32_t n_params,
                                 int64_t param_stride, float eps, int32_t iters, float *uv_out, nfa_stream_t stream)
{
    NFA_REQUIRE(n_params == 5 || n_params == 8 || n_params == 12,
                "opencv_lens_undistortion: n_params must be 5, 8 or 12 (got %d)", n_params);
    const int rc = check_lens_args("opencv_lens_undistortion", uv, params, n_points, n_params, param_stride, iters, uv_out);
    if (rc != NFA_OK) return rc;
    if (n_points == 0) return NFA_OK;
    const bool shared = param_stride == 0;
    hipStream_t s = as_stream(stream);
    if (n_params == 5) launch_lens<0, 5>(uv, params, n_points, shared, eps, iters, uv_out, s);
    else if (n_params == 8) launch_lens<0, 8>(uv, params, n_points, shared, eps, iters, uv_out, s);
    else launch_lens<1, 12>(uv, params, n_points, shared, eps, iters, uv_out, s);
    NFA_CHECK_LAUNCH("opencv_lens_undistortion");
    return NFA_OK;
}

int nfa_opencv_lens_undistortion_fisheye(const float *uv, const float *params, int64_t n_points, int32_t n_params,
                                         int64_t param_stride, float eps, int32_t iters, float *uv_out,
                                         nfa_stream_t stream)
{
    NFA_REQUIRE(n_params == 4, "opencv_lens_undistortion_fisheye: n_params must be 4 (got %d)", n_params);
    const int rc = check_lens_args("opencv_lens_undistortion_fisheye", uv, params, n_points, n_params, param_stride, iters,
                                   uv_out);
    if (rc != NFA_OK) return rc;
    if (n_points == 0) return NFA_OK;
    launch_lens<2, 4>(uv, params, n_points, param_stride == 0, eps, iters, uv_out, as_stream(stream));
    NFA_CHECK_LAUNCH("opencv_lens_undistortion_fisheye");
    return NFA_OK;
}

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
#include "camera.h"

namespace nfa {

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

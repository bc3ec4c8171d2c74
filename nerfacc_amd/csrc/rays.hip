// rays.hip -- rays from pixels and cameras, with the lens undistortion fused in: the front of a training step.
//
// Replaces the "generate rays" block of the reference's loaders (ref: examples/datasets/nerf_synthetic.py:194-227,
// examples/datasets/nerf_360_v2.py:326-359), about a dozen gather / elementwise torch launches with (n_rays, 3, 4) and
// (n_rays, 3) temporaries, and the nerfacc.cameras call a distorted camera makes from inside it:
//
//   u = (x - cx + pixel_center) / fx,  v = (y - cy + pixel_center) / fy          (left to right, each operation rounded)
//   (u, v) <- undistort(u, v)            with a lens: the solvers of camera.h, the bits of nfa_opencv_lens_undistortion*
//   c = (u, s v, s),  s = -1 (OpenGL) or +1
//   d_i = (R_i0 c_0 + R_i1 c_1) + R_i2 c_2
//   viewdirs = d / sqrt((d_0^2 + d_1^2) + d_2^2) when normalising, else d;   origins = the camera's translation
//
// K rows are row-major 3x3 (fx = K[0], cx = K[2], fy = K[4], cy = K[5]), poses row-major with 4 columns (R_ij = P[4 i + j],
// t_i = P[4 i + 3]); a table with stride 0 is one row shared by every camera.  The tables are a few hundred rows of at most
// 16 floats: they stay in cache, and a shared row sits at a wave-uniform address.
//
// Forward: flat over rays, 4 consecutive rays per lane so that the two (n, 3) outputs leave as 16-byte stores (store_rows12);
// traffic 16-24 B in (x, y, camera id) and 24 B out per ray.
//
// Backward: the gradient of a camera's 12 pose floats and 4 intrinsics is a sum over that camera's rays, made without float
// atomics in two launches of fixed shape.  Rays are taken in camera order (`order`: sorted position -> ray) and cut into
// chunks of RAY_CHUNK; a chunk is one workgroup, one ray per lane.
//   1. Every maximal stretch of one camera inside a chunk is a run.  A wave adds the 16 terms of its rays run by run with a
//      segmented shuffle scan (fixed tree), the last lane of each run adds the wave's total to the run's row in LDS, wave 0
//      first, wave 3 last; the chunk then writes one partial row per run to row (chunk + camera) of `partials`.  Along the
//      sorted rays both numbers only grow and one of them grows at every new run, so no two runs share a row and
//      n_chunks + n_cameras - 1 rows hold them all -- no prefix sum over run counts, no read-back.
//   2. One workgroup per camera finds its rays [s, e) by binary search, adds its rows of chunks s / RAY_CHUNK ..
//      (e - 1) / RAY_CHUNK in 16 interleaved slices, each in chunk order, and the slices in slice order; a camera without
//      rays gets zeros.
// The result depends on RAY_CHUNK (a constant), never on scheduling.
#include "camera.h"

namespace nfa {

constexpr int RAY_CHUNK = 256;   // rays per chunk of the backward = its workgroup size
constexpr int RAY_TERMS = 16;    // {dR_00, dR_01, dR_02, dt_0, ... dt_2, dfx, dfy, dcx, dcy}

enum { LENS_NONE = 0, LENS_PINHOLE = 1, LENS_FISHEYE = 2 };
enum { PIX_F32 = 0, PIX_I32 = 1, PIX_I64 = 2 };

struct RayArgs {
    const void *x, *y;           // [n] pixels, by PIX
    const int64_t *ids;          // [n] camera of a ray (the backward: of a sorted position), or NULL: camera 0
    int64_t n, n_cameras;
    const float *K, *pose, *dist;
    int64_t k_stride, pose_stride, dist_stride;
    float sign, pixel_center, eps;
    int32_t iters, normalize;
};

template <int PIX>
__device__ __forceinline__ float pixel_value(const void *p, int64_t i)
{
    if constexpr (PIX == PIX_F32) return static_cast<const float *>(p)[i];
    else if constexpr (PIX == PIX_I32) return (float)static_cast<const int32_t *>(p)[i];
    else return (float)static_cast<const int64_t *>(p)[i];
}

// A ray in its camera's frame: the distorted and undistorted image point, c, and the camera's rows.
struct RayFrame {
    float ud, vd, u, v, c[3], R[9], t[3], fx, fy;
    LensParams L;
};

// camera `cam` (in range) and pixel (xf, yf)
template <int LENS>
__device__ __forceinline__ RayFrame ray_frame(const RayArgs &a, int64_t cam, float xf, float yf)
{
    RayFrame f;
    const float *K = a.K + cam * a.k_stride, *P = a.pose + cam * a.pose_stride;
    f.fx = K[0]; f.fy = K[4];
    f.ud = (xf - K[2] + a.pixel_center) / f.fx;
    f.vd = (yf - K[5] + a.pixel_center) / f.fy;
    f.u = f.ud; f.v = f.vd;
    f.L = LensParams{};
    if constexpr (LENS == LENS_PINHOLE) {
        f.L = load_params<8>(a.dist + cam * a.dist_stride);
        const float2 p = undistort_newton(make_float2(f.ud, f.vd), f.L, a.eps, a.iters);
        f.u = p.x; f.v = p.y;
    } else if constexpr (LENS == LENS_FISHEYE) {
        f.L = load_params<4>(a.dist + cam * a.dist_stride);
        const float2 p = undistort_fisheye(make_float2(f.ud, f.vd), f.L, a.eps, a.iters);
        f.u = p.x; f.v = p.y;
    }
    f.c[0] = f.u; f.c[1] = a.sign * f.v; f.c[2] = a.sign;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f.R[3 * i] = P[4 * i]; f.R[3 * i + 1] = P[4 * i + 1]; f.R[3 * i + 2] = P[4 * i + 2];
        f.t[i] = P[4 * i + 3];
    }
    return f;
}

__device__ __forceinline__ void ray_direction(const RayFrame &f, float d[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = f.R[3 * i] * f.c[0] + f.R[3 * i + 1] * f.c[1] + f.R[3 * i + 2] * f.c[2];
}
__device__ __forceinline__ float ray_norm(const float d[3]) { return sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); }

template <int PIX, int LENS>
__global__ __launch_bounds__(256) void generate_rays_kernel(RayArgs a, float *__restrict__ origins, float *__restrict__ viewdirs,
                                                            bool aligned)
{
    const int64_t n_quads = (a.n + 3) / 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float bad = __builtin_nanf("");
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += stride) {
        const int64_t e = 4 * q;
        const int cnt = a.n - e >= 4 ? 4 : (int)(a.n - e);
        float o[12], w[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = j < cnt ? e + j : e;   // (in range: cnt >= 1)
            const int64_t cam = a.ids ? a.ids[i] : 0;
            // a camera outside [0, n_cameras) reads camera 0 and yields NaN rows (never an address outside the tables)
            const bool ok = (uint64_t)cam < (uint64_t)a.n_cameras;
            const RayFrame f = ray_frame<LENS>(a, ok ? cam : 0, pixel_value<PIX>(a.x, i), pixel_value<PIX>(a.y, i));
            float d[3];
            ray_direction(f, d);
            const float nrm = a.normalize ? ray_norm(d) : 1.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[3 * j + k] = ok ? f.t[k] : bad;
                w[3 * j + k] = ok ? (a.normalize ? d[k] / nrm : d[k]) : bad;
            }
        }
        store_rows12(origins, e, aligned && cnt == 4, cnt, o);
        store_rows12(viewdirs, e, aligned && cnt == 4, cnt, w);
    }
}

// The 16 terms of one ray: its share of the gradient of its camera's pose rows and of fx, fy, cx, cy.
template <int LENS>
__device__ __forceinline__ void ray_terms(const RayArgs &a, const RayFrame &f, const float go[3], const float gw[3],
                                          float term[RAY_TERMS])
{
    // gradient towards the unnormalised direction: w = d / |d|,  g_d = (g_w - w (w . g_w)) / |d|
    float gd[3] = {gw[0], gw[1], gw[2]};
    if (a.normalize) {
        float d[3], w[3];
        ray_direction(f, d);
        const float nrm = ray_norm(d);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = d[k] / nrm;
        const float dot = w[0] * gw[0] + w[1] * gw[1] + w[2] * gw[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) gd[k] = (gw[k] - w[k] * dot) / nrm;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) term[4 * i + j] = gd[i] * f.c[j];
        term[4 * i + 3] = go[i];
    }
    // towards the image point: g_c = R^T g_d, (g_u, g_v) = (g_c0, s g_c1); through the lens by the inverse of the (symmetric)
    // distortion Jacobian at the solution; then u_d = (x - cx + pixel_center) / fx
    float gu = f.R[0] * gd[0] + f.R[3] * gd[1] + f.R[6] * gd[2];
    float gv = a.sign * (f.R[1] * gd[0] + f.R[4] * gd[1] + f.R[7] * gd[2]);
    if constexpr (LENS == LENS_PINHOLE) {
        const NewtonTerms t = newton_terms(f.u, f.v, make_float2(f.ud, f.vd), f.L);
        const float det = t.jxx * t.jyy - t.jxy * t.jxy;
        const bool ok = !(fabsf(det) < a.eps);   // the test that rejects a Newton step
        const float gud = (t.jyy * gu - t.jxy * gv) / det, gvd = (t.jxx * gv - t.jxy * gu) / det;
        gu = ok ? gud : 0.0f;
        gv = ok ? gvd : 0.0f;
    } else if constexpr (LENS == LENS_FISHEYE) {
        gu = gv = 0.0f;   // (the fisheye solve is not differentiated: the entry point takes no grad_K with it)
    }
    const float gcx = -gu / f.fx, gcy = -gv / f.fy;
    term[12] = gcx * f.ud;
    term[13] = gcy * f.vd;
    term[14] = gcx;
    term[15] = gcy;
}

template <int PIX, int LENS>
__global__ __launch_bounds__(RAY_CHUNK) void generate_rays_bwd_runs_kernel(RayArgs a, const int64_t *__restrict__ order,
                                                                           const float *__restrict__ g_origins,
                                                                           const float *__restrict__ g_viewdirs,
                                                                           float *__restrict__ partials)
{
    __shared__ float acc[RAY_CHUNK][RAY_TERMS];   // a row per run of the chunk
    __shared__ int32_t run_cam[RAY_CHUNK];
    __shared__ int32_t wave_runs[RAY_CHUNK / NFA_WAVE];
    const int tid = threadIdx.x, lane = tid & (NFA_WAVE - 1), wave = tid / NFA_WAVE;
    const int64_t pos = (int64_t)blockIdx.x * RAY_CHUNK + tid;
    const bool in = pos < a.n;
    // the camera of a sorted position; -1: outside [0, n_cameras), -2: past the end -- runs that are not written
    auto cam_at = [&](int64_t p) -> int32_t {
        if (p >= a.n) return -2;
        const int64_t c = a.ids ? a.ids[p] : 0;
        return (uint64_t)c < (uint64_t)a.n_cameras ? (int32_t)c : -1;
    };
    const int32_t cam = cam_at(pos);
    const bool head = tid == 0 || cam_at(pos - 1) != cam;
    // the run of the lane, counted from the chunk's first ray
    const unsigned long long heads = __ballot(head);
    if (lane == 0) wave_runs[wave] = __popcll(heads);
    __syncthreads();
    int32_t run = -1, n_runs = 0;
#pragma unroll
    for (int w = 0; w < RAY_CHUNK / NFA_WAVE; ++w) {
        if (w < wave) run += wave_runs[w];
        n_runs += wave_runs[w];
    }
    run += __popcll(heads & (~0ull >> (63 - lane)));
    if (head) run_cam[run] = cam;
    for (int idx = tid; idx < n_runs * RAY_TERMS; idx += RAY_CHUNK) acc[idx / RAY_TERMS][idx % RAY_TERMS] = 0.0f;

    float term[RAY_TERMS];
#pragma unroll
    for (int j = 0; j < RAY_TERMS; ++j) term[j] = 0.0f;
    if (in && cam >= 0) {
        const int64_t ray = order ? order[pos] : pos;
        if ((uint64_t)ray < (uint64_t)a.n) {   // (never an address outside the arrays, whatever `order` holds)
            const RayFrame f = ray_frame<LENS>(a, cam, pixel_value<PIX>(a.x, ray), pixel_value<PIX>(a.y, ray));
            float go[3], gw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                go[k] = g_origins ? g_origins[3 * ray + k] : 0.0f;
                gw[k] = g_viewdirs ? g_viewdirs[3 * ray + k] : 0.0f;
            }
            ray_terms<LENS>(a, f, go, gw, term);
        }
    }
    // segmented inclusive scan over the wave: a lane ends with the sum of its run's lanes up to itself
#pragma unroll
    for (int off = 1; off < NFA_WAVE; off <<= 1) {
        const int32_t run_below = __shfl_up(run, off, NFA_WAVE);
        const bool take = run_below == run && lane >= off;
#pragma unroll
        for (int j = 0; j < RAY_TERMS; ++j) {
            const float up = __shfl_up(term[j], off, NFA_WAVE);
            if (take) term[j] += up;
        }
    }
    const int32_t next_run = __shfl_down(run, 1, NFA_WAVE);   // (by every lane: a shuffle must not sit behind a lane condition)
    const bool tail = lane == NFA_WAVE - 1 || next_run != run;
    __syncthreads();   // acc is zeroed, run_cam written
    for (int w = 0; w < RAY_CHUNK / NFA_WAVE; ++w) {
        if (w == wave && tail) {
#pragma unroll
            for (int j = 0; j < RAY_TERMS; ++j) acc[run][j] += term[j];
        }
        __syncthreads();
    }
    for (int idx = tid; idx < n_runs * RAY_TERMS; idx += RAY_CHUNK) {
        const int r = idx / RAY_TERMS, j = idx % RAY_TERMS;
        const int32_t c = run_cam[r];
        if (c >= 0) partials[((int64_t)blockIdx.x + c) * RAY_TERMS + j] = acc[r][j];
    }
}

// first sorted position whose camera is >= c
__device__ __forceinline__ int64_t first_position_of(const int64_t *__restrict__ ids, int64_t n, int64_t c)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void generate_rays_bwd_cameras_kernel(const int64_t *__restrict__ ids, int64_t n,
                                                                        const float *__restrict__ partials, int32_t pose_floats,
                                                                        float *__restrict__ grad_pose, float *__restrict__ grad_K)
{
    constexpr int SLICES = 256 / RAY_TERMS;
    __shared__ float slice_sum[SLICES][RAY_TERMS];
    __shared__ float total[RAY_TERMS];
    const int64_t cam = blockIdx.x;
    const int j = threadIdx.x % RAY_TERMS, q = threadIdx.x / RAY_TERMS;
    const int64_t s = ids ? first_position_of(ids, n, cam) : 0, e = ids ? first_position_of(ids, n, cam + 1) : n;
    float sum = 0.0f;
    if (s < e) {
        const int64_t k_last = (e - 1) / RAY_CHUNK;
        for (int64_t k = s / RAY_CHUNK + q; k <= k_last; k += SLICES) sum += partials[(k + cam) * RAY_TERMS + j];
    }
    slice_sum[q][j] = sum;
    __syncthreads();
    if (threadIdx.x < RAY_TERMS) {
        float t = slice_sum[0][threadIdx.x];
        for (int k = 1; k < SLICES; ++k) t += slice_sum[k][threadIdx.x];
        total[threadIdx.x] = t;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (grad_pose && t < pose_floats) grad_pose[cam * pose_floats + t] = t < 12 ? total[t] : 0.0f;   // (a 4x4's bottom row: 0)
    if (grad_K && t < 9) grad_K[cam * 9 + t] = t == 0 ? total[12] : t == 4 ? total[13] : t == 2 ? total[14] : t == 5 ? total[15] : 0.0f;
}

template <class F>
static void dispatch_ray_kernel(int pix, int lens, F &&f)
{
    auto with_lens = [&](auto P) {
        if (lens == LENS_PINHOLE) f(P, std::integral_constant<int, LENS_PINHOLE>{});
        else if (lens == LENS_FISHEYE) f(P, std::integral_constant<int, LENS_FISHEYE>{});
        else f(P, std::integral_constant<int, LENS_NONE>{});
    };
    if (pix == PIX_I32) with_lens(std::integral_constant<int, PIX_I32>{});
    else if (pix == PIX_I64) with_lens(std::integral_constant<int, PIX_I64>{});
    else with_lens(std::integral_constant<int, PIX_F32>{});
}

// What both entry points check, and the kernels' argument block.
static int ray_args(const char *name, const void *x, const void *y, int32_t pixel_dtype, const int64_t *camera_ids, int64_t n_rays,
                    int64_t n_cameras, const float *K, int64_t k_stride, const float *camtoworlds, int64_t pose_stride,
                    const float *distortion, int32_t n_dist, int64_t dist_stride, int32_t fisheye, int32_t opengl,
                    float pixel_center, int32_t normalize, float eps, int32_t iters, RayArgs &a, int &lens)
{
    NFA_REQUIRE(n_rays >= 0 && n_cameras >= 0, "%s: negative size", name);
    NFA_REQUIRE(n_cameras < ((int64_t)1 << 31) - 1, "%s: too many cameras", name);
    NFA_REQUIRE(pixel_dtype >= PIX_F32 && pixel_dtype <= PIX_I64, "%s: pixel_dtype must be 0 (float32), 1 (int32) or 2 (int64)", name);
    NFA_REQUIRE(fisheye ? n_dist == 4 : (n_dist == 0 || n_dist == 8),
                "%s: n_dist must be 0 (no lens) or 8 {k1,k2,p1,p2,k3,k4,k5,k6}, with fisheye 4 {k1,k2,k3,k4} (got %d)", name, n_dist);
    NFA_REQUIRE(iters >= 0, "%s: iters must be >= 0 (got %d)", name, iters);
    NFA_REQUIRE((k_stride == 0 || k_stride == 9) && (pose_stride == 0 || pose_stride == 12 || pose_stride == 16) &&
                    (dist_stride == 0 || dist_stride == n_dist),
                "%s: strides must be 0 (one shared row) or the row length: K 9, camtoworlds 12 or 16, distortion n_dist", name);
    if (n_rays == 0) return NFA_OK;
    NFA_REQUIRE(n_cameras >= 1, "%s: rays without a camera", name);
    NFA_REQUIRE(x && y && K && camtoworlds && (n_dist == 0) == (distortion == nullptr), "%s: null pointer", name);
    NFA_REQUIRE(camera_ids || n_cameras == 1, "%s: camera_ids may be NULL only with one camera", name);
    const uintptr_t pixel_align = pixel_dtype == PIX_I64 ? 8 : 4;
    NFA_REQUIRE((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % pixel_align == 0 &&
                    reinterpret_cast<uintptr_t>(camera_ids) % 8 == 0,
                "%s: x, y and camera_ids must be aligned to their element size", name);
    a.x = x; a.y = y; a.ids = camera_ids; a.n = n_rays; a.n_cameras = n_cameras;
    a.K = K; a.pose = camtoworlds; a.dist = distortion;
    a.k_stride = k_stride; a.pose_stride = pose_stride; a.dist_stride = dist_stride;
    a.sign = opengl ? -1.0f : 1.0f; a.pixel_center = pixel_center; a.eps = eps;
    a.iters = iters; a.normalize = normalize != 0;
    lens = n_dist == 0 ? LENS_NONE : (fisheye ? LENS_FISHEYE : LENS_PINHOLE);
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_generate_rays_chunk(void) { return RAY_CHUNK; }

int nfa_generate_rays_fwd(const void *x, const void *y, int32_t pixel_dtype, const int64_t *camera_ids, int64_t n_rays,
                          int64_t n_cameras, const float *K, int64_t k_stride, const float *camtoworlds, int64_t pose_stride,
                          const float *distortion, int32_t n_dist, int64_t dist_stride, int32_t fisheye, int32_t opengl,
                          float pixel_center, int32_t normalize, float eps, int32_t iters, float *origins, float *viewdirs,
                          nfa_stream_t stream)
{
    RayArgs a;
    int lens = LENS_NONE;
    const int rc = ray_args("generate_rays_fwd", x, y, pixel_dtype, camera_ids, n_rays, n_cameras, K, k_stride, camtoworlds,
                            pose_stride, distortion, n_dist, dist_stride, fisheye, opengl, pixel_center, normalize, eps, iters, a, lens);
    if (rc != NFA_OK || n_rays == 0) return rc;
    NFA_REQUIRE(origins && viewdirs, "generate_rays_fwd: null pointer");
    NFA_REQUIRE((reinterpret_cast<uintptr_t>(origins) | reinterpret_cast<uintptr_t>(viewdirs)) % 4 == 0,
                "generate_rays_fwd: origins and viewdirs must be 4-byte aligned");
    const bool aligned = all_aligned16(origins, viewdirs);
    const unsigned grid = grid_1d((n_rays + 3) / 4, 256);
    dispatch_ray_kernel(pixel_dtype, lens, [&](auto P, auto L) {
        hipLaunchKernelGGL((generate_rays_kernel<decltype(P)::value, decltype(L)::value>), dim3(grid), dim3(256), 0,
                           as_stream(stream), a, origins, viewdirs, aligned);
    });
    NFA_CHECK_LAUNCH("generate_rays_fwd");
    return NFA_OK;
}

int nfa_generate_rays_bwd(const void *x, const void *y, int32_t pixel_dtype, const int64_t *camera_ids, const int64_t *order,
                          int64_t n_rays, int64_t n_cameras, const float *K, int64_t k_stride, const float *camtoworlds,
                          int64_t pose_stride, const float *distortion, int32_t n_dist, int64_t dist_stride, int32_t fisheye,
                          int32_t opengl, float pixel_center, int32_t normalize, float eps, int32_t iters,
                          const float *g_origins, const float *g_viewdirs, float *partials, int64_t n_partial_rows,
                          int32_t pose_floats, float *grad_camtoworlds, float *grad_K, nfa_stream_t stream)
{
    RayArgs a;
    int lens = LENS_NONE;
    const int rc = ray_args("generate_rays_bwd", x, y, pixel_dtype, camera_ids, n_rays, n_cameras, K, k_stride, camtoworlds,
                            pose_stride, distortion, n_dist, dist_stride, fisheye, opengl, pixel_center, normalize, eps, iters, a, lens);
    if (rc != NFA_OK || n_rays == 0) return rc;
    NFA_REQUIRE(pose_floats == 12 || pose_floats == 16, "generate_rays_bwd: pose_floats must be 12 or 16 (got %d)", pose_floats);
    NFA_REQUIRE(!(fisheye && grad_K), "generate_rays_bwd: no gradient towards K through the fisheye lens");
    NFA_REQUIRE((g_origins || g_viewdirs) && partials && (grad_camtoworlds || grad_K), "generate_rays_bwd: null pointer");
    const int64_t n_chunks = ceil_div64(n_rays, RAY_CHUNK);
    NFA_REQUIRE(n_chunks < ((int64_t)1 << 31) - 1, "generate_rays_bwd: too many rays");
    NFA_REQUIRE(n_partial_rows >= n_chunks + n_cameras - 1,
                "generate_rays_bwd: partials must hold ceil(n_rays / chunk) + n_cameras - 1 = %lld rows (got %lld)",
                (long long)(n_chunks + n_cameras - 1), (long long)n_partial_rows);
    hipStream_t s = as_stream(stream);
    dispatch_ray_kernel(pixel_dtype, lens, [&](auto P, auto L) {
        hipLaunchKernelGGL((generate_rays_bwd_runs_kernel<decltype(P)::value, decltype(L)::value>), dim3((unsigned)n_chunks),
                           dim3(RAY_CHUNK), 0, s, a, order, g_origins, g_viewdirs, partials);
    });
    NFA_CHECK_LAUNCH("generate_rays_bwd");
    hipLaunchKernelGGL(generate_rays_bwd_cameras_kernel, dim3((unsigned)n_cameras), dim3(256), 0, s, camera_ids, n_rays, partials,
                       pose_floats, grad_camtoworlds, grad_K);
    NFA_CHECK_LAUNCH("generate_rays_bwd");
    return NFA_OK;
}

}  // extern "C"

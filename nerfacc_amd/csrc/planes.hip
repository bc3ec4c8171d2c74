// planes.hip -- the plane-factorised multiscale encoding of K-Planes (Fridovich-Keil et al. 2023, "K-Planes: Explicit
// Radiance Fields in Space, Time, and Appearance"): `interpolate_ms_features` with concat_features = True, for D = 3 (static:
// 3 planes) or D = 4 (dynamic, axis 3 is time: 6 planes) inputs in [0, 1]^D (K-Planes' u in [-1, 1] is x = (u + 1) / 2).
//
// Planes: the axis pairs (a, b), a < b, in lexicographic order -- (0,1) (0,2) (1,2) at D = 3, (0,1) (0,2) (0,3) (1,2) (1,3)
// (2,3) at D = 4.  Scale s has the resolution R_{s,d} per axis (res[s * D + d], every one >= 2); plane (s, k) is a dense
// row-major [R_b, R_a, F] block of one flat float32 table, the blocks in scale-major, then plane order, so a corner's F
// features are contiguous (4 F bytes).  F = 4, 8, 16 or 32; at most 8 scales; fewer than 2^31 floats in all.
//
// All arithmetic is float32, every operation rounded on its own (the library builds with -ffp-contract=off).
// Per axis d of a (point, scale), R = R_{s,d}:
//   p = x_d * (float)(R - 1)
//   in_d = (p >= 0 && p <= R - 1)
//   q = p >= 0 ? p : 0 (NaN gives 0), then q = q <= R - 1 ? q : R - 1      (fminf(fmaxf(p, 0), R - 1), -0 kept as it is)
//   i = min((int)floorf(q), R - 2),   f = q - (float)i                     (f in [0, 1]; 1 only at the upper border)
// i and i + 1 lie in [0, R - 1] for every input, NaN and +-inf included: nothing is read or written outside a plane.
// Per plane k = (a, b) and feature j, corners c = c_a + 2 c_b in the order 0..3:
//   w_c = (c_a ? f_a : 1 - f_a) * (c_b ? f_b : 1 - f_b)
//   v_k[j] = sum_c w_c * T_k[((i_b + c_b) R_a + i_a + c_a) F + j], summed from 0 in corner order
// which is F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True) of the [1, F, R_b, R_a] plane.
//   y[n, s F + j] = ((v_0 * v_1) * v_2) ...  left-associated in plane order (NFA_PLANE_PRODUCT), or
//                   ((v_0 + v_1) + v_2) ...                                  (NFA_PLANE_SUM, EG3D-style tri-planes).
// nerfacc_amd/encodings.py (_planegrid_torch) restates the forward in torch, bit for bit.
//
// Backward, per (point, scale), with g[j] the point's dL/dy value of column s F + j; the v_k are recomputed (nothing but x
// is kept from the forward):
//   o_k[j] = the left-associated product of the OTHER planes' v in ascending plane order (NFA_PLANE_SUM: g is used as it is)
//   gk = g[j] * o_k[j]
//   table gradient:  G_k[corner c][j] += w_c * gk          (no-return global_atomic_add_f32 into a zeroed float32 gradient)
//   dv_a, dv_b = axis.h's plane_slopes of the corner values                (d v_k / d f_a, d v_k / d f_b, corner order)
//   t_d  = sum over the planes that contain axis d, in plane order from 0, of gk * dv_d
//   share_d = sum over the scales, in scale order from 0, of (in_d ? t_d * (float)(R_{s,d} - 1) : 0)       (per lane)
//   dL/dx[n, d] = the sum of the F lanes' share_d by an xor butterfly (distances F/2, F/4, .. 1; a + b is commutative, so
//   every lane holds the same bits): no atomics, the same bits on every run.  An axis whose coordinate is outside [0, 1] or
//   not finite gets 0 (grid_sample's border rule).  No second order.
//
// Layout: lanes run over FEATURES.  A point is F consecutive lanes, a wave holds 64 / F points, a workgroup 256 / F.  A
// gather or an atomic wave-instruction is then 64 / F row segments of 4 F contiguous bytes (F = 32: two 128-byte segments,
// the shape at which float atomics run at the full chip-wide rate), and the output piece of a (point, scale) is one
// contiguous 4 F-byte store (2 F bytes for a half element type).  The F lanes of a point load the same x (one address per
// point) and compute the same indices.  The forward runs one scale per workgroup row (blockIdx.y), so a launch row reads one
// scale's planes; the backward loops over the scales inside the lane group, keeping the dL/dx shares in registers.
// Element types: y / dL/dy are float, fp16 or bf16 (NFA_ELEM_*): float32 arithmetic, one rounding as the value is stored,
// one lane per element.  x needs no alignment beyond its 4 bytes.
#include "common.hip.h"
#include "axis.h"           // Axis, locate_axis, the taps, store_elem / load_elem (shared with vmgrid.hip)
#include "plane_layout.h"   // PlaneGridDesc, plane_a / plane_b, plane_layout (shared with planereg.hip)

namespace nfa {

// Forward: one scale per workgroup row, F lanes per point.
template <int D, int F, class E, int RED>
__global__ __launch_bounds__(256) void planegrid_fwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                            int64_t n_points, const PlaneGridDesc P, E *__restrict__ y)
{
    constexpr int K = n_planes<D>(), PPB = 256 / F;
    const int s = (int)blockIdx.y;
    const int j = (int)threadIdx.x % F, lp = (int)threadIdx.x / F;
    const int64_t width = (int64_t)P.n_scales * F;
    for (int64_t n = (int64_t)blockIdx.x * PPB + lp; n < n_points; n += (int64_t)gridDim.x * PPB) {
        Axis ax[D];
#pragma unroll
        for (int d = 0; d < D; ++d) ax[d] = locate_axis(x[n * D + d], P.res[s][d]);
        float out = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int a = plane_a<D>(k), b = plane_b<D>(k);
            const Taps c = plane_taps(P.offset[s][k] + (uint32_t)j, ax[a], ax[b], (uint32_t)P.res[s][a], F);
            float T[4];
            load_taps(params, c, 0, T);
            const float v = plane_value(c.w, T);
            out = k == 0 ? v : RED == NFA_PLANE_PRODUCT ? out * v : out + v;
        }
        store_elem(y + n * width + (int64_t)s * F + j, out);
    }
}

// Backward: F lanes per point, the scales in a loop; either output may be NULL.  Every lane of a wave runs every iteration
// (the lanes past the last point recompute it and write nothing), so the butterfly below is always among live lanes.
template <int D, int F, class E, int RED>
__global__ __launch_bounds__(256) void planegrid_bwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                            const E *__restrict__ g_y, int64_t n_points, const PlaneGridDesc P,
                                                            float *__restrict__ g_params, float *__restrict__ g_x)
{
    constexpr int K = n_planes<D>(), PPB = 256 / F;
    const int j = (int)threadIdx.x % F, lp = (int)threadIdx.x / F;
    const int64_t width = (int64_t)P.n_scales * F;
    const bool want_v = g_x != nullptr || RED == NFA_PLANE_PRODUCT;   // (a sum's table gradient reads no parameter)
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < n_points; base += (int64_t)gridDim.x * PPB) {
        const bool valid = base + lp < n_points;
        const int64_t n = valid ? base + lp : n_points - 1;
        float xs[D], share[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { xs[d] = x[n * D + d]; share[d] = 0.0f; }
#pragma nounroll
        for (int s = 0; s < P.n_scales; ++s) {
            Axis ax[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ax[d] = locate_axis(xs[d], P.res[s][d]);
            const float g = load_elem(g_y + n * width + (int64_t)s * F + j);
            // a plane's taps and corner values in one object: kept apart, the same arithmetic compiles to more register moves
            // (about 1 % of this kernel's time at D = 3, measured)
            struct { Taps c; float T[4]; } ct[K];
            float v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int a = plane_a<D>(k), b = plane_b<D>(k);
                ct[k].c = plane_taps(P.offset[s][k] + (uint32_t)j, ax[a], ax[b], (uint32_t)P.res[s][a], F);
                v[k] = 0.0f;
                if (want_v) {
                    load_taps(params, ct[k].c, 0, ct[k].T);
                    v[k] = plane_value(ct[k].c.w, ct[k].T);
                }
            }
            float t[D];
#pragma unroll
            for (int d = 0; d < D; ++d) t[d] = 0.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float gk = g;
                if constexpr (RED == NFA_PLANE_PRODUCT) {
                    float o = 1.0f;
                    bool first = true;
#pragma unroll
                    for (int m = 0; m < K; ++m) {
                        if (m == k) continue;
                        o = first ? v[m] : o * v[m];
                        first = false;
                    }
                    gk = g * o;
                }
                if (g_params != nullptr && valid) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) unsafeAtomicAdd(g_params + ct[k].c.e[q], ct[k].c.w[q] * gk);
                }
                if (g_x != nullptr) {
                    const int a = plane_a<D>(k), b = plane_b<D>(k);
                    float dva, dvb;
                    plane_slopes(ax[a].f, ax[b].f, ct[k].T, dva, dvb);
                    t[a] = t[a] + gk * dva;
                    t[b] = t[b] + gk * dvb;
                }
            }
            if (g_x != nullptr) {
#pragma unroll
                for (int d = 0; d < D; ++d) share[d] = share[d] + (ax[d].in ? t[d] * ax[d].rm1 : 0.0f);
            }
        }
        if (g_x != nullptr) {
#pragma unroll
            for (int off = F / 2; off > 0; off >>= 1) {
#pragma unroll
                for (int d = 0; d < D; ++d) share[d] = share[d] + __shfl_xor(share[d], off, NFA_WAVE);
            }
            if (valid && j < D) {
                float out = share[0];
#pragma unroll
                for (int d = 1; d < D; ++d) out = j == d ? share[d] : out;
                g_x[n * D + j] = out;
            }
        }
    }
}

// ---------------------------------------------------------------- host side
struct PlaneGridArgs {
    int32_t n_dims, reduce, elem;
    int64_t n_points;
    int32_t n_scales, n_features;
    const int32_t *res_host;
};

// The checks every entry makes, in this order, and the plane table of the checked description.
static int planegrid_desc(const char *name, const PlaneGridArgs &A, PlaneGridDesc &P)
{
    NFA_REQUIRE(A.n_points >= 0, "%s: negative n_points", name);
    NFA_REQUIRE(A.n_dims == 3 || A.n_dims == 4, "%s: n_dims must be 3 or 4 (got %d)", name, A.n_dims);
    NFA_REQUIRE(A.reduce == NFA_PLANE_PRODUCT || A.reduce == NFA_PLANE_SUM,
                "%s: reduce must be NFA_PLANE_PRODUCT (0) or NFA_PLANE_SUM (1) (got %d)", name, A.reduce);
    NFA_REQUIRE(A.elem == NFA_ELEM_F32 || A.elem == NFA_ELEM_F16 || A.elem == NFA_ELEM_BF16,
                "%s: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", name, A.elem);
    NFA_REQUIRE(A.n_features == 4 || A.n_features == 8 || A.n_features == 16 || A.n_features == 32,
                "%s: n_features must be 4, 8, 16 or 32 (got %d)", name, A.n_features);
    NFA_REQUIRE(A.n_scales >= 1 && A.n_scales <= NFA_PG_MAX_SCALES, "%s: n_scales must be in 1..8 (got %d)", name, A.n_scales);
    return plane_layout(name, A.n_dims, A.n_features, A.n_scales, A.res_host, P);
}

template <class Fn>
static void dispatch_planegrid(const PlaneGridArgs &A, Fn &&f)
{
    dispatch_value<3, 4>(A.n_dims, [&](auto d) {
        dispatch_value<NFA_PLANE_PRODUCT, NFA_PLANE_SUM>(A.reduce, [&](auto r) {
            dispatch_value<4, 8, 16, 32>(A.n_features, [&](auto n) {
                dispatch_elem(A.elem, [&](auto tag) { f(d, n, r, tag); });
            });
        });
    });
}

static int planegrid_fwd(const PlaneGridArgs &A, const float *x, const float *params, void *y, nfa_stream_t stream)
{
    if (A.n_points == 0) return NFA_OK;
    PlaneGridDesc P;
    const int rc = planegrid_desc("planegrid_fwd", A, P);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(x && params && y, "planegrid_fwd: null pointer");
    const int ppb = 256 / A.n_features;
    const dim3 grid(grid_1d(A.n_points, ppb, 256 * 16 / A.n_scales + 1), A.n_scales), block(256);
    dispatch_planegrid(A, [&](auto d, auto n, auto r, auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL((planegrid_fwd_kernel<d(), n(), E, r()>), grid, block, 0, as_stream(stream), x, params, A.n_points, P,
                           static_cast<E *>(y));
    });
    NFA_CHECK_LAUNCH("planegrid_fwd");
    return NFA_OK;
}

static int planegrid_bwd(const PlaneGridArgs &A, const float *x, const float *params, const void *grad_y, float *grad_params,
                         float *grad_x, nfa_stream_t stream)
{
    if (A.n_points == 0) return NFA_OK;
    PlaneGridDesc P;
    const int rc = planegrid_desc("planegrid_bwd", A, P);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(x && params && grad_y && (grad_params || grad_x), "planegrid_bwd: null pointer");
    const int ppb = 256 / A.n_features;
    const dim3 grid(grid_1d(A.n_points, ppb)), block(256);
    dispatch_planegrid(A, [&](auto d, auto n, auto r, auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL((planegrid_bwd_kernel<d(), n(), E, r()>), grid, block, 0, as_stream(stream), x, params,
                           static_cast<const E *>(grad_y), A.n_points, P, grad_params, grad_x);
    });
    NFA_CHECK_LAUNCH("planegrid_bwd");
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int nfa_planegrid_fwd(int32_t n_dims, int32_t reduce, int32_t elem, const float *x, const float *params, int64_t n_points,
                      int32_t n_scales, int32_t n_features, const int32_t *res_host, void *y, nfa_stream_t stream)
{
    return planegrid_fwd(PlaneGridArgs{n_dims, reduce, elem, n_points, n_scales, n_features, res_host}, x, params, y, stream);
}

int nfa_planegrid_bwd(int32_t n_dims, int32_t reduce, int32_t elem, const float *x, const float *params, const void *grad_y,
                      int64_t n_points, int32_t n_scales, int32_t n_features, const int32_t *res_host, float *grad_params,
                      float *grad_x, nfa_stream_t stream)
{
    return planegrid_bwd(PlaneGridArgs{n_dims, reduce, elem, n_points, n_scales, n_features, res_host}, x, params, grad_y,
                         grad_params, grad_x, stream);
}

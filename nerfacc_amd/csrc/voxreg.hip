// voxreg.hip -- the regularisers of the dense voxel grid of voxgrid.hip (shape checks: vox_layout.h): total variation along
// the three axes with an l2, l1 or Huber penalty, and the L1 pull towards 0, on the base table g[z, y, x, c] (one flat float32
// block, row-major [R_z, R_y, R_x, C]; strides play no part).  These formulas are the contract; nothing beyond them is claimed.
//   kind    rho(d)                                  psi(d) = rho'(d)
//   l2      d d                                     2 d
//   l1      |d|                                     sign0(d)   (plane_tiles.h: 0 at 0, NaN stays NaN)
//   huber   |d| <= 1 ? 0.5 (d d) : |d| - 0.5        d < -1 ? -1 : d > 1 ? 1 : d   (NaN stays NaN)
//   tv_x = sum rho(g[z,y,x+1,c] - g[z,y,x,c]) / n_x,  n_x = C R_z R_y (R_x - 1)      likewise tv_y, tv_z
//   l1   = sum |g| / (C R_z R_y R_x)                  terms = (tv_x, tv_y, tv_z, l1)
// reduction "mean" divides by (float)n_t, the count formed on the host in double and rounded once (plane_tiles.h's
// term_scale); "sum" divides by 1.  All arithmetic is float32, every operation rounded on its own (-ffp-contract=off).
//
// Tiling.  The table is walked as the N4 = ceil(N / 4) aligned 16-byte QUADS of the flat table (N = C R_z R_y R_x floats; the
// last quad is short when N is no multiple of 4, and is then read and written float by float).  Quad q holds the floats
// 4 q .. 4 q + 3; float f sits at row = f / L (L = R_x C), xc = f - row L, z = row / R_y, y = row - z R_y (two divisions by
// multiply-and-shift, exact for every uint32), and its neighbours are the floats f -+ C (where xc >= C / xc + C < L), f -+ L
// (y >= 1 / y + 1 < R_y) and f -+ R_y L (z >= 1 / z + 1 < R_z).  For C a multiple of 4 a quad lies in one node, its six
// neighbours are aligned quads and one set of flags serves its four floats.  For C = 1 and C = 2 a quad spans nodes (and rows,
// when L is no multiple of 4): each float has its own flags; the x-neighbours come from the quad itself and from one or two
// floats next to it, the y- and z-neighbours from one 16-byte load at 4-byte alignment where all four exist and float by float
// otherwise.  A neighbour that does not exist is never loaded.  Neighbour loads are bytes another lane owns: they are served
// by a cache, not kept in registers (there is no walk along an axis).
//
// Forward, first launch, voxreg_fwd_kernel: workgroup b of NFA_VXR_LANES = 256 lanes takes the quads [2048 b, 2048 (b + 1));
// lane t the quads 2048 b + 256 k + t for k = 0 .. NFA_VXR_FWD_QUADS - 1 = 7 in that order.  Per quad, per float in address
// order, each sum takes its term where the neighbour exists, from 0:
//   sx = sx + rho(g[x+1] - g)   sy = sy + rho(g[y+1] - g)   sz = sz + rho(g[z+1] - g)   sl = sl + |g|
// (at most 4 * 8 = 32 additions per lane and sum).  plane_tiles.h's block_sum adds the lanes' (6 additions) and the 4 waves'
// (3), and the workgroup stores its quad of sums as partials[b].  Second launch, voxreg_finish_kernel, one workgroup of
// NFA_VXR_FIN = 512 lanes: plane_tiles.h's sum_partials in runs of NFA_VXR_RUN = 128 rows (at most 127 additions in a run; a
// table has at most 2^29 quads, 2^18 partial rows, 4 runs: 3 more), block_sum over 8 waves (6 + 7), terms = sum / count.
// No atomics: the same bits on every run.  The longest chain of float32 additions a term passes through:
//   4 NFA_VXR_FWD_QUADS + (6 + 3) + (NFA_VXR_RUN - 1) + (2^18 / (NFA_VXR_FIN NFA_VXR_RUN) - 1) + (6 + 7) = 32 + 9 + 127 + 3 + 13 = 184
// and every summand is non-negative, so a term's relative error is below 184 * 2^-24.
//
// Backward, voxreg_bwd_kernel, one launch in gather form: workgroup b takes the quads [1024 b, 1024 (b + 1)), lane t the quads
// 1024 b + 256 k + t, k < NFA_VXR_BWD_QUADS = 4.  With c_t = grad_terms[t] * scale_t (scale_t = (float)(1 / n_t), term_scale's
// reciprocal, or 1 with "sum"), P = the identity and k_t = 2 c_t for l2, P = psi and k_t = c_t for l1 and huber, every
// difference towards a neighbour that does not exist replaced by the literal 0:
//   gx = (x >= 1 ? P(g - g[x-1]) : 0) - (x + 1 < R_x ? P(g[x+1] - g) : 0)          likewise gy, gz
//   v  = k_x gx;   v = v + k_y gy;   v = v + k_z gz;   v = v + c_l sign0(g)
// grad_params = v: every float is written with a plain store.  nfa_voxreg_add_grad is the same kernel in place: c_t =
// weights[t] * scale_t is formed on the host by the same single float32 multiplication, and grad = grad + v where dense != 0 or
// grad != 0 (a NaN counts as non-zero).  A quad none of whose floats qualifies is neither stored nor are its neighbours
// loaded; in a stored quad the floats that do not qualify keep their bits.  nerfacc_amd/losses.py (_voxel_terms_grad_torch)
// restates v in torch, bit for bit.
//
// Indices are uint32 counts of floats or quads (a table holds fewer than 2^31 floats); they are widened to 64 bits before they
// scale a pointer, so a table beyond 4 GiB is addressed correctly.  No index depends on data.  params, partials, grad_params
// and grad must be 16-byte aligned.
#include "common.hip.h"
#include "plane_tiles.h"   // load_quad, sign0, block_sum, sum_partials, term_scale
#include "vox_layout.h"

namespace nfa {

#define NFA_VXR_LANES 256      // lanes of a workgroup of the forward and the backward
#define NFA_VXR_FWD_QUADS 8    // quads a lane of the forward adds
#define NFA_VXR_BWD_QUADS 4    // quads a lane of the backward writes
#define NFA_VXR_FIN 512        // lanes of the finish kernel
#define NFA_VXR_RUN 128        // partial rows a lane of the finish kernel adds before it starts a new run

enum : uint32_t { VX_LEFT = 1, VX_RIGHT = 2, VX_UP = 4, VX_DOWN = 8, VX_BACK = 16, VX_FRONT = 32, VX_VALID = 64 };

// n / d for every uint32 n (Granlund and Montgomery 1994, the round-up method): t = umulhi(m, n), (t + ((n - t) >> s1)) >> s2
struct VXDiv {
    uint32_t m, s1, s2;
};
__host__ __device__ __forceinline__ uint32_t vx_quot(uint32_t n, const VXDiv &d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = __umulhi(d.m, n);
#else
    const uint32_t t = (uint32_t)(((uint64_t)d.m * n) >> 32);
#endif
    return (t + ((n - t) >> d.s1)) >> d.s2;
}

struct VXDesc {
    uint32_t n, n4;        // floats and quads of the table
    uint32_t C, L, S;      // the x-, y- and z-neighbour's distance in floats: C, R_x C, R_y R_x C
    uint32_t Ry, Rz;
    VXDiv by_L, by_Ry;
};
struct VXVec {
    float v[4];
};

typedef float vx_v4f_u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at any float's address

template <int KIND>
__device__ __forceinline__ float vx_rho(float d)
{
    if constexpr (KIND == NFA_VOXREG_L2) return d * d;
    else if constexpr (KIND == NFA_VOXREG_L1) return fabsf(d);
    else return fabsf(d) <= 1.0f ? 0.5f * (d * d) : fabsf(d) - 0.5f;
}
// P of the backward: the identity for l2 (the factor 2 is in k_t), psi otherwise
template <int KIND>
__device__ __forceinline__ float vx_p(float d)
{
    if constexpr (KIND == NFA_VOXREG_L2) return d;
    else if constexpr (KIND == NFA_VOXREG_L1) return sign0(d);
    else return d < -1.0f ? -1.0f : d > 1.0f ? 1.0f : d;
}

// which neighbours the float at (xc, y, z) has
__device__ __forceinline__ uint32_t vx_flags(const VXDesc &D, uint32_t xc, uint32_t y, uint32_t z)
{
    return (xc >= D.C ? VX_LEFT : 0u) | (xc + D.C < D.L ? VX_RIGHT : 0u) | (y >= 1u ? VX_UP : 0u) | (y + 1u < D.Ry ? VX_DOWN : 0u) |
           (z >= 1u ? VX_BACK : 0u) | (z + 1u < D.Rz ? VX_FRONT : 0u) | VX_VALID;
}

// the four floats at p where their flag `bit` is set; the others are not loaded and come back 0
template <int CF>
__device__ __forceinline__ nfa_v4f vx_load(const float *p, const uint32_t (&fl)[4], uint32_t bit)
{
    nfa_v4f r = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (CF == 0) {   // one node: the flags agree, the neighbour is an aligned quad
        if (fl[0] & bit) r = load_quad(p);
    } else if (fl[0] & fl[1] & fl[2] & fl[3] & bit) {
        r = *reinterpret_cast<const vx_v4f_u *>(p);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (fl[e] & bit) r[e] = p[e];
        }
    }
    return r;
}

// A quad with its neighbours: v, and per axis the floats before (m) and after (p) it (BOTH: the forward needs `after` only).
struct VXQuad {
    nfa_v4f v, xm, xp, ym, yp, zm, zp;
    uint32_t fl[4];
};
// CF: 1 or 2 = C, 0: C is a multiple of 4.  `own` is the quad's address, f0 = 4 q its first float.
template <int CF, bool BOTH>
__device__ __forceinline__ void vx_gather(const float *__restrict__ own, const VXDesc &D, uint32_t f0, VXQuad &Q)
{
    const uint32_t row = vx_quot(f0, D.by_L), z0 = vx_quot(row, D.by_Ry);
    uint32_t xc = f0 - row * D.L, y = row - z0 * D.Ry, z = z0;
    const uint32_t nv = min(4u, D.n - f0);   // (4 when C is a multiple of 4)
    if constexpr (CF == 0) {
        Q.fl[0] = Q.fl[1] = Q.fl[2] = Q.fl[3] = vx_flags(D, xc, y, z);
        Q.v = load_quad(own);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Q.fl[e] = (uint32_t)e < nv ? vx_flags(D, xc, y, z) : 0u;
            if (++xc == D.L) {
                xc = 0u;
                if (++y == D.Ry) {
                    y = 0u;
                    ++z;
                }
            }
        }
        Q.v = vx_load<CF>(own, Q.fl, VX_VALID);
    }
    if constexpr (BOTH) {
        Q.ym = vx_load<CF>(own - D.L, Q.fl, VX_UP);
        Q.zm = vx_load<CF>(own - D.S, Q.fl, VX_BACK);
    }
    Q.yp = vx_load<CF>(own + D.L, Q.fl, VX_DOWN);
    Q.zp = vx_load<CF>(own + D.S, Q.fl, VX_FRONT);
    if constexpr (CF == 0) {
        if constexpr (BOTH) Q.xm = vx_load<0>(own - D.C, Q.fl, VX_LEFT);
        Q.xp = vx_load<0>(own + D.C, Q.fl, VX_RIGHT);
    } else {   // the neighbour CF floats away is in the quad itself, except at the quad's ends
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (BOTH) Q.xm[e] = e >= CF ? Q.v[e >= CF ? e - CF : 0] : (Q.fl[e] & VX_LEFT) ? own[e - CF] : 0.0f;
            Q.xp[e] = e + CF < 4 ? Q.v[e + CF < 4 ? e + CF : 0] : (Q.fl[e] & VX_RIGHT) ? own[e + CF] : 0.0f;
        }
    }
}

template <int KIND, int CF>
__global__ __launch_bounds__(NFA_VXR_LANES) void voxreg_fwd_kernel(const float *__restrict__ params, const VXDesc D,
                                                                   float *__restrict__ partials)
{
    __shared__ float lds[NFA_VXR_LANES / NFA_WAVE * 4];
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t q0 = blockIdx.x * (NFA_VXR_LANES * NFA_VXR_FWD_QUADS) + threadIdx.x;   // (< 2^29 + 2^11)
#pragma unroll 2
    for (uint32_t k = 0; k < NFA_VXR_FWD_QUADS; ++k) {
        const uint32_t q = q0 + k * NFA_VXR_LANES;
        if (q >= D.n4) break;
        VXQuad Q;
        vx_gather<CF, false>(params + (size_t)q * 4, D, q * 4u, Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = Q.v[e];
            if (Q.fl[e] & VX_RIGHT) sum[0] = sum[0] + vx_rho<KIND>(Q.xp[e] - v);
            if (Q.fl[e] & VX_DOWN) sum[1] = sum[1] + vx_rho<KIND>(Q.yp[e] - v);
            if (Q.fl[e] & VX_FRONT) sum[2] = sum[2] + vx_rho<KIND>(Q.zp[e] - v);
            if (Q.fl[e] & VX_VALID) sum[3] = sum[3] + fabsf(v);
        }
    }
    block_sum<4, NFA_VXR_LANES / NFA_WAVE>(sum, lds);
    if (threadIdx.x == 0) store_f4(partials + (size_t)blockIdx.x * 4, sum[0], sum[1], sum[2], sum[3]);
}

__global__ __launch_bounds__(NFA_VXR_FIN) void voxreg_finish_kernel(const float *__restrict__ partials, uint32_t n_rows, const VXVec count,
                                                                    float *__restrict__ terms)
{
    __shared__ float lds[NFA_VXR_FIN / NFA_WAVE * 4];
    const nfa_v4f ps = sum_partials<NFA_VXR_FIN, NFA_VXR_RUN>(partials, 0u, n_rows);
    float acc[4] = {ps[0], ps[1], ps[2], ps[3]};
    block_sum<4, NFA_VXR_FIN / NFA_WAVE>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) terms[t] = acc[t] / count.v[t];
    }
}

// ADD: grad_terms is not read, cw holds c_t itself and `out` is the gradient added to in place; otherwise c_t = grad_terms[t] cw[t]
template <int KIND, int CF, bool ADD>
__global__ __launch_bounds__(NFA_VXR_LANES) void voxreg_bwd_kernel(const float *__restrict__ params, const VXDesc D,
                                                                   const float *__restrict__ grad_terms, const VXVec cw, int32_t dense,
                                                                   float *out)
{
    float c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = ADD ? cw.v[t] : grad_terms[t] * cw.v[t];
    const float two = KIND == NFA_VOXREG_L2 ? 2.0f : 1.0f;   // (k_t = 2 c_t for l2; 1 c_t is c_t)
    const float kx = two * c[0], ky = two * c[1], kz = two * c[2], cl = c[3];
    const uint32_t q0 = blockIdx.x * (NFA_VXR_LANES * NFA_VXR_BWD_QUADS) + threadIdx.x;   // (< 2^29 + 2^10)
#pragma unroll 2
    for (uint32_t k = 0; k < NFA_VXR_BWD_QUADS; ++k) {
        const uint32_t q = q0 + k * NFA_VXR_LANES;
        if (q >= D.n4) break;
        const uint32_t nv = min(4u, D.n - q * 4u);
        float *dst = out + (size_t)q * 4;
        nfa_v4f g = {0.0f, 0.0f, 0.0f, 0.0f};
        bool take[4] = {true, true, true, true};
        if constexpr (ADD) {
            if (CF == 0 || nv == 4u) g = load_quad(dst);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((uint32_t)e < nv) g[e] = dst[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) take[e] = (uint32_t)e < nv && (dense != 0 || g[e] != 0.0f);
            if (!(take[0] || take[1] || take[2] || take[3])) continue;
        }
        VXQuad Q;
        vx_gather<CF, true>(params + (size_t)q * 4, D, q * 4u, Q);
        nfa_v4f o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = Q.v[e];
            const uint32_t fl = Q.fl[e];
            const float gx = ((fl & VX_LEFT) ? vx_p<KIND>(p - Q.xm[e]) : 0.0f) - ((fl & VX_RIGHT) ? vx_p<KIND>(Q.xp[e] - p) : 0.0f);
            const float gy = ((fl & VX_UP) ? vx_p<KIND>(p - Q.ym[e]) : 0.0f) - ((fl & VX_DOWN) ? vx_p<KIND>(Q.yp[e] - p) : 0.0f);
            const float gz = ((fl & VX_BACK) ? vx_p<KIND>(p - Q.zm[e]) : 0.0f) - ((fl & VX_FRONT) ? vx_p<KIND>(Q.zp[e] - p) : 0.0f);
            float v = kx * gx;
            v = v + ky * gy;
            v = v + kz * gz;
            v = v + cl * sign0(p);
            o[e] = ADD ? (take[e] ? g[e] + v : g[e]) : v;
        }
        if (CF == 0 || nv == 4u) *reinterpret_cast<nfa_v4f *>(dst) = o;
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((uint32_t)e < nv) dst[e] = o[e];
            }
        }
    }
}

// ---------------------------------------------------------------- host side
static VXDiv vx_div(uint32_t d)   // 1 <= d < 2^31
{
    uint32_t l = 0;
    while (((uint64_t)1 << l) < d) ++l;   // ceil(log2 d)
    VXDiv r;
    r.m = (uint32_t)(((((uint64_t)1 << l) - d) << 32) / d + 1);
    r.s1 = l < 1 ? l : 1;
    r.s2 = l > 0 ? l - 1 : 0;
    return r;
}

struct VXHost {
    VXDesc D;
    VXVec count, scale;   // per term: the divisor (forward), the factor of its gradient (backward); 1 with "sum"
    uint32_t rows, blocks_bwd;
    int cf;               // C for C <= 2, else 0
};

// The checks every entry makes, in this order: n_features; res_host (null; a resolution below 2; the size limit); kind;
// reduction; then the tiling and the counts of the checked shape.
static int voxreg_plan(const char *name, int32_t C, const int32_t *res_host, int32_t kind, int32_t reduction, VXHost &h)
{
    int rc = vox_check_c(name, C);
    if (rc != NFA_OK) return rc;
    int32_t res[3];
    int64_t total;
    if ((rc = vox_check_res(name, "", C, res_host, res, total)) != NFA_OK) return rc;
    NFA_REQUIRE(kind >= NFA_VOXREG_L2 && kind <= NFA_VOXREG_HUBER,
                "%s: kind must be NFA_VOXREG_L2, NFA_VOXREG_L1 or NFA_VOXREG_HUBER (got %d)", name, kind);
    NFA_REQUIRE(reduction == NFA_VOXREG_MEAN || reduction == NFA_VOXREG_SUM, "%s: reduction must be NFA_VOXREG_MEAN or NFA_VOXREG_SUM (got %d)",
                name, reduction);
    h = {};
    VXDesc &D = h.D;
    D.n = (uint32_t)total;
    D.n4 = (uint32_t)ceil_div64(total, 4);
    D.C = (uint32_t)C;
    D.L = (uint32_t)res[0] * D.C;   // (each a divisor of the total: < 2^31)
    D.S = (uint32_t)res[1] * D.L;
    D.Ry = (uint32_t)res[1];
    D.Rz = (uint32_t)res[2];
    D.by_L = vx_div(D.L);
    D.by_Ry = vx_div(D.Ry);
    const double c = C, rx = res[0], ry = res[1], rz = res[2];
    const double cnt[4] = {c * rz * ry * (rx - 1.0), c * rz * (ry - 1.0) * rx, c * (rz - 1.0) * ry * rx, c * rz * ry * rx};
    for (int t = 0; t < 4; ++t) {
        term_scale(cnt[t], h.count.v[t], h.scale.v[t]);
        if (reduction == NFA_VOXREG_SUM) h.count.v[t] = h.scale.v[t] = 1.0f;
    }
    h.rows = (uint32_t)ceil_div64(D.n4, NFA_VXR_LANES * NFA_VXR_FWD_QUADS);        // (at most 2^18)
    h.blocks_bwd = (uint32_t)ceil_div64(D.n4, NFA_VXR_LANES * NFA_VXR_BWD_QUADS);  // (at most 2^19)
    h.cf = C <= 2 ? C : 0;
    return NFA_OK;
}

template <bool ADD>
static void voxreg_launch_bwd(const VXHost &h, int32_t kind, const float *params, const float *grad_terms, const VXVec &cw, int32_t dense,
                              float *out, nfa_stream_t stream)
{
    dispatch_value<NFA_VOXREG_L2, NFA_VOXREG_L1, NFA_VOXREG_HUBER>(kind, [&](auto k) {
        dispatch_value<0, 1, 2>(h.cf, [&](auto cf) {
            hipLaunchKernelGGL((voxreg_bwd_kernel<k(), cf(), ADD>), dim3(h.blocks_bwd), dim3(NFA_VXR_LANES), 0, as_stream(stream), params,
                               h.D, grad_terms, cw, dense, out);
        });
    });
}

}  // namespace nfa

using namespace nfa;

int64_t nfa_voxreg_partials(int32_t n_features, const int32_t *res_host)
{
    VXHost h;
    if (voxreg_plan("voxreg_partials", n_features, res_host, NFA_VOXREG_L2, NFA_VOXREG_MEAN, h) != NFA_OK) return -1;
    return (int64_t)h.rows;
}

int nfa_voxreg_fwd(const float *params, int32_t n_features, const int32_t *res_host, int32_t kind, int32_t reduction, float *partials,
                   int64_t n_partials, float *terms, nfa_stream_t stream)
{
    VXHost h;
    const int rc = voxreg_plan("voxreg_fwd", n_features, res_host, kind, reduction, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && partials && terms, "voxreg_fwd: null pointer");
    NFA_REQUIRE(all_aligned16(params, partials), "voxreg_fwd: params and partials must be 16-byte aligned");
    NFA_REQUIRE(n_partials >= (int64_t)h.rows, "voxreg_fwd: n_partials is below nfa_voxreg_partials (%lld < %lld)", (long long)n_partials,
                (long long)h.rows);
    dispatch_value<NFA_VOXREG_L2, NFA_VOXREG_L1, NFA_VOXREG_HUBER>(kind, [&](auto k) {
        dispatch_value<0, 1, 2>(h.cf, [&](auto cf) {
            hipLaunchKernelGGL((voxreg_fwd_kernel<k(), cf()>), dim3(h.rows), dim3(NFA_VXR_LANES), 0, as_stream(stream), params, h.D, partials);
        });
    });
    hipLaunchKernelGGL(voxreg_finish_kernel, dim3(1), dim3(NFA_VXR_FIN), 0, as_stream(stream), partials, h.rows, h.count, terms);
    NFA_CHECK_LAUNCH("voxreg_fwd");
    return NFA_OK;
}

int nfa_voxreg_bwd(const float *params, int32_t n_features, const int32_t *res_host, int32_t kind, int32_t reduction,
                   const float *grad_terms, float *grad_params, nfa_stream_t stream)
{
    VXHost h;
    const int rc = voxreg_plan("voxreg_bwd", n_features, res_host, kind, reduction, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && grad_terms && grad_params, "voxreg_bwd: null pointer");
    NFA_REQUIRE(all_aligned16(params, grad_params), "voxreg_bwd: params and grad_params must be 16-byte aligned");
    voxreg_launch_bwd<false>(h, kind, params, grad_terms, h.scale, 1, grad_params, stream);
    NFA_CHECK_LAUNCH("voxreg_bwd");
    return NFA_OK;
}

int nfa_voxreg_add_grad(const float *params, int32_t n_features, const int32_t *res_host, int32_t kind, int32_t reduction,
                        const float *weights, int32_t dense, float *grad, nfa_stream_t stream)
{
    VXHost h;
    const int rc = voxreg_plan("voxreg_add_grad", n_features, res_host, kind, reduction, h);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(params && weights && grad, "voxreg_add_grad: null pointer");
    NFA_REQUIRE(all_aligned16(params, grad), "voxreg_add_grad: params and grad must be 16-byte aligned");
    VXVec c;
    for (int t = 0; t < 4; ++t) c.v[t] = weights[t] * h.scale.v[t];   // (one float32 multiplication, as the backward's)
    voxreg_launch_bwd<true>(h, kind, params, nullptr, c, dense, grad, stream);
    NFA_CHECK_LAUNCH("voxreg_add_grad");
    return NFA_OK;
}

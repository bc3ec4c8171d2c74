// voxgrid.hip -- a dense 3-D feature grid sampled trilinearly: DVGO's density (C = 1) and feature (C = 12) grids (Sun et al.
// 2022, "Direct Voxel Grid Optimization"), TiNeuVox's feature volume with its multi-distance interpolation (Fang et al. 2022,
// "Fast Dynamic Radiance Fields with Time-Aware Neural Voxels": `mult_dist_interp`), ReLU-Fields-style grids; x [N, 3] in
// [0, 1]^3, and the resampling of the table (DVGO's `scale_volume_grid`).
//
// Parameters: one flat float32 table of fewer than 2^31 floats, a row-major [R_z, R_y, R_x, C] block: x runs fastest among the
// nodes, a node's C values are contiguous.  Every R_d >= 2; C is 1, 2 or a multiple of 4 up to 64.  (With the table seen as
// g[z, y, x, c], g.permute(3, 2, 1, 0)[None] is the [1, C, N_x, N_y, N_z] tensor DVGO and TiNeuVox hand to grid_sample with
// the coordinates flipped.)
//
// Strides s_0 .. s_{S-1} (S in 1..4, each in 1..8): stride s has the nodes at the table indices 0, s, 2 s, .. per axis,
// n_d = ceil(R_d / s) >= 2 of them, the last one at s (n_d - 1) <= R_d - 1: the view grid[:, :, ::s, ::s, ::s].  Stride k fills
// the columns k C .. k C + C - 1 of y [N, S C].
//
// All arithmetic is float32, every operation rounded on its own (the library builds with -ffp-contract=off).  Per stride and
// axis d the locate step is axis.h's locate_axis(x_d, n_d) (border clamp, NaN -> node 0, the `in` flag, i <= n_d - 2, f in
// [0, 1]), the lower node at the table index s i.  Per component j, corners k = k_x + 2 k_y + 4 k_z in the order 0..7:
//   w_k = ((k_x ? f_x : 1 - f_x) * (k_y ? f_y : 1 - f_y)) * (k_z ? f_z : 1 - f_z)                      (axis.h's volume_taps)
//   T_k = table[(((s (i_z + k_z)) R_y + s (i_y + k_y)) R_x + s (i_x + k_x)) C + j]
//   y[n, k C + j] = sum_k w_k * T_k, summed from 0 in corner order                                     (axis.h's volume_value)
// which is F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True) of the strided view.
// nerfacc_amd/encodings.py (_voxgrid_torch) restates the forward in torch, bit for bit.
//
// Backward, per point; nothing but x is kept from the forward.  g[j] is dL/dy of column k C + j:
//   table gradient:  G[corner k][j] += w_k * g[j]          (no-return global_atomic_add_f32 into a zeroed float32 gradient)
//   dv_x, dv_y, dv_z = axis.h's volume_slopes (d value / d f_d, corner order)
//   t_d += g[j] * dv_d over the lane's components in ascending order, from 0, per stride
//   acc_d += in_d ? t_d * (float)(n_d - 1) : 0 over the strides in ascending order, from 0, per lane
//   dL/dx[n, d] = the L lanes' acc_d combined by an xor butterfly at the distances L / 2, L / 4, .. 1
// No atomics on dL/dx: the same bits on every run.  An axis whose coordinate is outside [0, 1] or not finite gets 0.
// Either gradient is switched off by a null pointer.  No second order.
//
// Layout: lanes run over COMPONENTS.  L = the largest power of two <= 32 that divides C for C >= 4 (4 -> 4, 12 -> 4, 16 -> 16,
// 24 -> 8, 48 -> 16, 64 -> 32); a point is L consecutive lanes, lane l owns the components l, l + L, ..., so a corner gather and
// a corner's atomics of one round are 64 / L row pieces of 4 L contiguous bytes per wave-instruction, and an output piece one
// contiguous 4 L-byte store.  C = 1 and C = 2: one lane per point (L = 1); the lane loads a whole cell, and at stride 1 the two
// x-neighbours of a corner pair are adjacent in memory, so the cell is 4 loads of 8 C bytes instead of 8 of 4 C.  The strides
// are a loop inside the pass: the point is read once and every output row written once.  Every lane of a wave runs every
// iteration (the lanes past the last point recompute it and write nothing), so a butterfly is always among live lanes.
// Element types: y / dL/dy are float, fp16 or bf16 (NFA_ELEM_*): float32 arithmetic, one rounding as the value is stored.
// Indices into the table are uint32 counts of floats (< 2^31); they are widened to 64 bits before they scale a pointer, so a
// table beyond 4 GiB is addressed correctly.
//
// Resampling (nfa_voxgrid_resample): every destination node is the trilinear sample of the source table at, per axis,
// p = (float)i' * ((float)(R - 1) / (float)(R' - 1)) (the quotient formed once on the host), located by axis.h's locate_pos
// and combined with the forward's tap arithmetic: F.interpolate(mode="trilinear", align_corners=True).  A destination
// node is a group of L lanes (the forward's mapping: its taps are formed once, its components are the lanes' loop) and a
// workgroup a piece of a destination x-row, so the y and z positions are the workgroup's and no lane divides an index; the
// stores of a workgroup are one contiguous piece of the table.  Each axis has its own R and
// R': up, down or unchanged.  At R' = R, p = i' exactly and a node copies its source (finite values; the sum from 0 turns a
// -0 into +0).
#include "common.hip.h"
#include "axis.h"   // Axis, locate_axis / locate_pos, the volume taps, store_elem / load_elem (shared with planes.hip, vmgrid.hip)
#include "vox_layout.h"   // vox_check_c, vox_check_res (shared with voxreg.hip)

namespace nfa {

#define NFA_VOX_MAX_STRIDES 4
#define NFA_VOX_BLOCK 256

struct VoxDesc {
    int32_t res[3];                        // (R_x, R_y, R_z)
    int32_t C, n_strides;
    int32_t stride[NFA_VOX_MAX_STRIDES];
    int32_t n[NFA_VOX_MAX_STRIDES][3];     // nodes per axis of stride k
};

// A point's position in stride k of the table.
struct VoxCell {
    Axis ax[3];
    VolumeTaps t;
    bool adjacent;   // the x-neighbours of a corner pair are adjacent nodes of the table (stride 1)
};
__device__ __forceinline__ VoxCell vox_cell(const float (&p)[3], const VoxDesc &V, int k)
{
    VoxCell c;
#pragma unroll
    for (int d = 0; d < 3; ++d) c.ax[d] = locate_axis(p[d], V.n[k][d]);
    const uint32_t s = (uint32_t)V.stride[k], C = (uint32_t)V.C, Rx = (uint32_t)V.res[0], Ry = (uint32_t)V.res[1];
    const uint32_t da = s * C, db = da * Rx, dc = db * Ry;
    c.t = volume_taps(c.ax[2].i * dc + c.ax[1].i * db + c.ax[0].i * da, c.ax[0], c.ax[1], c.ax[2], da, db, dc);
    c.adjacent = s == 1;
    return c;
}

// body(j, T) for the lane's components j with their 8 corner values T (zeros when `load` is false).  CF > 0: the lane owns all
// CF components and loads the cell's nodes whole; CF == 0: lane l of L owns l, l + L, ..
template <int L, int CF, class Body>
__device__ __forceinline__ void for_components(const float *__restrict__ table, const VoxCell &c, int l, int C, bool load, Body &&body)
{
    if constexpr (CF > 0) {
        typedef float Pair __attribute__((ext_vector_type(2 * CF), aligned(4)));   // two adjacent nodes, 4-byte aligned
        float p[4][2 * CF] = {};
        if (load) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (c.adjacent) {
                    const Pair v = *reinterpret_cast<const Pair *>(table + c.t.e[2 * q]);
#pragma unroll
                    for (int i = 0; i < 2 * CF; ++i) p[q][i] = v[i];
                } else {
                    __builtin_memcpy(p[q], table + c.t.e[2 * q], 4 * CF);
                    __builtin_memcpy(p[q] + CF, table + c.t.e[2 * q + 1], 4 * CF);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CF; ++j) {
            float T[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) T[k] = p[k >> 1][(k & 1) * CF + j];
            body(j, T);
        }
    } else {
        for (int j = l; j < C; j += L) {
            float T[8] = {};
            if (load) {
#pragma unroll
                for (int k = 0; k < 8; ++k) T[k] = table[c.t.e[k] + (uint32_t)j];
            }
            body(j, T);
        }
    }
}

// Forward: L lanes per point, the strides and the lane's components in loops.
template <int L, int CF, class E>
__global__ __launch_bounds__(NFA_VOX_BLOCK) void voxgrid_fwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                                    int64_t n_points, const VoxDesc V, E *__restrict__ y)
{
    constexpr int PPB = NFA_VOX_BLOCK / L;
    const int l = (int)threadIdx.x % L, lp = (int)threadIdx.x / L;
    const int C = V.C, width = V.n_strides * C;
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < n_points; base += (int64_t)gridDim.x * PPB) {
        const bool valid = base + lp < n_points;
        const int64_t n = valid ? base + lp : n_points - 1;
        const float p[3] = {x[n * 3], x[n * 3 + 1], x[n * 3 + 2]};
        for (int k = 0; k < V.n_strides; ++k) {
            const VoxCell c = vox_cell(p, V, k);
            E *row = y + n * width + k * C;
            for_components<L, CF>(params, c, l, C, true, [&](int j, const float (&T)[8]) {
                const float v = volume_value(c.t.w, T);
                if (valid) store_elem(row + j, v);
            });
        }
    }
}

// Backward: L lanes per point; either output may be NULL.
template <int L, int CF, class E>
__global__ __launch_bounds__(NFA_VOX_BLOCK) void voxgrid_bwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                                    const E *__restrict__ g_y, int64_t n_points, const VoxDesc V,
                                                                    float *__restrict__ g_params, float *__restrict__ g_x)
{
    constexpr int PPB = NFA_VOX_BLOCK / L;
    const int l = (int)threadIdx.x % L, lp = (int)threadIdx.x / L;
    const int C = V.C, width = V.n_strides * C;
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < n_points; base += (int64_t)gridDim.x * PPB) {
        const bool valid = base + lp < n_points;
        const int64_t n = valid ? base + lp : n_points - 1;
        const float p[3] = {x[n * 3], x[n * 3 + 1], x[n * 3 + 2]};
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < V.n_strides; ++k) {
            const VoxCell c = vox_cell(p, V, k);
            const E *g_row = g_y + n * width + k * C;
            float t[3] = {0.0f, 0.0f, 0.0f};
            for_components<L, CF>(params, c, l, C, g_x != nullptr, [&](int j, const float (&T)[8]) {
                const float g = load_elem(g_row + j);
                if (g_params != nullptr && valid) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) unsafeAtomicAdd(g_params + (c.t.e[q] + (uint32_t)j), c.t.w[q] * g);
                }
                if (g_x != nullptr) {
                    float dv[3];
                    volume_slopes(c.ax[0].f, c.ax[1].f, c.ax[2].f, T, dv[0], dv[1], dv[2]);
#pragma unroll
                    for (int d = 0; d < 3; ++d) t[d] = t[d] + g * dv[d];
                }
            });
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[d] = acc[d] + (c.ax[d].in ? t[d] * c.ax[d].rm1 : 0.0f);
        }
        if (g_x != nullptr) {
#pragma unroll
            for (int off = L / 2; off > 0; off >>= 1) {
#pragma unroll
                for (int d = 0; d < 3; ++d) acc[d] = acc[d] + __shfl_xor(acc[d], off, NFA_WAVE);
            }
            if constexpr (L == 1) {
                if (valid) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) g_x[n * 3 + d] = acc[d];
                }
            } else {
                if (valid && l < 3) g_x[n * 3 + l] = l == 0 ? acc[0] : l == 1 ? acc[1] : acc[2];   // lane d of the group owns dL/dx[n, d]
            }
        }
    }
}

// Resample: L lanes per destination node, a workgroup per piece of a destination x-row (blockIdx.x: rows (i'_y, i'_z),
// blockIdx.y: pieces of 256 / L nodes along x).
struct VoxResample {
    int32_t src_res[3], dst_res[3];
    float scale[3];     // (float)(R_d - 1) / (float)(R'_d - 1)
    uint32_t C;
};
template <int L>
__global__ __launch_bounds__(256) void voxgrid_resample_kernel(const float *__restrict__ src, const VoxResample R, float *__restrict__ dst)
{
    constexpr uint32_t NPB = 256 / L;
    const uint32_t l = threadIdx.x % L, ln = threadIdx.x / L;
    const uint32_t C = R.C, Wx = (uint32_t)R.dst_res[0], Wy = (uint32_t)R.dst_res[1], n_rows = Wy * (uint32_t)R.dst_res[2];
    const uint32_t da = C, db = C * (uint32_t)R.src_res[0], dc = db * (uint32_t)R.src_res[1];
    for (uint32_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const Axis b = locate_pos((float)(row % Wy) * R.scale[1], R.src_res[1]);
        const Axis c = locate_pos((float)(row / Wy) * R.scale[2], R.src_res[2]);
        for (uint32_t ix = blockIdx.y * NPB + ln; ix < Wx; ix += gridDim.y * NPB) {
            const Axis a = locate_pos((float)ix * R.scale[0], R.src_res[0]);
            const VolumeTaps t = volume_taps(c.i * dc + b.i * db + a.i * da, a, b, c, da, db, dc);
            float *out = dst + (row * Wx + ix) * C;   // (a count of floats below 2^31, widened before it scales the pointer)
            for (uint32_t j = l; j < C; j += L) {
                float T[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) T[k] = src[t.e[k] + j];
                out[j] = volume_value(t.w, T);
            }
        }
    }
}

// ---------------------------------------------------------------- host side
// (the checks of a feature count and a resolution table: vox_layout.h's vox_check_c and vox_check_res)
struct VoxArgs {
    int32_t elem;
    int64_t n_points;
    int32_t C;
    const int32_t *res_host;
    int32_t n_strides;
    const int32_t *strides_host;
};
static int vox_desc(const char *name, const VoxArgs &A, VoxDesc &V)
{
    V = {};
    NFA_REQUIRE(A.n_points >= 0, "%s: negative n_points", name);
    NFA_REQUIRE(A.elem == NFA_ELEM_F32 || A.elem == NFA_ELEM_F16 || A.elem == NFA_ELEM_BF16,
                "%s: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", name, A.elem);
    int rc = vox_check_c(name, A.C);
    if (rc != NFA_OK) return rc;
    int64_t total;
    if ((rc = vox_check_res(name, "", A.C, A.res_host, V.res, total)) != NFA_OK) return rc;
    V.C = A.C;
    NFA_REQUIRE(A.n_strides >= 1 && A.n_strides <= NFA_VOX_MAX_STRIDES, "%s: n_strides must be in 1..%d (got %d)", name,
                NFA_VOX_MAX_STRIDES, A.n_strides);
    NFA_REQUIRE(A.strides_host != nullptr, "%s: null stride table", name);
    V.n_strides = A.n_strides;
    for (int k = 0; k < A.n_strides; ++k) {
        const int32_t s = A.strides_host[k];
        NFA_REQUIRE(s >= 1 && s <= 8, "%s: stride %d is %d (must be in 1..8)", name, k, s);
        V.stride[k] = s;
        for (int d = 0; d < 3; ++d) {
            V.n[k][d] = (V.res[d] + s - 1) / s;
            NFA_REQUIRE(V.n[k][d] >= 2, "%s: stride %d leaves fewer than 2 nodes along axis %d (resolution %d)", name, s, d, V.res[d]);
        }
    }
    return NFA_OK;
}

// the lane-group width: one lane per point for C <= 2, else the largest power of two <= 32 that divides C
static int vox_lanes(int32_t C) { return C <= 2 ? 1 : C % 32 == 0 ? 32 : C % 16 == 0 ? 16 : C % 8 == 0 ? 8 : 4; }

// f(lanes, whole-cell component count (0: the lanes share the components), element tag)
template <class Fn>
static void dispatch_vox(const VoxArgs &A, Fn &&f)
{
    dispatch_elem(A.elem, [&](auto tag) {
        if (A.C <= 2) dispatch_value<1, 2>(A.C, [&](auto cf) { f(std::integral_constant<int, 1>{}, cf, tag); });
        else dispatch_value<4, 8, 16, 32>(vox_lanes(A.C), [&](auto lanes) { f(lanes, std::integral_constant<int, 0>{}, tag); });
    });
}

static int voxgrid_fwd(const VoxArgs &A, const float *x, const float *params, void *y, nfa_stream_t stream)
{
    if (A.n_points == 0) return NFA_OK;
    VoxDesc V;
    const int rc = vox_desc("voxgrid_fwd", A, V);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(x && params && y, "voxgrid_fwd: null pointer");
    const dim3 grid(grid_1d(A.n_points, NFA_VOX_BLOCK / vox_lanes(A.C))), block(NFA_VOX_BLOCK);
    dispatch_vox(A, [&](auto lanes, auto cf, auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL((voxgrid_fwd_kernel<lanes(), cf(), E>), grid, block, 0, as_stream(stream), x, params, A.n_points, V,
                           static_cast<E *>(y));
    });
    NFA_CHECK_LAUNCH("voxgrid_fwd");
    return NFA_OK;
}

static int voxgrid_bwd(const VoxArgs &A, const float *x, const float *params, const void *grad_y, float *grad_params, float *grad_x,
                       nfa_stream_t stream)
{
    if (A.n_points == 0) return NFA_OK;
    VoxDesc V;
    const int rc = vox_desc("voxgrid_bwd", A, V);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(x && params && grad_y && (grad_params || grad_x), "voxgrid_bwd: null pointer");
    const dim3 grid(grid_1d(A.n_points, NFA_VOX_BLOCK / vox_lanes(A.C))), block(NFA_VOX_BLOCK);
    dispatch_vox(A, [&](auto lanes, auto cf, auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL((voxgrid_bwd_kernel<lanes(), cf(), E>), grid, block, 0, as_stream(stream), x, params,
                           static_cast<const E *>(grad_y), A.n_points, V, grad_params, grad_x);
    });
    NFA_CHECK_LAUNCH("voxgrid_bwd");
    return NFA_OK;
}

static int voxgrid_resample(const float *src, const int32_t *src_res, float *dst, const int32_t *dst_res, int32_t C, nfa_stream_t stream)
{
    const char *name = "voxgrid_resample";
    int rc = vox_check_c(name, C);
    if (rc != NFA_OK) return rc;
    VoxResample R;
    int64_t n_src, n_dst;
    if ((rc = vox_check_res(name, "source ", C, src_res, R.src_res, n_src)) != NFA_OK) return rc;
    if ((rc = vox_check_res(name, "destination ", C, dst_res, R.dst_res, n_dst)) != NFA_OK) return rc;
    NFA_REQUIRE(src && dst, "%s: null pointer", name);
    for (int d = 0; d < 3; ++d) R.scale[d] = (float)(R.src_res[d] - 1) / (float)(R.dst_res[d] - 1);
    R.C = (uint32_t)C;
    const int lanes = vox_lanes(C);
    const int64_t n_rows = (int64_t)R.dst_res[1] * R.dst_res[2];   // (< 2^31: the size check above)
    // pieces along x, then as many workgroups over the rows as keep the launch at the usual grid-stride cap
    const unsigned pieces = grid_1d(R.dst_res[0], 256 / lanes, 64);
    const dim3 grid((unsigned)std::min<int64_t>(n_rows, std::max(1u, 256 * 16 / pieces)), pieces);
    dispatch_value<1, 4, 8, 16, 32>(lanes, [&](auto w) {
        hipLaunchKernelGGL(voxgrid_resample_kernel<w()>, grid, dim3(256), 0, as_stream(stream), src, R, dst);
    });
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int nfa_voxgrid_fwd(int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_features, const int32_t *res_host,
                    int32_t n_strides, const int32_t *strides_host, void *y, nfa_stream_t stream)
{
    return voxgrid_fwd(VoxArgs{elem, n_points, n_features, res_host, n_strides, strides_host}, x, params, y, stream);
}

int nfa_voxgrid_bwd(int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points, int32_t n_features,
                    const int32_t *res_host, int32_t n_strides, const int32_t *strides_host, float *grad_params, float *grad_x,
                    nfa_stream_t stream)
{
    return voxgrid_bwd(VoxArgs{elem, n_points, n_features, res_host, n_strides, strides_host}, x, params, grad_y, grad_params, grad_x,
                       stream);
}

int nfa_voxgrid_resample(const float *src_params, const int32_t *src_res_host, float *dst_params, const int32_t *dst_res_host,
                         int32_t n_features, nfa_stream_t stream)
{
    return voxgrid_resample(src_params, src_res_host, dst_params, dst_res_host, n_features, stream);
}

// vmgrid.hip -- the vector-matrix (VM) decomposition of TensoRF (Chen et al. 2022, "TensoRF: Tensorial Radiance Fields"),
// `TensorVMSplit`: three modes, each a feature plane times a feature line, for x [N, 3] in [0, 1]^3 (TensoRF's u in
// [-1, 1] is x = (u + 1) / 2), and the resampling of its tables (`up_sampling_VM`).
//
// Modes m = 0, 1, 2: plane axes (a, b) = (0,1) (0,2) (1,2) (matMode), line axis c = 2, 1, 0 (vecMode).  The resolution
// (R_0, R_1, R_2), every one >= 2, is shared by the modes, and so is the component count C, a multiple of 4 in 4..96.
// Parameters: one flat float32 table without gaps of fewer than 2^31 floats; for m in order the plane, a row-major
// [R_b, R_a, C] block, then the line, a [R_c, C] block: a node's C values are contiguous.
//
// All arithmetic is float32, every operation rounded on its own (the library builds with -ffp-contract=off).  Per axis
// the locate step is axis.h's (border clamp, NaN -> node 0, the `in` flag, i <= R - 2, f in [0, 1]).  Per mode and
// component j, with P the mode's plane and Ln its line:
//   w_k = (k_a ? f_a : 1 - f_a) * (k_b ? f_b : 1 - f_b),  corners k = k_a + 2 k_b in the order 0..3
//   pv[j] = sum_k w_k * P[((i_b + k_b) R_a + i_a + k_a) C + j], summed from 0 in corner order  (axis.h's plane_value)
//   lv[j] = (0 + (1 - f_c) * Ln[i_c C + j]) + f_c * Ln[(i_c + 1) C + j]
//   t_m[j] = pv[j] * lv[j]
// which is F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True) of the [1, C, R_b, R_a] plane and of
// the [1, C, R_c, 1] line, multiplied.
//   NFA_VM_CONCAT: y[n, m C + j] = t_m[j], [N, 3 C]                              (compute_appfeature before basis_mat)
//   NFA_VM_SUM:    y[n, 0] = sum_m sum_j t_m[j], [N, 1]                                      (compute_densityfeature)
// The order of that sum: with L the lane-group width (below), lane l < L starts at 0 and adds t_m[l + r L] with m the outer
// loop (ascending) and r = 0 .. C / L - 1 the inner one (ascending); the L lane sums are then combined by an xor butterfly at
// the distances L / 2, L / 4, .. 1 (a + b is commutative, so every lane ends with the same bits).
// nerfacc_amd/encodings.py (_vmgrid_torch) restates the forward in torch, bit for bit.
//
// Backward, per point; pv and lv are recomputed (nothing but x is kept from the forward).  g[j] is dL/dy of column m C + j
// (concat) or of the point's one column (sum); T_k the plane's corner values, L_0 / L_1 the line's two nodes:
//   gk = g[j] * lv[j],  gl = g[j] * pv[j]
//   plane gradient:  G[corner k][j] += w_k * gk        (no-return global_atomic_add_f32 into a zeroed float32 gradient)
//   line gradient:   G[i_c][j] += (1 - f_c) * gl,  G[i_c + 1][j] += f_c * gl                              (see below)
//   dv_a, dv_b = axis.h's plane_slopes (d pv / d f_a, d pv / d f_b, corner order);  dl = L_1 - L_0
//   t_a += gk * dv_a,  t_b += gk * dv_b,  t_c += gl * dl, over the lane's components in ascending order, from 0
//   share_d = in_d ? t_d * (float)(R_d - 1) : 0, summed over the L lanes by the xor butterfly
//   dL/dx[n, d] = ((share_d of mode 0) + share_d of mode 1) + share_d of mode 2
// The kernel runs the modes one after the other (the line gradient's reason), so the lane that owns dL/dx[n, d] stores
// mode 0's share and adds the other two to its own earlier store with a plain load and store: no atomics, the same bits on
// every run.  An axis whose coordinate is outside [0, 1] or not finite gets 0.  No second order.
//
// The line gradient.  All N points add into 3 R_c rows of 4 C bytes: a few KB that every workgroup of the launch would hit
// with two global atomics per point and mode (same-row contention costs an order of magnitude of the atomic rate).  So a
// workgroup keeps a private copy of ONE mode's line gradient in LDS (R_c C floats, zeroed), its points add into it with
// ds_add_f32, and after the workgroup's points it adds the copy's non-zero values to the global gradient, one global
// atomic per value and workgroup.  That is why the modes are the outer loop.  LDS budget: NFA_VM_LDS_BYTES = 64 KiB per
// workgroup (the size a launch may ask for without raising the kernel's limit; 300 nodes x 48 components is 57,600 bytes).
// A resolution whose longest line does not fit (4 max(R) C > 65,536) takes the same kernel with the line adds as direct
// global atomics.
//
// Layout: lanes run over COMPONENTS.  L = the largest power of two <= 32 that divides C (4 -> 4, 16 -> 16, 24 -> 8, 48 -> 16,
// 96 -> 32).  A point is L consecutive lanes; lane l owns the components l, l + L, ...  A gather or an atomic
// wave-instruction is 64 / L row segments of 4 L contiguous bytes, the concat output piece of a (point, mode, r) one
// contiguous 4 L-byte store; with "sum" lane 0 of the group stores the point's value.  Every lane of a wave runs every
// iteration (the lanes past the last point recompute it and write nothing), so a butterfly is always among live lanes.
// Element types: y / dL/dy are float, fp16 or bf16 (NFA_ELEM_*): float32 arithmetic, one rounding as the value is stored.
//
// Resampling (nfa_vmgrid_resample): every destination node of every plane and line is the bilinear / linear sample of the
// source block at, per axis, p = (float)i' * ((float)(R - 1) / (float)(R' - 1)) (the quotient formed once on the host),
// located by axis.h's locate_pos and combined with the forward's tap arithmetic: F.interpolate(mode="bilinear",
// align_corners=True).  One lane per destination float in table order, so lanes run over components and the stores are
// contiguous.  Each axis has its own R and R': up, down or unchanged.  At R' = R, p = i' exactly and a node copies its
// source (finite values; the sum from 0 turns a -0 into +0).
#include "common.hip.h"
#include "axis.h"        // Axis, locate_axis / locate_pos, the taps, store_elem / load_elem (shared with planes.hip)
#include "vm_layout.h"   // vm_a / vm_b / vm_c, VMDesc, vm_check_c, vm_layout (shared with vmreg.hip)

namespace nfa {

#define NFA_VM_LDS_BYTES 65536   // the line copy a workgroup of the backward may keep in LDS
#define NFA_VM_BWD_BLOCK 512

// Forward: L lanes per point, the modes and the lane's components in loops.
template <int L, int RED, class E>
__global__ __launch_bounds__(256) void vmgrid_fwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                         int64_t n_points, const VMDesc V, E *__restrict__ y)
{
    constexpr int PPB = 256 / L;
    const int l = (int)threadIdx.x % L, lp = (int)threadIdx.x / L;
    const int C = V.C;
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < n_points; base += (int64_t)gridDim.x * PPB) {
        const bool valid = base + lp < n_points;
        const int64_t n = valid ? base + lp : n_points - 1;
        Axis ax[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) ax[d] = locate_axis(x[n * 3 + d], V.res[d]);
        float acc = 0.0f;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const Axis &c = ax[vm_c(m)];
            const Taps t = plane_taps(V.plane[m], ax[vm_a(m)], ax[vm_b(m)], (uint32_t)V.res[vm_a(m)], (uint32_t)C);
            const uint32_t el = V.line[m] + c.i * (uint32_t)C;   // the lower line node, component 0
            for (int j = l; j < C; j += L) {
                float T[4];
                load_taps(params, t, (uint32_t)j, T);
                const float l0 = params[el + (uint32_t)j], l1 = params[el + (uint32_t)(C + j)];
                const float term = plane_value(t.w, T) * line_value(c.f, l0, l1);
                if constexpr (RED == NFA_VM_CONCAT) {
                    if (valid) store_elem(y + n * (3 * C) + (m * C + j), term);
                } else {
                    acc = acc + term;
                }
            }
        }
        if constexpr (RED == NFA_VM_SUM) {
#pragma unroll
            for (int off = L / 2; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, NFA_WAVE);
            if (valid && l == 0) store_elem(y + n, acc);
        }
    }
}

// Backward: L lanes per point, the modes as the outer loop (one line copy in LDS at a time); either output may be NULL.
// LDS: the line gradient goes through the workgroup's copy (needs g_params); otherwise straight to global memory.
template <int L, int RED, class E, bool LDS>
__global__ __launch_bounds__(NFA_VM_BWD_BLOCK) void vmgrid_bwd_kernel(const float *__restrict__ x, const float *__restrict__ params,
                                                                      const E *__restrict__ g_y, int64_t n_points, const VMDesc V,
                                                                      float *__restrict__ g_params, float *g_x)
{
    extern __shared__ float line_acc[];   // [R_c, C] of the current mode (LDS only)
    constexpr int PPB = NFA_VM_BWD_BLOCK / L;
    const int l = (int)threadIdx.x % L, lp = (int)threadIdx.x / L;
    const int C = V.C;
#pragma nounroll
    for (int m = 0; m < 3; ++m) {
        const int da = vm_a(m), db = vm_b(m), dc = vm_c(m);
        const int n_line = V.res[dc] * C;
        if constexpr (LDS) {
            for (int i = (int)threadIdx.x; i < n_line; i += NFA_VM_BWD_BLOCK) line_acc[i] = 0.0f;
            __syncthreads();
        }
        for (int64_t base = (int64_t)blockIdx.x * PPB; base < n_points; base += (int64_t)gridDim.x * PPB) {
            const bool valid = base + lp < n_points;
            const int64_t n = valid ? base + lp : n_points - 1;
            const Axis a = locate_axis(x[n * 3 + da], V.res[da]), b = locate_axis(x[n * 3 + db], V.res[db]),
                       c = locate_axis(x[n * 3 + dc], V.res[dc]);
            const Taps t = plane_taps(V.plane[m], a, b, (uint32_t)V.res[da], (uint32_t)C);
            const uint32_t el = V.line[m] + c.i * (uint32_t)C;   // the lower line node, component 0
            const float wc0 = 1.0f - c.f;
            const E *g_row = RED == NFA_VM_CONCAT ? g_y + n * (3 * C) + m * C : g_y + n;
            float ta = 0.0f, tb = 0.0f, tc = 0.0f;
            for (int j = l; j < C; j += L) {
                const float g = load_elem(RED == NFA_VM_CONCAT ? g_row + j : g_row);
                float T[4];
                load_taps(params, t, (uint32_t)j, T);
                const float l0 = params[el + (uint32_t)j], l1 = params[el + (uint32_t)(C + j)];
                const float pv = plane_value(t.w, T), lv = line_value(c.f, l0, l1);
                const float gk = g * lv, gl = g * pv;
                if (g_params != nullptr && valid) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) unsafeAtomicAdd(g_params + (t.e[k] + (uint32_t)j), t.w[k] * gk);
                    if constexpr (LDS) {
                        float *acc = line_acc + ((int)c.i * C + j);
                        __hip_atomic_fetch_add(acc, wc0 * gl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(acc + C, c.f * gl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        unsafeAtomicAdd(g_params + (el + (uint32_t)j), wc0 * gl);
                        unsafeAtomicAdd(g_params + (el + (uint32_t)(C + j)), c.f * gl);
                    }
                }
                if (g_x != nullptr) {
                    float dva, dvb;
                    plane_slopes(a.f, b.f, T, dva, dvb);
                    ta = ta + gk * dva;
                    tb = tb + gk * dvb;
                    tc = tc + gl * (l1 - l0);
                }
            }
            if (g_x != nullptr) {
                float sa = a.in ? ta * a.rm1 : 0.0f, sb = b.in ? tb * b.rm1 : 0.0f, sc = c.in ? tc * c.rm1 : 0.0f;
#pragma unroll
                for (int off = L / 2; off > 0; off >>= 1) {
                    sa = sa + __shfl_xor(sa, off, NFA_WAVE);
                    sb = sb + __shfl_xor(sb, off, NFA_WAVE);
                    sc = sc + __shfl_xor(sc, off, NFA_WAVE);
                }
                if (valid && l < 3) {   // lane d of the group owns dL/dx[n, d], in every mode
                    const float share = l == da ? sa : l == db ? sb : sc;
                    float *out = g_x + n * 3 + l;
                    *out = m == 0 ? share : *out + share;
                }
            }
        }
        if constexpr (LDS) {
            __syncthreads();
            for (int i = (int)threadIdx.x; i < n_line; i += NFA_VM_BWD_BLOCK) {
                const float v = line_acc[i];
                if (v != 0.0f) unsafeAtomicAdd(g_params + (V.line[m] + (uint32_t)i), v);
            }
            __syncthreads();   // (the next mode zeroes the copy)
        }
    }
}

// Resample: one lane per destination float, in table order.
struct VMResample {
    VMDesc src, dst;
    float scale[3];     // (float)(R_d - 1) / (float)(R'_d - 1)
    uint32_t n_dst;     // floats of the destination table
};
__global__ __launch_bounds__(256) void vmgrid_resample_kernel(const float *__restrict__ src, const VMResample R, float *__restrict__ dst)
{
    const uint32_t C = (uint32_t)R.dst.C;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < R.n_dst; e += gridDim.x * 256u) {
        int m = e >= R.dst.plane[2] ? 2 : e >= R.dst.plane[1] ? 1 : 0;
        const int da = vm_a(m), db = vm_b(m), dc = vm_c(m);
        float v;
        if (e >= R.dst.line[m]) {
            const uint32_t rel = e - R.dst.line[m], node = rel / C, j = rel % C;
            const Axis c = locate_pos((float)node * R.scale[dc], R.src.res[dc]);
            const uint32_t el = R.src.line[m] + c.i * C + j;
            v = line_value(c.f, src[el], src[el + C]);
        } else {
            const uint32_t rel = e - R.dst.plane[m], node = rel / C, j = rel % C, Wd = (uint32_t)R.dst.res[da];
            const Axis a = locate_pos((float)(node % Wd) * R.scale[da], R.src.res[da]);
            const Axis b = locate_pos((float)(node / Wd) * R.scale[db], R.src.res[db]);
            const Taps t = plane_taps(R.src.plane[m], a, b, (uint32_t)R.src.res[da], C);
            float T[4];
            load_taps(src, t, j, T);
            v = plane_value(t.w, T);
        }
        dst[e] = v;
    }
}

// ---------------------------------------------------------------- host side
struct VMArgs {
    int32_t reduce, elem;
    int64_t n_points;
    int32_t C;
    const int32_t *res_host;
};
static int vm_desc(const char *name, const VMArgs &A, VMDesc &V)
{
    NFA_REQUIRE(A.n_points >= 0, "%s: negative n_points", name);
    NFA_REQUIRE(A.reduce == NFA_VM_CONCAT || A.reduce == NFA_VM_SUM, "%s: reduce must be NFA_VM_CONCAT (0) or NFA_VM_SUM (1) (got %d)",
                name, A.reduce);
    NFA_REQUIRE(A.elem == NFA_ELEM_F32 || A.elem == NFA_ELEM_F16 || A.elem == NFA_ELEM_BF16,
                "%s: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got %d)", name, A.elem);
    const int rc = vm_check_c(name, A.C);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(A.res_host != nullptr, "%s: null resolution table", name);
    int64_t total;
    return vm_layout(name, "", A.C, A.res_host, V, total);
}

// the lane-group width: the largest power of two <= 32 that divides C
static int vm_lanes(int32_t C) { return C % 32 == 0 ? 32 : C % 16 == 0 ? 16 : C % 8 == 0 ? 8 : 4; }

template <class Fn>
static void dispatch_vm(const VMArgs &A, Fn &&f)
{
    dispatch_value<4, 8, 16, 32>(vm_lanes(A.C), [&](auto lanes) {
        dispatch_value<NFA_VM_CONCAT, NFA_VM_SUM>(A.reduce, [&](auto r) {
            dispatch_elem(A.elem, [&](auto tag) { f(lanes, r, tag); });
        });
    });
}

static int vmgrid_fwd(const VMArgs &A, const float *x, const float *params, void *y, nfa_stream_t stream)
{
    if (A.n_points == 0) return NFA_OK;
    VMDesc V;
    const int rc = vm_desc("vmgrid_fwd", A, V);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(x && params && y, "vmgrid_fwd: null pointer");
    const dim3 grid(grid_1d(A.n_points, 256 / vm_lanes(A.C))), block(256);
    dispatch_vm(A, [&](auto lanes, auto r, auto tag) {
        using E = typename decltype(tag)::type;
        hipLaunchKernelGGL((vmgrid_fwd_kernel<lanes(), r(), E>), grid, block, 0, as_stream(stream), x, params, A.n_points, V,
                           static_cast<E *>(y));
    });
    NFA_CHECK_LAUNCH("vmgrid_fwd");
    return NFA_OK;
}

static int vmgrid_bwd(const VMArgs &A, const float *x, const float *params, const void *grad_y, float *grad_params, float *grad_x,
                      nfa_stream_t stream)
{
    if (A.n_points == 0) return NFA_OK;
    VMDesc V;
    const int rc = vm_desc("vmgrid_bwd", A, V);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(x && params && grad_y && (grad_params || grad_x), "vmgrid_bwd: null pointer");
    const int64_t line_bytes = (int64_t)std::max(V.res[0], std::max(V.res[1], V.res[2])) * A.C * 4;
    const bool lds = grad_params != nullptr && line_bytes <= NFA_VM_LDS_BYTES;
    // With a line copy: as many workgroups as the LDS of 256 CUs holds at once (at most 4 each), so that a copy collects
    // many points before it is flushed; without: the usual grid-stride cap.
    const int64_t cap = lds ? 256 * std::min<int64_t>(4, 160 * 1024 / line_bytes) : 256 * 8;
    const dim3 grid(grid_1d(A.n_points, NFA_VM_BWD_BLOCK / vm_lanes(A.C), cap)), block(NFA_VM_BWD_BLOCK);
    dispatch_vm(A, [&](auto lanes, auto r, auto tag) {
        using E = typename decltype(tag)::type;
        dispatch_bool(lds, [&](auto use_lds) {
            hipLaunchKernelGGL((vmgrid_bwd_kernel<lanes(), r(), E, use_lds()>), grid, block, lds ? (size_t)line_bytes : 0,
                               as_stream(stream), x, params, static_cast<const E *>(grad_y), A.n_points, V, grad_params, grad_x);
        });
    });
    NFA_CHECK_LAUNCH("vmgrid_bwd");
    return NFA_OK;
}

static int vmgrid_resample(const float *src, const int32_t *src_res, float *dst, const int32_t *dst_res, int32_t C, nfa_stream_t stream)
{
    const char *name = "vmgrid_resample";
    int rc = vm_check_c(name, C);
    if (rc != NFA_OK) return rc;
    NFA_REQUIRE(src_res != nullptr && dst_res != nullptr, "%s: null resolution table", name);
    VMResample R;
    int64_t n_src, n_dst;
    if ((rc = vm_layout(name, "source ", C, src_res, R.src, n_src)) != NFA_OK) return rc;
    if ((rc = vm_layout(name, "destination ", C, dst_res, R.dst, n_dst)) != NFA_OK) return rc;
    NFA_REQUIRE(src && dst, "%s: null pointer", name);
    for (int d = 0; d < 3; ++d) R.scale[d] = (float)(R.src.res[d] - 1) / (float)(R.dst.res[d] - 1);
    R.n_dst = (uint32_t)n_dst;
    hipLaunchKernelGGL(vmgrid_resample_kernel, dim3(grid_1d(n_dst, 256)), dim3(256), 0, as_stream(stream), src, R, dst);
    NFA_CHECK_LAUNCH(name);
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

int nfa_vmgrid_fwd(int32_t reduce, int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_components,
                   const int32_t *res_host, void *y, nfa_stream_t stream)
{
    return vmgrid_fwd(VMArgs{reduce, elem, n_points, n_components, res_host}, x, params, y, stream);
}

int nfa_vmgrid_bwd(int32_t reduce, int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                   int32_t n_components, const int32_t *res_host, float *grad_params, float *grad_x, nfa_stream_t stream)
{
    return vmgrid_bwd(VMArgs{reduce, elem, n_points, n_components, res_host}, x, params, grad_y, grad_params, grad_x, stream);
}

int nfa_vmgrid_resample(const float *src_params, const int32_t *src_res_host, float *dst_params, const int32_t *dst_res_host,
                        int32_t n_components, nfa_stream_t stream)
{
    return vmgrid_resample(src_params, src_res_host, dst_params, dst_res_host, n_components, stream);
}

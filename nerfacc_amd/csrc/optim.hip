// optim.hip -- the fused multi-tensor Adam / AdamW step with on-device loss scaling and LR schedule (include/nerfacc_hip.h,
// "fused optimiser").  Three kernels, one launch each, cut where every element needs what every other element decided:
//   optim_scan_kernel     any non-finite gradient in the list -> scaler->found            (only with a scaler)
//   optim_decide_kernel   one wave: the flag, the counters and the host's settings -> this step's scalars; advances the state
//   optim_update_kernel   the update proper, streaming p, grad, m, v once
// The list is a device table of tensors plus a work list of (tensor, chunk) pairs; a workgroup strides over the work list.
#include "common.hip.h"

namespace nfa {

constexpr int OPTIM_BLOCK = 256;
static_assert(NFA_OPTIM_CHUNK % (4 * OPTIM_BLOCK) == 0, "a chunk is a whole number of 16-byte passes of a workgroup");
static_assert(NFA_OPTIM_MAX_GROUPS <= NFA_WAVE, "the decide launch gives each group a lane of one wave");
static_assert(sizeof(nfa_optim_tensor) == 48 && sizeof(nfa_optim_group) == 48 && sizeof(nfa_optim_group_scalars) == 48 &&
              sizeof(nfa_optim_scaler) == 32, "the Python layer mirrors these layouts");

// One entry of the work list: the tensor's row and the element range, or cnt = 0 for an entry that names no tensor.
struct OptimPiece {
    nfa_optim_tensor t;
    int64_t start;
    int32_t cnt;
    bool vec;   // 16-byte pieces: all four pointers aligned (the start of a chunk is a multiple of 4 elements)
};
__device__ __forceinline__ OptimPiece optim_piece(const nfa_optim_tensor *table, int32_t n_tensors, const nfa_optim_chunk *work, int64_t c,
                                                  bool grad_only)
{
    OptimPiece o = {};
    const nfa_optim_chunk w = work[c];
    if ((uint32_t)w.tensor >= (uint32_t)n_tensors || w.chunk < 0) return o;
    o.t = table[w.tensor];
    o.start = (int64_t)w.chunk * NFA_OPTIM_CHUNK;
    const int64_t left = o.t.n - o.start;
    if (left <= 0) return o;
    o.cnt = left < NFA_OPTIM_CHUNK ? (int32_t)left : NFA_OPTIM_CHUNK;
    uintptr_t bits = reinterpret_cast<uintptr_t>(o.t.grad);
    if (!grad_only) bits |= reinterpret_cast<uintptr_t>(o.t.p) | reinterpret_cast<uintptr_t>(o.t.exp_avg) | reinterpret_cast<uintptr_t>(o.t.exp_avg_sq);
    o.vec = (bits & 15) == 0;
    return o;
}

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(OPTIM_BLOCK) void optim_scan_kernel(const nfa_optim_tensor *__restrict__ table, int32_t n_tensors,
                                                                 const nfa_optim_chunk *__restrict__ work, int64_t n_chunks,
                                                                 nfa_optim_scaler *scaler)
{
    bool bad = false;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptimPiece o = optim_piece(table, n_tensors, work, c, true);
        const float *g = o.t.grad + o.start;
        const int32_t n_vec = o.vec ? o.cnt >> 2 : 0;
        for (int32_t i = threadIdx.x; i < n_vec; i += OPTIM_BLOCK) {
            const nfa_v4f x = reinterpret_cast<const nfa_v4f *>(g)[i];
            bad |= !(finite_bits(x.x) && finite_bits(x.y) && finite_bits(x.z) && finite_bits(x.w));
        }
        for (int32_t i = 4 * n_vec + threadIdx.x; i < o.cnt; i += OPTIM_BLOCK) bad |= !finite_bits(g[i]);
    }
    // every writer stores the same value: no atomic, no order
    if (bad) scaler->found = 1;
}

__global__ __launch_bounds__(NFA_WAVE) void optim_decide_kernel(const nfa_optim_args a, nfa_optim_state *state, nfa_optim_scaler *scaler)
{
    const int lane = threadIdx.x;
    const bool is_group = lane < a.n_groups;
    // ---- everything that is read, before anything is written
    const int64_t calls = state->calls, step = state->step;
    const bool found = scaler && scaler->found != 0;
    const float scale = scaler ? scaler->scale : 1.0f;
    const int32_t tracker = scaler ? scaler->tracker : 0;
    const int64_t skipped = scaler ? scaler->skipped : 0;
    double b1p = is_group ? state->beta1_pow[lane] : 1.0, b2p = is_group ? state->beta2_pow[lane] : 1.0;
    __syncthreads();

    double factor = 1.0;
    if (a.warmup_iters > 0) {
        const int64_t t = calls < a.warmup_iters ? calls : a.warmup_iters;
        factor = a.start_factor + (1.0 - a.start_factor) * (double)t / (double)a.warmup_iters;
    }
    for (int32_t k = 0; k < a.n_milestones; ++k)
        if (a.milestones[k] <= calls) factor = factor * a.gamma;

    if (is_group && !found) {
        const nfa_optim_group g = a.groups[lane];
        b1p = b1p * g.beta1;
        b2p = b2p * g.beta2;
        const double lr = g.lr * factor;
        nfa_optim_group_scalars s;
        s.step_size = (float)(lr / (1.0 - b1p));
        s.bc2_sqrt = (float)sqrt(1.0 - b2p);
        s.decay = (float)(1.0 - lr * g.weight_decay);
        s.one_minus_beta1 = (float)(1.0 - g.beta1);
        s.beta2 = (float)g.beta2;
        s.one_minus_beta2 = (float)(1.0 - g.beta2);
        s.eps = (float)g.eps;
        s.weight_decay = (float)g.weight_decay;
        s.flags = g.flags;
        s.reserved[0] = s.reserved[1] = s.reserved[2] = 0;
        state->group[lane] = s;
        state->beta1_pow[lane] = b1p;
        state->beta2_pow[lane] = b2p;
    }
    if (lane == 0) {
        state->calls = calls + 1;
        state->step = found ? step : step + 1;
        state->inv_scale = (float)(1.0 / (double)scale);
        state->skip = found ? 1 : 0;
        state->factor = (float)factor;
        if (scaler) {
            float new_scale = scale;
            int32_t new_tracker = tracker;
            if (found) {
                new_scale = scale * a.backoff_factor;
                new_tracker = 0;
            } else if (a.growth_interval > 0) {
                new_tracker = tracker + 1;
                if (new_tracker == a.growth_interval) {
                    const float grown = scale * a.growth_factor;
                    if (finite_bits(grown)) new_scale = grown;
                    new_tracker = 0;
                }
            }
            scaler->scale = new_scale;
            scaler->tracker = new_tracker;
            scaler->found = 0;
            scaler->skipped = found ? skipped + 1 : skipped;
        }
    }
}

// The per-element step (nerfacc_hip.h lists it; tests/optim_reference.py restates it).  false: p, m, v are not to be written.
__device__ __forceinline__ bool adam_element(const nfa_optim_group_scalars &G, float inv_scale, float grad, float &p, float &m, float &v)
{
    float g = grad * inv_scale;
    if ((G.flags & NFA_OPTIM_SKIP_ZERO_GRAD) && g == 0.0f) return false;
    if (G.flags & NFA_OPTIM_DECOUPLED) p = p * G.decay;
    else if (G.weight_decay != 0.0f) g = g + G.weight_decay * p;
    m = m + G.one_minus_beta1 * (g - m);
    v = G.beta2 * v + G.one_minus_beta2 * (g * g);
    p = p - (G.step_size * m) / (sqrtf(v) / G.bc2_sqrt + G.eps);
    return true;
}

template <bool ZERO_GRAD>
__global__ __launch_bounds__(OPTIM_BLOCK) void optim_update_kernel(const nfa_optim_tensor *__restrict__ table, int32_t n_tensors,
                                                                   const nfa_optim_chunk *__restrict__ work, int64_t n_chunks,
                                                                   const nfa_optim_state *__restrict__ state)
{
    const bool skip = state->skip != 0;
    if (skip && !ZERO_GRAD) return;
    const float inv_scale = state->inv_scale;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptimPiece o = optim_piece(table, n_tensors, work, c, skip);
        if (o.cnt == 0) continue;
        float *__restrict__ gp = o.t.grad + o.start;
        const int32_t n_vec = o.vec ? o.cnt >> 2 : 0;
        if (skip) {   // (ZERO_GRAD) a skipped step still leaves the gradients zero
            for (int32_t i = threadIdx.x; i < n_vec; i += OPTIM_BLOCK) store_f4(gp + 4 * i, 0.f, 0.f, 0.f, 0.f);
            for (int32_t i = 4 * n_vec + threadIdx.x; i < o.cnt; i += OPTIM_BLOCK) gp[i] = 0.f;
            continue;
        }
        const nfa_optim_group_scalars G = state->group[o.t.group & (NFA_OPTIM_MAX_GROUPS - 1)];
        const bool skip_zero = (G.flags & NFA_OPTIM_SKIP_ZERO_GRAD) != 0;
        float *__restrict__ pp = o.t.p + o.start, *__restrict__ mp = o.t.exp_avg + o.start, *__restrict__ vp = o.t.exp_avg_sq + o.start;
#pragma unroll 2
        for (int32_t i = threadIdx.x; i < n_vec; i += OPTIM_BLOCK) {
            const nfa_v4f g4 = reinterpret_cast<const nfa_v4f *>(gp)[i];
            // a piece of zeros under skip_zero_grad costs its 16 bytes of gradient only
            if (skip_zero && g4.x == 0.f && g4.y == 0.f && g4.z == 0.f && g4.w == 0.f) continue;
            const nfa_v4f p4 = reinterpret_cast<const nfa_v4f *>(pp)[i], m4 = reinterpret_cast<const nfa_v4f *>(mp)[i],
                          v4 = reinterpret_cast<const nfa_v4f *>(vp)[i];
            float g[4] = {g4.x, g4.y, g4.z, g4.w}, p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w},
                  v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pn = p[k], mn = m[k], vn = v[k];
                if (adam_element(G, inv_scale, g[k], pn, mn, vn)) { p[k] = pn; m[k] = mn; v[k] = vn; }
            }
            store_f4(pp + 4 * i, p[0], p[1], p[2], p[3]);
            store_f4(mp + 4 * i, m[0], m[1], m[2], m[3]);
            store_f4(vp + 4 * i, v[0], v[1], v[2], v[3]);
            if (ZERO_GRAD) store_f4(gp + 4 * i, 0.f, 0.f, 0.f, 0.f);
        }
        for (int32_t i = 4 * n_vec + threadIdx.x; i < o.cnt; i += OPTIM_BLOCK) {
            float pn = pp[i], mn = mp[i], vn = vp[i];
            if (adam_element(G, inv_scale, gp[i], pn, mn, vn)) { pp[i] = pn; mp[i] = mn; vp[i] = vn; }
            if (ZERO_GRAD) gp[i] = 0.f;
        }
    }
}

static inline unsigned optim_grid(int64_t n_chunks) { return grid_1d(n_chunks, 1, 256 * 8); }

}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_optim_chunk_elems(void) { return NFA_OPTIM_CHUNK; }

int nfa_optim_scan(int32_t dtype, const nfa_optim_tensor *table, int32_t n_tensors, const nfa_optim_chunk *work, int64_t n_chunks,
                   nfa_optim_scaler *scaler, nfa_stream_t stream)
{
    NFA_REQUIRE(dtype == NFA_ELEM_F32, "optim_scan: float32 tensors only (dtype code %d)", dtype);
    NFA_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "optim_scan: negative count");
    NFA_REQUIRE(scaler, "optim_scan: null scaler");
    if (n_tensors == 0 || n_chunks == 0) return NFA_OK;
    NFA_REQUIRE(table && work, "optim_scan: null pointer");
    hipLaunchKernelGGL(optim_scan_kernel, dim3(optim_grid(n_chunks)), dim3(OPTIM_BLOCK), 0, as_stream(stream), table, n_tensors, work,
                       n_chunks, scaler);
    NFA_CHECK_LAUNCH("optim_scan");
    return NFA_OK;
}

int nfa_optim_decide(const nfa_optim_args *args_host, nfa_optim_state *state, nfa_optim_scaler *scaler, nfa_stream_t stream)
{
    NFA_REQUIRE(args_host && state, "optim_decide: null pointer");
    NFA_REQUIRE(args_host->n_groups >= 0 && args_host->n_milestones >= 0 && args_host->warmup_iters >= 0, "optim_decide: negative count");
    NFA_REQUIRE(args_host->n_groups <= NFA_OPTIM_MAX_GROUPS, "optim_decide: at most %d param groups", NFA_OPTIM_MAX_GROUPS);
    NFA_REQUIRE(args_host->n_milestones <= NFA_OPTIM_MAX_MILESTONES, "optim_decide: at most %d milestones", NFA_OPTIM_MAX_MILESTONES);
    hipLaunchKernelGGL(optim_decide_kernel, dim3(1), dim3(NFA_WAVE), 0, as_stream(stream), *args_host, state, scaler);
    NFA_CHECK_LAUNCH("optim_decide");
    return NFA_OK;
}

int nfa_optim_update(int32_t dtype, const nfa_optim_tensor *table, int32_t n_tensors, const nfa_optim_chunk *work, int64_t n_chunks,
                     const nfa_optim_state *state, int32_t zero_grad, nfa_stream_t stream)
{
    NFA_REQUIRE(dtype == NFA_ELEM_F32, "optim_update: float32 tensors only (dtype code %d)", dtype);
    NFA_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "optim_update: negative count");
    NFA_REQUIRE(state, "optim_update: null state");
    if (n_tensors == 0 || n_chunks == 0) return NFA_OK;
    NFA_REQUIRE(table && work, "optim_update: null pointer");
    dispatch_bool(zero_grad != 0, [&](auto Z) {
        hipLaunchKernelGGL((optim_update_kernel<decltype(Z)::value>), dim3(optim_grid(n_chunks)), dim3(OPTIM_BLOCK), 0, as_stream(stream),
                           table, n_tensors, work, n_chunks, state);
    });
    NFA_CHECK_LAUNCH("optim_update");
    return NFA_OK;
}

}  // extern "C"

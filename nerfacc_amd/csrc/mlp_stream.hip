// mlp_stream.hip -- the fused MLP of mlp.hip for networks whose packed weights do not fit the LDS: 128 or 256 neurons, up to 8
// hidden layers, up to 320 inputs and 288 outputs, biases and skip connections (nfa_mlp_desc): NeRF's 63 -> 8 x 256 trunk.
//
// Image format, k orders, arithmetic and rounding points are mlp.hip's, bit for bit (mlp_tiles.h holds the shared code, the pack
// kernel included).  What differs is where the image lives: it stays in global memory (L2-resident: the trunk's is 1.1 MiB) and
// passes through the LDS in PIECES while the workgroup's points wait in registers.
//
//   piece    one row tile of one layer: 32 rows x all k-steps = kq_l KiB, contiguous in the image (16 KiB for a 256-wide
//            layer, 20 KiB for the trunk's cat layer, 4 KiB for its layer 0, at most 36 KiB).  The x rows of a cat layer's
//            backward image are pieces of their own, used when dL/dx is formed.
//   ring     ST_SLOTS = 2 slots of the largest piece.  Step i: every thread issues the global loads of piece i + 1 into
//            registers, the waves run their MFMAs on slot i & 1, the registers go to slot (i + 1) & 1, one workgroup barrier.
//            The slot written in step i was last read in step i - 1, before that step's barrier, so one barrier per piece
//            orders both hand-overs; a third slot would matter only if pieces were handed over less often than every step.
//            The order of the pieces is a table in LDS that thread 0 writes once (build_pieces), and it repeats every pass,
//            so the last piece of a pass prefetches the first piece of the next.
//   pass     ST_WAVES = 4 waves x ST_PT = 1 point tile of 32: 128 points see every piece once (NFA_MLP_STREAM_POINTS), one
//            16-byte LDS read per MFMA.  At 256 neurons a wave holds 8 accumulator tiles (128 registers) and 16 B fragments
//            (64) besides the staged piece: 373 registers, no scratch.  The two choices with 256 points per pass both spill
//            with this compiler (4 waves x 2 tiles: 380 to 428 B of scratch per lane at the 512-register limit; 8 waves x 1
//            tile: 96 to 232 B at the 256-register limit), so they are not used.  Every wave runs every step of every pass of
//            its workgroup: a wave whose tile lies beyond n_points clamps its loads and masks its stores, as in mlp.hip, and
//            reaches every barrier.
//   biases   float32, staged once per workgroup behind the piece table (at most 9.3 KiB); an accumulator starts from its rows.
//   B from memory   layer 0's x fragments, a cat layer's, and the first backward product's dL/dy fragments are loaded again for
//            every row tile (the registers hold the accumulators instead).  They are issued behind the step's fetch and global
//            loads return in order, so such a step waits for its prefetch: holding them across the row tiles is what to do next
//            (a first form of it spilled).
//
// Weight gradient: grid (slice, layer, macro tile), a macro tile = 128 x 128 of dW_l (16 MFMA tiles, four per wave); the
// workgroup stages only its 128 columns of dZ_l and its 128 columns of [H_{l-1}, x] (128 | W, so a macro tile never straddles
// the two sources).  Split-K over point slices with the ordered sum of mlp.hip; the slice count is
// clamp(ceil(n_points / 256), 1, 16), a function of n_points alone.  db_l is summed by the macro tiles of column 0.
#include "mlp_tiles.h"

namespace nfa {
namespace {

constexpr int ST_WAVES = 4;                               // waves per workgroup of the streamed fused passes
constexpr int ST_PT = 1;                                  // point tiles per wave
constexpr int ST_THREADS = ST_WAVES * NFA_WAVE;
constexpr int64_t ST_STAGE_BYTES = (int64_t)ST_WAVES * 32 * STAGE_LD * 4;
constexpr int ST_POINTS = ST_WAVES * ST_PT * 32;         // points of a workgroup per pass of the image
constexpr int ST_SLOTS = 2;
constexpr int ST_MAX_PIECES = 160;                        // forward <= 8 * 8 + 9, backward <= 8 * 8 + 10 * 8
constexpr int ST_MAX_IN = 320, ST_MAX_OUT = 288, ST_MAX_HIDDEN = 8;
static_assert(ST_POINTS == NFA_MLP_STREAM_POINTS, "include/nerfacc_hip.h states the points per pass");

struct Piece { int32_t off16, n16; };   // of the image, in 16-byte fragments

// The order in which a pass consumes the pieces; returns their number, writes them to tab (if given) and the largest to max_n16.
__host__ __device__ inline int build_pieces(const Shape &S, bool backward, bool need_dx, Piece *tab, int *max_n16)
{
    const int L = S.layers(), MT = S.W / 32;
    int n = 0, mx = 0;
    auto put = [&](int64_t off16, int n16) {
        if (tab) tab[n] = Piece{(int32_t)off16, n16};
        mx = n16 > mx ? n16 : mx;
        ++n;
    };
    if (!backward) {
        for (int l = 0; l < L; ++l)
            for (int m = 0; m < S.fwd_mt(l); ++m) put(S.fwd_off(l) / 8 + (int64_t)m * S.fwd_kq(l) * 64, S.fwd_kq(l) * 64);
    } else {
        for (int l = L - 1; l >= 1; --l)   // the chain: the H rows of every layer
            for (int m = 0; m < MT; ++m) put(S.bwd_off(l) / 8 + (int64_t)m * S.bwd_kq(l) * 64, S.bwd_kq(l) * 64);
        for (int m = 0; need_dx && m < S.bwd_mt(0); ++m) {   // dL/dx, 32 features at a time: layer 0, then the cat layers ascending
            put((int64_t)m * S.bwd_kq(0) * 64, S.bwd_kq(0) * 64);
            for (int l = 2; l < L; ++l)
                if (S.cat(l)) put(S.bwd_off(l) / 8 + (int64_t)(MT + m) * S.bwd_kq(l) * 64, S.bwd_kq(l) * 64);
        }
    }
    if (max_n16) *max_n16 = mx;
    return n;
}

// LDS of a streamed pass: the ring, the four waves' store staging tiles, the piece table, the forward's biases
__host__ __device__ inline int64_t stream_lds_bytes(int slot16, int bias_floats)
{
    return (int64_t)ST_SLOTS * slot16 * 16 + ST_STAGE_BYTES + (int64_t)ST_MAX_PIECES * sizeof(Piece) + (int64_t)bias_floats * 4;
}

template <int MAXV>
struct Ring {
    const nfa_v4u *img;
    nfa_v4u *slots;
    const Piece *tab;
    int slot16, n_pieces, next, cur;
    nfa_v4u regs[MAXV];

    // thread 0 has written the table; stages piece 0
    __device__ __forceinline__ void start()
    {
        __syncthreads();
        const Piece e = tab[0];
        for (int i = threadIdx.x; i < e.n16; i += ST_THREADS) slots[i] = img[e.off16 + i];
        __syncthreads();
        cur = 0;
        next = 1;   // every network has at least two pieces
    }
    __device__ __forceinline__ const nfa_v4u *piece() const { return slots + cur * slot16; }
    // issues the loads of the next piece; the current one is read between fetch() and hand_over()
    __device__ __forceinline__ void fetch()
    {
        const Piece e = tab[next];
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int i = threadIdx.x + v * ST_THREADS;
            if (i < e.n16) regs[v] = img[e.off16 + i];
        }
    }
    __device__ __forceinline__ void hand_over()
    {
        const Piece e = tab[next];
        nfa_v4u *d = slots + (cur ^ 1) * slot16;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int i = threadIdx.x + v * ST_THREADS;
            if (i < e.n16) d[i] = regs[v];
        }
        __syncthreads();
        cur ^= 1;
        next = next + 1 == n_pieces ? 0 : next + 1;
    }
};

__device__ __forceinline__ void zero_acc(f32x16 &a)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

// ---------------------------------------------------------------- forward

template <class E, int W>
__global__ __launch_bounds__(ST_THREADS) void mlp_stream_fwd_kernel(Shape S, const void *__restrict__ x, int x_f32, int x_vec,
                                                                   const uint16_t *__restrict__ image, int slot16, int n_pieces,
                                                                   const float *__restrict__ bias, int64_t N, void *__restrict__ y,
                                                                   int y_f32, uint16_t *__restrict__ save)
{
    constexpr int MT = W / 32, KQ = W / 16, MAXV = ((KQ + ST_MAX_IN / 16) * 64 + ST_THREADS - 1) / ST_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    float *st = reinterpret_cast<float *>(st_lds + (int64_t)ST_SLOTS * slot16 * 16) + wave * 32 * STAGE_LD;
    Piece *tab = reinterpret_cast<Piece *>(st_lds + (int64_t)ST_SLOTS * slot16 * 16 + ST_STAGE_BYTES);
    // the biases, staged once behind the table: layer l at l W, the output layer padded to whole row tiles with zeros.  (Read
    // from global memory as each accumulator starts, they would queue behind the fetch of the next piece: loads return in order.)
    float *lb = reinterpret_cast<float *>(tab + ST_MAX_PIECES);
    const bool has_bias = bias != nullptr;
    const int n_lb = has_bias ? S.stream_bias_floats() : 0;
    for (int i = threadIdx.x; i < n_lb; i += ST_THREADS) lb[i] = i - S.n_hidden * W < S.n_out ? bias[i] : 0.f;
    if (threadIdx.x == 0) build_pieces(S, false, false, tab, nullptr);
    Ring<MAXV> ring;
    ring.img = reinterpret_cast<const nfa_v4u *>(image);
    ring.slots = reinterpret_cast<nfa_v4u *>(st_lds);
    ring.tab = tab;
    ring.slot16 = slot16;
    ring.n_pieces = n_pieces;
    ring.start();
    const int kq0 = S.fwd_kq(0), mto = S.fwd_mt(S.n_hidden);
    const bool xf = x_f32 != 0, xv = x_vec != 0;
    const int64_t n_pass = ceil_div64(N, ST_POINTS);
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        int64_t p[ST_PT], pc[ST_PT];
#pragma unroll
        for (int t = 0; t < ST_PT; ++t) {
            p[t] = ((pass * ST_WAVES + wave) * ST_PT + t) * 32 + r;
            pc[t] = p[t] < N ? p[t] : N - 1;
        }
        f32x16 acc[ST_PT][MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {   // layer 0: the B fragments are rows of x
            ring.fetch();
            const nfa_v4u *A = ring.piece();
#pragma unroll
            for (int t = 0; t < ST_PT; ++t) init_acc(acc[t][m], has_bias, lb + 32 * m, h);
            for (int q = 0; q < kq0; ++q) {
                const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                for (int t = 0; t < ST_PT; ++t)
                    acc[t][m] = mfma<E>(a, load_row8<E>(x, xf, pc[t], S.n_in, 16 * q + 8 * h, xv), acc[t][m]);
            }
            ring.hand_over();
        }
        nfa_v4u hf[ST_PT][KQ];
        for (int l = 1;; ++l) {
            // H_{l-1} = relu(acc) rounded: the next product's B fragments, and what the backward reads
#pragma unroll
            for (int t = 0; t < ST_PT; ++t) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[t][m][i] = acc[t][m][i] < 0.f ? 0.f : acc[t][m][i];
                    hf[t][2 * m] = acc_frag<E>(acc[t][m], 0);
                    hf[t][2 * m + 1] = acc_frag<E>(acc[t][m], 1);
                    if (save && p[t] < N) store_tile_row<W>(save + (int64_t)(l - 1) * N * W, p[t], m, h, hf[t][2 * m], hf[t][2 * m + 1]);
                }
            }
            if (l == S.n_hidden) break;
            const bool cat = S.cat(l);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                ring.fetch();
                const nfa_v4u *A = ring.piece();
#pragma unroll
                for (int t = 0; t < ST_PT; ++t) init_acc(acc[t][m], has_bias, lb + l * W + 32 * m, h);
#pragma unroll
                for (int q = 0; q < KQ; ++q) {
                    const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                    for (int t = 0; t < ST_PT; ++t) acc[t][m] = mfma<E>(a, hf[t][q], acc[t][m]);
                }
                if (cat) {
                    for (int q = 0; q < kq0; ++q) {
                        const nfa_v4u a = A[(KQ + q) * 64 + lane];
#pragma unroll
                        for (int t = 0; t < ST_PT; ++t)
                            acc[t][m] = mfma<E>(a, load_row8<E>(x, xf, pc[t], S.n_in, 16 * q + 8 * h, xv), acc[t][m]);
                    }
                }
                ring.hand_over();
            }
        }
        const bool cat = S.cat(S.n_hidden);
        for (int m = 0; m < mto; ++m) {   // the output layer, 32 outputs at a time
            ring.fetch();
            const nfa_v4u *A = ring.piece();
            f32x16 o[ST_PT];
#pragma unroll
            for (int t = 0; t < ST_PT; ++t) init_acc(o[t], has_bias, lb + S.n_hidden * W + 32 * m, h);
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                for (int t = 0; t < ST_PT; ++t) o[t] = mfma<E>(a, hf[t][q], o[t]);
            }
            if (cat) {
                for (int q = 0; q < kq0; ++q) {
                    const nfa_v4u a = A[(KQ + q) * 64 + lane];
#pragma unroll
                    for (int t = 0; t < ST_PT; ++t) o[t] = mfma<E>(a, load_row8<E>(x, xf, pc[t], S.n_in, 16 * q + 8 * h, xv), o[t]);
                }
            }
            ring.hand_over();
            const int ncols = S.n_out - 32 * m < 32 ? S.n_out - 32 * m : 32;
#pragma unroll
            for (int t = 0; t < ST_PT; ++t) {
                const int64_t row0 = p[t] - r, left = N - row0;
                stage_store<E>(o[t], st, y, y_f32 != 0, row0, (int)(left < 0 ? 0 : (left < 32 ? left : 32)), S.n_out, 32 * m, ncols, lane);
            }
        }
    }
}

// ---------------------------------------------------------------- data gradient

template <class E, int W>
__global__ __launch_bounds__(ST_THREADS) void mlp_stream_bwd_data_kernel(Shape S, const void *__restrict__ g, int g_f32, int g_vec,
                                                                        const uint16_t *__restrict__ hidden,
                                                                        const uint16_t *__restrict__ image, int slot16, int n_pieces,
                                                                        int64_t N, uint16_t *__restrict__ dz,
                                                                        uint16_t *__restrict__ dz_out, void *__restrict__ dx, int dx_f32)
{
    constexpr int MT = W / 32, KQ = W / 16, MAXV = ((KQ + ST_MAX_IN / 16) * 64 + ST_THREADS - 1) / ST_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    float *st = reinterpret_cast<float *>(st_lds + (int64_t)ST_SLOTS * slot16 * 16) + wave * 32 * STAGE_LD;
    Piece *tab = reinterpret_cast<Piece *>(st_lds + (int64_t)ST_SLOTS * slot16 * 16 + ST_STAGE_BYTES);
    if (threadIdx.x == 0) build_pieces(S, true, dx != nullptr, tab, nullptr);
    Ring<MAXV> ring;
    ring.img = reinterpret_cast<const nfa_v4u *>(image);
    ring.slots = reinterpret_cast<nfa_v4u *>(st_lds);
    ring.tab = tab;
    ring.slot16 = slot16;
    ring.n_pieces = n_pieces;
    ring.start();
    const int L = S.layers(), kqo = S.bwd_kq(L - 1), mt0 = S.bwd_mt(0);
    const bool gf = g_f32 != 0, gv = g_vec != 0;
    const int64_t n_pass = ceil_div64(N, ST_POINTS);
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        int64_t p[ST_PT], pc[ST_PT];
#pragma unroll
        for (int t = 0; t < ST_PT; ++t) {
            p[t] = ((pass * ST_WAVES + wave) * ST_PT + t) * 32 + r;
            pc[t] = p[t] < N ? p[t] : N - 1;
        }
        f32x16 acc[ST_PT][MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {   // dH_last = W_L^T dZ_L, dZ_L = g rounded
            ring.fetch();
            const nfa_v4u *A = ring.piece();
#pragma unroll
            for (int t = 0; t < ST_PT; ++t) zero_acc(acc[t][m]);
            for (int q = 0; q < kqo; ++q) {
                const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                for (int t = 0; t < ST_PT; ++t) {
                    const nfa_v4u b = load_row8<E>(g, gf, pc[t], S.n_out, 16 * q + 8 * h, gv);
                    if (m == 0 && dz_out && p[t] < N) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int k = 16 * q + 8 * h + j;
                            if (k < S.n_out) dz_out[p[t] * S.n_out + k] = (uint16_t)(b[j >> 1] >> (16 * (j & 1)));
                        }
                    }
                    acc[t][m] = mfma<E>(a, b, acc[t][m]);
                }
            }
            ring.hand_over();
        }
        nfa_v4u df[ST_PT][KQ];
        for (int l = S.n_hidden - 1;; --l) {
            // dZ_l = dH_l * (H_l > 0), rounded
            const uint16_t *hl = hidden + (int64_t)l * N * W;
#pragma unroll
            for (int t = 0; t < ST_PT; ++t) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    mask_tile_row<E, W>(acc[t][m], hl, pc[t], m, h);
                    df[t][2 * m] = acc_frag<E>(acc[t][m], 0);
                    df[t][2 * m + 1] = acc_frag<E>(acc[t][m], 1);
                    if (p[t] < N) store_tile_row<W>(dz + (int64_t)l * N * W, p[t], m, h, df[t][2 * m], df[t][2 * m + 1]);
                }
            }
            if (l == 0) break;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                ring.fetch();
                const nfa_v4u *A = ring.piece();
#pragma unroll
                for (int t = 0; t < ST_PT; ++t) zero_acc(acc[t][m]);
#pragma unroll
                for (int q = 0; q < KQ; ++q) {
                    const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                    for (int t = 0; t < ST_PT; ++t) acc[t][m] = mfma<E>(a, df[t][q], acc[t][m]);
                }
                ring.hand_over();
            }
        }
        if (dx) {   // dx = W_0^T dZ_0 + sum over the cat layers W_l[:, W:]^T dZ_l, 32 input features at a time
            if (S.skip_mask) {
                // df[] holds dZ_0 by now, so a cat layer's dZ_l comes back from dz.  A lane with a point reads the two 8-byte pieces
                // it stored itself, so making the wave's own stores visible to the wave is enough.  A lane beyond N reads row
                // N - 1, which another wave may have stored; its column of the product is never stored, and a column of an MFMA
                // result depends on that column of B alone, so whatever it reads changes nothing that is written.
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            for (int m = 0; m < mt0; ++m) {
                f32x16 o[ST_PT];
                ring.fetch();
                {
                    const nfa_v4u *A = ring.piece();
#pragma unroll
                    for (int t = 0; t < ST_PT; ++t) zero_acc(o[t]);
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                        const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                        for (int t = 0; t < ST_PT; ++t) o[t] = mfma<E>(a, df[t][q], o[t]);
                    }
                }
                ring.hand_over();
                for (int l = 2; l < L; ++l) {
                    if (!S.cat(l)) continue;
                    ring.fetch();
                    const nfa_v4u *A = ring.piece();
                    if (l == L - 1) {   // dZ_L = g, natural k order as in the first product
                        for (int q = 0; q < kqo; ++q) {
                            const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                            for (int t = 0; t < ST_PT; ++t) o[t] = mfma<E>(a, load_row8<E>(g, gf, pc[t], S.n_out, 16 * q + 8 * h, gv), o[t]);
                        }
                    } else {
                        const uint16_t *dzl = dz + (int64_t)l * N * W;
#pragma unroll
                        for (int q = 0; q < KQ; ++q) {
                            const nfa_v4u a = A[q * 64 + lane];
#pragma unroll
                            for (int t = 0; t < ST_PT; ++t) o[t] = mfma<E>(a, load_tile_frag<W>(dzl, pc[t], q, h), o[t]);
                        }
                    }
                    ring.hand_over();
                }
                const int ncols = S.n_in - 32 * m < 32 ? S.n_in - 32 * m : 32;
#pragma unroll
                for (int t = 0; t < ST_PT; ++t) {
                    const int64_t row0 = p[t] - r, left = N - row0;
                    stage_store<E>(o[t], st, dx, dx_f32 != 0, row0, (int)(left < 0 ? 0 : (left < 32 ? left : 32)), S.n_in, 32 * m, ncols, lane);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- weight gradient

constexpr int WS_CHUNK = 64;          // points staged per step
constexpr int WS_LD = WS_CHUNK + 8;   // halves per row of the transposed LDS images (16-byte aligned rows)
constexpr int WS_MACRO = 128;         // rows and columns of dW_l per workgroup

// Columns col0 .. col0+colsP-1 of rows c0 .. c0+63 of src [*, ld] (float32 or E; rows >= n1 and columns >= ld read as zero),
// transposed into T [colsP][WS_LD].
template <class E>
__device__ __forceinline__ void stage_cols_transposed(uint16_t *T, const void *src, bool is_f32, int ld, int col0, int colsP, int64_t c0,
                                                      int64_t n1, bool vec)
{
    const int units = (colsP / 8) * WS_CHUNK;
    for (int u = threadIdx.x; u < units; u += blockDim.x) {
        const int n = u & (WS_CHUNK - 1), cg = u >> 6;
        nfa_v4u f = {0u, 0u, 0u, 0u};
        if (c0 + n < n1) f = load_row8<E>(src, is_f32, c0 + n, ld, col0 + 8 * cg, vec);
#pragma unroll
        for (int j = 0; j < 8; ++j) T[(8 * cg + j) * WS_LD + n] = (uint16_t)(f[j >> 1] >> (16 * (j & 1)));
    }
}

// Workgroup (slice, layer, macro tile): the slice's partial of rows a0 .. a0+127, columns b0 .. b0+127 of dW_l = dZ_l^T [H_{l-1}, x],
// its 32 x 32 tiles dealt round-robin to the four waves.  The macro tiles of column 0 also write the slice's partial
// db_l = sum_p dZ_l[p, :] for their rows, in float32, the points in ascending order, eight at a time as a fixed tree.
template <class E, int W>
__global__ __launch_bounds__(256) void mlp_stream_wgrad_kernel(Shape S, const void *__restrict__ x, int x_f32, int x_vec,
                                                               const uint16_t *__restrict__ hidden, const uint16_t *__restrict__ dz,
                                                               const uint16_t *__restrict__ dz_out, int dzo_vec, int64_t N,
                                                               int64_t slice_len, float *__restrict__ partials, int64_t P, int zero_bias)
{
    constexpr int MAXT = (WS_MACRO / 32) * (WS_MACRO / 32) / 4;
    __shared__ __attribute__((aligned(16))) uint16_t Ta[WS_MACRO * WS_LD];
    __shared__ __attribute__((aligned(16))) uint16_t Tb[WS_MACRO * WS_LD];
    const int l = blockIdx.y, L = S.layers();
    const int M = S.out_dim(l), K = S.in_dim(l);
    const int nn = (K + WS_MACRO - 1) / WS_MACRO, mm = (M + WS_MACRO - 1) / WS_MACRO;
    if ((int)blockIdx.z >= mm * nn) return;   // the whole workgroup
    const int zm = blockIdx.z / nn, zn = blockIdx.z - zm * nn, a0 = WS_MACRO * zm, b0 = WS_MACRO * zn;
    const int mtl = (M - a0 < WS_MACRO ? M - a0 + 31 : WS_MACRO) / 32, ntl = (K - b0 < WS_MACRO ? K - b0 + 31 : WS_MACRO) / 32;
    const int n_tile = mtl * ntl;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const void *a_src = l == L - 1 ? (const void *)dz_out : (const void *)(dz + (int64_t)l * N * W);
    const bool a_vec = l == L - 1 ? dzo_vec != 0 : true;
    // the 128 columns of [H_{l-1}, x] (of x at layer 0) from b0 on: one source, since 128 divides W
    const bool from_x = l == 0 || b0 >= W;
    const void *b_src = from_x ? x : (const void *)(hidden + (int64_t)(l - 1) * N * W);
    const bool b_f32 = from_x && x_f32 != 0, b_vec = from_x ? x_vec != 0 : true;
    const int b_ld = from_x ? S.n_in : W, b_col0 = l == 0 || !from_x ? b0 : b0 - W;
    const bool has_bias = S.bias != 0 && zn == 0 && (int)threadIdx.x < WS_MACRO && a0 + (int)threadIdx.x < M;
    const bool col_sum = has_bias && !zero_bias;
    float db = 0.f;
    f32x16 acc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i) zero_acc(acc[i]);
    const int64_t n0 = (int64_t)blockIdx.x * slice_len, n1 = n0 + slice_len < N ? n0 + slice_len : N;
    for (int64_t c0 = n0; c0 < n1; c0 += WS_CHUNK) {
        __syncthreads();
        stage_cols_transposed<E>(Ta, a_src, false, M, a0, mtl * 32, c0, n1, a_vec);
        stage_cols_transposed<E>(Tb, b_src, b_f32, b_ld, b_col0, ntl * 32, c0, n1, b_vec);
        __syncthreads();
        if (col_sum) {   // points beyond the slice were staged as zeros
#pragma unroll
            for (int n8 = 0; n8 < WS_CHUNK / 8; ++n8) {
                const nfa_v4u f = *reinterpret_cast<const nfa_v4u *>(Ta + threadIdx.x * WS_LD + 8 * n8);
                const float s0 = unpack_half<E>(f[0], 0) + unpack_half<E>(f[0], 1), s1 = unpack_half<E>(f[1], 0) + unpack_half<E>(f[1], 1);
                const float s2 = unpack_half<E>(f[2], 0) + unpack_half<E>(f[2], 1), s3 = unpack_half<E>(f[3], 0) + unpack_half<E>(f[3], 1);
                db += (s0 + s1) + (s2 + s3);
            }
        }
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            const int tile = wave + 4 * i;
            if (tile < n_tile) {   // wave-uniform
                const int tm = tile / ntl, tn = tile - tm * ntl;
#pragma unroll
                for (int ks = 0; ks < WS_CHUNK / 16; ++ks) {
                    const nfa_v4u a = *reinterpret_cast<const nfa_v4u *>(Ta + (32 * tm + r) * WS_LD + 16 * ks + 8 * h);
                    const nfa_v4u b = *reinterpret_cast<const nfa_v4u *>(Tb + (32 * tn + r) * WS_LD + 16 * ks + 8 * h);
                    acc[i] = mfma<E>(a, b, acc[i]);
                }
            }
        }
    }
    if (has_bias) partials[(int64_t)blockIdx.x * P + S.bias_off(l) + a0 + threadIdx.x] = db;
    float *out = partials + (int64_t)blockIdx.x * P + S.master_off(l);
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int tile = wave + 4 * i;
        if (tile < n_tile) {
            const int tm = tile / ntl, tn = tile - tm * ntl, col = b0 + 32 * tn + r;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = a0 + 32 * tm + acc_row(reg, h);
                if (row < M && col < K) out[(int64_t)row * K + col] = acc[i][reg];
            }
        }
    }
}

// ---------------------------------------------------------------- host side

// The one statement of what the streamed passes hold.
int check_stream_shape(const char *who, int32_t elem, const nfa_mlp_desc *net, int64_t n_points, Shape *S)
{
    NFA_REQUIRE(net, "%s: the network descriptor is null", who);
    const int32_t n_in = net->n_in, n_out = net->n_out, width = net->width, n_hidden = net->n_hidden;
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the network's type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    NFA_REQUIRE(width == 128 || width == 256, "%s: width %d: 128 or 256 neurons are supported", who, width);
    NFA_REQUIRE(n_hidden >= 1 && n_hidden <= ST_MAX_HIDDEN, "%s: n_hidden %d: 1 to %d hidden layers are supported", who, n_hidden, ST_MAX_HIDDEN);
    NFA_REQUIRE(n_in >= 1 && n_in <= ST_MAX_IN, "%s: n_in %d: 1 to %d input features are supported", who, n_in, ST_MAX_IN);
    NFA_REQUIRE(n_out >= 1 && n_out <= ST_MAX_OUT, "%s: n_out %d: 1 to %d outputs are supported", who, n_out, ST_MAX_OUT);
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    NFA_REQUIRE(net->bias == 0 || net->bias == 1, "%s: bias %d: 0 or 1", who, net->bias);
    NFA_REQUIRE((net->skip_mask & ~((2 << n_hidden) - 4)) == 0, "%s: skip_mask 0x%x: only bits 2 to n_hidden (%d) may be set: layer 0 "
                "takes x itself and layer 1 follows it", who, (unsigned)net->skip_mask, n_hidden);
    *S = Shape{n_in, n_out, width, n_hidden, net->bias, net->skip_mask};
    int f16 = 0, b16 = 0;
    const int nf = build_pieces(*S, false, false, nullptr, &f16), nb = build_pieces(*S, true, true, nullptr, &b16);
    const int64_t piece = (int64_t)(f16 > b16 ? f16 : b16) * 16, fb = (int64_t)S->stream_bias_floats() * 4,
                  lds = stream_lds_bytes(f16 > b16 ? f16 : b16, S->stream_bias_floats());
    NFA_REQUIRE(lds <= LDS_BUDGET && nf <= ST_MAX_PIECES && nb <= ST_MAX_PIECES,
                "%s: the ring does not fit the LDS: %d slots of the largest piece (%lld B) with %lld B of store staging, %lld B of "
                "piece table and %lld B of biases are %lld B, against %lld B per compute unit (n_in %d, n_out %d, width %d, n_hidden %d, bias %d, skip_mask 0x%x)",
                who, ST_SLOTS, (long long)piece, (long long)ST_STAGE_BYTES, (long long)(ST_MAX_PIECES * sizeof(Piece)), (long long)fb, (long long)lds,
                (long long)LDS_BUDGET, n_in, n_out, width, n_hidden, net->bias, (unsigned)net->skip_mask);
    return NFA_OK;
}

template <class F>
void dispatch_stream(int32_t elem, const Shape &S, F &&f)
{
    auto widths = [&](auto tag) {
        if (S.W == 128) f(tag, std::integral_constant<int, 128>{});
        else f(tag, std::integral_constant<int, 256>{});
    };
    if (elem == NFA_ELEM_F16) widths(ElemTag<nfa_f16>{});
    else widths(ElemTag<nfa_bf16>{});
}

unsigned stream_grid(int64_t n_points)
{
    const int64_t want = ceil_div64(n_points, ST_POINTS);
    return (unsigned)(want < NFA_MLP_STREAM_GROUPS ? want : NFA_MLP_STREAM_GROUPS);
}

int64_t stream_slice_len(int64_t n_points)
{
    int64_t s = ceil_div64(n_points, NFA_MLP_STREAM_WGRAD_MIN_SLICE);
    s = s > NFA_MLP_STREAM_WGRAD_MAX_SLICES ? NFA_MLP_STREAM_WGRAD_MAX_SLICES : (s < 1 ? 1 : s);
    return ceil_div64(ceil_div64(n_points, s), WS_CHUNK) * WS_CHUNK;
}

}  // namespace
}  // namespace nfa

using namespace nfa;

int nfa_mlp_stream_pack_weights(int32_t elem, const nfa_mlp_desc *net, const float *params, void *fwd_image, int64_t fwd_elems,
                                void *bwd_image, int64_t bwd_elems, nfa_stream_t stream)
{
    const char *who = "nfa_mlp_stream_pack_weights";
    Shape S;
    if (int rc = check_stream_shape(who, elem, net, 0, &S)) return rc;
    const int64_t fe = S.fwd_off(S.layers()), be = S.bwd_off(S.layers());
    NFA_REQUIRE(fwd_elems == fe && bwd_elems == be, "%s: the images hold %lld and %lld elements for this shape, got %lld and %lld", who,
                (long long)fe, (long long)be, (long long)fwd_elems, (long long)bwd_elems);
    NFA_REQUIRE(params && fwd_image && bwd_image, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(fwd_image, 16) && aligned_to(bwd_image, 16), "%s: the images must be 16-byte aligned", who);
    dispatch_stream(elem, S, [&](auto tag, auto) {
        using E = typename decltype(tag)::type;
        mlp_pack_kernel<E><<<grid_1d(fe + be, 256), 256, 0, as_stream(stream)>>>(S, params, static_cast<uint16_t *>(fwd_image),
                                                                               static_cast<uint16_t *>(bwd_image), fe, be);
    });
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int nfa_mlp_stream_fwd(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *fwd_image, const float *bias,
                       int64_t n_points, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream)
{
    const char *who = "nfa_mlp_stream_fwd";
    Shape S;
    if (int rc = check_stream_shape(who, elem, net, n_points, &S)) return rc;
    NFA_REQUIRE(x_elem == NFA_ELEM_F32 || x_elem == elem, "%s: x_elem %d: float32 or the network's type (%d)", who, x_elem, elem);
    NFA_REQUIRE(y_elem == NFA_ELEM_F32 || y_elem == elem, "%s: y_elem %d: float32 or the network's type (%d)", who, y_elem, elem);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && fwd_image && y && (!save_hidden || hidden) && (!S.bias || bias), "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(fwd_image, 16) && aligned_to(hidden, 8) && aligned_to(x, x_elem == NFA_ELEM_F32 ? 4 : 2) &&
                aligned_to(y, y_elem == NFA_ELEM_F32 ? 4 : 2) && aligned_to(bias, 4),
                "%s: misaligned pointer (image 16, hidden 8, x, y and bias their element)", who);
    int slot16 = 0;
    const int n_pieces = build_pieces(S, false, false, nullptr, &slot16);
    const int64_t lds = stream_lds_bytes(slot16, S.stream_bias_floats());
    int rc = NFA_OK;
    dispatch_stream(elem, S, [&](auto tag, auto w) {
        using E = typename decltype(tag)::type;
        auto kern = mlp_stream_fwd_kernel<E, decltype(w)::value>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        kern<<<stream_grid(n_points), ST_THREADS, (size_t)lds, as_stream(stream)>>>(
            S, x, x_elem == NFA_ELEM_F32, row8_vec(x, S.n_in), static_cast<const uint16_t *>(fwd_image), slot16, n_pieces,
            S.bias ? bias : nullptr, n_points, y, y_elem == NFA_ELEM_F32, save_hidden ? static_cast<uint16_t *>(hidden) : nullptr);
    });
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int nfa_mlp_stream_bwd_data(int32_t elem, const nfa_mlp_desc *net, const void *grad_y, int32_t g_elem, const void *hidden,
                            const void *bwd_image, int64_t n_points, void *dz, void *dz_out, void *grad_x, int32_t x_elem,
                            nfa_stream_t stream)
{
    const char *who = "nfa_mlp_stream_bwd_data";
    Shape S;
    if (int rc = check_stream_shape(who, elem, net, n_points, &S)) return rc;
    NFA_REQUIRE(g_elem == NFA_ELEM_F32 || g_elem == elem, "%s: g_elem %d: float32 or the network's type (%d)", who, g_elem, elem);
    NFA_REQUIRE(x_elem == NFA_ELEM_F32 || x_elem == elem, "%s: x_elem %d: float32 or the network's type (%d)", who, x_elem, elem);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(grad_y && hidden && bwd_image && dz, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(bwd_image, 16) && aligned_to(hidden, 8) && aligned_to(dz, 8) && aligned_to(dz_out, 2) &&
                aligned_to(grad_y, g_elem == NFA_ELEM_F32 ? 4 : 2) && aligned_to(grad_x, x_elem == NFA_ELEM_F32 ? 4 : 2),
                "%s: misaligned pointer (image 16, hidden and dz 8, the others their element)", who);
    int slot16 = 0;
    const int n_pieces = build_pieces(S, true, grad_x != nullptr, nullptr, &slot16);
    const int64_t lds = stream_lds_bytes(slot16, 0);
    int rc = NFA_OK;
    dispatch_stream(elem, S, [&](auto tag, auto w) {
        using E = typename decltype(tag)::type;
        auto kern = mlp_stream_bwd_data_kernel<E, decltype(w)::value>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        kern<<<stream_grid(n_points), ST_THREADS, (size_t)lds, as_stream(stream)>>>(
            S, grad_y, g_elem == NFA_ELEM_F32, row8_vec(grad_y, S.n_out), static_cast<const uint16_t *>(hidden),
            static_cast<const uint16_t *>(bwd_image), slot16, n_pieces, n_points, static_cast<uint16_t *>(dz),
            static_cast<uint16_t *>(dz_out), grad_x, x_elem == NFA_ELEM_F32);
    });
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int nfa_mlp_stream_bwd_weights(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *hidden, const void *dz,
                               const void *dz_out, int64_t n_points, float *partials, int64_t partial_floats, float *grad_params,
                               int32_t zero_bias, nfa_stream_t stream)
{
    const char *who = "nfa_mlp_stream_bwd_weights";
    Shape S;
    if (int rc = check_stream_shape(who, elem, net, n_points, &S)) return rc;
    NFA_REQUIRE(x_elem == NFA_ELEM_F32 || x_elem == elem, "%s: x_elem %d: float32 or the network's type (%d)", who, x_elem, elem);
    NFA_REQUIRE(partial_floats >= 0, "%s: partial_floats %lld is negative", who, (long long)partial_floats);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(x && hidden && dz && dz_out && partials && grad_params, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(hidden, 16) && aligned_to(dz, 16) && aligned_to(dz_out, 2) && aligned_to(x, x_elem == NFA_ELEM_F32 ? 4 : 2) &&
                aligned_to(partials, 4) && aligned_to(grad_params, 4),
                "%s: misaligned pointer (hidden and dz 16, the others their element)", who);
    const int64_t P = S.n_params(), slice_len = stream_slice_len(n_points), n_slices = ceil_div64(n_points, slice_len);
    NFA_REQUIRE(partial_floats >= n_slices * P, "%s: partials holds %lld floats, %lld slices of %lld parameters need %lld", who,
                (long long)partial_floats, (long long)n_slices, (long long)P, (long long)(n_slices * P));
    int macro = 1;
    for (int l = 0; l < S.layers(); ++l) {
        const int t = ((S.out_dim(l) + WS_MACRO - 1) / WS_MACRO) * ((S.in_dim(l) + WS_MACRO - 1) / WS_MACRO);
        macro = t > macro ? t : macro;
    }
    dispatch_stream(elem, S, [&](auto tag, auto w) {
        using E = typename decltype(tag)::type;
        mlp_stream_wgrad_kernel<E, decltype(w)::value><<<dim3((unsigned)n_slices, (unsigned)S.layers(), (unsigned)macro), 256, 0, as_stream(stream)>>>(
            S, x, x_elem == NFA_ELEM_F32, row8_vec(x, S.n_in), static_cast<const uint16_t *>(hidden), static_cast<const uint16_t *>(dz),
            static_cast<const uint16_t *>(dz_out), row8_vec(dz_out, S.n_out), n_points, slice_len, partials, P, zero_bias != 0);
    });
    NFA_CHECK_LAUNCH(who);
    mlp_wgrad_sum_kernel<<<(unsigned)ceil_div64(P, 256), 256, 0, as_stream(stream)>>>(partials, n_slices, P, grad_params);
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

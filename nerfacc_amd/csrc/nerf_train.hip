// nerf_train.hip -- the data gradients of the vanilla NeRF field's two networks as ONE launch (nfa_nerf_train_bwd): from dL/d rgb
// and dL/d sigma to every dZ of the colour head and of the trunk, which nfa_mlp_stream_bwd_weights then turns into the weight
// gradients.  The composed chain runs this as two streamed data-gradient launches with torch's sigmoid / relu backward in front,
// torch's cat / split backward between them and a [N, W + 27] gradient row in memory; here the gradient never leaves registers
// between the two networks.
//
// Launch shape, ring, images and arithmetic are nerf_field.hip's and mlp_stream.hip's: a persistent grid, 4 waves x one 32-point
// tile, the BACKWARD images of nfa_mlp_stream_pack_weights (A = W_l^T) streamed one piece (a row tile of a layer, all its
// k-steps) per step through two LDS slots, one workgroup barrier per piece, EXEC all ones around every MFMA and cross-lane read.
//
//   piece table   the head's pieces, then the trunk's, in the order the chain runs backwards: the head's output layer (4 row
//                 tiles of one k-step), its hidden layers Dh-1 .. 1 (4 x 8 k-steps), the FIRST W / 32 row tiles of its layer 0 (the
//                 bottleneck's columns: the 27 direction columns need no gradient and their tile is never fetched), the trunk's
//                 output layer (W / 32 tiles of W / 16 + 1 k-steps, the largest piece: 17 KiB), its hidden layers D-1 .. 1.  The
//                 trunk's layer 0 and the x rows of every cat layer are left out, as build_pieces(.., need_dx = false) leaves them
//                 out: 24 + 64 pieces at the reference's shape.
//   dZ of the outputs   formed in registers: raw mode rounds g once; activated mode forms (g (1 - y)) y (torch's sigmoid backward,
//                 in its order) and y > 0 ? g : 0 in float32 from the stored outputs and rounds the product once.  The colour's three
//                 values are the one B fragment (natural k order) of the head's first product; they leave as 6 bytes per lane.
//   chain         per layer: the accumulators are masked by the saved activation (mask_tile_row: a select), rounded once with
//                 acc_frag, stored with store_tile_row (8-byte pieces, the lane halves alternating: 64-byte runs) and are the B
//                 fragments of the next product, as in mlp_stream.hip.
//   hand-off      the head's layer-0 product runs on W / 32 row tiles.  Each accumulator tile is rounded once with acc_frag (the
//                 head's grad_x rounding), its two fragments are brought from acc_frag's permuted k order into the natural order of
//                 the trunk's output layer in the backward image by one exchange between the lane halves (two ds_bpermute per
//                 fragment: lane half 0 keeps k 0..3 and receives 4..7, half 1 receives 8..11 and keeps 12..15), and they stay in
//                 registers as the first W / 16 B fragments of the trunk's first product; sigma's gradient is k-step W / 16.  The
//                 products sum in nfa_mlp_stream_bwd_data's order, so with equal dZ they give its bits.  The same fragments are
//                 dropped into the wave's LDS tile and leave once as the [N, W + 1] rows the weight gradient reads (nerf_field.h:
//                 one contiguous span per wave, 16-byte pieces).  The [N, W + 27] row, the cat / split backward and the reload of
//                 dL/dy for every row tile do not exist.
//   budget, W = 256   registers: 8 accumulator tiles (128), 16 hand-off fragments (64) or 16 dZ fragments (64), 5 ring registers
//                 (20): 222 + 128 by the compiler's count, no scratch.  LDS: 2 x 17 KiB ring, 1.25 KiB table, 4 x 16.1 KiB staging =
//                 99.5 KiB ("Fused NeRF field: training", has every instantiation's figures).
//
// The WARP instantiations (nfa_tnerf_train_bwd) are the T-NeRF field's backward: the chain above with nothing changed, then, in
// the same launch, what the composed chain runs as the trunk's dL/dx, the sinusoidal backward and the warp network's data gradient.
//   trunk dL/dx   the pieces of build_pieces(.., need_dx = true) follow the chain's in the table: per 32-feature tile of the 63
//                 inputs, layer 0's rows, then the x rows of every cat layer, ascending.  One accumulator sums them in
//                 mlp_stream_bwd_data_kernel's order: dZ_0 from registers, a cat layer's dZ_l read back from trunk_dz (the
//                 lane's own pieces, behind a wave-scope fence), a cat OUTPUT layer's dZ from trunk_dz_out in natural k order.
//                 It is rounded once to the half type (the composed chain's grad_x rounding) into the wave's LDS tile, idle by
//                 now: 32 rows of 66 halves.  The [N, 63] row never reaches memory.
//   sinusoidal    sinenc.hip's backward on that row (sinenc_dev.h), float32: lane half h forms the 15 terms tx_kd of frequencies
//                 5 h .. 5 h + 4 from sincosf(x'_d 2^k) of the saved x'; lane half 0 receives the other 15 (ds_bpermute) and sums
//                 ((g_id + tx_0d) + tx_1d) + .. in k order: dL/dx', which is the warp's dL/dy (x + delta passes it through).
//   warp chain    dL/dx' rounded once is warp_dz_out [N, 3] and the one B fragment (natural k order) of W_out^T dZ_out; then
//                 mlp.hip's backward chain on FusedMLP's backward image, RESIDENT in LDS behind the staging tiles (42 KiB at the
//                 reference's warp, 52 KiB at most), masks from the saved activations, warp_dz [D_w, N, 64] with store_tile_row.
//                 No dL/d(input row): the composed chain's need_x = False.  This stage has no ring traffic and no barrier.
//   budget, W = 256   LDS 99.5 + 42 = 141.5 KiB; registers and scratch: DESIGN.md, "Fused T-NeRF field: training".
#include "nerf_field.h"
#include "sinenc_dev.h"

namespace nfa {
namespace {

struct TrainBwdArgs {
    Shape T, H;
    const uint16_t *timg, *himg;   // the backward images
    int32_t slot16, n_pieces, n_head;
    int64_t N;
    const void *g_rgb, *g_sigma, *y_rgb, *y_sigma;
    int32_t g_rgb_f32, g_sigma_f32, y_rgb_f32, y_sigma_f32, activated;
    const uint16_t *th, *hh;       // the saved activations
    uint16_t *hdz, *hdzo, *tdz, *tdzo;
};
// what a WARP instantiation takes beside them
struct WarpBwdArgs {
    Shape S;
    const uint16_t *img;   // FusedMLP's backward image
    int32_t img16;         // in 16-byte fragments
    const float *xw;       // x' [N, 3]
    const uint16_t *wh;    // the warp's saved activations
    uint16_t *wdz, *wdzo;
};
struct TTrainBwdArgs : TrainBwdArgs { WarpBwdArgs w; };

constexpr int NT_DX_LD = 66;   // halves per row of the rounded dL/dx rows in a wave's tile (33 words: no bank conflicts)
constexpr int NT_DX_MT = (NF_POS_DIMS + 31) / 32;

// The order in which a pass consumes the pieces (header: piece table): the head's (n_head of them), then the trunk's; need_dx:
// then those of the trunk's dL/dx (header: trunk dL/dx).
__host__ __device__ inline int train_bwd_pieces(const Shape &T, const Shape &H, Piece *tab, int *max_n16, int *n_head, bool need_dx = false)
{
    int n = 0, mx = 0;
    auto put = [&](int64_t off16, int n16) {
        if (tab) tab[n] = Piece{(int32_t)off16, n16};
        mx = n16 > mx ? n16 : mx;
        ++n;
    };
    const int D = T.n_hidden, Dc = H.n_hidden, MT = T.W / 32, HMT = NF_HEAD_W / 32;
    for (int l = Dc; l >= 1; --l)
        for (int m = 0; m < HMT; ++m) put(H.bwd_off(l) / 8 + (int64_t)m * H.bwd_kq(l) * 64, H.bwd_kq(l) * 64);
    for (int m = 0; m < MT; ++m) put((int64_t)m * H.bwd_kq(0) * 64, H.bwd_kq(0) * 64);
    if (n_head) *n_head = n;
    for (int l = D; l >= 1; --l)
        for (int m = 0; m < MT; ++m) put(T.bwd_off(l) / 8 + (int64_t)m * T.bwd_kq(l) * 64, T.bwd_kq(l) * 64);
    for (int m = 0; need_dx && m < NT_DX_MT; ++m) {
        put((int64_t)m * T.bwd_kq(0) * 64, T.bwd_kq(0) * 64);
        for (int l = 2; l <= D; ++l)
            if (T.cat(l)) put(T.bwd_off(l) / 8 + (int64_t)(MT + m) * T.bwd_kq(l) * 64, T.bwd_kq(l) * 64);
    }
    if (max_n16) *max_n16 = mx;
    return n;
}

__host__ __device__ inline int64_t train_bwd_lds_bytes(int slot16, int W)
{
    return (int64_t)NF_SLOTS * slot16 * 16 + (int64_t)NF_MAX_PIECES * sizeof(Piece) + (int64_t)NF_WAVES * row_stage_bytes(W + 1);
}

__device__ __forceinline__ void zero_acc(f32x16 &a)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

// An acc_frag fragment (k = 8 (j >> 2) + 4 h + (j & 3)) as the fragment of the same k-step in natural order (k = 8 h + j)
__device__ __forceinline__ nfa_v4u frag_to_natural(const nfa_v4u &f, int lane, int h)
{
    const int other = (lane ^ 32) << 2;
    const uint32_t g0 = (uint32_t)__builtin_amdgcn_ds_bpermute(other, (int)(h ? f[0] : f[2]));
    const uint32_t g1 = (uint32_t)__builtin_amdgcn_ds_bpermute(other, (int)(h ? f[1] : f[3]));
    return h ? nfa_v4u{g0, g1, f[2], f[3]} : nfa_v4u{f[0], f[1], g0, g1};
}

// dL/dx' of the lane's point on lane half 0 from the rounded dL/dx row in the wave's tile (header: sinusoidal)
template <class E>
__device__ __forceinline__ void sin_bwd_stage(const uint16_t *row, const float (&xw)[3], int lane, int h, float (&gx)[3])
{
    constexpr int L = NF_POS_L, HALF = 3 * L / 2;
    static_assert(L % 2 == 0, "the frequencies are split between the lane halves");
    const int other = (lane ^ 32) << 2;
    float tx[2 * HALF];
#pragma unroll
    for (int t = 0; t < HALF; ++t) {   // item (k, d) = (t / 3 + 5 h, t % 3): columns 3 + 3 k + d and 33 + 3 k + d
        const float sc = h ? (float)(1 << (t / 3 + L / 2)) : (float)(1 << (t / 3));
        float s, c;
        sincosf(xw[t % 3] * sc, &s, &c);
        const int col = 3 + t + HALF * h;
        const float own = sin_bwd_tx(sc, 1.0f, half_value<E>(row[col]), half_value<E>(row[3 * L + col]), s, c);
        tx[t] = own;
        tx[HALF + t] = __int_as_float(__builtin_amdgcn_ds_bpermute(other, __float_as_int(own)));   // lane half 0: frequencies 5 .. 9
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) gx[d] = sin_bwd_sum(half_value<E>(row[d]), tx + d, L, 3);
}

// WARP: the T-NeRF field's backward, the stages of the header behind the chain; the plain instantiations never see WarpBwdArgs.
template <class E, int W, bool WARP = false>
__global__ __launch_bounds__(NF_THREADS) void nerf_train_bwd_kernel(const std::conditional_t<WARP, TTrainBwdArgs, TrainBwdArgs> a)
{
    constexpr int MT = W / 32, KQ = W / 16, HW = NF_HEAD_W, HMT = HW / 32, HKQ = HW / 16, ZO = W + 1;
    constexpr int MAXV = ((KQ + 1) * 64 + NF_THREADS - 1) / NF_THREADS;   // the trunk's output layer, the largest piece
    static_assert(HMT <= MT && HKQ <= KQ, "the head's chain fits the trunk's registers");
    extern __shared__ __attribute__((aligned(16))) unsigned char nt_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int D = a.T.n_hidden, Dc = a.H.n_hidden;
    Piece *tab = reinterpret_cast<Piece *>(nt_lds + (int64_t)NF_SLOTS * a.slot16 * 16);
    uint16_t *st = reinterpret_cast<uint16_t *>(tab + NF_MAX_PIECES) + wave * (row_stage_bytes(ZO) / 2);
    FieldRing<MAXV> ring;
    if (threadIdx.x == 0) train_bwd_pieces(a.T, a.H, tab, nullptr, nullptr, WARP);
    [[maybe_unused]] const nfa_v4u *wimg = reinterpret_cast<const nfa_v4u *>(reinterpret_cast<unsigned char *>(tab + NF_MAX_PIECES) + NF_WAVES * row_stage_bytes(ZO));
    if constexpr (WARP) {   // the warp's backward image, resident behind the staging tiles; ring.start()'s barriers publish it
        nfa_v4u *dst = const_cast<nfa_v4u *>(wimg);
        const nfa_v4u *src = reinterpret_cast<const nfa_v4u *>(a.w.img);
        for (int i = threadIdx.x; i < a.w.img16; i += NF_THREADS) dst[i] = src[i];
    }
    ring.img0 = reinterpret_cast<const nfa_v4u *>(a.himg);
    ring.img1 = reinterpret_cast<const nfa_v4u *>(a.timg);
    ring.slots = reinterpret_cast<nfa_v4u *>(nt_lds);
    ring.tab = tab;
    ring.slot16 = a.slot16;
    ring.n0 = a.n_head;
    ring.n_pieces = a.n_pieces;
    ring.start();
    const bool act = a.activated != 0;
    const int64_t N = a.N, n_pass = ceil_div64(N, NF_POINTS);
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int64_t p = (pass * NF_WAVES + wave) * 32 + r, pc = p < N ? p : N - 1, row0 = p - r;
        // ---- dZ of the two outputs (header)
        uint32_t cb[3], sb;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float g = a.g_rgb ? load_elem<E>(a.g_rgb, a.g_rgb_f32 != 0, 3 * pc + k) : 0.f;
            if (act && a.g_rgb) {
                const float y = load_elem<E>(a.y_rgb, a.y_rgb_f32 != 0, 3 * pc + k);
                g = (g * (1.f - y)) * y;
            }
            cb[k] = half_bits<E>(g);
        }
        {
            float g = a.g_sigma ? load_elem<E>(a.g_sigma, a.g_sigma_f32 != 0, pc) : 0.f;
            if (act && a.g_sigma) g = load_elem<E>(a.y_sigma, a.y_sigma_f32 != 0, pc) > 0.f ? g : 0.f;
            sb = half_bits<E>(g);
        }
        if (h == 0 && p < N) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.hdzo[3 * p + k] = (uint16_t)cb[k];
        }
        const nfa_v4u go = {h ? 0u : (cb[0] | (cb[1] << 16)), h ? 0u : cb[2], 0u, 0u};   // natural k order: columns 8 h .. 8 h + 7
        const nfa_v4u gs = {h ? 0u : sb, 0u, 0u, 0u};                                      // k-step W / 16: column W is sigma
        // ---- the head's chain
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < HMT; ++m) {   // dH_last = W_out^T dZ_out: one k-step
            ring.fetch();
            const nfa_v4u *A = ring.piece();
            zero_acc(acc[m]);
            acc[m] = mfma<E>(A[lane], go, acc[m]);
            ring.hand_over();
        }
        nfa_v4u df[KQ];
        for (int l = Dc - 1;; --l) {   // dZ_l = dH_l * (H_l > 0), rounded
            const uint16_t *hl = a.hh + (int64_t)l * N * HW;
#pragma unroll
            for (int m = 0; m < HMT; ++m) {
                mask_tile_row<E, HW>(acc[m], hl, pc, m, h);
                df[2 * m] = acc_frag<E>(acc[m], 0);
                df[2 * m + 1] = acc_frag<E>(acc[m], 1);
                if (p < N) store_tile_row<HW>(a.hdz + (int64_t)l * N * HW, p, m, h, df[2 * m], df[2 * m + 1]);
            }
            if (l == 0) break;
#pragma unroll
            for (int m = 0; m < HMT; ++m) {
                ring.fetch();
                const nfa_v4u *A = ring.piece();
                zero_acc(acc[m]);
#pragma unroll
                for (int q = 0; q < HKQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], df[q], acc[m]);
                ring.hand_over();
            }
        }
        // ---- the hand-off: the bottleneck's columns of the head's layer-0 data gradient become the trunk's dZ_out
        nfa_v4u gb[KQ];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            ring.fetch();
            const nfa_v4u *A = ring.piece();
            f32x16 o;
            zero_acc(o);
#pragma unroll
            for (int q = 0; q < HKQ; ++q) o = mfma<E>(A[q * 64 + lane], df[q], o);
            ring.hand_over();
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                gb[2 * m + s] = frag_to_natural(acc_frag<E>(o, s), lane, h);
                stage_put8(st, ZO, r, 32 * m + 16 * s + 8 * h, gb[2 * m + s]);
            }
        }
        if (h == 0) st[r * ZO + W] = (uint16_t)sb;
        stage_flush(st, a.tdzo, row0, tile_rows(row0, N), ZO, lane);
        // ---- the trunk's chain
#pragma unroll
        for (int m = 0; m < MT; ++m) {   // dH_last = W_D[:, :W]^T dZ_out, nfa_mlp_stream_bwd_data's k order
            ring.fetch();
            const nfa_v4u *A = ring.piece();
            zero_acc(acc[m]);
#pragma unroll
            for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], gb[q], acc[m]);
            acc[m] = mfma<E>(A[KQ * 64 + lane], gs, acc[m]);
            ring.hand_over();
        }
        for (int l = D - 1;; --l) {
            const uint16_t *hl = a.th + (int64_t)l * N * W;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                mask_tile_row<E, W>(acc[m], hl, pc, m, h);
                df[2 * m] = acc_frag<E>(acc[m], 0);
                df[2 * m + 1] = acc_frag<E>(acc[m], 1);
                if (p < N) store_tile_row<W>(a.tdz + (int64_t)l * N * W, p, m, h, df[2 * m], df[2 * m + 1]);
            }
            if (l == 0) break;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                ring.fetch();
                const nfa_v4u *A = ring.piece();
                zero_acc(acc[m]);
#pragma unroll
                for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], df[q], acc[m]);
                ring.hand_over();
            }
        }
        if constexpr (WARP) {
            // ---- the trunk's dL/dx (header): df[] holds dZ_0; the wave's own stores of trunk_dz and trunk_dz_out become visible to it
            wave_sync_lds();
#pragma unroll
            for (int m = 0; m < NT_DX_MT; ++m) {
                f32x16 o;
                zero_acc(o);
                ring.fetch();
                {
                    const nfa_v4u *A = ring.piece();
#pragma unroll
                    for (int q = 0; q < KQ; ++q) o = mfma<E>(A[q * 64 + lane], df[q], o);
                }
                ring.hand_over();
                for (int l = 2; l <= D; ++l) {
                    if (!a.T.cat(l)) continue;
                    ring.fetch();
                    const nfa_v4u *A = ring.piece();
                    if (l == D) {   // dZ_D = [the bottleneck's gradient, sigma's], natural k order as in the chain's first product
                        for (int q = 0; q <= KQ; ++q) o = mfma<E>(A[q * 64 + lane], load_row8<E>(a.tdzo, false, pc, ZO, 16 * q + 8 * h, false), o);
                    } else {
                        const uint16_t *dzl = a.tdz + (int64_t)l * N * W;
#pragma unroll
                        for (int q = 0; q < KQ; ++q) o = mfma<E>(A[q * 64 + lane], load_tile_frag<W>(dzl, pc, q, h), o);
                    }
                    ring.hand_over();
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) st[r * NT_DX_LD + 32 * m + acc_row(reg, h)] = (uint16_t)half_bits<E>(o[reg]);
            }
            wave_sync_lds();
            // ---- the sinusoidal backward (header): dL/dx' on lane half 0
            float xw[3], gx[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) xw[k] = a.w.xw[3 * pc + k];
            sin_bwd_stage<E>(st + r * NT_DX_LD, xw, lane, h, gx);
            wave_sync_lds();   // the tile is read: the next pass may write it
            // ---- the warp's chain (header): mlp.hip's backward on the resident image, no dL/d(input row)
            constexpr int WW = NF_WARP_W, WMT = WW / 32, WKQ = WW / 16;
            const Shape &S = a.w.S;
            uint32_t wb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) wb[k] = half_bits<E>(gx[k]);
            if (h == 0 && p < N) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.w.wdzo[3 * p + k] = (uint16_t)wb[k];
            }
            const nfa_v4u wgo = {h ? 0u : (wb[0] | (wb[1] << 16)), h ? 0u : wb[2], 0u, 0u};
            f32x16 wacc[WMT];
            int off16 = (int)(S.bwd_off(S.n_hidden) / 8);
#pragma unroll
            for (int m = 0; m < WMT; ++m) {   // dH_last = W_out[:, :64]^T dZ_out: one k-step (bwd_kq of 3 outputs)
                zero_acc(wacc[m]);
                wacc[m] = mfma<E>(wimg[off16 + m * 64 + lane], wgo, wacc[m]);
            }
            nfa_v4u wdf[WKQ];
            for (int l = S.n_hidden - 1;; --l) {
                const uint16_t *hl = a.w.wh + (int64_t)l * N * WW;
#pragma unroll
                for (int m = 0; m < WMT; ++m) {
                    mask_tile_row<E, WW>(wacc[m], hl, pc, m, h);
                    wdf[2 * m] = acc_frag<E>(wacc[m], 0);
                    wdf[2 * m + 1] = acc_frag<E>(wacc[m], 1);
                    if (p < N) store_tile_row<WW>(a.w.wdz + (int64_t)l * N * WW, p, m, h, wdf[2 * m], wdf[2 * m + 1]);
                }
                if (l == 0) break;
                off16 = (int)(S.bwd_off(l) / 8);
#pragma unroll
                for (int m = 0; m < WMT; ++m) {
                    zero_acc(wacc[m]);
#pragma unroll
                    for (int q = 0; q < WKQ; ++q) wacc[m] = mfma<E>(wimg[off16 + (m * WKQ + q) * 64 + lane], wdf[q], wacc[m]);
                }
            }
        }
    }
}

// Both entries.  warp (its shape checked by the caller), warp_image, wsaved and wgrads: nfa_tnerf_train_bwd's, checked next to
// the vanilla pass's descriptors, pointers and alignment.
int train_bwd(const char *who, int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *trunk_bwd_image,
              const void *head_bwd_image, int64_t n_points, int32_t activated, const nfa_nerf_saved *saved, const nfa_nerf_grads *grads,
              nfa_stream_t stream, const Shape *warp = nullptr, const void *warp_bwd_image = nullptr, const nfa_tnerf_saved *wsaved = nullptr,
              const nfa_tnerf_grads *wgrads = nullptr)
{
    Shape T, H;
    if (int rc = check_field_shape(who, elem, trunk, head, 0, n_points, &T, &H)) return rc;
    NFA_REQUIRE(saved && (!warp || wsaved), "%s: the saved-buffers descriptor is null", who);
    NFA_REQUIRE(grads && (!warp || wgrads), "%s: the gradients descriptor is null", who);
    NFA_REQUIRE(activated == 0 || activated == 1, "%s: activated must be 0 (raw outputs) or 1 (relu, sigmoid) (got %d)", who, activated);
    const nfa_nerf_grads &g = *grads;
    auto elem_ok = [&](int32_t e) { return e == NFA_ELEM_F32 || e == elem; };
    NFA_REQUIRE(elem_ok(g.g_rgb_elem), "%s: g_rgb_elem %d: float32 or the networks' type (%d)", who, g.g_rgb_elem, elem);
    NFA_REQUIRE(elem_ok(g.g_sigma_elem), "%s: g_sigma_elem %d: float32 or the networks' type (%d)", who, g.g_sigma_elem, elem);
    NFA_REQUIRE(!activated || (elem_ok(g.y_rgb_elem) && elem_ok(g.y_sigma_elem)), "%s: y_rgb_elem %d, y_sigma_elem %d: float32 or the networks' "
                "type (%d)", who, g.y_rgb_elem, g.y_sigma_elem, elem);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(trunk_bwd_image && head_bwd_image && (!warp || warp_bwd_image), "%s: null pointer (image)", who);
    NFA_REQUIRE(saved->trunk_hidden && saved->head_hidden, "%s: null pointer (trunk_hidden or head_hidden)", who);
    NFA_REQUIRE(!warp || (wsaved->warp_hidden && wsaved->warped), "%s: null pointer (warp_hidden or warped)", who);
    NFA_REQUIRE(g.head_dz && g.head_dz_out && g.trunk_dz && g.trunk_dz_out, "%s: null pointer (head_dz, head_dz_out, trunk_dz or trunk_dz_out)", who);
    NFA_REQUIRE(!warp || (wgrads->warp_dz && wgrads->warp_dz_out), "%s: null pointer (warp_dz or warp_dz_out)", who);
    NFA_REQUIRE(!activated || ((!g.g_rgb || g.y_rgb) && (!g.g_sigma || g.y_sigma)), "%s: activated: y_rgb and y_sigma are read next to g_rgb "
                "and g_sigma", who);
    auto el = [](int32_t e) { return (uintptr_t)(e == NFA_ELEM_F32 ? 4 : 2); };
    NFA_REQUIRE(aligned_to(trunk_bwd_image, 16) && aligned_to(head_bwd_image, 16) && aligned_to(saved->trunk_hidden, 16) &&
                aligned_to(saved->head_hidden, 16) && aligned_to(g.head_dz, 16) && aligned_to(g.trunk_dz, 16) && aligned_to(g.trunk_dz_out, 16) &&
                aligned_to(g.head_dz_out, 2) && aligned_to(g.g_rgb, el(g.g_rgb_elem)) && aligned_to(g.g_sigma, el(g.g_sigma_elem)) &&
                (!activated || (aligned_to(g.y_rgb, el(g.y_rgb_elem)) && aligned_to(g.y_sigma, el(g.y_sigma_elem)))),
                "%s: misaligned pointer (images, hidden, dz and trunk_dz_out 16, the others their element)", who);
    NFA_REQUIRE(!warp || (aligned_to(warp_bwd_image, 16) && aligned_to(wsaved->warp_hidden, 16) && aligned_to(wgrads->warp_dz, 16) &&
                          aligned_to(wsaved->warped, 4) && aligned_to(wgrads->warp_dz_out, 2)),
                "%s: misaligned pointer (warp image, warp_hidden and warp_dz 16, the others their element)", who);
    TTrainBwdArgs ta = {};
    TrainBwdArgs &a = ta;
    a.T = T, a.H = H;
    a.timg = static_cast<const uint16_t *>(trunk_bwd_image), a.himg = static_cast<const uint16_t *>(head_bwd_image);
    int slot16 = 0, n_head = 0;
    a.n_pieces = train_bwd_pieces(T, H, nullptr, &slot16, &n_head, warp != nullptr);
    a.slot16 = slot16, a.n_head = n_head, a.N = n_points;
    a.g_rgb = g.g_rgb, a.g_sigma = g.g_sigma, a.y_rgb = g.y_rgb, a.y_sigma = g.y_sigma;
    a.g_rgb_f32 = g.g_rgb_elem == NFA_ELEM_F32, a.g_sigma_f32 = g.g_sigma_elem == NFA_ELEM_F32;
    a.y_rgb_f32 = g.y_rgb_elem == NFA_ELEM_F32, a.y_sigma_f32 = g.y_sigma_elem == NFA_ELEM_F32;
    a.activated = activated;
    a.th = static_cast<const uint16_t *>(saved->trunk_hidden), a.hh = static_cast<const uint16_t *>(saved->head_hidden);
    a.hdz = static_cast<uint16_t *>(g.head_dz), a.hdzo = static_cast<uint16_t *>(g.head_dz_out);
    a.tdz = static_cast<uint16_t *>(g.trunk_dz), a.tdzo = static_cast<uint16_t *>(g.trunk_dz_out);
    int64_t lds = train_bwd_lds_bytes(slot16, T.W);
    if (warp) {
        const int64_t img = warp->bwd_off(warp->layers()) * 2;
        NFA_REQUIRE(lds + img <= LDS_BUDGET, "%s: the warp's backward image (%lld B) does not fit the LDS behind the ring, the piece table and "
                    "the staging tiles (%lld B), against %lld B per compute unit", who, (long long)img, (long long)lds, (long long)LDS_BUDGET);
        lds += img;
        ta.w.S = *warp, ta.w.img = static_cast<const uint16_t *>(warp_bwd_image), ta.w.img16 = (int32_t)(img / 16);
        ta.w.xw = wsaved->warped, ta.w.wh = static_cast<const uint16_t *>(wsaved->warp_hidden);
        ta.w.wdz = static_cast<uint16_t *>(wgrads->warp_dz), ta.w.wdzo = static_cast<uint16_t *>(wgrads->warp_dz_out);
    }
    const int64_t want = ceil_div64(n_points, NF_POINTS);
    const unsigned grid = (unsigned)(want < NFA_MLP_STREAM_GROUPS ? want : NFA_MLP_STREAM_GROUPS);
    int rc = NFA_OK;
    auto launch = [&](auto tag, auto w) {
        using E = typename decltype(tag)::type;
        dispatch_bool(warp != nullptr, [&](auto warp_c) {
            auto kern = nerf_train_bwd_kernel<E, decltype(w)::value, decltype(warp_c)::value>;
            if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
            if constexpr (decltype(warp_c)::value) kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(ta);
            else kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(a);
        });
    };
    auto by_width = [&](auto tag) {
        if (T.W == 128) launch(tag, std::integral_constant<int, 128>{});
        else launch(tag, std::integral_constant<int, 256>{});
    };
    if (elem == NFA_ELEM_F16) by_width(ElemTag<nfa_f16>{});
    else by_width(ElemTag<nfa_bf16>{});
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

}  // namespace
}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_nerf_train_bwd(int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *trunk_bwd_image,
                       const void *head_bwd_image, int64_t n_points, int32_t activated, const nfa_nerf_saved *saved,
                       const nfa_nerf_grads *grads, nfa_stream_t stream)
{
    return train_bwd("nfa_nerf_train_bwd", elem, trunk, head, trunk_bwd_image, head_bwd_image, n_points, activated, saved, grads, stream);
}

int nfa_tnerf_train_bwd(int32_t elem, const nfa_mlp_desc *warp, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head,
                        const void *warp_bwd_image, const void *trunk_bwd_image, const void *head_bwd_image, int64_t n_points,
                        int32_t activated, const nfa_nerf_saved *saved, const nfa_tnerf_saved *warp_saved, const nfa_nerf_grads *grads,
                        const nfa_tnerf_grads *warp_grads, nfa_stream_t stream)
{
    const char *who = "nfa_tnerf_train_bwd";
    Shape S;
    if (int rc = check_warp_shape(who, elem, warp, &S)) return rc;
    return train_bwd(who, elem, trunk, head, trunk_bwd_image, head_bwd_image, n_points, activated, saved, grads, stream, &S, warp_bwd_image,
                     warp_saved, warp_grads);
}

}  // extern "C"

// ndr_warp.h -- the invertible warp of the reference's NDR T-NeRF field (ref: examples/radiance_fields/mlp.py,
// NDRTNeRFRadianceField; arXiv 2206.15258) as a stage of the fused NeRF query (nerf_field.hip, WARP == 2) and as the kernel of its
// own behind nfa_ndr_warp.  Three coupling blocks i = 0, 1, 2 on x = (u, v, w), t_enc the 9-wide encoded time:
//   dw = net1_i(cat[enc(u, v) (18), time1_i(t_enc) (64)])     82 -> 2 x 128 -> 1          w  = w + dw
//   rt = net2_i(cat[enc(w) (9),     time2_i(t_enc) (64)])     73 -> 1 x 128 -> 3          (theta, tu, tv) = rt
//   (u, v) = (cos du + sin dv, -sin du + cos dv),  du = u - tu, dv = v - tv
// with the axes rolled to (v, w, u) behind block 0 and to (w, u, v) behind block 1.
//
//   weights       21 small matrices and six time matrices, 288 KiB: more than LDS.  They are ONE device image, the warp's pieces
//                 in front of the trunk's in the piece table, and go through the same two-slot ring: per block 2 row tiles of
//                 time layer 1 (1 KiB each), 4 + 4 + 1 of net 1 (6, 8 and 8 KiB), 2 of time layer 2, 4 + 1 of net 2 (5 and 8 KiB):
//                 18 pieces, 54 per pass, the largest 8 KiB against the trunk's 20 KiB slot.  The nets' parts are FusedMLP's
//                 forward images unchanged; a time layer's is a layer-0 image (natural k order, one k-step).  Unlike T-NeRF's
//                 resident image every wave takes every barrier of the stage: EXEC is all ones around every MFMA and every
//                 cross-lane read, a partial tile clamps its loads and masks only its stores.
//   biases        one float32 block, 576 floats per coupling block (64, 128, 128, 32, 64, 128, 32: the one-tile output layers
//                 padded with zeros by the packer), 6.75 KiB, staged once behind the trunk's and the head's.
//   t_enc         one B fragment in natural k order (t, four sines, four cosines, zeros), formed once per pass: the bits
//                 SinusoidalEncoding (1, 0, 4) stores.  time_tile is the time layer's arithmetic, FusedMLP's without an
//                 activation: half operands, an accumulator that starts from the float32 bias, one rounding (acc_frag);
//                 nfa_ndr_time_features, the composed chain's pass, calls the same function.
//   cat rows      FusedMLP's layer 0 reads its row from memory in natural k order, and the order of an MFMA's operands is part
//                 of a float32 sum's bits.  So that dw and rt ARE the composed chain's bits, a wave assembles the 82- and
//                 73-wide rows in its own LDS tile (32 rows of 96 halves, 6 KiB): each lane drops the encoder columns it
//                 evaluated itself (lane half h takes frequencies 2 h and 2 h + 1: no exchange) and the halves of its time
//                 accumulators at cat's column (stage_put's 2-byte LDS writes), and reads its k-steps back as 16-byte fragments.
//                 The rows never reach global memory.
//   coupling      dw and (theta, tu, tv) are registers 0 .. 2 of lane half 0 of a one-tile output layer, float32, never rounded;
//                 lane half 1 reads them from the lane 32 away.  w + dw, u - tu, the four products and two sums of the rotation
//                 and the axis rolls are float32 register work on both halves, every operation rounded on its own (the file is
//                 built with -ffp-contract=off); sin and cos of theta are one sincosf, SinusoidalEncoding (1, 0, 1)'s.
//   budget        LDS at W = 256: 2 x 20 KiB ring, 1.25 KiB table, 9.75 KiB trunk and head biases, 6.75 KiB warp biases, 4 x 6 KiB
//                 cat tiles = 81.75 KiB of 160.  Registers and scratch: nerf_field.hip's header.
#pragma once
#include "nerf_field.h"

namespace nfa {
namespace {

constexpr int ND_BLOCKS = 3, ND_W = 128, ND_TW = 64, ND_TDIMS = 9;
constexpr int ND_UV_DIMS = 18, ND_W_DIMS = 9;                        // SinusoidalEncoding (2, 0, 4) and (1, 0, 4) with identity
constexpr int ND_KQ1 = (ND_UV_DIMS + ND_TW + 15) / 16, ND_KQ2 = (ND_W_DIMS + ND_TW + 15) / 16, ND_KQ = ND_W / 16;   // 6, 5, 8
constexpr int ND_MT = ND_W / 32, ND_TMT = ND_TW / 32;
constexpr int ND_LD = 96;                                            // halves of a row of a wave's cat tile
constexpr int ND_STAGE_BYTES = 32 * ND_LD * 2;
// the image of a coupling block in 16-byte fragments: time 1, net 1 (layer 0, layer 1, output), time 2, net 2 (layer 0, output)
constexpr int ND_TIME16 = ND_TMT * 64;
constexpr int ND_OFF_T1 = 0, ND_OFF_N1 = ND_OFF_T1 + ND_TIME16, ND_N1_16 = (ND_MT * ND_KQ1 + ND_MT * ND_KQ + ND_KQ) * 64;
constexpr int ND_OFF_T2 = ND_OFF_N1 + ND_N1_16, ND_OFF_N2 = ND_OFF_T2 + ND_TIME16, ND_N2_16 = (ND_MT * ND_KQ2 + ND_KQ) * 64;
constexpr int ND_BLOCK16 = ND_OFF_N2 + ND_N2_16;                     // 6144: 96 KiB
constexpr int64_t ND_IMAGE_ELEMS = (int64_t)ND_BLOCKS * ND_BLOCK16 * 8;
constexpr int ND_BLOCK_PIECES = 2 * ND_TMT + 3 * ND_MT + 2, ND_PIECES = ND_BLOCKS * ND_BLOCK_PIECES;   // 18, 54
constexpr int ND_MAX_PIECE16 = ND_KQ * 64;
// the biases of a coupling block in floats
constexpr int ND_B_T1 = 0, ND_B_N1 = ND_B_T1 + ND_TW, ND_B_T2 = ND_B_N1 + 2 * ND_W + 32, ND_B_N2 = ND_B_T2 + ND_TW;
constexpr int ND_BLOCK_BIAS = ND_B_N2 + ND_W + 32, ND_BIAS_FLOATS = ND_BLOCKS * ND_BLOCK_BIAS;   // 576, 1728
static_assert(ND_BLOCK16 == 6144 && ND_BLOCK_BIAS == 576 && ND_PIECES + 73 + 17 <= NF_MAX_PIECES, "the sizes the header states");
static_assert(ND_UV_DIMS + ND_TW <= ND_LD && 16 * ND_KQ1 <= ND_LD && 16 * ND_KQ2 <= ND_LD, "the cat rows fit the tile");

// The order in which a pass consumes the warp's pieces.  Returns their number.
__host__ __device__ inline int ndr_pieces(Piece *tab)
{
    int n = 0;
    auto put = [&](int off16, int tiles, int kq) {
        for (int m = 0; m < tiles; ++m) tab[n++] = Piece{off16 + m * kq * 64, kq * 64};
    };
    for (int b = 0; b < ND_BLOCKS; ++b) {
        const int o = b * ND_BLOCK16;
        put(o + ND_OFF_T1, ND_TMT, 1);
        put(o + ND_OFF_N1, ND_MT, ND_KQ1);
        put(o + ND_OFF_N1 + ND_MT * ND_KQ1 * 64, ND_MT, ND_KQ);
        put(o + ND_OFF_N1 + ND_MT * (ND_KQ1 + ND_KQ) * 64, 1, ND_KQ);
        put(o + ND_OFF_T2, ND_TMT, 1);
        put(o + ND_OFF_N2, ND_MT, ND_KQ2);
        put(o + ND_OFF_N2 + ND_MT * ND_KQ2 * 64, 1, ND_KQ);
    }
    return n;
}

// what the NDR instantiations take beside NerfArgs
struct NdrWarp {
    const uint16_t *img;
    const float *bias;
    const float *times;   // [N] in the position form, [n_rays] in the ray-sample form
    float *warped;        // [N, 3], optional
};

// The B fragment of the encoded time (header: t_enc).  Lane half h evaluates frequencies 2 h and 2 h + 1.
template <class E>
__device__ __forceinline__ nfa_v4u time_frag(float t, int lane, int h)
{
    uint32_t tt[4];
    const int other = (lane ^ 32) << 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float sc = h ? (float)(1 << (j + 2)) : (float)(1 << j);
        float s, c;
        sincosf(t * sc, &s, &c);
        const uint32_t own = pack_halves<E>(s, c);
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(other, (int)own);
        tt[j] = h ? got : own;
        tt[2 + j] = h ? own : got;
    }
    auto sn = [&](int k) { return tt[k] & 0xFFFFu; };
    auto cs = [&](int k) { return tt[k] >> 16; };
    const nfa_v4u lo = {half_bits<E>(t) | (sn(0) << 16), sn(1) | (sn(2) << 16), sn(3) | (cs(0) << 16), cs(1) | (cs(2) << 16)};
    const nfa_v4u hi = {cs(3), 0u, 0u, 0u};
    return h ? hi : lo;
}

// One row tile of a time layer: A its 64 fragments (LDS or global memory), b its 32 biases
template <class E>
__device__ __forceinline__ f32x16 time_tile(const nfa_v4u *A, const float *b, const nfa_v4u &te, int lane, int h)
{
    f32x16 acc;
    init_acc(acc, true, b, h);
    return mfma<E>(A[lane], te, acc);
}

__device__ __forceinline__ void put_half(uint16_t *st, int r, int c, uint32_t bits) { st[r * ND_LD + c] = (uint16_t)bits; }

// Row r of the wave's cat tile: [enc(v[0 .. D-1]) (D (1 + 8) columns), the 64 time features, zeros up to 16 KQ], and the lane's
// KQ fragments of it (header: cat rows)
template <class E, int D, int KQ>
__device__ __forceinline__ void cat_frags(uint16_t *st, const float *v, const f32x16 (&tf)[ND_TMT], int lane, int r, int h, nfa_v4u (&f)[KQ])
{
    constexpr int ENC = 9 * D;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (h == 0) put_half(st, r, d, half_bits<E>(v[d]));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = 2 * h + j;
            float s, c;
            sincosf(v[d] * (h ? (float)(1 << (j + 2)) : (float)(1 << j)), &s, &c);
            put_half(st, r, D + k * D + d, half_bits<E>(s));
            put_half(st, r, 5 * D + k * D + d, half_bits<E>(c));
        }
    }
#pragma unroll
    for (int m = 0; m < ND_TMT; ++m) {
        stage_put_acc_frag(st + ENC, ND_LD, r, h, m, 0, acc_frag<E>(tf[m], 0));
        stage_put_acc_frag(st + ENC, ND_LD, r, h, m, 1, acc_frag<E>(tf[m], 1));
    }
    if (h == 1) {
#pragma unroll
        for (int c = ENC + ND_TW; c < 16 * KQ; ++c) put_half(st, r, c, 0u);
    }
    wave_sync_lds();
#pragma unroll
    for (int q = 0; q < KQ; ++q) f[q] = *reinterpret_cast<const nfa_v4u *>(st + r * ND_LD + 16 * q + 8 * h);
    wave_sync_lds();
}

// ReLU, one rounding: the accumulators of a 128-wide layer as the next product's B fragments
template <class E>
__device__ __forceinline__ void relu_frags(f32x16 (&acc)[ND_MT], nfa_v4u (&hf)[ND_KQ])
{
#pragma unroll
    for (int m = 0; m < ND_MT; ++m) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = acc[m][i] < 0.f ? 0.f : acc[m][i];
        hf[2 * m] = acc_frag<E>(acc[m], 0);
        hf[2 * m + 1] = acc_frag<E>(acc[m], 1);
    }
}

// a 128-wide layer on KQ fragments: four pieces of the ring
template <class E, int KQ, class Ring>
__device__ __forceinline__ void ndr_layer(Ring &ring, const float *b, const nfa_v4u (&in)[KQ], f32x16 (&acc)[ND_MT], int lane, int h)
{
#pragma unroll
    for (int m = 0; m < ND_MT; ++m) {
        ring.fetch();
        const nfa_v4u *A = ring.piece();
        init_acc(acc[m], true, b + 32 * m, h);
#pragma unroll
        for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], in[q], acc[m]);
        ring.hand_over();
    }
}

// a one-tile output layer: rows 0 .. N - 1 of the tile, registers 0 .. N - 1 of lane half 0, on both lane halves
template <class E, int N, class Ring>
__device__ __forceinline__ void ndr_output(Ring &ring, const float *b, const nfa_v4u (&hf)[ND_KQ], float (&out)[N], int lane, int h)
{
    f32x16 o;
    ring.fetch();
    {
        const nfa_v4u *A = ring.piece();
        init_acc(o, true, b, h);
#pragma unroll
        for (int q = 0; q < ND_KQ; ++q) o = mfma<E>(A[q * 64 + lane], hf[q], o);
    }
    ring.hand_over();
    const int other = (lane ^ 32) << 2;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float got = __int_as_float(__builtin_amdgcn_ds_bpermute(other, __float_as_int(o[k])));
        out[k] = h ? got : o[k];
    }
}

template <class E, class Ring>
__device__ __forceinline__ void time_layer(Ring &ring, const float *b, const nfa_v4u &te, f32x16 (&tf)[ND_TMT], int lane, int h)
{
#pragma unroll
    for (int m = 0; m < ND_TMT; ++m) {
        ring.fetch();
        tf[m] = time_tile<E>(ring.piece(), b + 32 * m, te, lane, h);
        ring.hand_over();
    }
}

// x <- warp(x, t) for the wave's 32 points, on both lane halves: the ring's next ND_PIECES pieces, wb the staged biases, st the
// wave's cat tile.  Every wave of the workgroup calls it in every pass.
template <class E, class Ring>
__device__ __forceinline__ void ndr_stage(Ring &ring, const float *wb, uint16_t *st, float (&x)[3], float t, int lane_)
{
    int lane = lane_;   // as warp_stage: nothing of the stage is hoisted out of the pass loop
    asm volatile("" : "+v"(lane));
    const int r = lane & 31, h = lane >> 5;
    const nfa_v4u te = time_frag<E>(t, lane, h);
#pragma unroll 1
    for (int b = 0; b < ND_BLOCKS; ++b) {
        const float *bb = wb + b * ND_BLOCK_BIAS;
        f32x16 tf[ND_TMT], acc[ND_MT];
        nfa_v4u hf[ND_KQ];
        {   // w += net 1
            time_layer<E>(ring, bb + ND_B_T1, te, tf, lane, h);
            nfa_v4u xf[ND_KQ1];
            cat_frags<E, 2, ND_KQ1>(st, x, tf, lane, r, h, xf);
            ndr_layer<E, ND_KQ1>(ring, bb + ND_B_N1, xf, acc, lane, h);
            relu_frags<E>(acc, hf);
            ndr_layer<E, ND_KQ>(ring, bb + ND_B_N1 + ND_W, hf, acc, lane, h);
            relu_frags<E>(acc, hf);
            float dw[1];
            ndr_output<E, 1>(ring, bb + ND_B_N1 + 2 * ND_W, hf, dw, lane, h);
            x[2] = x[2] + dw[0];
        }
        {   // (u, v) <- R(theta)^-1 ((u, v) - tr), from net 2
            time_layer<E>(ring, bb + ND_B_T2, te, tf, lane, h);
            nfa_v4u xf[ND_KQ2];
            cat_frags<E, 1, ND_KQ2>(st, x + 2, tf, lane, r, h, xf);
            ndr_layer<E, ND_KQ2>(ring, bb + ND_B_N2, xf, acc, lane, h);
            relu_frags<E>(acc, hf);
            float rt[3];
            ndr_output<E, 3>(ring, bb + ND_B_N2 + ND_W, hf, rt, lane, h);
            float s, c;
            sincosf(rt[0], &s, &c);
            const float du = x[0] - rt[1], dv = x[1] - rt[2];
            const float cu = c * du, sv = s * dv, su = s * du, cv = c * dv;
            x[0] = cu + sv;
            x[1] = cv - su;
        }
        const float u = x[0], v = x[1], w = x[2];
        if (b == 0) x[0] = v, x[1] = w, x[2] = u;        // [1, 2, 0]
        else if (b == 1) x[0] = w, x[1] = u, x[2] = v;   // [2, 0, 1]
    }
}

}  // namespace
}  // namespace nfa

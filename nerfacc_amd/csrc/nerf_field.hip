// nerf_field.hip -- the no-grad query of the reference's vanilla NeRF field as ONE launch: both sinusoidal encoders, the trunk,
// the colour head and the output activations (ref: examples/radiance_fields/mlp.py, VanillaNeRFRadianceField over NerfMLP).
// Nothing is saved for a backward, except by the training forward below.  The composed chain (SinusoidalEncoding twice,
// StreamedMLP, split, cat, StreamedMLP, activations) moves about 1.9 KB per point through memory at the reference's shape; this
// pass reads 24 B (a position and a direction, or 16 B of a ray sample) and writes 4 to 16 B.
//
// Work split, image format, arithmetic and rounding points are mlp_stream.hip's: a persistent grid, 4 waves x one 32-point
// tile, 128 points per pass of the images (NFA_MLP_STREAM_POINTS), the weights as the A operand of v_mfma_f32_32x32x16, one
// piece (a row tile of a layer, all its k-steps) per step through a ring of two LDS slots, one workgroup barrier per piece.
// A point is a column of every tile and stays on lane (point & 31) of both lane halves.  EXEC is all ones around every MFMA
// and every cross-lane read: a partial tile clamps the point index of its loads and masks only its stores, and every wave
// runs every step of every pass of its workgroup, so every wave reaches every barrier.
//
//   piece table   the trunk's pieces in layer order, then the head's: 73 + 5 entries at the reference's shape (63 -> 8 x 256 ->
//                 257, then 283 -> 128 -> 3), the largest piece 20 KiB (the trunk's cat layer).  It repeats every pass, so the
//                 head's last piece prefetches the trunk's first.  nfa_nerf_density leaves out the head and the W / 32 row
//                 tiles of the trunk's output layer that hold only the bottleneck: one output tile instead of nine.
//   position      the 63-wide encoded row never exists in memory.  Lane (r, h) holds for k-step q the eight halves 16 q + 8 h
//                 .. + 7 of point r's row (x, the sine block, the cosine block: SinusoidalEncoding's order; column 63 is zero)
//                 in four B fragments, formed once per pass before layer 0's first fetch and held across all row tiles of
//                 layer 0 and of every cat layer.  Values: the same sincosf(x * 2^k) as sinenc.hip, rounded once to the half
//                 type, so the fragments are the bits SinusoidalEncoding(out_dtype=elem) stores.  A point's thirty sincosf
//                 are split between its two lanes (lane half h takes frequencies 5 h .. 5 h + 4) and each packed (sin, cos)
//                 pair crosses the lane halves with one ds_bpermute: 15 evaluations and 15 exchanges per lane instead of the
//                 18 or 19 evaluations a lane would need for its own columns alone.
//   bottleneck    the merged output matrix of the trunk has rows 0 .. W-1 for the bottleneck and row W for sigma.  The
//                 bottleneck's accumulator tiles are rounded once with acc_frag, without an activation, and ARE the first W / 16
//                 B fragments of the head's layer 0; sigma is register 0 of lane half 0 of the last tile, in float32.
//   head layer 0  K = W + 27: k-steps 0 .. W/16-1 consume the bottleneck in acc_frag's permuted k order, the last two the
//                 encoded direction (27 columns padded to 32) in natural order, two fragments formed like the position's
//                 from the per-sample or per-ray direction.  That is a cat layer's image with an H part wider than the
//                 head's own 128 neurons, which nerf_head_pack_kernel writes (Shape has one width); every other layer is
//                 packed as mlp_pack_kernel packs it.  The 283-wide row and its element loads do not exist.
//   outputs       rows 0 .. 2 of the head's output tile are registers 0 .. 2 of lane half 0: a lane stores its point's sigma
//                 and its three colours itself (12 contiguous bytes per lane), so there is no store staging.
//
// Rounding points are the composed chain's: the encoded rows once, every hidden activation after its ReLU, the bottleneck
// once.  Raw sigma and raw colour leave as the float32 accumulators, or rounded once when the output is the half type.  The
// activated outputs are float32 functions of the raw values ROUNDED to the half type, as the composed chain applies them to
// NerfMLP's half outputs: relu, and 1 / (1 + expf(-c)).  The trunk sees the composed chain's operands in its order, so sigma
// has its bits; the head's layer 0 sums its k-steps in another order than load_row8's natural one (bottleneck permuted,
// direction behind it), so the raw colour may differ in the last bit of a float32 sum.
//
// Training forward (the SAVE instantiations, nfa_nerf_train_fwd): the same pass, the same accumulators and outputs, which also
// stores what nerf_train.hip's backward and nfa_mlp_stream_bwd_weights read.  The rows exist only as operand fragments:
//   hidden        [D, N, W] and [Dh, N, 128]: a lane's fragments of a row tile are 8-byte pieces of its point's row, and the two
//                 lane halves' pieces alternate, so store_tile_row writes whole 64-byte runs (mlp_stream.hip's store).
//   63 and W + 27 the encoded position rows and the head's input rows (bottleneck rounded once, then the encoded direction) are
//                 no 16-byte rows, but a wave's 32 of them are one contiguous 16-byte aligned span: the lanes drop their
//                 fragments' halves into the wave's LDS tile (row-major, 2-byte LDS writes), and the wave copies the tile out
//                 as 16-byte pieces, 1 KiB per store instruction (nerf_field.h).  No row leaves as per-lane element stores.
//   budget, W = 256   LDS: 2 x 20 KiB ring, 1.25 KiB table, 9.75 KiB biases, 4 x 17.7 KiB staging = 121.75 KiB of 160 (one
//                 workgroup per CU, as the registers allow anyway).  Registers: 256 + 190 (the plain full query: 256 + 155), no
//                 scratch ("Fused NeRF field: training").  Per point it writes 126 + 566 B of rows and 512 D + 256 Dh B
//                 of activations.
//
// The WARP instantiations are the reference's T-NeRF field (ref: examples/radiance_fields/mlp.py, TNeRFRadianceField): in front
// of the pass above a wave moves its points by the warp network, x' = x + warp([enc(x), enc(t)]), and x' takes x's place.
//   warp weights  FusedMLP's packed forward image of (36 -> n_hidden x 64 -> 3), unchanged, RESIDENT in LDS behind the ring, the
//                 table and the biases, with its float32 biases next to it: copied once per workgroup, read by every pass.  The
//                 warp stage has no ring traffic and no barrier; a wave runs it at its own pace while the trunk's first piece,
//                 prefetched by the previous pass's last hand_over, waits in its slot.
//   warp input    the 36-wide row (x, 12 sines, 12 cosines, t, 4 sines, 4 cosines; zeros up to 48) never exists in memory: three
//                 B fragments in natural k order, the bits SinusoidalEncoding (3, 0, 4) and (1, 0, 4) store and torch.cat
//                 joins.  The 12 + 4 sincosf of a point are split between its two lanes (lane half h takes frequencies 2 h and
//                 2 h + 1 of both encoders) and exchanged: 8 evaluations and 8 exchanges per lane.
//   chain         mlp.hip's: two row tiles per hidden layer, biases the values the accumulators start from, acc_frag between
//                 layers, a cat layer's three k-steps on the held input fragments BEHIND its four H k-steps, one output tile.
//                 Every accumulator sees FusedMLP's operands in FusedMLP's order, so the deformation has its bits.
//   hand-off      the deformation is registers 0 .. 2 of lane half 0 of the output tile, float32, never rounded; lane half 1
//                 reads it from the lane 32 away; x' = x + deformation in float32 on both halves.  Lane half 0 stores x' if
//                 `warped` is asked for (12 contiguous bytes per lane).  nfa_tnerf_warp is this stage alone (tnerf_warp_kernel).
//
// T-NeRF training forward (WARP with SAVE, nfa_tnerf_train_fwd): both of the above in one instantiation, the same accumulators, so
// rgb, sigma and warped are nfa_tnerf_field's bits and the four buffers are what nfa_nerf_train_fwd stores at x'.  The warp stage
// also stores its input rows [N, 36] (through the wave's staging tile) and its activations [D_w, N, 64] (store_tile_row); x' is
// `warped`.  The plain training forward's LDS and the resident warp image do not fit together (121.75 + 41.1 KiB), so here the
// head's input rows leave as TWO spans of 16 rows (16 (W + 27) halves are a multiple of 16 bytes): lanes r < 16 stage and the wave
// flushes, then lanes r >= 16.  The staging halves (4 x 8.8 KiB at W = 256; 127.5 KiB in all), no arithmetic changes, and the
// bottleneck fragments are held until the head's layer 0 anyway ("Fused T-NeRF field: training").
//
// The NDR instantiations (WARP == 2) are the reference's NDRTNeRFRadianceField: the invertible warp of ndr_warp.h in front of the
// same pass.  Its 54 pieces stand in front of the trunk's in the piece table and come from an image of their own (FieldRing's PRE),
// so the head's last piece prefetches the warp's first; its biases and the four waves' cat tiles lie behind the head's biases.
// Budget of the full query at W = 256: 81.75 KiB of LDS (ndr_warp.h), 256 + 174 registers, no scratch (density: 217 + 128; W = 128:
// 204 + 64 and 149 + 64); nfa_ndr_warp, the stage alone (ndr_warp_kernel: the same ring over the warp's pieces only), 47.2 KiB,
// 126 + 64 registers, no scratch (-Rpass-analysis=kernel-resource-usage).
#include "ndr_warp.h"
#include "samples.h"

namespace nfa {
namespace {

// The order in which a pass consumes the pieces: the trunk's (n_trunk of them), then the head's.  Returns their number.
__host__ __device__ inline int nerf_pieces(const Shape &T, const Shape &H, bool full, Piece *tab, int *max_n16, int *n_trunk)
{
    int n = 0, mx = 0;
    auto put = [&](int64_t off16, int n16) {
        if (tab) tab[n] = Piece{(int32_t)off16, n16};
        mx = n16 > mx ? n16 : mx;
        ++n;
    };
    const int D = T.n_hidden, MT = T.W / 32;
    for (int l = 0; l < D; ++l)
        for (int m = 0; m < MT; ++m) put(T.fwd_off(l) / 8 + (int64_t)m * T.fwd_kq(l) * 64, T.fwd_kq(l) * 64);
    for (int m = full ? 0 : MT; m <= MT; ++m) put(T.fwd_off(D) / 8 + (int64_t)m * T.fwd_kq(D) * 64, T.fwd_kq(D) * 64);
    if (n_trunk) *n_trunk = n;
    for (int l = 0; full && l <= H.n_hidden; ++l)
        for (int m = 0; m < H.fwd_mt(l); ++m) put(H.fwd_off(l) / 8 + (int64_t)m * H.fwd_kq(l) * 64, H.fwd_kq(l) * 64);
    if (max_n16) *max_n16 = mx;
    return n;
}

// floats of a network's biases in LDS: layer l at l W, the output layer padded to whole row tiles with zeros
__host__ __device__ inline int trunk_bias_floats(const Shape &T) { return T.n_hidden * T.W + T.W + 32; }
__host__ __device__ inline int head_bias_floats(const Shape &H) { return H.n_hidden * NF_HEAD_W + 32; }

__host__ __device__ inline int64_t nerf_lds_bytes(int slot16, int bias_floats)
{
    return (int64_t)NF_SLOTS * slot16 * 16 + (int64_t)NF_MAX_PIECES * sizeof(Piece) + (int64_t)bias_floats * 4;
}

struct NerfArgs {
    Shape T, H;
    const uint16_t *timg, *himg;
    const float *tbias, *hbias;
    int32_t slot16, n_pieces;
    const float *x, *dirs;                    // the position form
    const float *o, *d, *ts, *te;             // the ray-sample form
    const int64_t *ri;
    int64_t n_rays, N;
    void *sigma, *rgb;
    int32_t sigma_f32, rgb_f32, activated;
    uint16_t *sv_x, *sv_th, *sv_hx, *sv_hh;   // SAVE: the training forward's four buffers (header: training forward)
};

// what a WARP instantiation takes beside them
struct WarpArgs {
    Shape S;
    const uint16_t *img;
    const float *bias;
    const float *times;   // [N] in the position form, [n_rays] in the ray-sample form
    float *warped;        // [N, 3], optional
    int32_t img16;        // the image in 16-byte fragments
};
struct TNerfArgs : NerfArgs { WarpArgs w; };
// WARP with SAVE (nfa_tnerf_train_fwd): the warp's input rows [N, 36] and hidden activations [D_w, N, 64]; x' is w.warped
struct TNerfTrainArgs : TNerfArgs { uint16_t *sv_win, *sv_wh; };
struct NdrArgs : NerfArgs { NdrWarp n; };
// what the warp stage of that instantiation stores, and the wave's staging tile
struct WarpSave { uint16_t *in, *hidden, *st; int64_t N, p; };

// ---------------------------------------------------------------- the encoders in registers

// The packed (sin, cos) pairs of all 3 L items (k, d), item 3 k + d, of the lane's point on every lane: lane half h evaluates
// the items of frequencies (L / 2) h .. (L / 2) h + L / 2 - 1 and reads the other half's from the lane 32 away.
template <class E, int L>
__device__ __forceinline__ void sin_items(const float (&x)[3], int lane, int h, uint32_t (&it)[3 * L])
{
    static_assert(L % 2 == 0, "the frequencies are split between the lane halves");
    constexpr int HALF = 3 * L / 2;
    const int other = (lane ^ 32) << 2;
#pragma unroll
    for (int t = 0; t < HALF; ++t) {
        const float sc = h ? (float)(1 << (t / 3 + L / 2)) : (float)(1 << (t / 3));   // ldexpf(1, k): x * sc is exact
        float s, c;
        sincosf(x[t % 3] * sc, &s, &c);
        const uint32_t own = pack_halves<E>(s, c);
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(other, (int)own);
        it[t] = h ? got : own;
        it[HALF + t] = h ? own : got;
    }
}

// column c (a constant once the loops are unrolled) of the encoded row: x, the sine block, the cosine block, zeros
template <int L>
__device__ __forceinline__ uint32_t enc_col(const uint32_t (&xb)[3], const uint32_t (&it)[3 * L], int c)
{
    if (c < 3) return xb[c];
    if (c < 3 + 3 * L) return it[c - 3] & 0xFFFFu;
    if (c < 3 + 6 * L) return it[c - 3 - 3 * L] >> 16;
    return 0u;
}

// The NQ B fragments of the encoded row of x: fragment q on lane half h is columns 16 q + 8 h .. + 7
template <class E, int L, int NQ>
__device__ __forceinline__ void enc_frags(const float (&x)[3], int lane, int h, nfa_v4u (&f)[NQ])
{
    static_assert(3 + 6 * L <= 16 * NQ, "the row fits the fragments");
    uint32_t it[3 * L], xb[3];
    sin_items<E, L>(x, lane, h, it);
#pragma unroll
    for (int k = 0; k < 3; ++k) xb[k] = half_bits<E>(x[k]);   // the identity columns: x rounded as the encoder stores it
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t lo = enc_col<L>(xb, it, 16 * q + 2 * d) | (enc_col<L>(xb, it, 16 * q + 2 * d + 1) << 16);
            const uint32_t hi = enc_col<L>(xb, it, 16 * q + 8 + 2 * d) | (enc_col<L>(xb, it, 16 * q + 8 + 2 * d + 1) << 16);
            f[q][d] = h ? hi : lo;
        }
    }
}

// ---------------------------------------------------------------- the warp stage (WARP instantiations, tnerf_warp_kernel)

// The three B fragments of the warp network's input row [enc(x), enc(t)] in natural k order (header: warp input)
template <class E>
__device__ __forceinline__ void warp_frags(const float (&x)[3], float t, int lane, int h, nfa_v4u (&f)[NF_WARP_KQ0])
{
    constexpr int L = NF_WARP_L, XD = 3 + 6 * L;
    uint32_t it[3 * L], xb[3], tt[L];
    sin_items<E, L>(x, lane, h, it);
#pragma unroll
    for (int k = 0; k < 3; ++k) xb[k] = half_bits<E>(x[k]);
    const int other = (lane ^ 32) << 2;
#pragma unroll
    for (int j = 0; j < L / 2; ++j) {
        const float sc = h ? (float)(1 << (j + L / 2)) : (float)(1 << j);
        float s, c;
        sincosf(t * sc, &s, &c);
        const uint32_t own = pack_halves<E>(s, c);
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(other, (int)own);
        tt[j] = h ? got : own;
        tt[L / 2 + j] = h ? own : got;
    }
    const uint32_t tb = half_bits<E>(t);
    auto col = [&](int c) __attribute__((always_inline)) -> uint32_t {
        if (c < XD) return enc_col<L>(xb, it, c);
        if (c == XD) return tb;
        if (c < XD + 1 + L) return tt[c - XD - 1] & 0xFFFFu;
        if (c < XD + 1 + 2 * L) return tt[c - XD - 1 - L] >> 16;
        return 0u;
    };
#pragma unroll
    for (int q = 0; q < NF_WARP_KQ0; ++q) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t lo = col(16 * q + 2 * d) | (col(16 * q + 2 * d + 1) << 16);
            const uint32_t hi = col(16 * q + 8 + 2 * d) | (col(16 * q + 8 + 2 * d + 1) << 16);
            f[q][d] = h ? hi : lo;
        }
    }
}

// floats of the warp's biases in LDS: Shape::lds_bias_floats, layer l at 64 l, the output layer padded to a row tile
__device__ __forceinline__ void stage_warp(const WarpArgs &w, nfa_v4u *wimg, float *wb)
{
    const nfa_v4u *src = reinterpret_cast<const nfa_v4u *>(w.img);
    for (int i = threadIdx.x; i < w.img16; i += NF_THREADS) wimg[i] = src[i];
    const int n = w.S.lds_bias_floats();
    for (int i = threadIdx.x; i < n; i += NF_THREADS) wb[i] = i - w.S.n_hidden * NF_WARP_W < 3 ? w.bias[i] : 0.f;
}

// x <- x + warp([enc(x), enc(t)]) for the wave's 32 points, on both lane halves (header: chain, hand-off).  No barrier.
// SAVE: the input rows leave through the wave's staging tile, the activations as store_tile_row's 64-byte runs.
template <class E, bool SAVE = false>
__device__ __forceinline__ void warp_stage(const Shape &S, const nfa_v4u *wimg, const float *wb, float (&x)[3], float t, int lane_,
                                           const WarpSave *sv = nullptr)
{
    constexpr int W = NF_WARP_W, MT = W / 32, KQ = W / 16, KQ0 = NF_WARP_KQ0;
    // The stage's per-lane addresses and selects are formed from a lane index the compiler cannot see through: hoisted out of
    // the pass loop they would stay live across the trunk and the head, and W = 128 would lose its second wave per SIMD.
    int lane = lane_;
    asm volatile("" : "+v"(lane));
    const int h = lane >> 5;
    nfa_v4u xf[KQ0];
    warp_frags<E>(x, t, lane, h, xf);
    if constexpr (SAVE) {
        const int r = lane & 31;
#pragma unroll
        for (int q = 0; q < KQ0; ++q) stage_put8(sv->st, NF_WARP_DIMS, r, 16 * q + 8 * h, xf[q]);
        stage_flush(sv->st, sv->in, sv->p - r, tile_rows(sv->p - r, sv->N), NF_WARP_DIMS, lane);
    }
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        init_acc(acc[m], true, wb + 32 * m, h);
#pragma unroll
        for (int q = 0; q < KQ0; ++q) acc[m] = mfma<E>(wimg[(m * KQ0 + q) * 64 + lane], xf[q], acc[m]);
    }
    int off16 = MT * KQ0 * 64;
    nfa_v4u hf[KQ];
    for (int l = 1;; ++l) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][i] = acc[m][i] < 0.f ? 0.f : acc[m][i];
            hf[2 * m] = acc_frag<E>(acc[m], 0);
            hf[2 * m + 1] = acc_frag<E>(acc[m], 1);
            if constexpr (SAVE)
                if (sv->p < sv->N) store_tile_row<W>(sv->hidden + (int64_t)(l - 1) * sv->N * W, sv->p, m, h, hf[2 * m], hf[2 * m + 1]);
        }
        if (l == S.n_hidden) break;
        const bool cat = S.cat(l);
        const int kql = KQ + (cat ? KQ0 : 0);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const nfa_v4u *A = wimg + off16 + m * kql * 64 + lane;
            init_acc(acc[m], true, wb + l * W + 32 * m, h);
#pragma unroll
            for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(A[q * 64], hf[q], acc[m]);
            if (cat) {
#pragma unroll
                for (int q = 0; q < KQ0; ++q) acc[m] = mfma<E>(A[(KQ + q) * 64], xf[q], acc[m]);
            }
        }
        off16 += MT * kql * 64;
    }
    f32x16 o;
    init_acc(o, true, wb + S.n_hidden * W, h);
    const nfa_v4u *A = wimg + off16 + lane;
#pragma unroll
    for (int q = 0; q < KQ; ++q) o = mfma<E>(A[q * 64], hf[q], o);
    if (S.cat(S.n_hidden)) {
#pragma unroll
        for (int q = 0; q < KQ0; ++q) o = mfma<E>(A[(KQ + q) * 64], xf[q], o);
    }
    const int other = (lane ^ 32) << 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // rows 0 .. 2 of the tile: registers 0 .. 2 of lane half 0
        const float got = __int_as_float(__builtin_amdgcn_ds_bpermute(other, __float_as_int(o[k])));
        x[k] = x[k] + (h ? got : o[k]);
    }
}

// the point of a lane and its time (and, FULL, its direction) in either input form
template <bool RAYS, bool DIRS, class A>
__device__ __forceinline__ void load_point(const A &a, const float *times, int64_t pc, float (&x)[3], float (&dir)[3], float &t)
{
    if constexpr (RAYS) {
        float ro[3];
        const int64_t ray = a.ri[pc];
        ray_rows(a.o, a.d, ray, a.n_rays, ro, dir);
        sample_point(ro, dir, a.ts[pc], a.te[pc], x);
        if (times) {
            const bool ok = (uint64_t)ray < (uint64_t)a.n_rays;
            const float v = times[ok ? ray : 0];
            t = ok ? v : __builtin_nanf("");
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = a.x[3 * pc + k];
            if constexpr (DIRS) dir[k] = a.dirs[3 * pc + k];
        }
        if (times) t = times[pc];
    }
}

// an output value: raw (the accumulator, rounded once if the output is the half type) or activated (header)
template <class E>
__device__ __forceinline__ void put_out(void *out, bool out_f32, int64_t i, float v, bool activated, bool colour)
{
    if (activated) {
        v = half_value<E>(half_bits<E>(v));
        v = colour ? 1.0f / (1.0f + expf(-v)) : (v < 0.f ? 0.f : v);
    }
    if (out_f32) static_cast<float *>(out)[i] = v;
    else static_cast<uint16_t *>(out)[i] = (uint16_t)half_bits<E>(v);
}

// ---------------------------------------------------------------- the query

// W: the trunk's width.  RAYS: the ray-sample input form.  FULL: sigma and colour; otherwise the pass ends with sigma's tile.
// WARP: the T-NeRF field, the warp stage in front of every pass; the instantiations without it never see WarpArgs.
// A W = 128 WARP instantiation asks for the two waves per SIMD its plain twin has by itself (1: no request).
// SAVE: nfa_nerf_train_fwd, the full query that also stores what the backward reads; the arithmetic is untouched.
// WARP with SAVE: nfa_tnerf_train_fwd (header: T-NeRF training forward); one workgroup per CU by its LDS, so no request either.
// WARP == 2: the NDR field, ndr_warp.h's stage in front of every pass (never with SAVE).
template <class E, int W, bool RAYS, bool FULL, int WARP = 0, bool SAVE = false>
__global__ __launch_bounds__(NF_THREADS) __attribute__((amdgpu_waves_per_eu(WARP == 1 && !SAVE && W == 128 ? 2 : 1))) void nerf_field_kernel(
    const std::conditional_t<WARP == 2, NdrArgs, std::conditional_t<WARP == 1, std::conditional_t<SAVE, TNerfTrainArgs, TNerfArgs>, NerfArgs>> a)
{
    static_assert(WARP != 2 || !SAVE, "the NDR field has no training forward");
    constexpr int MT = W / 32, KQ = W / 16, KQX = (NF_POS_DIMS + 15) / 16, KQD = (NF_DIR_DIMS + 15) / 16;
    constexpr int HW = NF_HEAD_W, HMT = HW / 32, HKQ = HW / 16;
    constexpr int MAXV = ((KQ + KQX) * 64 + NF_THREADS - 1) / NF_THREADS;   // the trunk's cat layer, the largest piece
    static_assert(KQ + KQD <= KQ + KQX && HKQ <= KQ, "no piece of the head is larger");
    static_assert(!SAVE || FULL, "the training forward is a full query");
    constexpr int HX = W + NF_DIR_DIMS;   // the head's input row
    constexpr int ST_BYTES = WARP ? 16 * HX * 2 : row_stage_bytes(HX);   // WARP: the head's input rows leave as two spans of 16
    static_assert(ST_BYTES % 16 == 0 && ST_BYTES >= row_stage_bytes(NF_POS_DIMS) && ST_BYTES >= row_stage_bytes(NF_WARP_DIMS), "every staged tile fits");
    extern __shared__ __attribute__((aligned(16))) unsigned char nf_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const Shape &T = a.T, &H = a.H;
    const int D = T.n_hidden, Dc = H.n_hidden;
    Piece *tab = reinterpret_cast<Piece *>(nf_lds + (int64_t)NF_SLOTS * a.slot16 * 16);
    // the biases, staged once behind the table (read from global memory they would queue behind the fetch of the next piece)
    float *tb = reinterpret_cast<float *>(tab + NF_MAX_PIECES);
    const int n_tb = trunk_bias_floats(T), n_hb = FULL ? head_bias_floats(H) : 0;
    float *hb = tb + n_tb;
    for (int i = threadIdx.x; i < n_tb; i += NF_THREADS) tb[i] = i - D * W < W + 1 ? a.tbias[i] : 0.f;
    for (int i = threadIdx.x; i < n_hb; i += NF_THREADS) hb[i] = i - Dc * HW < 3 ? a.hbias[i] : 0.f;
    nfa_v4u *wimg = reinterpret_cast<nfa_v4u *>(hb + n_hb);   // WARP: the resident image, 16-byte aligned (every part before it is)
    uint16_t *st = reinterpret_cast<uint16_t *>(hb + n_hb) + wave * (ST_BYTES / 2);   // SAVE: the wave's staging tile, there instead
    float *wb = nullptr;
    if constexpr (WARP == 1) {
        wb = reinterpret_cast<float *>(wimg + a.w.img16);
        stage_warp(a.w, wimg, wb);   // ring.start()'s barriers publish it
        if constexpr (SAVE) st = reinterpret_cast<uint16_t *>(wb + a.w.S.lds_bias_floats()) + wave * (ST_BYTES / 2);   // behind both
    }
    constexpr int N_PRE = WARP == 2 ? ND_PIECES : 0;
    if constexpr (WARP == 2) {   // the warp's biases (padded by the packer), then the waves' cat tiles
        wb = hb + n_hb;
        for (int i = threadIdx.x; i < ND_BIAS_FLOATS; i += NF_THREADS) wb[i] = a.n.bias[i];
        st = reinterpret_cast<uint16_t *>(wb + ND_BIAS_FLOATS) + wave * (ND_STAGE_BYTES / 2);
    }
    FieldRing<MAXV, WARP == 2> ring;
    if (threadIdx.x == 0) {
        if constexpr (WARP == 2) ndr_pieces(tab);
        nerf_pieces(T, H, FULL, tab + N_PRE, nullptr, nullptr);
    }
    if constexpr (WARP == 2) ring.pre = reinterpret_cast<const nfa_v4u *>(a.n.img), ring.n_pre = N_PRE;
    ring.img0 = reinterpret_cast<const nfa_v4u *>(a.timg);
    ring.img1 = reinterpret_cast<const nfa_v4u *>(a.himg);
    ring.slots = reinterpret_cast<nfa_v4u *>(nf_lds);
    ring.tab = tab;
    ring.slot16 = a.slot16;
    ring.n0 = N_PRE + D * MT + (FULL ? MT + 1 : 1);
    ring.n_pieces = a.n_pieces;
    ring.start();
    const int64_t N = a.N, n_pass = ceil_div64(N, NF_POINTS);
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int64_t p = (pass * NF_WAVES + wave) * 32 + r, pc = p < N ? p : N - 1;
        // ---- the point and both encoded rows, before layer 0's first fetch
        float x[3], dir[3] = {0.f, 0.f, 0.f}, t = 0.f;
        if constexpr (WARP == 2) {
            load_point<RAYS, FULL>(a, a.n.times, pc, x, dir, t);
            ndr_stage<E>(ring, wb, st, x, t, lane);
            if (a.n.warped && h == 0 && p < N) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.n.warped[3 * p + k] = x[k];
            }
        } else if constexpr (WARP == 1) {
            load_point<RAYS, FULL>(a, a.w.times, pc, x, dir, t);
            if constexpr (SAVE) {
                const WarpSave sv = {a.sv_win, a.sv_wh, st, N, p};
                warp_stage<E, true>(a.w.S, wimg, wb, x, t, lane, &sv);
            } else {
                warp_stage<E>(a.w.S, wimg, wb, x, t, lane);
            }
            if (a.w.warped && h == 0 && p < N) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.w.warped[3 * p + k] = x[k];
            }
        } else {
            load_point<RAYS, FULL>(a, nullptr, pc, x, dir, t);
        }
        nfa_v4u xf[KQX], df[KQD];
        enc_frags<E, NF_POS_L, KQX>(x, lane, h, xf);
        if constexpr (FULL) enc_frags<E, NF_DIR_L, KQD>(dir, lane, h, df);
        const int64_t row0 = p - r;
        if constexpr (SAVE) {   // the encoded position rows [N, 63]
#pragma unroll
            for (int q = 0; q < KQX; ++q) stage_put8(st, NF_POS_DIMS, r, 16 * q + 8 * h, xf[q]);
            stage_flush(st, a.sv_x, row0, tile_rows(row0, N), NF_POS_DIMS, lane);
        }
        // ---- the trunk
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            ring.fetch();
            const nfa_v4u *A = ring.piece();
            init_acc(acc[m], true, tb + 32 * m, h);
#pragma unroll
            for (int q = 0; q < KQX; ++q) acc[m] = mfma<E>(A[q * 64 + lane], xf[q], acc[m]);
            ring.hand_over();
        }
        nfa_v4u hf[KQ];
        for (int l = 1;; ++l) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {   // H_{l-1} = relu(acc) rounded: the next product's B fragments
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[m][i] = acc[m][i] < 0.f ? 0.f : acc[m][i];
                hf[2 * m] = acc_frag<E>(acc[m], 0);
                hf[2 * m + 1] = acc_frag<E>(acc[m], 1);
                if constexpr (SAVE)
                    if (p < N) store_tile_row<W>(a.sv_th + (int64_t)(l - 1) * N * W, p, m, h, hf[2 * m], hf[2 * m + 1]);
            }
            if (l == D) break;
            const bool cat = T.cat(l);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                ring.fetch();
                const nfa_v4u *A = ring.piece();
                init_acc(acc[m], true, tb + l * W + 32 * m, h);
#pragma unroll
                for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], hf[q], acc[m]);
                if (cat) {
#pragma unroll
                    for (int q = 0; q < KQX; ++q) acc[m] = mfma<E>(A[(KQ + q) * 64 + lane], xf[q], acc[m]);
                }
                ring.hand_over();
            }
        }
        // the merged output layer: W / 32 bottleneck tiles (the full query), then the tile whose row 0 is sigma
        const bool cat_out = T.cat(D);
        nfa_v4u bf[FULL ? KQ : 1];
        f32x16 o;
#pragma unroll
        for (int m = FULL ? 0 : MT; m <= MT; ++m) {
            ring.fetch();
            const nfa_v4u *A = ring.piece();
            init_acc(o, true, tb + D * W + 32 * m, h);
#pragma unroll
            for (int q = 0; q < KQ; ++q) o = mfma<E>(A[q * 64 + lane], hf[q], o);
            if (cat_out) {
#pragma unroll
                for (int q = 0; q < KQX; ++q) o = mfma<E>(A[(KQ + q) * 64 + lane], xf[q], o);
            }
            ring.hand_over();
            if constexpr (FULL) {
                if (m < MT) {   // no activation: the bottleneck is a linear layer
                    bf[2 * m] = acc_frag<E>(o, 0);
                    bf[2 * m + 1] = acc_frag<E>(o, 1);
                    if constexpr (SAVE && !WARP) {
                        stage_put_acc_frag(st, HX, r, h, m, 0, bf[2 * m]);
                        stage_put_acc_frag(st, HX, r, h, m, 1, bf[2 * m + 1]);
                    }
                }
            }
        }
        if constexpr (SAVE && !WARP) {   // the head's input rows [N, W + 27]: the bottleneck staged above, then the encoded direction
#pragma unroll
            for (int q = 0; q < KQD; ++q) stage_put8(st, HX, r, W + 16 * q + 8 * h, df[q]);
            stage_flush(st, a.sv_hx, row0, tile_rows(row0, N), HX, lane);
        }
        if constexpr (SAVE && WARP) {   // the same rows as two spans of 16: half the staging (header: T-NeRF training forward)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if ((r >> 4) == s) {
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        stage_put_acc_frag(st, HX, r & 15, h, m, 0, bf[2 * m]);
                        stage_put_acc_frag(st, HX, r & 15, h, m, 1, bf[2 * m + 1]);
                    }
#pragma unroll
                    for (int q = 0; q < KQD; ++q) stage_put8(st, HX, r & 15, W + 16 * q + 8 * h, df[q]);
                }
                const int left = tile_rows(row0, N) - 16 * s;
                stage_flush(st, a.sv_hx, row0 + 16 * s, left < 0 ? 0 : (left < 16 ? left : 16), HX, lane);
            }
        }
        const bool live = h == 0 && p < N;
        if (live && a.sigma) put_out<E>(a.sigma, a.sigma_f32 != 0, p, o[0], a.activated != 0, false);
        if constexpr (FULL) {
            // ---- the head: layer 0 on [bottleneck, encoded direction], its hidden layers, its 3-row output tile
#pragma unroll
            for (int m = 0; m < HMT; ++m) {
                ring.fetch();
                const nfa_v4u *A = ring.piece();
                init_acc(acc[m], true, hb + 32 * m, h);
#pragma unroll
                for (int q = 0; q < KQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], bf[q], acc[m]);
#pragma unroll
                for (int q = 0; q < KQD; ++q) acc[m] = mfma<E>(A[(KQ + q) * 64 + lane], df[q], acc[m]);
                ring.hand_over();
            }
            nfa_v4u hc[HKQ];
            for (int l = 1;; ++l) {
#pragma unroll
                for (int m = 0; m < HMT; ++m) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[m][i] = acc[m][i] < 0.f ? 0.f : acc[m][i];
                    hc[2 * m] = acc_frag<E>(acc[m], 0);
                    hc[2 * m + 1] = acc_frag<E>(acc[m], 1);
                    if constexpr (SAVE)
                        if (p < N) store_tile_row<HW>(a.sv_hh + (int64_t)(l - 1) * N * HW, p, m, h, hc[2 * m], hc[2 * m + 1]);
                }
                if (l == Dc) break;
#pragma unroll
                for (int m = 0; m < HMT; ++m) {
                    ring.fetch();
                    const nfa_v4u *A = ring.piece();
                    init_acc(acc[m], true, hb + l * HW + 32 * m, h);
#pragma unroll
                    for (int q = 0; q < HKQ; ++q) acc[m] = mfma<E>(A[q * 64 + lane], hc[q], acc[m]);
                    ring.hand_over();
                }
            }
            ring.fetch();
            {
                const nfa_v4u *A = ring.piece();
                init_acc(o, true, hb + Dc * HW, h);
#pragma unroll
                for (int q = 0; q < HKQ; ++q) o = mfma<E>(A[q * 64 + lane], hc[q], o);
            }
            ring.hand_over();
            if (live && a.rgb) {   // rows 0 .. 2 of the tile: registers 0 .. 2 of lane half 0
#pragma unroll
                for (int i = 0; i < 3; ++i) put_out<E>(a.rgb, a.rgb_f32 != 0, 3 * p + i, o[i], a.activated != 0, true);
            }
        }
    }
}

// The warp stage alone (nfa_tnerf_warp): a wave per 32-point tile, the image resident as above, x' to memory.
template <class E, bool RAYS>
__global__ __launch_bounds__(NF_THREADS) void tnerf_warp_kernel(const TNerfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char nf_lds[];
    nfa_v4u *wimg = reinterpret_cast<nfa_v4u *>(nf_lds);
    float *wb = reinterpret_cast<float *>(wimg + a.w.img16);
    stage_warp(a.w, wimg, wb);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t N = a.N, n_tiles = ceil_div64(N, 32);
    for (int64_t tile = (int64_t)blockIdx.x * NF_WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * NF_WAVES) {
        const int64_t p = tile * 32 + r, pc = p < N ? p : N - 1;
        float x[3], dir[3], t = 0.f;
        load_point<RAYS, false>(a, a.w.times, pc, x, dir, t);
        warp_stage<E>(a.w.S, wimg, wb, x, t, lane);
        if (h == 0 && p < N) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.w.warped[3 * p + k] = x[k];
        }
    }
}

// The NDR warp alone (nfa_ndr_warp): the query's pass loop with the warp's pieces as the whole table.
__host__ __device__ inline int64_t ndr_warp_lds_bytes()
{
    return (int64_t)NF_SLOTS * ND_MAX_PIECE16 * 16 + (int64_t)ND_PIECES * sizeof(Piece) + ND_BIAS_FLOATS * 4 + NF_WAVES * ND_STAGE_BYTES;
}

template <class E, bool RAYS>
__global__ __launch_bounds__(NF_THREADS) void ndr_warp_kernel(const NdrArgs a)
{
    constexpr int MAXV = (ND_MAX_PIECE16 + NF_THREADS - 1) / NF_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char nf_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    Piece *tab = reinterpret_cast<Piece *>(nf_lds + (int64_t)NF_SLOTS * ND_MAX_PIECE16 * 16);
    float *wb = reinterpret_cast<float *>(tab + ND_PIECES);
    uint16_t *st = reinterpret_cast<uint16_t *>(wb + ND_BIAS_FLOATS) + wave * (ND_STAGE_BYTES / 2);
    for (int i = threadIdx.x; i < ND_BIAS_FLOATS; i += NF_THREADS) wb[i] = a.n.bias[i];
    if (threadIdx.x == 0) ndr_pieces(tab);
    FieldRing<MAXV> ring;
    ring.img0 = ring.img1 = reinterpret_cast<const nfa_v4u *>(a.n.img);
    ring.slots = reinterpret_cast<nfa_v4u *>(nf_lds);
    ring.tab = tab;
    ring.slot16 = ND_MAX_PIECE16;
    ring.n0 = ring.n_pieces = ND_PIECES;
    ring.start();
    const int64_t N = a.N, n_pass = ceil_div64(N, NF_POINTS);
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int64_t p = (pass * NF_WAVES + wave) * 32 + r, pc = p < N ? p : N - 1;
        float x[3], dir[3], t = 0.f;
        load_point<RAYS, false>(a, a.n.times, pc, x, dir, t);
        ndr_stage<E>(ring, wb, st, x, t, lane);
        if (h == 0 && p < N) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.n.warped[3 * p + k] = x[k];
        }
    }
}

// The six time layers of the NDR warp on t [n]: out [n, 6, 64], feature row 2 i + s is time_layers_{s+1}[i].  A wave per 32
// points, the twelve row tiles straight from the image (12 KiB, cached): time_tile is what the fused stage calls.
template <class E>
__global__ __launch_bounds__(NF_THREADS) void ndr_time_features_kernel(const nfa_v4u *__restrict__ img, const float *__restrict__ bias,
                                                                       const float *__restrict__ times, int64_t N, uint16_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t n_tiles = ceil_div64(N, 32);
    for (int64_t tile = (int64_t)blockIdx.x * NF_WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * NF_WAVES) {
        const int64_t p = tile * 32 + r, pc = p < N ? p : N - 1;
        const nfa_v4u te = time_frag<E>(times[pc], lane, h);
#pragma unroll 1
        for (int j = 0; j < 2 * ND_BLOCKS; ++j) {
#pragma unroll
            for (int m = 0; m < ND_TMT; ++m) {
                const f32x16 acc = time_tile<E>(img + (j * ND_TMT + m) * 64, bias + j * ND_TW + 32 * m, te, lane, h);
                if (p < N) store_tile_row<ND_TW>(out, p * (2 * ND_BLOCKS) + j, m, h, acc_frag<E>(acc, 0), acc_frag<E>(acc, 1));
            }
        }
    }
}

// The head's forward image: mlp_pack_kernel's image of (tw + 27 -> Dc x 128 -> 3), except that layer 0 is a cat layer whose H
// part is the trunk's tw bottleneck columns in the permuted k order and whose x part, the 27 direction columns, starts on a
// k-step of its own in natural order.  tw is a multiple of 16, so the sizes are those of the plain shape.
template <class E>
__global__ __launch_bounds__(256) void nerf_head_pack_kernel(Shape S, int tw, const float *__restrict__ params, uint16_t *__restrict__ img,
                                                             int64_t elems)
{
    const int L = S.layers();
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < elems; e += (int64_t)gridDim.x * 256) {
        int l = 0;
        int64_t off = 0;
        for (;; ++l) {
            const int64_t sz = (int64_t)S.fwd_mt(l) * S.fwd_kq(l) * 512;
            if (e < off + sz || l == L - 1) break;
            off += sz;
        }
        const int64_t local = e - off;
        const int j = (int)(local & 7), lane = (int)((local >> 3) & 63), hh = lane >> 5;
        const int64_t blk = local >> 9;
        const int KQ = S.fwd_kq(l), q = (int)(blk % KQ), m = (int)(blk / KQ), row = 32 * m + (lane & 31);
        const bool dir_part = l == 0 && q >= tw / 16;
        const int k = 16 * q + kpos(!dir_part, hh, j);
        const int in = S.in_dim(l), out = S.out_dim(l);
        float v = 0.f;
        if (row < out && k < in) v = params[S.master_off(l) + (int64_t)row * in + k];
        img[e] = (uint16_t)half_bits<E>(v);
    }
}

// ---------------------------------------------------------------- host side

// bytes of the resident warp image and its biases in LDS
int64_t warp_lds_bytes(const Shape &S) { return S.fwd_off(S.layers()) * 2 + (int64_t)S.lds_bias_floats() * 4; }

int check_warp_pointers(const char *who, const WarpArgs &w)
{
    NFA_REQUIRE(w.img && w.bias && w.times, "%s: null pointer (warp image, warp bias or times)", who);
    NFA_REQUIRE(aligned_to(w.img, 16) && aligned_to(w.bias, 4) && aligned_to(w.times, 4) && aligned_to(w.warped, 4),
                "%s: misaligned pointer (warp image 16, warp bias, times and warped 4)", who);
    return NFA_OK;
}

WarpArgs warp_args(const Shape &S, const void *image, const float *bias, const float *times, float *warped)
{
    WarpArgs w = {};
    w.S = S;
    w.img = static_cast<const uint16_t *>(image), w.bias = bias, w.times = times, w.warped = warped;
    w.img16 = (int32_t)(S.fwd_off(S.layers()) / 8);
    return w;
}

int check_ndr_pointers(const char *who, const NdrWarp &n);

int nerf_query(const char *who, bool full, int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *trunk_image,
               const void *head_image, const float *trunk_bias, const float *head_bias, const nfa_ngp_input *in, int64_t N,
               int32_t activated, void *sigma, int32_t sigma_elem, void *rgb, int32_t rgb_elem, nfa_stream_t stream,
               const WarpArgs *warp = nullptr,   // the T-NeRF entries: S checked, the pointers as the caller gave them
               bool train = false, const nfa_nerf_saved *save = nullptr,   // nfa_nerf_train_fwd
               const nfa_tnerf_saved *wsave = nullptr,                     // nfa_tnerf_train_fwd, next to warp and save
               const NdrWarp *ndr = nullptr)                                // the NDR entries: checked by check_ndr_warp
{
    Shape T, H = {};
    if (int rc = check_field_shape(who, elem, trunk, head, 0, N, &T, full ? &H : nullptr)) return rc;
    NFA_REQUIRE(in, "%s: the input descriptor is null", who);
    NFA_REQUIRE(!train || (save && (!warp || wsave)), "%s: the saved-buffers descriptor is null", who);
    NFA_REQUIRE(activated == 0 || activated == 1, "%s: activated must be 0 (raw outputs) or 1 (relu, sigmoid) (got %d)", who, activated);
    NFA_REQUIRE(sigma_elem == NFA_ELEM_F32 || sigma_elem == elem, "%s: sigma_elem %d: float32 or the networks' type (%d)", who, sigma_elem, elem);
    NFA_REQUIRE(!full || rgb_elem == NFA_ELEM_F32 || rgb_elem == elem, "%s: rgb_elem %d: float32 or the networks' type (%d)", who, rgb_elem, elem);
    if (N == 0) return NFA_OK;
    const bool rays = in->positions == nullptr;
    NFA_REQUIRE(!rays || (in->n_rays >= 1 && in->n_rays < ((int64_t)1 << 31) - 64), "%s: n_rays %lld out of range", who, (long long)in->n_rays);
    NFA_REQUIRE(trunk_image && trunk_bias && (!full || (head_image && head_bias)), "%s: null pointer (image or bias)", who);
    NFA_REQUIRE(rays ? (in->rays_o && in->rays_d && in->t_starts && in->t_ends && in->ray_indices) : (!full || in->dirs),
                "%s: null input pointer (positions with dirs, or rays_o, rays_d, t_starts, t_ends and ray_indices)", who);
    NFA_REQUIRE(sigma || (full && rgb), "%s: no output requested", who);
    NFA_REQUIRE(aligned_to(trunk_image, 16) && aligned_to(head_image, 16) && aligned_to(trunk_bias, 4) && aligned_to(head_bias, 4) &&
                aligned_to(in->positions, 4) && aligned_to(in->dirs, 4) && aligned_to(in->rays_o, 4) && aligned_to(in->rays_d, 4) &&
                aligned_to(in->t_starts, 4) && aligned_to(in->t_ends, 4) && aligned_to(in->ray_indices, 8) &&
                aligned_to(sigma, sigma_elem == NFA_ELEM_F32 ? 4 : 2) && aligned_to(rgb, rgb_elem == NFA_ELEM_F32 ? 4 : 2),
                "%s: misaligned pointer (images 16, ray_indices 8, the others their element)", who);
    if (warp)
        if (int rc = check_warp_pointers(who, *warp)) return rc;
    if (ndr)
        if (int rc = check_ndr_pointers(who, *ndr)) return rc;
    NerfArgs a = {};
    if (train) {
        NFA_REQUIRE(save->enc_x && save->trunk_hidden && save->head_in && save->head_hidden,
                    "%s: null pointer (enc_x, trunk_hidden, head_in or head_hidden)", who);
        NFA_REQUIRE(!warp || (wsave->warp_in && wsave->warp_hidden && wsave->warped), "%s: null pointer (warp_in, warp_hidden or warped)", who);
        NFA_REQUIRE(aligned_to(save->enc_x, 16) && aligned_to(save->trunk_hidden, 16) && aligned_to(save->head_in, 16) &&
                    aligned_to(save->head_hidden, 16) && (!warp || (aligned_to(wsave->warp_in, 16) && aligned_to(wsave->warp_hidden, 16))),
                    "%s: misaligned pointer (the saved buffers 16)", who);
        a.sv_x = static_cast<uint16_t *>(save->enc_x), a.sv_th = static_cast<uint16_t *>(save->trunk_hidden);
        a.sv_hx = static_cast<uint16_t *>(save->head_in), a.sv_hh = static_cast<uint16_t *>(save->head_hidden);
    }
    a.T = T, a.H = H;
    a.timg = static_cast<const uint16_t *>(trunk_image), a.himg = static_cast<const uint16_t *>(head_image);
    a.tbias = trunk_bias, a.hbias = head_bias;
    int slot16 = 0;
    a.n_pieces = nerf_pieces(T, H, full, nullptr, &slot16, nullptr) + (ndr ? ND_PIECES : 0);
    a.slot16 = ndr && slot16 < ND_MAX_PIECE16 ? ND_MAX_PIECE16 : slot16;
    slot16 = a.slot16;
    a.x = in->positions, a.dirs = in->dirs;
    a.o = in->rays_o, a.d = in->rays_d, a.ts = in->t_starts, a.te = in->t_ends, a.ri = in->ray_indices;
    a.n_rays = in->n_rays, a.N = N;
    a.sigma = sigma, a.sigma_f32 = sigma_elem == NFA_ELEM_F32;
    a.rgb = full ? rgb : nullptr, a.rgb_f32 = rgb_elem == NFA_ELEM_F32;
    a.activated = activated;
    const int64_t lds = nerf_lds_bytes(slot16, trunk_bias_floats(T) + (full ? head_bias_floats(H) : 0)) + (warp ? warp_lds_bytes(warp->S) : 0) +
                        (train ? (int64_t)NF_WAVES * (warp ? 16 * (T.W + NF_DIR_DIMS) * 2 : row_stage_bytes(T.W + NF_DIR_DIMS)) : 0) +
                        (ndr ? (int64_t)ND_BIAS_FLOATS * 4 + NF_WAVES * ND_STAGE_BYTES : 0);
    const int64_t want = ceil_div64(N, NF_POINTS);
    const unsigned grid = (unsigned)(want < NFA_MLP_STREAM_GROUPS ? want : NFA_MLP_STREAM_GROUPS);
    int rc = NFA_OK;
    auto launch = [&](auto tag, auto w, auto rays_c, auto full_c, auto warp_c) {
        using E = typename decltype(tag)::type;
        constexpr bool WARP = decltype(warp_c)::value;
        if constexpr (decltype(full_c)::value) {
            if (train) {
                auto kern = nerf_field_kernel<E, decltype(w)::value, decltype(rays_c)::value, true, WARP, true>;
                if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
                if constexpr (WARP) {
                    TNerfTrainArgs ta = {};
                    static_cast<NerfArgs &>(ta) = a;
                    ta.w = *warp;
                    ta.sv_win = static_cast<uint16_t *>(wsave->warp_in), ta.sv_wh = static_cast<uint16_t *>(wsave->warp_hidden);
                    kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(ta);
                } else {
                    kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(a);
                }
                return;
            }
        }
        auto kern = nerf_field_kernel<E, decltype(w)::value, decltype(rays_c)::value, decltype(full_c)::value, WARP>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        if constexpr (WARP) {
            TNerfArgs ta = {};
            static_cast<NerfArgs &>(ta) = a;
            ta.w = *warp;
            kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(ta);
        } else {
            kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(a);
        }
    };
    auto launch_ndr = [&](auto tag, auto w, auto rays_c, auto full_c) {
        auto kern = nerf_field_kernel<typename decltype(tag)::type, decltype(w)::value, decltype(rays_c)::value, decltype(full_c)::value, 2>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        NdrArgs na = {};
        static_cast<NerfArgs &>(na) = a;
        na.n = *ndr;
        kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(na);
    };
    auto by_form = [&](auto tag, auto w) {
        dispatch_bool(rays, [&](auto rays_c) {
            dispatch_bool(full, [&](auto full_c) {
                if (ndr) launch_ndr(tag, w, rays_c, full_c);
                else dispatch_bool(warp != nullptr, [&](auto warp_c) { launch(tag, w, rays_c, full_c, warp_c); });
            });
        });
    };
    auto by_width = [&](auto tag) {
        if (T.W == 128) by_form(tag, std::integral_constant<int, 128>{});
        else by_form(tag, std::integral_constant<int, 256>{});
    };
    if (elem == NFA_ELEM_F16) by_width(ElemTag<nfa_f16>{});
    else by_width(ElemTag<nfa_bf16>{});
    if (rc != NFA_OK) return rc;
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

// The one statement of what the NDR entries take as the warp: checked after elem and before the trunk and the head.
int check_ndr_warp(const char *who, int32_t elem, const void *image, int64_t image_elems, const float *bias, int64_t bias_floats,
                   const float *times, float *warped, NdrWarp *n)
{
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the networks' type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    NFA_REQUIRE(image_elems == ND_IMAGE_ELEMS, "%s: the warp image holds %lld elements, got %lld", who, (long long)ND_IMAGE_ELEMS, (long long)image_elems);
    NFA_REQUIRE(bias_floats == ND_BIAS_FLOATS, "%s: the warp's bias block holds %d floats, got %lld", who, ND_BIAS_FLOATS, (long long)bias_floats);
    *n = NdrWarp{static_cast<const uint16_t *>(image), bias, times, warped};
    return NFA_OK;
}

// its pointers, checked with the other pointers: behind the return for n_points == 0, as in every other entry
int check_ndr_pointers(const char *who, const NdrWarp &n)
{
    NFA_REQUIRE(n.img && n.bias && n.times, "%s: null pointer (warp image, warp bias or times)", who);
    NFA_REQUIRE(aligned_to(n.img, 16) && aligned_to(n.bias, 4) && aligned_to(n.times, 4) && aligned_to(n.warped, 4),
                "%s: misaligned pointer (warp image 16, warp bias, times and warped 4)", who);
    return NFA_OK;
}

}  // namespace
}  // namespace nfa

using namespace nfa;

extern "C" {

int nfa_nerf_pack_head(int32_t elem, const nfa_mlp_desc *head, int32_t trunk_width, const float *params, void *head_image,
                       int64_t image_elems, nfa_stream_t stream)
{
    const char *who = "nfa_nerf_pack_head";
    Shape H;
    if (int rc = check_field_shape(who, elem, nullptr, head, trunk_width, 0, nullptr, &H)) return rc;
    const int64_t want = H.fwd_off(H.layers());
    NFA_REQUIRE(image_elems == want, "%s: the image holds %lld elements for this shape, got %lld", who, (long long)want, (long long)image_elems);
    NFA_REQUIRE(params && head_image, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(head_image, 16) && aligned_to(params, 4), "%s: misaligned pointer (image 16, params 4)", who);
    if (elem == NFA_ELEM_F16)
        nerf_head_pack_kernel<nfa_f16><<<grid_1d(want, 256), 256, 0, as_stream(stream)>>>(H, trunk_width, params, static_cast<uint16_t *>(head_image), want);
    else
        nerf_head_pack_kernel<nfa_bf16><<<grid_1d(want, 256), 256, 0, as_stream(stream)>>>(H, trunk_width, params, static_cast<uint16_t *>(head_image), want);
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int nfa_nerf_density(int32_t elem, const nfa_mlp_desc *trunk, const void *trunk_image, const float *trunk_bias, const nfa_ngp_input *in,
                     int64_t n_points, int32_t activated, void *sigma, int32_t sigma_elem, nfa_stream_t stream)
{
    return nerf_query("nfa_nerf_density", false, elem, trunk, nullptr, trunk_image, nullptr, trunk_bias, nullptr, in, n_points, activated, sigma,
                      sigma_elem, nullptr, NFA_ELEM_F32, stream);
}

int nfa_nerf_field(int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *trunk_image, const void *head_image,
                   const float *trunk_bias, const float *head_bias, const nfa_ngp_input *in, int64_t n_points, int32_t activated,
                   void *sigma, int32_t sigma_elem, void *rgb, int32_t rgb_elem, nfa_stream_t stream)
{
    return nerf_query("nfa_nerf_field", true, elem, trunk, head, trunk_image, head_image, trunk_bias, head_bias, in, n_points, activated, sigma,
                      sigma_elem, rgb, rgb_elem, stream);
}

int nfa_nerf_train_fwd(int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *trunk_image, const void *head_image,
                       const float *trunk_bias, const float *head_bias, const nfa_ngp_input *in, int64_t n_points, int32_t activated,
                       const nfa_nerf_saved *save, void *sigma, int32_t sigma_elem, void *rgb, int32_t rgb_elem, nfa_stream_t stream)
{
    return nerf_query("nfa_nerf_train_fwd", true, elem, trunk, head, trunk_image, head_image, trunk_bias, head_bias, in, n_points, activated,
                      sigma, sigma_elem, rgb, rgb_elem, stream, nullptr, true, save);
}

int nfa_tnerf_field(int32_t elem, const nfa_mlp_desc *warp, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *warp_image,
                    const void *trunk_image, const void *head_image, const float *warp_bias, const float *trunk_bias, const float *head_bias,
                    const nfa_ngp_input *in, const float *times, int64_t n_points, int32_t activated, void *sigma, int32_t sigma_elem,
                    void *rgb, int32_t rgb_elem, float *warped, nfa_stream_t stream)
{
    const char *who = "nfa_tnerf_field";
    Shape S;
    if (int rc = check_warp_shape(who, elem, warp, &S)) return rc;
    const WarpArgs w = warp_args(S, warp_image, warp_bias, times, warped);
    return nerf_query(who, true, elem, trunk, head, trunk_image, head_image, trunk_bias, head_bias, in, n_points, activated, sigma, sigma_elem,
                      rgb, rgb_elem, stream, &w);
}

int nfa_tnerf_train_fwd(int32_t elem, const nfa_mlp_desc *warp, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *warp_image,
                        const void *trunk_image, const void *head_image, const float *warp_bias, const float *trunk_bias,
                        const float *head_bias, const nfa_ngp_input *in, const float *times, int64_t n_points, int32_t activated,
                        const nfa_nerf_saved *save, const nfa_tnerf_saved *warp_save, void *sigma, int32_t sigma_elem, void *rgb,
                        int32_t rgb_elem, nfa_stream_t stream)
{
    const char *who = "nfa_tnerf_train_fwd";
    Shape S;
    if (int rc = check_warp_shape(who, elem, warp, &S)) return rc;
    const WarpArgs w = warp_args(S, warp_image, warp_bias, times, warp_save ? warp_save->warped : nullptr);
    return nerf_query(who, true, elem, trunk, head, trunk_image, head_image, trunk_bias, head_bias, in, n_points, activated, sigma, sigma_elem,
                      rgb, rgb_elem, stream, &w, true, save, warp_save);
}

int nfa_tnerf_density(int32_t elem, const nfa_mlp_desc *warp, const nfa_mlp_desc *trunk, const void *warp_image, const void *trunk_image,
                      const float *warp_bias, const float *trunk_bias, const nfa_ngp_input *in, const float *times, int64_t n_points,
                      int32_t activated, void *sigma, int32_t sigma_elem, float *warped, nfa_stream_t stream)
{
    const char *who = "nfa_tnerf_density";
    Shape S;
    if (int rc = check_warp_shape(who, elem, warp, &S)) return rc;
    const WarpArgs w = warp_args(S, warp_image, warp_bias, times, warped);
    return nerf_query(who, false, elem, trunk, nullptr, trunk_image, nullptr, trunk_bias, nullptr, in, n_points, activated, sigma, sigma_elem,
                      nullptr, NFA_ELEM_F32, stream, &w);
}

int nfa_tnerf_warp(int32_t elem, const nfa_mlp_desc *warp, const void *warp_image, const float *warp_bias, const nfa_ngp_input *in,
                   const float *times, int64_t n_points, float *warped, nfa_stream_t stream)
{
    const char *who = "nfa_tnerf_warp";
    Shape S;
    if (int rc = check_warp_shape(who, elem, warp, &S)) return rc;
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    NFA_REQUIRE(in, "%s: the input descriptor is null", who);
    if (n_points == 0) return NFA_OK;
    const bool rays = in->positions == nullptr;
    NFA_REQUIRE(!rays || (in->n_rays >= 1 && in->n_rays < ((int64_t)1 << 31) - 64), "%s: n_rays %lld out of range", who, (long long)in->n_rays);
    NFA_REQUIRE(!rays || (in->rays_o && in->rays_d && in->t_starts && in->t_ends && in->ray_indices),
                "%s: null input pointer (positions, or rays_o, rays_d, t_starts, t_ends and ray_indices)", who);
    NFA_REQUIRE(warped, "%s: no output requested", who);
    NFA_REQUIRE(aligned_to(in->positions, 4) && aligned_to(in->rays_o, 4) && aligned_to(in->rays_d, 4) && aligned_to(in->t_starts, 4) &&
                aligned_to(in->t_ends, 4) && aligned_to(in->ray_indices, 8), "%s: misaligned pointer (ray_indices 8, the others their element)", who);
    TNerfArgs a = {};
    a.w = warp_args(S, warp_image, warp_bias, times, warped);
    if (int rc = check_warp_pointers(who, a.w)) return rc;
    a.x = in->positions;
    a.o = in->rays_o, a.d = in->rays_d, a.ts = in->t_starts, a.te = in->t_ends, a.ri = in->ray_indices;
    a.n_rays = in->n_rays, a.N = n_points;
    const int64_t lds = warp_lds_bytes(S), want = ceil_div64(n_points, NF_POINTS);
    const unsigned grid = (unsigned)(want < 2 * NFA_MLP_STREAM_GROUPS ? want : 2 * NFA_MLP_STREAM_GROUPS);   // 42 KiB: two workgroups a CU and more
    dispatch_bool(elem == NFA_ELEM_F16, [&](auto f16) {
        using E = std::conditional_t<decltype(f16)::value, nfa_f16, nfa_bf16>;
        dispatch_bool(rays, [&](auto rays_c) {
            tnerf_warp_kernel<E, decltype(rays_c)::value><<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(a);
        });
    });
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int nfa_ndr_field(int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *warp_image, int64_t warp_image_elems,
                  const void *trunk_image, const void *head_image, const float *warp_bias, int64_t warp_bias_floats, const float *trunk_bias,
                  const float *head_bias, const nfa_ngp_input *in, const float *times, int64_t n_points, int32_t activated, void *sigma,
                  int32_t sigma_elem, void *rgb, int32_t rgb_elem, float *warped, nfa_stream_t stream)
{
    const char *who = "nfa_ndr_field";
    NdrWarp n;
    if (int rc = check_ndr_warp(who, elem, warp_image, warp_image_elems, warp_bias, warp_bias_floats, times, warped, &n)) return rc;
    return nerf_query(who, true, elem, trunk, head, trunk_image, head_image, trunk_bias, head_bias, in, n_points, activated, sigma, sigma_elem,
                      rgb, rgb_elem, stream, nullptr, false, nullptr, nullptr, &n);
}

int nfa_ndr_density(int32_t elem, const nfa_mlp_desc *trunk, const void *warp_image, int64_t warp_image_elems, const void *trunk_image,
                    const float *warp_bias, int64_t warp_bias_floats, const float *trunk_bias, const nfa_ngp_input *in, const float *times,
                    int64_t n_points, int32_t activated, void *sigma, int32_t sigma_elem, float *warped, nfa_stream_t stream)
{
    const char *who = "nfa_ndr_density";
    NdrWarp n;
    if (int rc = check_ndr_warp(who, elem, warp_image, warp_image_elems, warp_bias, warp_bias_floats, times, warped, &n)) return rc;
    return nerf_query(who, false, elem, trunk, nullptr, trunk_image, nullptr, trunk_bias, nullptr, in, n_points, activated, sigma, sigma_elem,
                      nullptr, NFA_ELEM_F32, stream, nullptr, false, nullptr, nullptr, &n);
}

int nfa_ndr_warp(int32_t elem, const void *warp_image, int64_t warp_image_elems, const float *warp_bias, int64_t warp_bias_floats,
                 const nfa_ngp_input *in, const float *times, int64_t n_points, float *warped, nfa_stream_t stream)
{
    const char *who = "nfa_ndr_warp";
    NdrArgs a = {};
    if (int rc = check_ndr_warp(who, elem, warp_image, warp_image_elems, warp_bias, warp_bias_floats, times, warped, &a.n)) return rc;
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    NFA_REQUIRE(in, "%s: the input descriptor is null", who);
    if (n_points == 0) return NFA_OK;
    const bool rays = in->positions == nullptr;
    NFA_REQUIRE(!rays || (in->n_rays >= 1 && in->n_rays < ((int64_t)1 << 31) - 64), "%s: n_rays %lld out of range", who, (long long)in->n_rays);
    NFA_REQUIRE(!rays || (in->rays_o && in->rays_d && in->t_starts && in->t_ends && in->ray_indices),
                "%s: null input pointer (positions, or rays_o, rays_d, t_starts, t_ends and ray_indices)", who);
    NFA_REQUIRE(warped, "%s: no output requested", who);
    NFA_REQUIRE(aligned_to(in->positions, 4) && aligned_to(in->rays_o, 4) && aligned_to(in->rays_d, 4) && aligned_to(in->t_starts, 4) &&
                aligned_to(in->t_ends, 4) && aligned_to(in->ray_indices, 8), "%s: misaligned pointer (ray_indices 8, the others their element)", who);
    if (int rc = check_ndr_pointers(who, a.n)) return rc;
    a.x = in->positions;
    a.o = in->rays_o, a.d = in->rays_d, a.ts = in->t_starts, a.te = in->t_ends, a.ri = in->ray_indices;
    a.n_rays = in->n_rays, a.N = n_points;
    const int64_t lds = ndr_warp_lds_bytes(), want = ceil_div64(n_points, NF_POINTS);
    const unsigned grid = (unsigned)(want < 2 * NFA_MLP_STREAM_GROUPS ? want : 2 * NFA_MLP_STREAM_GROUPS);   // 48 KiB: two workgroups a CU and more
    dispatch_bool(elem == NFA_ELEM_F16, [&](auto f16) {
        using E = std::conditional_t<decltype(f16)::value, nfa_f16, nfa_bf16>;
        dispatch_bool(rays, [&](auto rays_c) {
            ndr_warp_kernel<E, decltype(rays_c)::value><<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(a);
        });
    });
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

int nfa_ndr_time_features(int32_t elem, const void *time_image, const float *time_bias, const float *times, int64_t n_points, void *out,
                          nfa_stream_t stream)
{
    const char *who = "nfa_ndr_time_features";
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the networks' type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    if (n_points == 0) return NFA_OK;
    NFA_REQUIRE(time_image && time_bias && times && out, "%s: null pointer", who);
    NFA_REQUIRE(aligned_to(time_image, 16) && aligned_to(time_bias, 16) && aligned_to(times, 4) && aligned_to(out, 16),
                "%s: misaligned pointer (image, bias and out 16, times 4)", who);
    const int64_t want = ceil_div64(n_points, NF_POINTS);
    const unsigned grid = (unsigned)(want < 8 * NFA_MLP_STREAM_GROUPS ? want : 8 * NFA_MLP_STREAM_GROUPS);
    if (elem == NFA_ELEM_F16)
        ndr_time_features_kernel<nfa_f16><<<grid, NF_THREADS, 0, as_stream(stream)>>>(static_cast<const nfa_v4u *>(time_image), time_bias, times, n_points,
                                                                                      static_cast<uint16_t *>(out));
    else
        ndr_time_features_kernel<nfa_bf16><<<grid, NF_THREADS, 0, as_stream(stream)>>>(static_cast<const nfa_v4u *>(time_image), time_bias, times, n_points,
                                                                                       static_cast<uint16_t *>(out));
    NFA_CHECK_LAUNCH(who);
    return NFA_OK;
}

}  // extern "C"

// nerf_field.hip -- the no-grad query of the reference's vanilla NeRF field as ONE launch: both sinusoidal encoders, the trunk,
// the colour head and the output activations (ref: examples/radiance_fields/mlp.py, VanillaNeRFRadianceField over NerfMLP).
// Inference only: nothing is saved for a backward.  The composed chain (SinusoidalEncoding twice, StreamedMLP, split, cat,
// StreamedMLP, activations) moves about 1.9 KB per point through memory at the reference's shape; this pass reads 24 B (a
// position and a direction, or 16 B of a ray sample) and writes 4 to 16 B.
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
#include "mlp_tiles.h"
#include "samples.h"

namespace nfa {
namespace {

constexpr int NF_WAVES = 4;
constexpr int NF_THREADS = NF_WAVES * NFA_WAVE;
constexpr int NF_POINTS = NF_WAVES * 32;   // points of a workgroup per pass of the images
constexpr int NF_SLOTS = 2;
constexpr int NF_MAX_PIECES = 160;         // 8 * 8 + 9 of the trunk and 4 * 4 + 1 of the head at most
constexpr int NF_MAX_HIDDEN = 8, NF_HEAD_MAX_HIDDEN = 4, NF_HEAD_W = 128;
constexpr int NF_POS_L = 10, NF_DIR_L = 4;                               // the reference's degrees (0, 10) and (0, 4)
constexpr int NF_POS_DIMS = 3 + 6 * NF_POS_L, NF_DIR_DIMS = 3 + 6 * NF_DIR_L;   // 63 and 27, with identity
static_assert(NF_POINTS == NFA_MLP_STREAM_POINTS, "the streamed passes' split");

struct Piece { int32_t off16, n16; };   // of its image, in 16-byte fragments

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

// mlp_stream.hip's ring over two images: pieces below n_trunk come from the trunk's, the others from the head's
template <int MAXV>
struct FieldRing {
    const nfa_v4u *timg, *himg;
    nfa_v4u *slots;
    const Piece *tab;
    int slot16, n_trunk, n_pieces, next, cur;
    nfa_v4u regs[MAXV];

    __device__ __forceinline__ const nfa_v4u *source(int i) const { return (i < n_trunk ? timg : himg) + tab[i].off16; }
    // thread 0 has written the table; stages piece 0
    __device__ __forceinline__ void start()
    {
        __syncthreads();
        const nfa_v4u *src = source(0);
        const int n16 = tab[0].n16;
        for (int i = threadIdx.x; i < n16; i += NF_THREADS) slots[i] = src[i];
        __syncthreads();
        cur = 0;
        next = 1;   // every network has at least two pieces
    }
    __device__ __forceinline__ const nfa_v4u *piece() const { return slots + cur * slot16; }
    // issues the loads of the next piece; the current one is read between fetch() and hand_over()
    __device__ __forceinline__ void fetch()
    {
        const nfa_v4u *src = source(next);
        const int n16 = tab[next].n16;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int i = threadIdx.x + v * NF_THREADS;
            if (i < n16) regs[v] = src[i];
        }
    }
    __device__ __forceinline__ void hand_over()
    {
        const int n16 = tab[next].n16;
        nfa_v4u *d = slots + (cur ^ 1) * slot16;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int i = threadIdx.x + v * NF_THREADS;
            if (i < n16) d[i] = regs[v];
        }
        __syncthreads();
        cur ^= 1;
        next = next + 1 == n_pieces ? 0 : next + 1;
    }
};

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
};

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
template <class E, int W, bool RAYS, bool FULL>
__global__ __launch_bounds__(NF_THREADS) void nerf_field_kernel(const NerfArgs a)
{
    constexpr int MT = W / 32, KQ = W / 16, KQX = (NF_POS_DIMS + 15) / 16, KQD = (NF_DIR_DIMS + 15) / 16;
    constexpr int HW = NF_HEAD_W, HMT = HW / 32, HKQ = HW / 16;
    constexpr int MAXV = ((KQ + KQX) * 64 + NF_THREADS - 1) / NF_THREADS;   // the trunk's cat layer, the largest piece
    static_assert(KQ + KQD <= KQ + KQX && HKQ <= KQ, "no piece of the head is larger");
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
    FieldRing<MAXV> ring;
    if (threadIdx.x == 0) nerf_pieces(T, H, FULL, tab, nullptr, nullptr);
    ring.timg = reinterpret_cast<const nfa_v4u *>(a.timg);
    ring.himg = reinterpret_cast<const nfa_v4u *>(a.himg);
    ring.slots = reinterpret_cast<nfa_v4u *>(nf_lds);
    ring.tab = tab;
    ring.slot16 = a.slot16;
    ring.n_trunk = D * MT + (FULL ? MT + 1 : 1);
    ring.n_pieces = a.n_pieces;
    ring.start();
    const int64_t N = a.N, n_pass = ceil_div64(N, NF_POINTS);
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int64_t p = (pass * NF_WAVES + wave) * 32 + r, pc = p < N ? p : N - 1;
        // ---- the point and both encoded rows, before layer 0's first fetch
        float x[3], dir[3] = {0.f, 0.f, 0.f};
        if constexpr (RAYS) {
            float ro[3];
            ray_rows(a.o, a.d, a.ri[pc], a.n_rays, ro, dir);
            sample_point(ro, dir, a.ts[pc], a.te[pc], x);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[k] = a.x[3 * pc + k];
                if constexpr (FULL) dir[k] = a.dirs[3 * pc + k];
            }
        }
        nfa_v4u xf[KQX], df[KQD];
        enc_frags<E, NF_POS_L, KQX>(x, lane, h, xf);
        if constexpr (FULL) enc_frags<E, NF_DIR_L, KQD>(dir, lane, h, df);
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
                }
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

// The one statement of the shapes the fused query holds (nerfacc_amd/fields.py: nerf_field_limits_error says the same words).
int check_field_shape(const char *who, int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, int32_t trunk_width,
                      int64_t n_points, Shape *T, Shape *H)
{
    NFA_REQUIRE(elem == NFA_ELEM_F16 || elem == NFA_ELEM_BF16, "%s: elem %d: the networks' type is NFA_ELEM_F16 or NFA_ELEM_BF16", who, elem);
    if (T) {
        NFA_REQUIRE(trunk, "%s: the network descriptor is null", who);
        const int w = trunk->width, d = trunk->n_hidden;
        NFA_REQUIRE(w == 128 || w == 256, "%s: trunk width %d: 128 or 256 neurons are supported", who, w);
        NFA_REQUIRE(d >= 1 && d <= NF_MAX_HIDDEN, "%s: trunk n_hidden %d: 1 to %d hidden layers are supported", who, d, NF_MAX_HIDDEN);
        NFA_REQUIRE(trunk->n_in == NF_POS_DIMS, "%s: trunk n_in %d: the encoded position has %d features", who, trunk->n_in, NF_POS_DIMS);
        NFA_REQUIRE(trunk->n_out == w + 1, "%s: trunk n_out %d: width + 1 = %d outputs (the bottleneck, then sigma)", who, trunk->n_out, w + 1);
        NFA_REQUIRE(trunk->bias == 1, "%s: trunk bias %d: the field's networks have biases (1)", who, trunk->bias);
        NFA_REQUIRE((trunk->skip_mask & ~((2 << d) - 4)) == 0, "%s: trunk skip_mask 0x%x: only bits 2 to n_hidden (%d) may be set: layer 0 "
                    "takes x itself and layer 1 follows it", who, (unsigned)trunk->skip_mask, d);
        *T = Shape{trunk->n_in, trunk->n_out, w, d, 1, trunk->skip_mask};
        trunk_width = w;
    }
    if (H) {
        NFA_REQUIRE(head, "%s: the network descriptor is null", who);
        NFA_REQUIRE(trunk_width == 128 || trunk_width == 256, "%s: trunk width %d: 128 or 256 neurons are supported", who, trunk_width);
        const int d = head->n_hidden;
        NFA_REQUIRE(head->width == NF_HEAD_W, "%s: head width %d: %d neurons are supported", who, head->width, NF_HEAD_W);
        NFA_REQUIRE(d >= 1 && d <= NF_HEAD_MAX_HIDDEN, "%s: head n_hidden %d: 1 to %d hidden layers are supported", who, d, NF_HEAD_MAX_HIDDEN);
        NFA_REQUIRE(head->n_in == trunk_width + NF_DIR_DIMS, "%s: head n_in %d: trunk width + %d = %d inputs (the bottleneck, then the encoded "
                    "direction)", who, head->n_in, NF_DIR_DIMS, trunk_width + NF_DIR_DIMS);
        NFA_REQUIRE(head->n_out == 3, "%s: head n_out %d: 3 outputs (the colour)", who, head->n_out);
        NFA_REQUIRE(head->bias == 1, "%s: head bias %d: the field's networks have biases (1)", who, head->bias);
        NFA_REQUIRE(head->skip_mask == 0, "%s: head skip_mask 0x%x: the head has no skip", who, (unsigned)head->skip_mask);
        *H = Shape{head->n_in, 3, NF_HEAD_W, d, 1, 0};
    }
    NFA_REQUIRE(n_points >= 0, "%s: n_points %lld is negative", who, (long long)n_points);
    return NFA_OK;
}

int nerf_query(const char *who, bool full, int32_t elem, const nfa_mlp_desc *trunk, const nfa_mlp_desc *head, const void *trunk_image,
               const void *head_image, const float *trunk_bias, const float *head_bias, const nfa_ngp_input *in, int64_t N,
               int32_t activated, void *sigma, int32_t sigma_elem, void *rgb, int32_t rgb_elem, nfa_stream_t stream)
{
    Shape T, H = {};
    if (int rc = check_field_shape(who, elem, trunk, head, 0, N, &T, full ? &H : nullptr)) return rc;
    NFA_REQUIRE(in, "%s: the input descriptor is null", who);
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
    NerfArgs a = {};
    a.T = T, a.H = H;
    a.timg = static_cast<const uint16_t *>(trunk_image), a.himg = static_cast<const uint16_t *>(head_image);
    a.tbias = trunk_bias, a.hbias = head_bias;
    int slot16 = 0;
    a.n_pieces = nerf_pieces(T, H, full, nullptr, &slot16, nullptr);
    a.slot16 = slot16;
    a.x = in->positions, a.dirs = in->dirs;
    a.o = in->rays_o, a.d = in->rays_d, a.ts = in->t_starts, a.te = in->t_ends, a.ri = in->ray_indices;
    a.n_rays = in->n_rays, a.N = N;
    a.sigma = sigma, a.sigma_f32 = sigma_elem == NFA_ELEM_F32;
    a.rgb = full ? rgb : nullptr, a.rgb_f32 = rgb_elem == NFA_ELEM_F32;
    a.activated = activated;
    const int64_t lds = nerf_lds_bytes(slot16, trunk_bias_floats(T) + (full ? head_bias_floats(H) : 0));
    const int64_t want = ceil_div64(N, NF_POINTS);
    const unsigned grid = (unsigned)(want < NFA_MLP_STREAM_GROUPS ? want : NFA_MLP_STREAM_GROUPS);
    int rc = NFA_OK;
    auto launch = [&](auto tag, auto w, auto rays_c, auto full_c) {
        using E = typename decltype(tag)::type;
        auto kern = nerf_field_kernel<E, decltype(w)::value, decltype(rays_c)::value, decltype(full_c)::value>;
        if ((rc = allow_lds(who, kern, lds)) != NFA_OK) return;
        kern<<<grid, NF_THREADS, (size_t)lds, as_stream(stream)>>>(a);
    };
    auto by_form = [&](auto tag, auto w) {
        dispatch_bool(rays, [&](auto rays_c) { dispatch_bool(full, [&](auto full_c) { launch(tag, w, rays_c, full_c); }); });
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

}  // extern "C"

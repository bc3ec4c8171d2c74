/*
 * nerfacc_hip.h -- C ABI of libnerfacc_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for nerfacc's native hot path.  The reference
 * binds its native layer through pybind11/ATen (nerfacc/cuda/csrc/nerfacc.cpp:
 * 100-129, resolved lazily by nerfacc/cuda/__init__.py:8-41); there is no C ABI
 * upstream.  Each entry point below replaces one of those pybind symbols (or
 * one ATen composite the Python layer builds around them) and takes only plain
 * device pointers, sizes and a stream: no torch types cross this line.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - fp32 data, int64 indices/counts, uint8 for bool tensors (torch.bool); the `_t` entries take an element type
 *     (NFA_ELEM_*) for the per-sample activation streams named in their comments, which then arrive as void *;
 *   - all work is enqueued on `stream` (hipStream_t passed as void*); nothing
 *     synchronises unless stated;
 *   - return value: 0 on success, otherwise a negative NFA_E* code; the text
 *     of the last error on the calling thread is nfa_last_error();
 *   - outputs are caller-allocated (the Python host layer allocates them with
 *     torch so they live in the caching allocator like the reference's).
 *
 * Citations "ref:" are relative to /root/reference/nerfacc/.
 */
#ifndef NERFACC_HIP_H
#define NERFACC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFA_OK 0
#define NFA_EINVAL (-1)   /* bad argument (shape, null pointer, unsupported mode) */
#define NFA_EHIP (-2)     /* HIP runtime error (launch failure, ...) */

#define NFA_MAX_GRID_LEVELS 8 /* fused in-kernel intersection+sort supports up to this many levels */

typedef void *nfa_stream_t; /* hipStream_t */

/* Element type of a per-sample activation stream of the `_t` entries.  Arithmetic is float32 whatever the code: a half
 * value widens exactly on load, and a store rounds the float32 value the NFA_ELEM_F32 entry would have stored once, to
 * nearest even (results in fp16's subnormal range included).  Any other code is NFA_EINVAL. */
#define NFA_ELEM_F32 0
#define NFA_ELEM_F16 1   /* IEEE binary16 */
#define NFA_ELEM_BF16 2  /* bfloat16 */

const char *nfa_last_error(void);
/* The version of THIS header.  Bumped whenever an entry point changes its arguments or what it expects of them; a caller
 * built against another value must not call the library (nerfacc_amd/_backend.py refuses to load it). */
#define NFA_VERSION 403
int nfa_version(void);          /* NFA_VERSION of the header the library was built from */
/* Knobs of the A/B tests and measurement scripts (which of two equivalent kernels a call takes, tile sizes); value NULL
 * or "" unsets.  Names: NFA_REFILL, NFA_REFILL_ALL, NFA_CONE_STAGED, NFA_SEG_TILE, NFA_WALK_NO_LATTICE.  Results never
 * depend on them.  Not thread-safe: set before the calls that should see them. */
int nfa_set_tuning(const char *name, const char *value);
int nfa_device_arch(char *buf, int buflen); /* gcnArchName of the current device */

/* ------------------------------------------------------------------ utilities */

/* starts[i] = sum(cnts[0..i)), *total = sum(cnts).  `scratch` needs
 * nfa_cumsum_scratch_bytes(n) bytes.  Replaces torch::cumsum in
 * ref: cuda/csrc/include/data_spec.hpp:86-105. */
int64_t nfa_cumsum_scratch_bytes(int64_t n);
int nfa_exclusive_cumsum_i64(const int64_t *cnts, int64_t n, int64_t *starts, int64_t *total,
                             void *scratch, nfa_stream_t stream);
/* Same scan, written as packed_info rows {start, count} (ref: data_specs.py:68-69 stacks them afterwards). */
int nfa_exclusive_cumsum_pairs_i64(const int64_t *cnts, int64_t n, int64_t *packed_info /*[n,2]*/, int64_t *total,
                                   void *scratch, nfa_stream_t stream);
/* The same with a coherence measure for the caller's next batch: total_and_stats[0] = total; over a sample of the input
 * (every 8th block of 2048 counts) [1] += sum over groups of 64 consecutive counts of the group's maximum and [2] += sum
 * of the counts ([1], [2] zeroed by the caller; n <= 4 M, else left untouched).  64 * [1] / [2] is how much longer a
 * wave of 64 neighbouring rays runs than its average ray. */
int nfa_exclusive_cumsum_pairs_stats_i64(const int64_t *cnts, int64_t n, int64_t *packed_info /*[n,2]*/,
                                         int64_t *total_and_stats /*[3]*/, void *scratch, nfa_stream_t stream);

/* packed_info[r] = {start, count} of ray r in a ray-sorted index stream; also
 * reports (flags[0]) whether ray_indices is non-decreasing and in range.
 * ref: pack.py:38-46 (index_add_ histogram + cumsum). scratch as above (n_rays). */
int nfa_pack_info(const int64_t *ray_indices, int64_t n, int64_t n_rays, int64_t *packed_info /*[n_rays,2]*/,
                  int32_t *flags /*[1], set to 1 if unsorted/out of range*/, void *scratch, nfa_stream_t stream);

/* Sample data between the packed layout (packed[n_packed, row], rows of ray r at packed_info[r] = {start, count}) and the
 * padded one (padded[n_rays, n_per_ray, row]); a row is row_bytes opaque bytes (any dtype, any feature width).  Which
 * padded slot a packed row belongs to:
 *   mask NULL   the first min(count, n_per_ray) rows of ray r's chunk are slots 0 .. min(count, n_per_ray) - 1 of row r;
 *               the rest of the chunk is dropped (nerfacc 0.3's unpack_data).  Chunks must not overlap;
 *   mask given  (uint8 [n_rays, n_per_ray]) the chunk's rows go to the set slots of row r in row-major order, count ==
 *               the row's popcount (data[mask]: nerfacc 0.3's pack_data, packed_info from nfa_mask_row_counts and
 *               nfa_exclusive_cumsum_pairs_i64).
 * Rows move in the widest chunks of 16, 8, 4, 2 or 1 bytes that row_bytes and both base pointers allow.  Deterministic (no
 * accumulation); packed rows outside [0, n_packed) are never touched.  The packed pointer may be NULL when n_packed == 0.
 * nfa_unpack_rows writes every padded slot: slots with no packed row get the pad value (pad_bytes bytes at pad_host,
 * repeated; pad_bytes 0 = zeros).
 * nfa_pack_rows writes the packed rows of the chunks: with mask NULL, rows dropped by nfa_unpack_rows get zeros (its
 * gradient); packed rows that no chunk covers are not written. */
int nfa_unpack_rows(const void *packed, const int64_t *packed_info /*[n_rays,2]*/, const uint8_t *mask, int64_t n_rays,
                    int64_t n_per_ray, int64_t n_packed, int64_t row_bytes, const void *pad_host, int32_t pad_bytes,
                    void *padded, nfa_stream_t stream);
int nfa_pack_rows(const void *padded, const int64_t *packed_info /*[n_rays,2]*/, const uint8_t *mask, int64_t n_rays,
                  int64_t n_per_ray, int64_t n_packed, int64_t row_bytes, void *packed, nfa_stream_t stream);
/* counts[r] = number of nonzero bytes in mask row r (uint8 [n_rows, n_cols]). */
int nfa_mask_row_counts(const uint8_t *mask, int64_t n_rows, int64_t n_cols, int64_t *counts, nfa_stream_t stream);

/* 1 bit per cell copy of a torch.bool grid [n_cells] (derived cache, never serialised).
 * Layout: cell i (any non-zero byte = occupied) is bit i & 31 of word i >> 5; the last word's unused bits are 0. */
int nfa_pack_bits(const uint8_t *binaries, int64_t n_cells, uint32_t *bits /*[(n_cells+31)/32]*/, nfa_stream_t stream);

/* ------------------------------------------------------------------ grid */

/* ref: cuda/csrc/grid.cu:477-519 (ray_aabb_intersect). */
int nfa_ray_aabb_intersect(const float *rays_o, const float *rays_d, int64_t n_rays,
                           const float *aabbs, int32_t n_aabbs, float near_plane, float far_plane,
                           float miss_value, float *t_mins, float *t_maxs, uint8_t *hits,
                           nfa_stream_t stream);

/* The sorted enter / exit events of every ray against the n_aabbs nested boxes, as the reference's Python forms them
 * (grid.py:156-162: ray_aabb_intersect(rays_o, rays_d, aabbs) with near = -inf, far = +inf, miss = +inf, then
 * torch.sort(torch.cat([t_mins, t_maxs], -1), -1)) in one pass: t_sorted f32 [n_rays, 2 n_aabbs], t_indices int64
 * [n_rays, 2 n_aabbs] (k < n_aabbs: entering box k, else leaving box k - n_aabbs), hits bool [n_rays, n_aabbs].
 * Stable: ties keep the order of the concatenation (the reference leaves it unspecified).  n_aabbs <= NFA_MAX_EVENT_LEVELS. */
#define NFA_MAX_EVENT_LEVELS 8
int nfa_ray_events(const float *rays_o, const float *rays_d, int64_t n_rays, const float *aabbs, int32_t n_aabbs,
                   float *t_sorted, int64_t *t_indices, uint8_t *hits, nfa_stream_t stream);

/* One launch of the traversal, ref: cuda/csrc/grid.cu:68-282 + host :320-474.
 *
 * mode 0  count pass  : writes iv_cnts / sm_cnts (whichever is non-null) and terminate_planes.
 * mode 1  fill pass   : reads iv_starts/iv_cnts, sm_starts/sm_cnts, writes the data arrays.
 * mode 2  one pass into over-allocated chunks (reads *_starts as the over-allocated offsets,
 *         honours rays_mask, writes the actual counts to *_cnts and terminate_planes).
 *
 * Intersections: pass t_sorted/t_indices/hits as produced by nfa_ray_aabb_intersect + sort,
 * or all three NULL to have the kernel intersect (and, for n_grids > 1, sort) in registers
 * (n_grids <= NFA_MAX_GRID_LEVELS).
 *
 * Sample-only fast path used by OccGridEstimator.sampling: pass iv_* NULL and
 * sm_t_starts/sm_t_ends non-null; the kernel then emits (t_starts, t_ends, ray_indices)
 * per sample directly instead of interval edges + masks (same values as
 * intervals.vals[is_left] / [is_right], ref: estimators/occ_grid.py:174-177).
 */
typedef struct nfa_traverse_args {
    int64_t n_rays;
    const float *rays_o;        /* [n_rays,3] */
    const float *rays_d;        /* [n_rays,3] */
    const uint8_t *rays_mask;   /* [n_rays] or NULL (mode 2 only) */
    int32_t n_grids;
    int32_t res[3];
    const uint8_t *binaries;    /* [n_grids,res0,res1,res2] torch.bool */
    const float *aabbs;         /* [n_grids,6] */
    const uint8_t *hits;        /* [n_rays,n_grids] or NULL */
    const float *t_sorted;      /* [n_rays,2*n_grids] or NULL */
    const int64_t *t_indices;   /* [n_rays,2*n_grids] or NULL */
    const float *near_planes;   /* [n_rays] */
    const float *far_planes;    /* [n_rays] */
    float step_size;
    float cone_angle;
    int32_t traverse_steps_limit; /* <= 0: none */
    int32_t mode;
    /* intervals (all NULL => not computed) */
    float *iv_vals; int64_t *iv_ray_indices; uint8_t *iv_is_left; uint8_t *iv_is_right;
    int64_t *iv_starts; int64_t *iv_cnts;
    /* samples */
    float *sm_vals; int64_t *sm_ray_indices; uint8_t *sm_is_valid;
    float *sm_t_starts; float *sm_t_ends;       /* sample-only fast path (sm_ray_indices may be NULL: see nfa_fill_ray_indices) */
    int64_t *sm_starts; int64_t *sm_cnts;
    float *terminate_planes;    /* [n_rays] or NULL */
    /* optional ray filter (mode 1): only rays with ray_filter[r] > ray_filter_min are processed */
    const int32_t *ray_filter;
    int32_t ray_filter_min;
    /* optional accelerator: the brick-packed copy of binaries made by nfa_pack_bricks (both or neither).
     * Occupancy is then read from 8-byte bricks (one load per 4x4x4 cells, 1/8 of the bool grid's footprint);
     * results are identical. */
    const uint64_t *bricks;
    const uint32_t *coarse;
    /* Optional DEVICE-side controls, for loops that must not wait for the host (the test-mode loop captured into a hipGraph):
     *   steps_limit_dev  (nfa_traverse_runs, mode 2) the step limit of this call, read from the device instead of
     *                    traverse_steps_limit (which must still be > 0: it selects the kernel); 0 = nothing to do, the
     *                    call leaves every output as it is;
     *   n_listed_dev     (nfa_traverse_runs with ray_order) the number of entries of ray_order to walk (<= n_order);
     *   run_if_nonzero   (nfa_traverse_grids) the launch does nothing when *run_if_nonzero == 0 (the fill pass for rays
     *                    with too many run records, whose count the host has not seen). */
    const int32_t *steps_limit_dev;
    const int64_t *n_listed_dev;
    const int32_t *run_if_nonzero;
} nfa_traverse_args;
int nfa_traverse_grids(const nfa_traverse_args *args, nfa_stream_t stream);

/* Run-length traversal used by the sampler and by traverse_grids when step_size > 0 and cone_angle == 0 (same
 * results as nfa_traverse_grids, one DDA walk instead of the reference's count + fill passes, ref: cuda/csrc/grid.cu:
 * 405-471; coalesced output):
 *   nfa_pack_walk_bits 1-bit-per-cell copy of the torch.bool grid in the walk's own cell order (the coordinate bits of
 *                      x, y, z interleaved: a 128-byte line is a 16 x 8 x 8 block of cells); nfa_walk_bits_words() uint32.
 *   nfa_traverse_runs  per ray: sample count (args->sm_cnts), edge count (args->iv_cnts, optional), terminate plane,
 *                      run count and up to max_runs (<= 32) run records {t_first:f32 | k_start:31, continues_previous:1}
 *                      in runs[max_runs][n_rays] (slot-major: record i of ray r at runs[i * n_rays + r]); rays with
 *                      more runs are counted in overflow_count[0] and must be filled with
 *                      nfa_traverse_grids(mode 1, ray_filter = run_cnts, ray_filter_min = max_runs).
 *                      args->mode: 0 = all rays, 2 = honour rays_mask (+ traverse_steps_limit).  At most 512 cells
 *                      per axis.  near_hint: the value EVERY entry of args->near_planes holds, NaN if there is no such
 *                      value.  With it the march runs on the lattice near, near + step, ... that all rays share (one
 *                      table built on the host from the two numbers); same results.  overflow_count is int32[2]:
 *                      overflow_count[1] != 0 reports rays the table did not serve (a near plane that differs from
 *                      near_hint, a march beyond the tabulated part of the sequence): the outputs are then
 *                      incomplete and the caller repeats the call with near_hint = NaN (the per-ray marcher).
 *   nfa_pack_bricks    torch.bool grid -> 4x4x4-cell 64-bit bricks + 1 bit per brick ("coarse") for the serial
 *                      kernels of nfa_traverse_grids (args->bricks / args->coarse);
 *                      bricks has nfa_bricks_words() entries, coarse (words+31)/32 uint32.
 *   nfa_expand_runs    runs + exclusive cumsum of the counts -> (t_starts, t_ends) or, when t_mids is given,
 *                      the API's sample values (t_start + t_end) / 2; and ray_indices. */
int64_t nfa_bricks_words(int32_t n_grids, const int32_t *res);
int nfa_pack_bricks(const uint8_t *binaries, int32_t n_grids, const int32_t *res, uint64_t *bricks,
                    uint32_t *coarse, nfa_stream_t stream);
int64_t nfa_walk_bits_words(int32_t n_grids, const int32_t *res);
int nfa_pack_walk_bits(const uint8_t *binaries, int32_t n_grids, const int32_t *res, uint32_t *bits, nfa_stream_t stream);
/* ray_order[n_order] (NULL: every ray, in index order): the rays to walk and the lane each gets.  n_order < n_rays walks
 * the listed rays only -- the others' sm_cnts / run_cnts / terminate_planes are left as the caller initialised them (the
 * test-mode loop lists its alive rays, so that dead rays cost no lanes). */
int nfa_traverse_runs(const nfa_traverse_args *args, const uint32_t *bits, int32_t *run_cnts, uint64_t *runs,
                      int32_t max_runs, int32_t *overflow_count, float near_hint, const int32_t *ray_order,
                      int64_t n_order, nfa_stream_t stream);
/* Lane -> ray assignment for nfa_traverse_runs (ray_order; NULL = identity): order[n_rays] = the ray ids sorted into 256
 * bins by the length of the ray's path through box[6] = {min xyz, max xyz} (the outermost grid box), so that the rays a
 * wave walks together are of similar length.  For batches of unrelated rays (training) the walk is ~1.6x faster;
 * image-ordered rays are coherent already.  Everything the walk writes stays indexed by ray id: results do not depend on
 * the order.  scratch: 1024 + n_rays bytes. */
int nfa_bin_rays(const float *rays_o, const float *rays_d, int64_t n_rays, const float *box, int32_t *order,
                 void *scratch, nfa_stream_t stream);
/* Between two iterations of the test-mode loop (ref: examples/utils.py:409-414): mask[r] = opacity[r] <= opacity_max &&
 * packed_info[r].count == n_samples (the ray is not opaque yet and used its whole budget), alive[0 .. *count) = the ids of
 * the rays with mask 1 (ascending inside stretches of 8192 rays, the stretches in arbitrary order: a ray_order for
 * nfa_traverse_runs / nfa_traverse_cone_walk with n_order = *count), *count = their number.  One launch. */
int nfa_alive_rays(const float *opacity, const int64_t *packed_info /*[n_rays,2]*/, int64_t n_samples, float opacity_max,
                   int64_t n_rays, uint8_t *mask, int32_t *alive, int64_t *count, nfa_stream_t stream);
/* The test-mode loop without the host in it (ref examples/utils.py:330-414; nerfacc_amd/marching.py, padded form): the
 * iteration schedule lives in state[8] (int32, zeroed before the first iteration):
 *   state[0] samples per ray of the CURRENT iteration, 0 = the loop is over (no ray alive, or max_samples handed out),
 *   state[1] samples per ray handed out so far, state[2] iterations that did something, state[4..5] (one int64) samples
 *   that entered the accumulation so far.
 * alive_count is int64[2]: [0] the alive rays (written by nfa_testmode_alive, n_rays before the first iteration), [1] its
 * value at the start of the current iteration (the walk's n_listed_dev).
 * nfa_testmode_begin   starts an iteration: state[0] = max(min(n_rays / alive_count[0], 64), min_samples) while rays are alive
 *                      and state[1] < max_samples (then state[1] += state[0]), else 0; alive_count[1] = alive_count[0],
 *                      alive_count[0] = 0; zeroes sm_cnts[n_rays], run_cnts[n_rays] and zero_words[n_zero] (int64: the
 *                      caller's counters of the iteration, e.g. nfa_traverse_runs' overflow_count -- a call with
 *                      steps_limit_dev set does not zero it itself, so that the iteration has no memset node);
 * nfa_testmode_alive   ends it: nfa_alive_rays with n_samples = state[0] (state[0] == 0: nothing happens, count[0] stays 0)
 *                      into count = alive_count, and state[4..5] += the iteration's samples (the last row of packed_info)
 *                      when count_samples != 0. */
int nfa_testmode_begin(int64_t *alive_count, int32_t *state, int64_t n_rays, int32_t min_samples, int32_t max_samples,
                       int64_t *sm_cnts, int32_t *run_cnts, int64_t *zero_words, int32_t n_zero, nfa_stream_t stream);
int nfa_testmode_alive(const float *opacity, const int64_t *packed_info, int32_t *state, float opacity_max, int64_t n_rays,
                       uint8_t *mask, int32_t *alive, int64_t *count, int32_t count_samples, nfa_stream_t stream);
/* The same for nested levels (aabbs[n_grids][6], finest first; e.g. rays that start inside the finest box): the key is the
 * number of cell boundaries the ray crosses from near_plane on, summed over the levels (the length inside level l but
 * outside level l - 1, times sum_k |d_k| res_k / extent_k).  ray_order of nfa_traverse_cone_runs / nfa_traverse_runs. */
int nfa_bin_rays_levels(const float *rays_o, const float *rays_d, int64_t n_rays, const float *aabbs, int32_t n_grids,
                        const int32_t *res, float near_plane, int32_t *order, void *scratch,
                        uint64_t *coherence /* [2] or NULL, zeroed by the caller: += sum over groups of 64 consecutive rays of
                        the group's largest key, += sum of the keys (64 * [0] / [1]: how much longer a wave of neighbouring
                        rays walks than its average ray) */, nfa_stream_t stream);
/* capacity: number of elements the output arrays hold; nothing is written at or beyond it (a caller that allocated the
 * outputs before the total was known to the host re-runs the expansion if the total turns out larger). */
int nfa_expand_runs(int64_t n_rays, float step_size, const int32_t *run_cnts, const uint64_t *runs,
                    int32_t max_runs, const int64_t *packed_info /*[n_rays,2] {start, count}*/, float *t_starts,
                    float *t_ends, float *t_mids, int64_t *ray_indices, int64_t capacity, nfa_stream_t stream);
/* ray_indices[k] = r for every k in [packed_info[r].start, packed_info[r].start + packed_info[r].count): the inverse of
 * nfa_pack_info for contiguous, ray-ordered segments (what the traversal produces), written as coalesced 32-byte
 * stores.  Used after nfa_traverse_grids' direct fill pass with sm_ray_indices == NULL, so that the per-ray serial
 * kernel does not scatter 8-byte indices (ref: grid.cu:247 writes them from the marching loop). */
int nfa_fill_ray_indices(int64_t n_rays, const int64_t *packed_info /*[n_rays,2]*/, int64_t *ray_indices,
                         nfa_stream_t stream);
/* Sampler path for distance-dependent steps (step_size > 0 and cone_angle > 0; ref grid.cu:207-262 recomputes
 * dt = max(step, t * cone) for every sample, so samples are not arithmetic runs):
 *   nfa_traverse_cone_runs  the count pass of nfa_traverse_grids (samples only; args->mode 0, or 2 = honour rays_mask and
 *                           traverse_steps_limit: the test-mode loop's compact form of over_allocate) that also leaves
 *                           run records {t_first:f32 | k_start:31, continues_previous:1} in runs[max_runs][n_rays]
 *                           (slot-major), one per chain of continuous samples and at least one per 64 samples; rays
 *                           with more records are counted in *overflow_count and must be filled with
 *                           nfa_traverse_grids(mode 1, ray_filter = run_cnts, ray_filter_min = max_runs).
 *                           With traverse_steps_limit > 0 the lanes of a wave are not bound to one ray each: a wave owns a
 *                           chunk of consecutive entries of the ray list and hands the next one to a lane whose ray is
 *                           finished (limited walks end after a geometric number of cells; results are the same).
 *                           Environment, for measurements: NFA_REFILL=0 (one ray per lane), NFA_REFILL=<chunk>,<min_busy>;
 *   nfa_expand_cone_runs    records + exclusive cumsum of the counts -> (t_starts, t_ends, ray_indices): every output
 *                           re-runs the serial recurrence t <- t + max(step, t * cone) from its record's t_first (at
 *                           most 63 steps), so the values are bit-identical to the marching loop's, and the second DDA
 *                           walk of the fill pass is replaced by coalesced stores. */
int nfa_traverse_cone_runs(const nfa_traverse_args *args, int32_t *run_cnts, uint64_t *runs, int32_t max_runs,
                           int32_t *overflow_count, const int32_t *ray_order /* as for nfa_traverse_runs, or NULL */,
                           int64_t n_order, nfa_stream_t stream);
/* nfa_traverse_cone_runs over the 1-bit grid copy of nfa_pack_walk_bits (grids of at most 512 cells per axis, as for
 * nfa_traverse_runs): the same outputs, bit for bit, with the constant-step walk's DDA (packed step counters, interleaved
 * bit index, one 4-byte load per cell) -- about half the instructions per cell.  args->bricks is not read.
 * (csrc/walk.hip: cone_walk_kernel, cone_refill_kernel; ref grid.cu:68-282.) */
/* arena (optional; NULL / 0: none): where the records go that do not fit a ray's max_runs slots, instead of sending the ray
 * to the serial fill pass (ref grid.cu:405-471: a second full walk).  arena_capacity entries of 16 bytes {t_first:f32,
 * k_start:31 | continues:1, ray:u32, samples:u32}, a multiple of 16, handed in ZEROED.  Such a ray keeps max_runs - 1 records
 * and a sentinel {NaN, samples so far} in its last slot (nfa_expand_cone_runs skips the rest of its range; run_cnts = max_runs).
 * overflow_count is int32[2]: [0] rays for the fill pass (without an arena: every ray with more records than slots; with one:
 * only rays that found it full), [1] arena entries handed out (16 at a time; entries with samples == 0 are unused) --
 * nfa_expand_cone_arena(arena, min(overflow_count[1], arena_capacity), ...) writes their samples. */
int nfa_traverse_cone_walk(const nfa_traverse_args *args, const uint32_t *bits, int32_t *run_cnts, uint64_t *runs,
                           int32_t max_runs, int32_t *overflow_count, uint32_t *arena, int32_t arena_capacity,
                           const int32_t *ray_order, int64_t n_order, nfa_stream_t stream);
int nfa_expand_cone_arena(const uint32_t *arena, int32_t n_entries, float step_size, float cone_angle,
                          const int64_t *packed_info /*[n_rays,2]*/, float *t_starts, float *t_ends, int64_t *ray_indices,
                          nfa_stream_t stream);
int nfa_expand_cone_runs(int64_t n_rays, float step_size, float cone_angle, const int32_t *run_cnts,
                         const uint64_t *runs, int32_t max_runs, const int64_t *packed_info, float *t_starts,
                         float *t_ends, int64_t *ray_indices, nfa_stream_t stream);
/* The interval stream of the API's traverse_grids from the same run records (ref: grid.cu:219-262; edge
 * values, ray_indices, is_left, is_right); iv_cnts as written by nfa_traverse_runs when args->iv_cnts is set
 * (edges = samples + one leading edge per chain of continuous samples), iv_packed_info its {start, count} rows. */
int nfa_expand_intervals(int64_t n_rays, float step_size, const int32_t *run_cnts, const uint64_t *runs,
                         int32_t max_runs, const int64_t *iv_packed_info /*[n_rays,2]*/, float *vals,
                         int64_t *ray_indices, uint8_t *is_left, uint8_t *is_right, nfa_stream_t stream);

/* ------------------------------------------------------------------ grid maintenance */

/* OccGridEstimator._update (ref: estimators/occ_grid.py:368-404) as kernels.
 *   nfa_grid_cell_points  x[i] = aabb_lo + (coords(indices[i]) + jitter[i]) / res * (aabb_hi - aabb_lo)   (ref :383-391;
 *                         indices are cell ids inside one level, x slowest; aabb = the level's 6 floats on the device)
 *   nfa_grid_ema_update   occs[cell_base + indices[i]] = max(occs[...] * ema_decay, occ[i])   (ref :393-398); a cell
 *                         listed several times gets max(occs * decay, max_i occ_i) -- deterministic, one of the values
 *                         the reference's index_put may leave.  max is torch.maximum for every float32: a NaN (stored
 *                         value times decay, or candidate) wins and is written as 0x7FC00000, -0 counts as zero.
 *                         scratch: n floats.
 *   nfa_grid_rebinarize   thre = min(mean(occs[occs >= 0]), occ_thre) reduced on the device, binaries = occs > thre
 *                         (ref :403-404) written as the torch.bool buffer AND as the walk's 1-bit grid copy
 *                         (nfa_pack_walk_bits layout); scratch: nfa_grid_rebinarize_scratch_bytes(), on return the two
 *                         floats at byte offset nfa_grid_rebinarize_scratch_bytes() - 16 hold {thre, mean} (the first two
 *                         of its last four floats; the last two are unused). */
int nfa_grid_cell_points(const int64_t *indices, const float *jitter /*[n,3]*/, int64_t n, const int32_t *res,
                         const float *aabb /*[6]*/, float *x /*[n,3]*/, nfa_stream_t stream);
int nfa_grid_ema_update(float *occs, int64_t cell_base, const int64_t *indices, int64_t n, const float *occ,
                        float ema_decay, float *scratch /*[n]*/, nfa_stream_t stream);
int64_t nfa_grid_rebinarize_scratch_bytes(void);
int nfa_grid_rebinarize(const float *occs, int32_t n_grids, const int32_t *res, float occ_thre, uint8_t *binaries,
                        uint32_t *walk_bits, void *scratch, nfa_stream_t stream);

/* ------------------------------------------------------------------ packed segments */

/* Ownership table for the flat segmented kernels: the element range is cut into n_tiles tiles of
 * tile_elems element offsets, and after every 256 rays (nfa_seg_plan picks tile_elems and n_tiles); a tile OWNS the rays whose chunk starts
 * inside it.  tiles holds nfa_seg_table_rows(n_tiles) int64 pairs: the (n_tiles + 1) {first ray, first element} entries.  Requires
 * contiguous chunks (starts[r+1] == starts[r] + cnts[r]); flags[0] is set to 1 when they are not,
 * in which case the caller must use the *_generic entry points (flags may be NULL for a packed_info the
 * caller knows to be contiguous: no check result, and no memset launch). */
void nfa_seg_plan(int64_t n_elems, int64_t n_rays, int64_t *tile_elems, int64_t *n_tiles);
/* int64 PAIRS the caller allocates for `tiles` (n_tiles + 1 today; ask instead of assuming). */
int64_t nfa_seg_table_rows(int64_t n_tiles);
int nfa_seg_build_tiles(const int64_t *packed_info /*[n_rays,2]*/, int64_t n_rays, int64_t n_elems,
                        int64_t tile_elems, int64_t n_tiles, int64_t *tiles /*[2*(n_tiles+1)]*/,
                        int32_t *flags, nfa_stream_t stream);

/* kind: 0 inclusive_sum 1 exclusive_sum 2 inclusive_prod 3 exclusive_prod.
 * reverse != 0 scans each chunk from its last element to its first: the reverse-iterator
 * launches of ref: cuda/csrc/scan.cu:41-51,100-110 (backward of the sums).
 * ref: cuda/csrc/scan.cu:9-165,217-257; kernels include/utils_scan.cuh:28-263. */
int nfa_packed_scan(int kind, int reverse, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                    int64_t n_rays, int64_t n_elems, const float *inputs, float *outputs,
                    nfa_stream_t stream);
/* Any (start,count) chunks (overlapping, unordered, gaps), one wave per ray; also implements
 * `normalize` (ref: include/utils_scan.cuh:102-110,229-237). */
int nfa_packed_scan_generic(int kind, int reverse, int normalize, const int64_t *packed_info,
                            int64_t n_rays, int64_t n_elems, const float *inputs, float *outputs,
                            nfa_stream_t stream);
/* grad_in = reverse_{incl|excl}_sum(grad_out * outputs) / max(inputs, 1e-10)
 * ref: cuda/csrc/scan.cu:169-214 (inclusive), :259-304 (exclusive). kind: 2 or 3. */
int nfa_packed_prod_backward(int kind, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                             int64_t n_rays, int64_t n_elems, const float *inputs,
                             const float *outputs, const float *grad_outputs, float *grad_inputs,
                             nfa_stream_t stream);

/* Fused transmittance / weights.  ref: volrend.py:256-264,358-362 (density) and
 * :200-206,305-309 (alpha).  Any of weights/trans/alphas may be NULL. */
int nfa_render_from_density_fwd(const float *t_starts, const float *t_ends, const float *sigmas,
                                const float *prefix_trans /*NULL ok*/, const int64_t *packed_info,
                                const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                                float *weights, float *trans, float *alphas, nfa_stream_t stream);
int nfa_render_from_alpha_fwd(const float *alphas, const float *prefix_trans, const int64_t *packed_info,
                              const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems,
                              float *weights, float *trans, nfa_stream_t stream);
/* Backward of the fused density op given the forward's saved trans/alphas:
 *   B_k = g_w_k T_k (1-a_k) + g_a_k (1-a_k) - sum_{i>k}(g_w_i w_i + g_T_i T_i)
 *   grad_sigmas = (t_ends - t_starts) * B,  grad_x = B  (either may be NULL). */
int nfa_render_from_density_bwd(const float *t_starts, const float *t_ends, const float *trans,
                                const float *alphas, const float *g_weights, const float *g_trans,
                                const float *g_alphas, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                                int64_t n_rays, int64_t n_elems, float *grad_sigmas, float *grad_x,
                                nfa_stream_t stream);
/* PropNetEstimator's level loop for batched rows of row_len samples (ref: estimators/prop_net.py:96-107, 139-142):
 * transmittance from the proposal density AND the resampler's CDF rows `1 - cat([T, 0], -1)` ([n_rays, row_len + 1]) in
 * one pass, and the backward from the gradient at those rows (g_T = -g_cdfs[:, :-1]) to the densities.  packed_info /
 * tiles describe n_rays chunks of exactly row_len elements.  Same arithmetic as nfa_render_from_density_{fwd,bwd};
 * alphas may be NULL in both (with only g_T arriving, alpha drops out of the backward). */
int nfa_density_cdf_rows_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *packed_info,
                             const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, int32_t row_len,
                             float *trans, float *alphas, float *cdfs /*[n_rays, row_len + 1]*/, nfa_stream_t stream);
int nfa_density_cdf_rows_bwd(const float *t_starts, const float *t_ends, const float *trans, const float *alphas,
                             const float *g_cdfs /*[n_rays, row_len + 1]*/, const int64_t *packed_info, const int64_t *tiles,
                             int64_t n_tiles, int64_t n_rays, int64_t n_elems, int32_t row_len, float *grad_sigmas,
                             nfa_stream_t stream);
/*   grad_alphas_k = g_w_k T_k - sum_{i>k}(g_w_i w_i + g_T_i T_i) / max(1 - a_k, 1e-10) */
int nfa_render_from_alpha_bwd(const float *alphas, const float *trans, const float *g_weights,
                              const float *g_trans, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                              int64_t n_rays, int64_t n_elems, float *grad_alphas, nfa_stream_t stream);

/* Visibility mask (ref: volrend.py:412-418,474-480) fused with the per-ray visible count that
 * the compaction of OccGridEstimator.sampling needs (ref: estimators/occ_grid.py:216-220).
 * sigmas_or_alphas is sigma when t_starts != NULL, alpha otherwise. vis_cnts may be NULL. */
int nfa_render_visibility(const float *t_starts, const float *t_ends, const float *sigmas_or_alphas,
                          const float *prefix_trans, float early_stop_eps, float alpha_thre,
                          const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                          int64_t n_elems, uint8_t *vis, int64_t *vis_cnts, nfa_stream_t stream);
/* Constant-step samples: the `_cs` entries are their siblings with `t_ends` replaced by `step`, for samples that satisfy
 * t_ends[i] == t_starts[i] + step (one fp32 add) for every i -- what the constant-step sampler (step_size > 0, no cone
 * angle) emits.  The t_ends stream is not read (4 bytes per sample less traffic); given such samples every result is
 * bit-identical to the sibling's.  step must be finite and > 0; densities only (t_starts is required). */
int nfa_render_visibility_cs(const float *t_starts, float step, const float *sigmas, const float *prefix_trans,
                             float early_stop_eps, float alpha_thre, const int64_t *packed_info, const int64_t *tiles,
                             int64_t n_tiles, int64_t n_rays, int64_t n_elems, uint8_t *vis, int64_t *vis_cnts,
                             nfa_stream_t stream);
/* Boolean-mask compaction of (ray_indices, t_starts, t_ends) with known per-ray output offsets (ref: estimators/
 * occ_grid.py:216-220, three boolean-index gathers).  capacity: elements the output arrays hold; nothing is written at or
 * beyond it (a caller that sized them from the previous batch, before this batch's total reached the host, repeats the call
 * into larger arrays when the total turns out larger). */
int nfa_compact_samples(const uint8_t *vis, const float *t_starts, const float *t_ends,
                        const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, const int64_t *out_starts,
                        int64_t n_rays, int64_t n_elems, int64_t *out_ray_indices,
                        float *out_t_starts, float *out_t_ends, int64_t capacity, nfa_stream_t stream);

/* out[r, :] (+)= sum_i w_i * values[i, :] over ray r's chunk, deterministic order.
 * values NULL => D = 1 and out = sum w.  accumulate != 0 adds to `out` (accumulate_along_rays_).
 * ref: volrend.py:483-573 (index_add_). */
int nfa_accumulate_along_rays(const float *weights, const float *values, int32_t D,
                              const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                              int64_t n_elems, int accumulate, float *out, nfa_stream_t stream);
/* Fallback for unsorted ray_indices: atomics, same contract as index_add_. out must be initialised. */
int nfa_accumulate_along_rays_atomic(const float *weights, const float *values, int32_t D,
                                     const int64_t *ray_indices, int64_t n_rays, int64_t n_elems,
                                     float *out, nfa_stream_t stream);
/* g_w[i] = sum_c g_out[ray(i),c] v[i,c];  g_v[i,c] = g_out[ray(i),c] w[i]. */
int nfa_accumulate_along_rays_bwd(const float *weights, const float *values, int32_t D,
                                  const float *g_out, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                                  int64_t n_rays, int64_t n_elems, float *g_weights, float *g_values,
                                  nfa_stream_t stream);
/* The three accumulations of `rendering` in one pass (ref: volrend.py:140-156):
 * colors[r,3] = sum w rgb, opacities[r] = sum w, depths[r] = sum w (ts+te)/2 (un-normalised). */
int nfa_render_accumulate_fwd(const float *weights, const float *rgbs, const float *t_starts,
                              const float *t_ends, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                              int64_t n_rays, int64_t n_elems, float *colors, float *opacities,
                              float *depths, nfa_stream_t stream);
int nfa_render_accumulate_bwd(const float *weights, const float *rgbs, const float *t_starts,
                              const float *t_ends, const float *g_colors, const float *g_opacities,
                              const float *g_depths, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                              int64_t n_rays, int64_t n_elems, float *g_weights, float *g_rgbs,
                              nfa_stream_t stream);

/* `rendering` with a density callback in one pass (ref: volrend.py:109-156 = render_weight_from_density
 * + three accumulate_along_rays): per-sample weights / trans / alphas (each may be NULL) and the per-ray
 * colors[r,3], opacities[r], un-normalised depths[r].  Results are bit-identical to
 * nfa_render_from_density_fwd followed by nfa_render_accumulate_fwd. */
int nfa_render_fused_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgbs,
                         const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                         int64_t n_elems, float *weights, float *trans, float *alphas, float *colors,
                         float *opacities, float *depths, nfa_stream_t stream);
/* Its backward in one reverse pass.  g_colors[r,3] / g_opacities[r] / g_depths[r]: gradients of the per-ray
 * outputs (NULL = zero); g_weights / g_trans / g_alphas: gradients arriving at the per-sample outputs
 * (NULL = zero).  Writes grad_sigmas[n] and/or grad_rgbs[n,3]. */
int nfa_render_fused_bwd(const float *t_starts, const float *t_ends, const float *rgbs, const float *trans,
                         const float *alphas, const float *g_colors, const float *g_opacities,
                         const float *g_depths, const float *g_weights, const float *g_trans,
                         const float *g_alphas, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                         int64_t n_rays, int64_t n_elems, float *grad_sigmas, float *grad_rgbs,
                         nfa_stream_t stream);
/* The two passes for constant-step samples (see nfa_render_visibility_cs). */
int nfa_render_fused_fwd_cs(const float *t_starts, float step, const float *sigmas, const float *rgbs,
                            const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                            int64_t n_elems, float *weights, float *trans, float *alphas, float *colors,
                            float *opacities, float *depths, nfa_stream_t stream);
int nfa_render_fused_bwd_cs(const float *t_starts, float step, const float *rgbs, const float *trans,
                            const float *alphas, const float *g_colors, const float *g_opacities,
                            const float *g_depths, const float *g_weights, const float *g_trans,
                            const float *g_alphas, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                            int64_t n_rays, int64_t n_elems, float *grad_sigmas, float *grad_rgbs,
                            nfa_stream_t stream);

/* `rendering` from the field's RAW outputs (ref: volrend.py:109-151 with the activations of
 * examples/radiance_fields/ngp.py:23-36,174-175,196 applied on load): nfa_render_fused_fwd with
 *   sigma = selector ? density_act(raw_sigma + density_bias) : 0     and     rgb = rgb_act(raw_rgb).
 * density_act: NFA_ACT_NONE, NFA_ACT_TRUNC_EXP (exp(z); its derivative is exp(min(z, 15))), NFA_ACT_EXP, NFA_ACT_RELU,
 * NFA_ACT_SOFTPLUS (beta 1, threshold 20); rgb_act: NFA_RGB_ACT_NONE, NFA_RGB_ACT_SIGMOID.  selector[n] (bytes, 0 = false;
 * may be NULL = all true) is a select: a non-finite raw density behind a false entry has no effect.  act_sigmas[n] and
 * act_rgbs[n,3] (each may be NULL) receive the activated values.  With NFA_ACT_NONE, NFA_RGB_ACT_NONE, bias 0 and no
 * selector the results are bit-identical to nfa_render_fused_fwd. */
#define NFA_ACT_NONE 0
#define NFA_ACT_TRUNC_EXP 1
#define NFA_ACT_EXP 2
#define NFA_ACT_RELU 3
#define NFA_ACT_SOFTPLUS 4
#define NFA_RGB_ACT_NONE 0
#define NFA_RGB_ACT_SIGMOID 1
int nfa_render_raw_fwd(const float *t_starts, const float *t_ends, const float *raw_sigmas, const float *raw_rgbs,
                       const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act,
                       const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                       int64_t n_elems, float *weights, float *trans, float *alphas, float *act_sigmas,
                       float *act_rgbs, float *colors, float *opacities, float *depths, nfa_stream_t stream);
/* Its backward in one reverse pass, from the raw inputs and the forward's trans alone: sigma, alpha and rgb are formed
 * again with the forward's expressions and the activations' derivatives are multiplied in.  Gradient arguments as for
 * nfa_render_fused_bwd.  Writes grad_raw_sigmas[n] (exactly 0 where selector is false) and/or grad_raw_rgbs[n,3]. */
int nfa_render_raw_bwd(const float *t_starts, const float *t_ends, const float *raw_sigmas, const float *raw_rgbs,
                       const uint8_t *selector, int32_t density_act, float density_bias, int32_t rgb_act,
                       const float *trans, const float *g_colors, const float *g_opacities, const float *g_depths,
                       const float *g_weights, const float *g_trans, const float *g_alphas,
                       const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                       int64_t n_elems, float *grad_raw_sigmas, float *grad_raw_rgbs, nfa_stream_t stream);
/* The two passes with raw_sigmas / raw_rgbs, and what is written in their shape (act_sigmas / act_rgbs forward,
 * grad_raw_sigmas / grad_raw_rgbs backward), as elements of type `elem` (NFA_ELEM_*); everything else stays float32.
 * nfa_render_raw_fwd / nfa_render_raw_bwd are the NFA_ELEM_F32 case.  A half stream takes the vector form when it is
 * 8-byte aligned (and every float32 per-sample array 16-byte aligned, as above); any other address, aligned to the element
 * (2 bytes), takes the scalar form, with identical results. */
int nfa_render_raw_fwd_t(int32_t elem, const float *t_starts, const float *t_ends, const void *raw_sigmas,
                         const void *raw_rgbs, const uint8_t *selector, int32_t density_act, float density_bias,
                         int32_t rgb_act, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                         int64_t n_rays, int64_t n_elems, float *weights, float *trans, float *alphas, void *act_sigmas,
                         void *act_rgbs, float *colors, float *opacities, float *depths, nfa_stream_t stream);
int nfa_render_raw_bwd_t(int32_t elem, const float *t_starts, const float *t_ends, const void *raw_sigmas,
                         const void *raw_rgbs, const uint8_t *selector, int32_t density_act, float density_bias,
                         int32_t rgb_act, const float *trans, const float *g_colors, const float *g_opacities,
                         const float *g_depths, const float *g_weights, const float *g_trans, const float *g_alphas,
                         const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                         int64_t n_elems, void *grad_raw_sigmas, void *grad_raw_rgbs, nfa_stream_t stream);

/* `rendering` of a signed-distance field: nfa_render_fused_fwd with the SDF-to-opacity conversion applied on load.  It
 * replaces the torch composition a surface model runs in front of render_weight_from_alpha / rendering (about fifteen
 * elementwise passes each way): NeuS' alpha from the logistic CDF of the SDF at the two ends of a sample (Wang et al.
 * 2021, models/renderer.py: the `((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).clip(0, 1)` block, here without its
 * 1e-5), or VolSDF's density, the Laplace CDF of the SDF times 1 / beta (Yariv et al. 2021, model/density.py).
 * With d = t_end - t_start, r = cos_anneal_ratio, s = *param (ONE float on the device, read by the kernel: inv_s for
 * NFA_SDF_NEUS, beta for NFA_SDF_VOLSDF; both must be > 0, which is not checked), float32 throughout:
 *   NFA_SDF_NEUS    ct = -(max(0.5 - 0.5 cos, 0) (1 - r) + max(-cos, 0) r);  h = ct d / 2;  n = sdf + h;  p = sdf - h;
 *                   x = max(sp(-s n) - sp(-s p), 0),  sp(y) = max(y, 0) + log1p(exp(-|y|))
 *   NFA_SDF_VOLSDF  e = exp(-|sdf| / s) / 2;  x = (sdf >= 0 ? e : 1 - e) / s * d
 *   alpha = 1 - exp(-x),  trans = exp(-(sum of x in front of the sample)),  weight = trans alpha,
 * and colours, opacities, depths as nfa_render_fused_fwd forms them from the weights and rgb = rgb_act(raw_rgb)
 * (NFA_RGB_ACT_*).  cos[n] is read by NFA_SDF_NEUS only (NULL otherwise).  selector[n] (bytes, 0 = false; may be NULL = all
 * true) is a select: where it is false x is exactly 0 and a non-finite sdf has no effect.  weights, trans, alphas: each
 * may be NULL.  Empty rays get zeros. */
#define NFA_SDF_NEUS 0
#define NFA_SDF_VOLSDF 1
int nfa_render_sdf_fwd(const float *t_starts, const float *t_ends, const float *sdfs, const float *cos,
                       const float *raw_rgbs, const uint8_t *selector, int32_t model, const float *param,
                       float cos_anneal_ratio, int32_t rgb_act, const int64_t *packed_info, const int64_t *tiles,
                       int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *weights, float *trans, float *alphas,
                       float *colors, float *opacities, float *depths, nfa_stream_t stream);
/* Its backward in one reverse pass, from the inputs and the forward's trans alone: x, alpha and rgb are formed again
 * with the forward's expressions and dL/dx is multiplied into the derivatives of x.  Gradient arguments as for
 * nfa_render_fused_bwd.  Writes grad_sdfs[n], grad_cos[n] (NFA_SDF_NEUS only; must be NULL otherwise), grad_param[n] --
 * PER SAMPLE, dL/dx dx/d(*param): the gradient of the parameter is the sum of that stream, left to the caller, so the
 * pass has no float atomics -- and grad_raw_rgbs[n,3]; each may be NULL (not needed, then neither formed nor written),
 * not all four.  Where selector is false, and for NFA_SDF_NEUS where x is 0, all of a sample's gradients but
 * grad_raw_rgbs are exactly 0. */
int nfa_render_sdf_bwd(const float *t_starts, const float *t_ends, const float *sdfs, const float *cos,
                       const float *raw_rgbs, const uint8_t *selector, int32_t model, const float *param,
                       float cos_anneal_ratio, int32_t rgb_act, const float *trans, const float *g_colors,
                       const float *g_opacities, const float *g_depths, const float *g_weights, const float *g_trans,
                       const float *g_alphas, const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles,
                       int64_t n_rays, int64_t n_elems, float *grad_sdfs, float *grad_cos, float *grad_param,
                       float *grad_raw_rgbs, nfa_stream_t stream);

/* Mip-NeRF 360 distortion loss per ray (Barron et al. 2022, eq. 15) over samples in non-decreasing midpoint order
 * within each ray: loss[r] = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 (t_end_i - t_start_i), m = (t_start + t_end) / 2
 * (input out of that order gets what the O(n) prefix-sum form gives; it is not detected).  Also writes the per-ray totals
 * w_tot[r] = sum w_i and s_tot[r] = sum w_i (m_i - m_first(r)) the backward needs.  Empty rays get 0. */
int nfa_distortion_fwd(const float *weights, const float *t_starts, const float *t_ends, const int64_t *packed_info,
                       const int64_t *tiles, int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *loss, float *w_tot,
                       float *s_tot, nfa_stream_t stream);
/* Its backward in one reverse pass: g_loss[r] is the gradient of loss[r]; w_tot / s_tot are the forward's.  Writes
 * grad_weights[n], grad_t_starts[n], grad_t_ends[n]; each may be NULL (not needed), not all three. */
int nfa_distortion_bwd(const float *weights, const float *t_starts, const float *t_ends, const float *w_tot,
                       const float *s_tot, const float *g_loss, const int64_t *packed_info, const int64_t *tiles,
                       int64_t n_tiles, int64_t n_rays, int64_t n_elems, float *grad_weights, float *grad_t_starts,
                       float *grad_t_ends, nfa_stream_t stream);

/* One iteration of the test-mode marching loop (ref: examples/utils.py:370-405) in one pass: weights from
 * densities with prefix_trans = 1 - opacities[ray], samples with alpha < alpha_thre dropped (alpha_thre <= 0:
 * none), and colors[r,3] / opacities[r] / depths[r] accumulated in place (+=).  Deterministic (a ray is owned by
 * one wave); replaces render_weight_from_density + boolean masks + 3 accumulate_along_rays_ launches.
 * n_visible (may be NULL): NFA_VISIBLE_SLOTS counters, zeroed by the caller before the first iteration; their sum is the number
 * of samples that passed the threshold so far (the loop's running sample count; one counter would serialise the launch on
 * its address). */
#define NFA_VISIBLE_SLOTS 1024
int nfa_render_step_accumulate(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgbs,
                               const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                               int64_t n_elems, float alpha_thre, float *colors, float *opacities, float *depths,
                               int64_t *n_visible, nfa_stream_t stream);

/* ------------------------------------------------------------------ pdf */

/* ref: cuda/csrc/pdf.cu:359-421 (int overload): S >= 1 samples + S+1 edges per ray, batched outputs (S == 1, which reads
 * out of bounds upstream (:211), is defined here: the single interval is the ray's whole range).
 * Input segments batched (in_packed_info NULL, n_edges_per_ray each) or packed.
 * stratified: one Philox4x32-10 uniform per ray, subsequence = ray id (pdf.cu:139-144). */
int nfa_importance_sampling(const float *in_vals, const float *cdfs, const int64_t *in_packed_info,
                            int64_t n_rays, int64_t n_edges_per_ray, int64_t n_samples,
                            int stratified, uint64_t seed, uint64_t offset,
                            float *out_intervals /*[n_rays,S+1]*/, float *out_samples /*[n_rays,S] or NULL*/,
                            nfa_stream_t stream);
/* The same resampling with the s -> t mapping of PropNetEstimator.sampling fused in (ref: estimators/prop_net.py:215-229):
 * besides the s-space intervals, the S+1 edges mapped to metric distance are written as contiguous rows
 * t_starts[n_rays,S] / t_ends[n_rays,S].  transform 1 = uniform: t = s*t_b + (1-s)*t_a with (t_a, t_b) = (t_min, t_max);
 * 2 = lindisp: t = 1 / (s*t_b + (1-s)*t_a) with (t_a, t_b) = (1/t_min, 1/t_max).  Same fp32 operation order as the
 * reference's tensor expression. */
int nfa_importance_sampling_t(const float *in_vals, const float *cdfs, const int64_t *in_packed_info, int64_t n_rays,
                              int64_t n_edges_per_ray, int64_t n_samples, int stratified, uint64_t seed,
                              uint64_t offset, float *out_intervals, float *out_samples, int transform, float t_a,
                              float t_b, float *out_t_starts, float *out_t_ends, nfa_stream_t stream);
/* The Tensor-count overload (ref: cuda/csrc/pdf.cu:294-355, non-functional upstream: :324 allocates zero samples): ray r is
 * resampled into sm_packed_info[r].count samples and count + 1 edges (none when count == 0), PACKED at the starts given by
 * sm_packed_info / iv_packed_info ({exclusive cumsum, count} rows made by the caller: iv count = (count + 1) * (count > 0),
 * :341-342).  Per-sample arithmetic of the int overload with n = count; a single sample's interval is the ray's whole
 * range.  iv_is_left / iv_is_right as compute_intervels_kernel sets them (:205-238). */
int nfa_importance_sampling_packed(const float *in_vals, const float *cdfs, const int64_t *in_packed_info, int64_t n_rays,
                                   int64_t n_edges_per_ray, const int64_t *sm_packed_info, const int64_t *iv_packed_info,
                                   int stratified, uint64_t seed, uint64_t offset, float *sm_vals, int64_t *sm_ray_indices,
                                   float *iv_vals, int64_t *iv_ray_indices, uint8_t *iv_is_left, uint8_t *iv_is_right,
                                   nfa_stream_t stream);
/* ref: cuda/csrc/pdf.cu:245-286,426-456. Batched query => ray-relative ids. */
int nfa_searchsorted(const float *q_vals, const int64_t *q_packed_info, const int64_t *q_ray_indices,
                     int64_t q_n_rays, int64_t q_per_ray, int64_t q_total,
                     const float *k_vals, const int64_t *k_packed_info, int64_t k_per_ray,
                     int64_t *ids_left, int64_t *ids_right, nfa_stream_t stream);

/* Interlevel (proposal) loss for batched rays (ref: estimators/prop_net.py:232-256): loss[r,j] =
 * max(w - w_outer, 0)^2 / (w + eps) with w = q_cdfs[r,j+1] - q_cdfs[r,j] and w_outer the key CDF mass between the
 * key edges that enclose query interval j (the reference's searchsorted + gathers), j < n_query_edges - 1.
 * key_ids[r,j] (optional) = left | right << 16, the key edge indices, kept for the backward pass.
 * Backward: g_k_cdfs[r, n_key_edges] (required) and g_q_cdfs[r, n_query_edges] (optional); rows of <= 1024 edges. */
int nfa_pdf_loss_fwd(const float *q_vals, const float *q_cdfs, const float *k_vals, const float *k_cdfs,
                     int64_t n_rays, int32_t n_query_edges, int32_t n_key_edges, float eps, float *loss,
                     uint32_t *key_ids, nfa_stream_t stream);
int nfa_pdf_loss_bwd(const float *q_cdfs, const float *k_cdfs, const uint32_t *key_ids, int64_t n_rays,
                     int32_t n_query_edges, int32_t n_key_edges, float eps, const float *g_loss, float *g_k_cdfs,
                     float *g_q_cdfs, nfa_stream_t stream);
/* The same loss as its MEAN over all (ray, interval) pairs, which is what PropNetEstimator.compute_loss uses (ref:
 * estimators/prop_net.py:151 `.mean()`): the forward writes nfa_pdf_loss_partials(...) per-wave partial sums instead of the
 * loss array (mean = sum of partials / (n_rays * (n_query_edges - 1)); the wave -> rows assignment is fixed, so the sum is
 * deterministic), the backward takes the gradient of the mean (one device float).  Saves the loss array's write + read and
 * its expanded gradient's write + read. */
int64_t nfa_pdf_loss_partials(int64_t n_rays, int32_t n_query_edges, int32_t n_key_edges);
int nfa_pdf_loss_sum_fwd(const float *q_vals, const float *q_cdfs, const float *k_vals, const float *k_cdfs,
                         int64_t n_rays, int32_t n_query_edges, int32_t n_key_edges, float eps, float *partials,
                         uint32_t *key_ids, nfa_stream_t stream);
int nfa_pdf_loss_mean_bwd(const float *q_cdfs, const float *k_cdfs, const uint32_t *key_ids, int64_t n_rays,
                          int32_t n_query_edges, int32_t n_key_edges, float eps, const float *g_mean, float *g_k_cdfs,
                          float *g_q_cdfs, nfa_stream_t stream);

/* ------------------------------------------------------------------ cameras */

/* OpenCV lens undistortion of n_points interleaved (u, v) pairs, uv / uv_out [n_points, 2] (8-byte aligned, not
 * aliased).  params: one set of n_params floats shared by every point (param_stride 0) or one set per point
 * (param_stride == n_params).  n_params 5 {k1,k2,p1,p2,k3} and 8 {k1,k2,p1,p2,k3,k4,k5,k6}: at most `iters` Newton
 * steps, stopping when |det J| < eps or both |dx|, |dy| < eps; 12 {k1..k6,p1,p2,s1..s4}: exactly `iters` thin-prism
 * fixed-point steps (eps unused), a point whose inverse radial factor turns negative is copied unchanged.
 * ref: cuda/csrc/camera.cu:37-107,114-147 (declared at nerfacc.cpp:88-92). */
int nfa_opencv_lens_undistortion(const float *uv, const float *params, int64_t n_points, int32_t n_params,
                                 int64_t param_stride, float eps, int32_t iters, float *uv_out, nfa_stream_t stream);
/* Fisheye undistortion, n_params 4 {k1,k2,k3,k4}: at most `iters` Newton steps on theta, stopping when |step| < eps.
 * A point that does not converge or whose theta flips sign, and a point with |uv| <= eps, is copied unchanged (the
 * reference leaves the former unwritten and writes 0 for the latter).
 * ref: cuda/csrc/camera.cu:9-35,149-183 (declared at nerfacc.cpp:93-97). */
int nfa_opencv_lens_undistortion_fisheye(const float *uv, const float *params, int64_t n_points, int32_t n_params,
                                         int64_t param_stride, float eps, int32_t iters, float *uv_out,
                                         nfa_stream_t stream);

/* ------------------------------------------------------------------ input encodings */

/* tiny-cuda-nn's `HashGrid` encoding (Instant-NGP's multiresolution hash grid, Mueller et al. 2022) with 3-D input and
 * linear interpolation (smoothstep: the `_i` entries below); the formulas are those of csrc/encoding.hip's header.
 * x [n_points, 3], y [n_points, n_levels * n_features], params the flat [sum(sizes) * n_features] table laid out
 * [level][entry][feature].  The level table
 * (n_levels entries each, host memory) is computed by the caller in float32: scale_l = exp2f(l log2f(per_level_scale)) *
 * base_resolution - 1, resolution_l = ceil(scale_l) + 1, size_l = min(roundup8(resolution_l^3), 2^log2_hashmap_size);
 * a size that does not follow from the resolution is rejected.  n_features 1, 2, 4 or 8, n_levels 1..32,
 * log2_hashmap_size 10..24, n_params = sum(sizes) * n_features < 2^31.  Every index is reduced modulo the level's size,
 * so any input (non-finite included) stays inside the table. */
int nfa_hashgrid_fwd(const float *x, const float *params, int64_t n_points, int32_t n_levels, int32_t n_features,
                     int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                     const int32_t *sizes_host, int64_t n_params, float *y, nfa_stream_t stream);
/* Backward of nfa_hashgrid_fwd given grad_y [n_points, n_levels * n_features]: grad_params (optional, ZEROED by the
 * caller) receives the scatter of w_c * grad_y through float atomics (the order of the adds is not fixed); grad_x
 * (optional, needs params) [n_points, 3] is written, summed over levels in level order (bitwise reproducible).  At
 * least one of the two is given. */
int nfa_hashgrid_bwd(const float *x, const float *params, const float *grad_y, int64_t n_points, int32_t n_levels,
                     int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                     const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                     float *grad_x, nfa_stream_t stream);
/* Second order: the backward of nfa_hashgrid_bwd's grad_x output (the formulas are in csrc/encoding.hip's header, "Second
 * order").  grad_grad_x [n_points, 3] (required) is the gradient that arrives for grad_x.  Outputs, each optional, at least
 * one: grad_grad_y [n_points, n_levels * n_features] (towards grad_y; needs params) is written; grad_params (towards params;
 * ZEROED by the caller, needs grad_y) receives float atomic adds like nfa_hashgrid_bwd's; grad_x [n_points, 3] (towards x:
 * the mixed second partials; needs params and grad_y) is written, summed over levels in level order.  grad_grad_y and
 * grad_x are bitwise reproducible.  The derivative of nfa_hashgrid_bwd's grad_params output is not provided. */
int nfa_hashgrid_bwd_bwd(const float *x, const float *params, const float *grad_y, const float *grad_grad_x, int64_t n_points,
                         int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                         const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_grad_y,
                         float *grad_params, float *grad_x, nfa_stream_t stream);
/* tiny-cuda-nn's `SphericalHarmonics` encoding: directions dirs [n_points, 3] in [0, 1]^3, u = 2 dirs - 1 (not
 * renormalised), degree 1..4, out [n_points, degree^2] (16-byte aligned) with Instant-NGP's real SH basis and constants.
 * The backward writes grad_dirs [n_points, 3] from grad_out [n_points, degree^2] (16-byte aligned). */
int nfa_sh_fwd(const float *dirs, int64_t n_points, int32_t degree, float *out, nfa_stream_t stream);
int nfa_sh_bwd(const float *dirs, const float *grad_out, int64_t n_points, int32_t degree, float *grad_dirs,
               nfa_stream_t stream);
/* The four encoding passes with y / grad_y and out / grad_out as elements of type `elem` (NFA_ELEM_*): a point's
 * n_features values of a level, and a direction's row, are converted once and moved as one vector.  x, dirs, params and
 * every gradient written stay float32.  The entries above are the NFA_ELEM_F32 case, with what they ask of their
 * pointers; half y, grad_y, out and grad_out must be 16-byte aligned. */
int nfa_hashgrid_fwd_t(int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_levels,
                       int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, void *y,
                       nfa_stream_t stream);
int nfa_hashgrid_bwd_t(int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                       int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                       float *grad_x, nfa_stream_t stream);
/* nfa_hashgrid_bwd_bwd with grad_y and grad_grad_y as elements of type `elem` (half: both 16-byte aligned). */
int nfa_hashgrid_bwd_bwd_t(int32_t elem, const float *x, const float *params, const void *grad_y, const float *grad_grad_x,
                           int64_t n_points, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                           const float *scales_host, const int32_t *resolutions_host, const int32_t *sizes_host,
                           int64_t n_params, void *grad_grad_y, float *grad_params, float *grad_x, nfa_stream_t stream);
/* The two hash-grid backward passes with a bitwise reproducible table gradient: arguments and results of
 * nfa_hashgrid_bwd_t / nfa_hashgrid_bwd_bwd_t (elem: any NFA_ELEM_* code, NFA_ELEM_F32 included), except that grad_params
 * (ZEROED by the caller) is formed without float atomics, in an order that depends on the arguments alone.  Per level:
 *   items i = 8 n + c (point n, corner c) carry the corner's entry index as key and are sorted by key with a stable radix
 *   sort, so equal keys stay in ascending point and then corner; the sorted array is cut into tiles of 256 items; the part
 *   of a run of equal keys inside one tile (a segment) is summed from its first term, left to right; a run inside one tile
 *   is its segment; a run across tile borders is the sum of its segments' sums in tile order, from the first one's.
 *   Each term is the float32 value the atomic pass adds: ((w0 w1) w2) grad_y[j], at second order a_c grad_y[j].
 * Entries that receive nothing are not written.  grad_x, grad_grad_y come from the passes above, unchanged.
 * scratch (device memory, 16-byte aligned, contents irrelevant before and after) holds scratch_bytes >=
 * nfa_hashgrid_sorted_scratch_bytes(n_points, n_levels, log2_hashmap_size) bytes:
 *   M = 8 n_points, level_bytes = 16 M + 1024 (ceil(M / 4096) + 1) + 64 ceil(M / 256),
 *   bytes = n_levels level_bytes where that is at most 2^29, else max(2^29, level_bytes); 0 for no points.  (The levels are
 *   sorted min(n_levels, max(1, floor(2^29 / level_bytes))) at a time, one slab each.)
 * 8 n_points must be below 2^32.  Without grad_params the calls are nfa_hashgrid_bwd_t / nfa_hashgrid_bwd_bwd_t and scratch
 * is not looked at.  Nothing is read back from the device; the launches follow from the arguments alone. */
int64_t nfa_hashgrid_sorted_scratch_bytes(int64_t n_points, int32_t n_levels, int32_t log2_hashmap_size);
int nfa_hashgrid_bwd_sorted(int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                            int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                            const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, float *grad_params,
                            float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream);
int nfa_hashgrid_bwd_bwd_sorted(int32_t elem, const float *x, const float *params, const void *grad_y,
                                const float *grad_grad_x, int64_t n_points, int32_t n_levels, int32_t n_features,
                                int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                                const int32_t *sizes_host, int64_t n_params, void *grad_grad_y, float *grad_params,
                                float *grad_x, void *scratch, int64_t scratch_bytes, nfa_stream_t stream);
/* The five hash-grid passes with the interpolation as a leading argument; everything else as in nfa_hashgrid_fwd_t,
 * nfa_hashgrid_bwd_t, nfa_hashgrid_bwd_bwd_t, nfa_hashgrid_bwd_sorted and nfa_hashgrid_bwd_bwd_sorted, which are the
 * NFA_INTERP_LINEAR case.  NFA_INTERP_SMOOTHSTEP is tiny-cuda-nn's "interpolation": "Smoothstep": the corner weights are
 * formed from S(f) = f^2 (3 - 2 f) instead of the fraction f, so the encoding is C^1 across cell faces and grad_x of the
 * second order gains the pure second partials (S'' = 6 - 12 f) next to the mixed ones; the operations, in float32 and in a
 * fixed order, are in csrc/encoding.hip's header, "Smoothstep interpolation".  What is bitwise reproducible, the order of
 * the sorted table gradient (with the smoothstep coefficient in place of the linear one) and the scratch are unchanged.
 * Any other interp is NFA_EINVAL, checked before every other argument. */
#define NFA_INTERP_LINEAR 0
#define NFA_INTERP_SMOOTHSTEP 1
int nfa_hashgrid_fwd_i(int32_t interp, int32_t elem, const float *x, const float *params, int64_t n_points,
                       int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, void *y,
                       nfa_stream_t stream);
int nfa_hashgrid_bwd_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                       int64_t n_points, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                       const float *scales_host, const int32_t *resolutions_host, const int32_t *sizes_host,
                       int64_t n_params, float *grad_params, float *grad_x, nfa_stream_t stream);
int nfa_hashgrid_bwd_bwd_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                           const float *grad_grad_x, int64_t n_points, int32_t n_levels, int32_t n_features,
                           int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                           const int32_t *sizes_host, int64_t n_params, void *grad_grad_y, float *grad_params,
                           float *grad_x, nfa_stream_t stream);
int nfa_hashgrid_bwd_sorted_i(int32_t interp, int32_t elem, const float *x, const float *params, const void *grad_y,
                              int64_t n_points, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                              const float *scales_host, const int32_t *resolutions_host, const int32_t *sizes_host,
                              int64_t n_params, float *grad_params, float *grad_x, void *scratch,
                              int64_t scratch_bytes, nfa_stream_t stream);
int nfa_hashgrid_bwd_bwd_sorted_i(int32_t interp, int32_t elem, const float *x, const float *params,
                                  const void *grad_y, const float *grad_grad_x, int64_t n_points, int32_t n_levels,
                                  int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                                  const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params,
                                  void *grad_grad_y, float *grad_params, float *grad_x, void *scratch,
                                  int64_t scratch_bytes, nfa_stream_t stream);
/* The forward, the first-order backward and its sorted form with the number of input dimensions as a leading argument:
 * tiny-cuda-nn's `GridEncoding<T, N_POS_DIMS, N_FEATURES_PER_LEVEL, HASH_TYPE>` (grid type Hash, CoherentPrime hash,
 * include/tiny-cuda-nn/encodings/grid.h) for N_POS_DIMS = n_dims = 2, 3 or 4: `kernel_grid` (forward), `kernel_grid_backward`
 * (table gradient) and `kernel_grid_backward_input` (grad_x).  n_dims = 3 is nfa_hashgrid_fwd_i, nfa_hashgrid_bwd_i and
 * nfa_hashgrid_bwd_sorted_i, bit for bit; those and every entry above are its n_dims = 3 case.  For n_dims = 2 and 4, per
 * csrc/encoding.hip's header, "Other dimensions":
 *   x and grad_x are [n_points, n_dims], contiguous, and must be 16-byte aligned (a point is one 8- or 16-byte access);
 *   a corner is c = sum_d c_d 2^d, visited in the order 0 .. 2^n_dims - 1, its weight the left-associated product of the
 *   first n_dims factors; a hashed level's index is q0 ^ q1 2654435761 ^ q2 805459861 ^ q3 3674653429 (the first n_dims
 *   terms) masked to the level, a dense level's (sum_d q_d res^d mod 2^32) mod size;
 *   size_l = min(roundup8(resolution_l^n_dims), 2^log2_hashmap_size), which the level table handed in must satisfy (scales
 *   and resolutions do not depend on n_dims);
 *   the sorted table gradient numbers its items i = 2^n_dims n + c: M = 2^n_dims n_points in the scratch formula above, and
 *   2^n_dims n_points must be below 2^32.
 * Everything else (interp, elem, which outputs are optional, what is bitwise reproducible) is as in the `_i` entries.  Any
 * other n_dims is NFA_EINVAL (nfa_hashgrid_sorted_scratch_bytes_d: -1) with a message that names the value.  The second
 * order exists for n_dims = 3 only. */
int nfa_hashgrid_fwd_d(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const float *params, int64_t n_points,
                       int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, const float *scales_host,
                       const int32_t *resolutions_host, const int32_t *sizes_host, int64_t n_params, void *y,
                       nfa_stream_t stream);
int nfa_hashgrid_bwd_d(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const float *params,
                       const void *grad_y, int64_t n_points, int32_t n_levels, int32_t n_features,
                       int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                       const int32_t *sizes_host, int64_t n_params, float *grad_params, float *grad_x, nfa_stream_t stream);
int nfa_hashgrid_bwd_sorted_d(int32_t n_dims, int32_t interp, int32_t elem, const float *x, const float *params,
                              const void *grad_y, int64_t n_points, int32_t n_levels, int32_t n_features,
                              int32_t log2_hashmap_size, const float *scales_host, const int32_t *resolutions_host,
                              const int32_t *sizes_host, int64_t n_params, float *grad_params, float *grad_x,
                              void *scratch, int64_t scratch_bytes, nfa_stream_t stream);
int64_t nfa_hashgrid_sorted_scratch_bytes_d(int32_t n_dims, int64_t n_points, int32_t n_levels, int32_t log2_hashmap_size);
int nfa_sh_fwd_t(int32_t elem, const float *dirs, int64_t n_points, int32_t degree, void *out, nfa_stream_t stream);
int nfa_sh_bwd_t(int32_t elem, const float *dirs, const void *grad_out, int64_t n_points, int32_t degree,
                 float *grad_dirs, nfa_stream_t stream);

/* The plane-factorised multiscale encoding of K-Planes (Fridovich-Keil et al. 2023; `interpolate_ms_features` with
 * concat_features = True) for n_dims = 3 (3 planes) or 4 (6 planes, axis 3 is time), x [n_points, n_dims] in [0, 1]
 * (K-Planes' u in [-1, 1] is x = (u + 1) / 2).  The planes of a scale are the axis pairs (a, b), a < b, in lexicographic
 * order.  res_host: n_scales * n_dims host ints read during the call, res_host[s * n_dims + d] = R_{s,d} >= 2, the nodes
 * of scale s along axis d.  params: one float32 table; plane (s, k) is a row-major [R_{s,b}, R_{s,a}, n_features] block,
 * the blocks in scale-major, then plane order without gaps (fewer than 2^31 floats in all).  A plane is sampled
 * bilinearly with the border rule of grid_sample(padding_mode="border", align_corners=True): node coordinate x_d (R - 1)
 * clamped to [0, R - 1] (NaN to 0), so every input reads and writes inside its planes.  The planes' samples of a scale are
 * multiplied (reduce = NFA_PLANE_PRODUCT) or added (NFA_PLANE_SUM) in plane order; y [n_points, n_scales * n_features],
 * scale-major, as elements of type `elem` (NFA_ELEM_*; float32 arithmetic, rounded once).  n_features: 4, 8, 16 or 32;
 * n_scales: 1..8.  Every operation is written out in csrc/planes.hip's header.
 * nfa_planegrid_bwd: grad_y [n_points, n_scales * n_features] in `elem`; grad_params (the table's size, float32, zeroed
 * by the caller; float atomics, so its last bits depend on the arrival order) and grad_x [n_points, n_dims] (no atomics:
 * bitwise reproducible; 0 on an axis whose coordinate is outside [0, 1] or not finite) are each optional, at least one.
 * The samples are recomputed from x and params.  No pointer needs more than its element's alignment.
 * n_points == 0 returns NFA_OK before anything else is looked at.  Otherwise the arguments are checked in this order, each
 * with its own message, before any launch: n_points, n_dims, reduce, elem, n_features, n_scales, res_host (null; a
 * resolution below 2; the size limit), null pointers. */
#define NFA_PLANE_PRODUCT 0
#define NFA_PLANE_SUM 1
int nfa_planegrid_fwd(int32_t n_dims, int32_t reduce, int32_t elem, const float *x, const float *params, int64_t n_points,
                      int32_t n_scales, int32_t n_features, const int32_t *res_host, void *y, nfa_stream_t stream);
int nfa_planegrid_bwd(int32_t n_dims, int32_t reduce, int32_t elem, const float *x, const float *params, const void *grad_y,
                      int64_t n_points, int32_t n_scales, int32_t n_features, const int32_t *res_host, float *grad_params,
                      float *grad_x, nfa_stream_t stream);

/* The regularisers K-Planes puts on the plane tables themselves, over the plane grid above (same n_dims, n_scales,
 * n_features, res_host and params layout).  Plane (s, k) seen as p[j, i, f], j < H = R_{s,b} rows, i < W = R_{s,a}, f < F:
 *   tv_h   = sum (p[j+1,i,f] - p[j,i,f])^2 / (F (H-1) W)          tv_w = sum (p[j,i+1,f] - p[j,i,f])^2 / (F H (W-1))
 *   smooth = sum ((p[j+2,i,f] - p[j+1,i,f]) - (p[j+1,i,f] - p[j,i,f]))^2 / (F (H-2) W)      (0 when H = 2)
 *   l1     = sum |1 - p[j,i,f]| / (F H W)
 * smooth and l1 exist on the time planes only (b == 3: planes 2, 4, 5 at n_dims = 4, the rows are the time axis); on a
 * spatial plane they are 0 and their incoming gradients are not looked at.
 * nfa_planereg_fwd: terms [n_scales, n_planes, 4] = (tv_h, tv_w, smooth, l1) per plane, two launches (per-tile sums into
 * partials, then one workgroup per plane), no atomics: the same bits on every run; the order of the sums is in
 * csrc/planereg.hip's header.  partials: device scratch of n_partials >= nfa_planereg_partials(n_dims, n_scales,
 * n_features, res_host) rows of 4 floats, contents irrelevant before and after.  nfa_planereg_partials is host-only
 * arithmetic on the shape (-1 with a message for a shape the passes refuse).
 * nfa_planereg_bwd: grad_terms [n_scales, n_planes, 4], a DEVICE pointer; grad_params (the table's size) receives
 * sum_t grad_terms[s, k, t] d terms[s, k, t] / d params in one launch with plain stores: every element is written (the
 * caller need not zero it) and the result is bitwise reproducible.  d |1 - p| / dp is 0 at p == 1.  NaN and Inf
 * parameters propagate; no index depends on data and nothing is read back from the device.
 * params, partials, terms and grad_params must be 16-byte aligned (every plane starts on a 16-byte piece of params).
 * The arguments are checked in this order, each with its own message, before any launch: n_dims, n_features, n_scales,
 * res_host (null; a resolution below 2; the size limit), null pointers, alignment, n_partials. */
int64_t nfa_planereg_partials(int32_t n_dims, int32_t n_scales, int32_t n_features, const int32_t *res_host);
int nfa_planereg_fwd(int32_t n_dims, const float *params, int32_t n_scales, int32_t n_features, const int32_t *res_host,
                     float *partials, int64_t n_partials, float *terms, nfa_stream_t stream);
int nfa_planereg_bwd(int32_t n_dims, const float *params, int32_t n_scales, int32_t n_features, const int32_t *res_host,
                     const float *grad_terms, float *grad_params, nfa_stream_t stream);

/* The vector-matrix (VM) decomposition of TensoRF (Chen et al. 2022; `TensorVMSplit`), x [n_points, 3] in [0, 1] (TensoRF's
 * u in [-1, 1] is x = (u + 1) / 2).  Modes m = 0, 1, 2: plane axes (a, b) = (0,1) (0,2) (1,2) (matMode), line axis c = 2, 1, 0
 * (vecMode).  res_host: 3 host ints read during the call, R_d >= 2 nodes along axis d.  n_components C: a multiple of 4 in
 * 4..96, the same for every mode.  params: one float32 table without gaps (fewer than 2^31 floats); for m in order the plane,
 * a row-major [R_b, R_a, C] block, then the line, a [R_c, C] block.  Plane and line are sampled bilinearly / linearly with
 * the border rule of grid_sample(padding_mode="border", align_corners=True) (node coordinate x_d (R - 1) clamped to
 * [0, R - 1], NaN to 0: every input reads and writes inside its blocks) and multiplied: t_m[j] = plane_m[j] * line_m[j].
 * reduce = NFA_VM_CONCAT: y [n_points, 3 C], y[n, m C + j] = t_m[j] (compute_appfeature before basis_mat);
 * NFA_VM_SUM: y [n_points, 1], the sum of all 3 C terms in the fixed order of csrc/vmgrid.hip's header
 * (compute_densityfeature).  y holds elements of type `elem` (NFA_ELEM_*; float32 arithmetic, rounded once).
 * nfa_vmgrid_bwd: grad_y in y's shape and `elem`; grad_params (the table's size, float32, zeroed by the caller; float
 * atomics -- the line blocks through a per-workgroup copy in LDS while a line fits 64 KiB -- so its last bits depend on the
 * arrival order) and grad_x [n_points, 3] (no atomics: bitwise reproducible; 0 on an axis whose coordinate is outside [0, 1]
 * or not finite) are each optional, at least one.  The samples are recomputed from x and params.  No pointer needs more
 * than its element's alignment.
 * n_points == 0 returns NFA_OK before anything else is looked at.  Otherwise the arguments are checked in this order, each
 * with its own message, before any launch: n_points, reduce, elem, n_components, res_host (null; a resolution below 2; the
 * size limit), null pointers.
 * nfa_vmgrid_resample (`up_sampling_VM`): dst_params, a table of the same layout at the resolution dst_res_host, receives
 * at every node of every plane and line the bilinear / linear sample of src_params' block at, per axis,
 * (float)i' * ((float)(R - 1) / (float)(R' - 1)): F.interpolate(mode="bilinear", align_corners=True).  Up, down or
 * unchanged, each axis on its own; equal resolutions copy (finite values).  The tables must not overlap.  Checked in this
 * order: n_components, the resolution tables (null; a source, then a destination resolution below 2 or beyond the size
 * limit), null pointers. */
#define NFA_VM_CONCAT 0
#define NFA_VM_SUM 1
int nfa_vmgrid_fwd(int32_t reduce, int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_components,
                   const int32_t *res_host, void *y, nfa_stream_t stream);
int nfa_vmgrid_bwd(int32_t reduce, int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points,
                   int32_t n_components, const int32_t *res_host, float *grad_params, float *grad_x, nfa_stream_t stream);
int nfa_vmgrid_resample(const float *src_params, const int32_t *src_res_host, float *dst_params, const int32_t *dst_res_host,
                        int32_t n_components, nfa_stream_t stream);

/* A dense 3-D feature grid sampled trilinearly (DVGO's density and feature grids, TiNeuVox's feature volume with
 * `mult_dist_interp`), x [n_points, 3] in [0, 1].  res_host: 3 host ints (R_x, R_y, R_z) read during the call, every one >= 2.
 * n_features C: 1, 2 or a multiple of 4 up to 64.  params: one float32 table of fewer than 2^31 floats, a row-major
 * [R_z, R_y, R_x, C] block (x fastest among the nodes, a node's C values contiguous); it may exceed 4 GiB.  strides_host:
 * n_strides (1..4) host ints in 1..8 read during the call; stride s has the nodes at the table indices 0, s, 2 s, .. per axis,
 * n_d = ceil(R_d / s) >= 2 of them (the view [::s, ::s, ::s]), sampled with the border rule of grid_sample(
 * padding_mode="border", align_corners=True) (node coordinate x_d (n_d - 1) clamped to [0, n_d - 1], NaN to 0: every input
 * reads and writes inside the table).  y [n_points, n_strides C], stride k at the columns k C .. k C + C - 1, elements of
 * type `elem` (NFA_ELEM_*; float32 arithmetic in the order of csrc/voxgrid.hip's header, rounded once).
 * nfa_voxgrid_bwd: grad_y in y's shape and `elem`; grad_params (the table's size, float32, zeroed by the caller; float
 * atomics, so its last bits depend on the arrival order) and grad_x [n_points, 3] (no atomics: bitwise reproducible; 0 on an
 * axis whose coordinate is outside [0, 1] or not finite) are each optional, at least one.  The samples are recomputed from
 * x and params.  No pointer needs more than its element's alignment.
 * n_points == 0 returns NFA_OK before anything else is looked at.  Otherwise the arguments are checked in this order, each
 * with its own message, before any launch: n_points, elem, n_features, res_host (null; a resolution below 2; the size
 * limit), n_strides, strides_host (null; a stride outside 1..8; fewer than 2 nodes), null pointers.
 * nfa_voxgrid_resample (DVGO's `scale_volume_grid`): dst_params, a table of the same layout at the resolution dst_res_host,
 * receives at every node the trilinear sample of src_params at, per axis, (float)i' * ((float)(R - 1) / (float)(R' - 1)):
 * F.interpolate(mode="trilinear", align_corners=True).  Up, down or unchanged, each axis on its own; equal resolutions copy
 * (finite values).  The tables must not overlap.  Checked in this order: n_features, the resolution tables (the source, then
 * the destination: null; a resolution below 2; the size limit), null pointers. */
int nfa_voxgrid_fwd(int32_t elem, const float *x, const float *params, int64_t n_points, int32_t n_features, const int32_t *res_host,
                    int32_t n_strides, const int32_t *strides_host, void *y, nfa_stream_t stream);
int nfa_voxgrid_bwd(int32_t elem, const float *x, const float *params, const void *grad_y, int64_t n_points, int32_t n_features,
                    const int32_t *res_host, int32_t n_strides, const int32_t *strides_host, float *grad_params, float *grad_x,
                    nfa_stream_t stream);
int nfa_voxgrid_resample(const float *src_params, const int32_t *src_res_host, float *dst_params, const int32_t *dst_res_host,
                         int32_t n_features, nfa_stream_t stream);

/* The regularisers TensoRF puts on the VM tables themselves, over the VM grid above (same n_components, res_host and params
 * layout).  Mode m with its plane seen as p[j, i, k], j < H = R_b rows, i < W = R_a, k < C, and its line as l[r, k], r < R = R_c:
 *   tv_h     = sum (p[j+1,i,k] - p[j,i,k])^2 / (C (H-1) W)         tv_line = sum (l[r+1,k] - l[r,k])^2 / (C (R-1))
 *   tv_w     = sum (p[j,i+1,k] - p[j,i,k])^2 / (C H (W-1))         l1_line = sum |l[r,k]| / (C R)
 *   l1_plane = sum |p[j,i,k]| / (C H W)                            ortho   = sum_{i<j} |G_ij| / (C (C-1) / 2)
 *   G_ij = sum_r l[r,i] l[r,j], r ascending from 0
 * (TensorVMSplit: TVLoss of a plane is 2 (tv_h + tv_w), density_L1 is sum_m (l1_plane + l1_line), vector_comp_diffs is
 * sum_m ortho.)
 * nfa_vmreg_fwd: terms [3, 6] = (tv_h, tv_w, l1_plane, tv_line, l1_line, ortho) per mode, two launches (per-tile sums of the
 * planes into partials, then one workgroup per mode), no atomics: the same bits on every run; the order of the sums is in
 * csrc/vmreg.hip's header.  partials: device scratch of n_partials >= nfa_vmreg_partials(n_components, res_host) rows of 4
 * floats, contents irrelevant before and after.  signs [3, C, C] receives sign(G_ij) (0 at 0, NaN stays NaN; the diagonal
 * is 0), which nfa_vmreg_bwd reads back: hand it the buffer of the forward over the same params.  nfa_vmreg_partials is
 * host-only arithmetic on the shape (-1 with a message for a shape the passes refuse).
 * nfa_vmreg_bwd: grad_terms [3, 6], a DEVICE pointer; grad_params (the table's size) receives sum_t grad_terms[m, t]
 * d terms[m, t] / d params in one launch with plain stores: every element is written (the caller need not zero it) and the
 * result is bitwise reproducible.  d |v| / dv is 0 at v == 0; d ortho / d l[r,i] = sum_{j != i} signs[m,i,j] l[r,j] / (C (C-1)
 * / 2).  NaN and Inf parameters propagate within their mode; no index depends on data and nothing is read back from the
 * device.  params, partials, signs and grad_params must be 16-byte aligned (every block starts on a 16-byte piece of params).
 * The arguments are checked in this order, each with its own message, before any launch: n_components, res_host (null; a
 * resolution below 2; the size limit), null pointers, alignment, n_partials. */
int64_t nfa_vmreg_partials(int32_t n_components, const int32_t *res_host);
int nfa_vmreg_fwd(const float *params, int32_t n_components, const int32_t *res_host, float *partials, int64_t n_partials,
                  float *signs, float *terms, nfa_stream_t stream);
int nfa_vmreg_bwd(const float *params, int32_t n_components, const int32_t *res_host, const float *grad_terms, const float *signs,
                  float *grad_params, nfa_stream_t stream);

/* The regularisers of the dense voxel grid above (same n_features, res_host and params layout; the base table, whatever the
 * strides): total variation along x, y and z under a penalty rho chosen by `kind`, and the L1 pull towards 0.  With the table
 * seen as g[z, y, x, c]:
 *   NFA_VOXREG_L2: rho(d) = d^2;  NFA_VOXREG_L1: |d|;  NFA_VOXREG_HUBER: d^2 / 2 for |d| <= 1, else |d| - 1/2 (smooth L1, beta 1)
 *   tv_x = sum rho(g[z,y,x+1,c] - g[z,y,x,c]) / n_x,  n_x = C R_z R_y (R_x - 1)        likewise tv_y, tv_z
 *   l1   = sum |g| / (C R_z R_y R_x)
 * `reduction`: NFA_VOXREG_MEAN divides by the counts as written, NFA_VOXREG_SUM by 1.  These formulas are the contract.
 * nfa_voxreg_fwd: terms [4] = (tv_x, tv_y, tv_z, l1), two launches (per-workgroup sums into partials, then one workgroup), no
 * atomics: the same bits on every run; the order of the sums and the longest chain of additions (184) are in
 * csrc/voxreg.hip's header.  partials: device scratch of n_partials >= nfa_voxreg_partials(n_features, res_host) rows of 4
 * floats, contents irrelevant before and after.  nfa_voxreg_partials is host-only arithmetic on the shape (-1 with a message
 * for a shape the passes refuse).
 * nfa_voxreg_bwd: grad_terms [4], a DEVICE pointer; grad_params (the table's size) receives sum_t grad_terms[t] d terms[t] / d
 * params in one launch with plain stores: every element is written (the caller need not zero it) and the result is bitwise
 * reproducible.  The derivative of |v| is 0 at 0, that of the Huber penalty clamp(d, -1, 1).
 * nfa_voxreg_add_grad (the form of DVGO's `total_variation_add_grad`): weights [4], a HOST pointer read during the call, take
 * grad_terms' place; grad (the table's size) becomes grad + that gradient, in place, in one launch, where dense != 0 or the
 * element of grad is not 0 (a NaN is not 0); elsewhere it keeps its bits.  The value added has the bits nfa_voxreg_bwd
 * writes for grad_terms = weights.
 * NaN and Inf parameters reach the terms and the elements whose stencil touches them; no index depends on data and nothing
 * is read back from the device.  params, partials, grad_params and grad must be 16-byte aligned; the table may exceed 4 GiB.
 * The arguments are checked in this order, each with its own message, before any launch: n_features, res_host (null; a
 * resolution below 2; the size limit), kind, reduction, null pointers, alignment, n_partials. */
#define NFA_VOXREG_L2 0
#define NFA_VOXREG_L1 1
#define NFA_VOXREG_HUBER 2
#define NFA_VOXREG_MEAN 0
#define NFA_VOXREG_SUM 1
int64_t nfa_voxreg_partials(int32_t n_features, const int32_t *res_host);
int nfa_voxreg_fwd(const float *params, int32_t n_features, const int32_t *res_host, int32_t kind, int32_t reduction, float *partials,
                   int64_t n_partials, float *terms, nfa_stream_t stream);
int nfa_voxreg_bwd(const float *params, int32_t n_features, const int32_t *res_host, int32_t kind, int32_t reduction,
                   const float *grad_terms, float *grad_params, nfa_stream_t stream);
int nfa_voxreg_add_grad(const float *params, int32_t n_features, const int32_t *res_host, int32_t kind, int32_t reduction,
                        const float *weights, int32_t dense, float *grad, nfa_stream_t stream);

/* NeRF's sinusoidal (positional) encoding (ref: examples/radiance_fields/mlp.py, SinusoidalEncoder) of x [n_points, n_dims],
 * n_dims D in 1..4, with the n_freqs L in 0..16 frequencies s_k = 2^(min_deg + k) (-16 <= min_deg, min_deg + L <= 32).  A row
 * has K = (identity ? D : 0) + 2 L D columns in the reference's order: x (identity != 0; bitwise copies), then
 * a_kd sin(s_k x_d) at column k D + d of the sine block, then a_kd cos(s_k x_d) in the same order;
 * a_kd = w_k exp(-1/2 s_k^2 var[n, d]) with w = freq_weights [L] (device float32; NULL: 1) and var [n_points, D] (NULL:
 * no factor; mip-NeRF's integrated encoding with a diagonal covariance).  The cosine is evaluated itself, not as the
 * reference's sin(fl32(s_k x + pi/2)); sine, cosine and exp are the device library's accurate functions, float32 throughout.
 * out / grad_out / grad_grad_out [n_points, K] hold elements of type `elem` (NFA_ELEM_*; rounded once as stored) and must be
 * 16-byte aligned: they move as contiguous 16-byte (float32) or 8-byte (halves) pieces.  Everything else is float32.
 * nfa_sinenc_bwd: grad_x [n_points, D] = g_id + sum_k s_k a_kd (g_sin cos - g_cos sin) and grad_var [n_points, D] =
 * -1/2 sum_k s_k^2 (g_sin out_sin + g_cos out_cos), each optional, at least one (grad_var needs var).
 * nfa_sinenc_bwd_bwd (no var): for gg_x [n_points, D], grad_grad_out (identity gg_x, sine gg_x s_k w_k cos, cosine
 * -gg_x s_k w_k sin) and grad_x [n_points, D] = -gg_x sum_k s_k^2 w_k (g_sin sin + g_cos cos), each optional, at least one.
 * Every sum runs in a fixed order in one lane: no atomics, bitwise reproducible; nothing is read back or allocated.
 * The arguments are checked in this order, each with its own message, before any HIP call: elem, n_dims, n_freqs, min_deg,
 * n_points (negative; above 2^31 - 1); then n_points == 0 (or K == 0) returns NFA_OK; then null pointers, alignment. */
int nfa_sinenc_fwd(int32_t elem, const float *x, const float *var, const float *freq_weights, int64_t n_points, int32_t n_dims,
                   int32_t min_deg, int32_t n_freqs, int32_t identity, void *out, nfa_stream_t stream);
int nfa_sinenc_bwd(int32_t elem, const float *x, const float *var, const float *freq_weights, const void *grad_out, int64_t n_points,
                   int32_t n_dims, int32_t min_deg, int32_t n_freqs, int32_t identity, float *grad_x, float *grad_var,
                   nfa_stream_t stream);
int nfa_sinenc_bwd_bwd(int32_t elem, const float *x, const float *freq_weights, const void *grad_out, const float *gg_x,
                       int64_t n_points, int32_t n_dims, int32_t min_deg, int32_t n_freqs, int32_t identity, void *grad_grad_out,
                       float *grad_x, nfa_stream_t stream);

/* ------------------------------------------------------------------ sample positions */

/* What every field does between sampling() and its encodings, in one pass over the samples.  Replaces the torch
 * composition of ref: examples/utils.py:83-85 (positions = rays_o[ray_indices] + rays_d[ray_indices] * (t_starts + t_ends)
 * [:, None] / 2.0) and of ref: examples/radiance_fields/ngp.py:42-66,158-164,185 (aabb normalisation, contract_to_unisphere,
 * the inside-the-box selector, (dir + 1) / 2).
 *   p = o[r] + (d[r] * (t_start + t_end)) / 2, each operation rounded on its own: bit-identical to the torch expression;
 *   with a box {min xyz, max xyz} (aabb_host: 6 host floats read during the call, or aabb: 6 device floats; not both)
 *   x = (p - min) / (max - min); contraction 1 (sphere, |.|_2) or 2 (cube, |.|_inf) then maps u = 2 x - 1, where the norm m
 *   exceeds 1, to (2 - 1/m) (u / m), and x = u / 4 + 0.5 (the box lands on [0.25, 0.75]^3).
 * rays_o / rays_d [n_rays, 3]; t_starts / t_ends [n_elems]; ray_indices [n_elems] in any order, or NULL for batched input
 * of n_rays rows of samples_per_ray samples (ray = element / samples_per_ray).  An index outside [0, n_rays) gives NaN rows.
 * Outputs, each optional, at least one: positions [n_elems, 3] (p, or x with a box); dirs [n_elems, 3] with dirs_mode 1
 * (d[r]) or 2 ((d[r] + 1) / 2), NULL with dirs_mode 0; selector [n_elems] (needs a box): all of 0 < x < 1. */
int nfa_sample_positions_fwd(const float *rays_o, const float *rays_d, const float *t_starts, const float *t_ends,
                             const int64_t *ray_indices, int64_t n_rays, int64_t n_elems, int64_t samples_per_ray,
                             const float *aabb_host, const float *aabb, int32_t contraction, int32_t dirs_mode,
                             float *positions, float *dirs, uint8_t *selector, nfa_stream_t stream);
/* Its backward.  g_positions [n_elems, 3] / g_dirs [n_elems, 3] are the gradients that arrived (either may be NULL); per
 * sample g_p = J^T g_positions at the recomputed point and grad_t_starts = grad_t_ends = 1/2 d[r] . g_p.
 * With grad_rays_o and / or grad_rays_d [n_rays, 3]: one pass of the segmented engine over samples grouped by ray
 * (packed_info / tiles as for the other packed-segment entry points; ray_indices is not read): grad_rays_o[r] = sum g_p,
 * grad_rays_d[r] = sum ((t_start + t_end) / 2 g_p + s g_dirs), s = 1 (dirs_mode 1) or 1/2 (2), each ray summed by one
 * wave: no atomics, bitwise reproducible, zeros for empty rays; grad_t_starts / grad_t_ends optional; grad_p NULL.
 * Without them: a flat pass for ray indices in any order (packed_info / tiles unused, g_positions required) that writes
 * grad_p [n_elems, 3] = g_p and / or grad_t_starts / grad_t_ends; the caller reduces grad_p over rays. */
int nfa_sample_positions_bwd(const float *rays_o, const float *rays_d, const float *t_starts, const float *t_ends,
                             const int64_t *ray_indices, const float *g_positions, const float *g_dirs,
                             const int64_t *packed_info, const int64_t *tiles, int64_t n_tiles, int64_t n_rays,
                             int64_t n_elems, int64_t samples_per_ray, const float *aabb_host, const float *aabb,
                             int32_t contraction, int32_t dirs_mode, float *grad_rays_o, float *grad_rays_d,
                             float *grad_t_starts, float *grad_t_ends, float *grad_p, nfa_stream_t stream);

/* ------------------------------------------------------------------ rays from cameras */

/* Rays of n_rays pixels in one pass.  Replaces the "generate rays" block of the loaders, ref: examples/datasets/
 * nerf_synthetic.py:194-227 and examples/datasets/nerf_360_v2.py:326-359 (camera_dirs, directions, origins, viewdirs), and
 * the undistortion call a distorted camera makes inside it (ref: cuda/csrc/camera.cu:9-107):
 *   u = (x - cx + pixel_center) / fx, v = (y - cy + pixel_center) / fy; with a lens (u, v) <- the undistorted point, by the
 *   solvers of nfa_opencv_lens_undistortion (n_dist 8) / _fisheye (fisheye != 0, n_dist 4) with their eps and iters, bit for
 *   bit; c = (u, s v, s) with s = -1 (opengl != 0) or 1; d_i = (R_i0 c_0 + R_i1 c_1) + R_i2 c_2; viewdirs = d / |d|
 *   (normalize != 0) or d; origins = the translation column.  Each operation is rounded on its own.
 * x / y [n_rays]: float32, int32 or int64 (pixel_dtype 0 / 1 / 2; integers are converted here), aligned to their element.
 * camera_ids [n_rays] in any order, or NULL with n_cameras == 1; an id outside [0, n_cameras) gives NaN rows.
 * K [n_cameras, 9] row-major (k_stride 9) or one shared row (k_stride 0); camtoworlds rows of 12 or 16 floats (3x4 or 4x4
 * row-major; pose_stride 12 / 16) or one shared row (0); distortion [n_cameras, n_dist] (dist_stride n_dist) or one shared
 * row (0), NULL with n_dist 0.  origins / viewdirs [n_rays, 3].  n_rays == 0 returns at once. */
int nfa_generate_rays_fwd(const void *x, const void *y, int32_t pixel_dtype, const int64_t *camera_ids, int64_t n_rays,
                          int64_t n_cameras, const float *K, int64_t k_stride, const float *camtoworlds, int64_t pose_stride,
                          const float *distortion, int32_t n_dist, int64_t dist_stride, int32_t fisheye, int32_t opengl,
                          float pixel_center, int32_t normalize, float eps, int32_t iters, float *origins, float *viewdirs,
                          nfa_stream_t stream);
/* Its backward towards the cameras: what differentiating those loader lines with respect to the poses (ref: docs/source/
 * examples/camera/barf.rst) and intrinsics gives, as per-camera sums without float atomics: bitwise reproducible.
 * g_origins / g_viewdirs [n_rays, 3] are the gradients that arrived (either may be NULL).  Rays are taken in camera
 * order: camera_ids [n_rays] holds the ids SORTED ascending and order [n_rays] the ray of each sorted position (NULL: the
 * rays are in that order already); x, y, g_origins and g_viewdirs are indexed by ray.  The sorted rays are cut into chunks of
 * nfa_generate_rays_chunk(); a workgroup sums each (chunk, camera) run in a fixed order and writes it to row chunk + camera of
 * partials [n_partial_rows >= ceil(n_rays / chunk) + n_cameras - 1, 16] (scratch, need not be initialised); a second
 * launch adds each camera's rows in a fixed order and writes grad_camtoworlds [n_cameras, pose_floats] (pose_floats 12 or
 * 16: the bottom row of a 4x4 gets 0) and grad_K [n_cameras, 9] (fx, fy, cx, cy; 0 elsewhere), either optional; a camera
 * without rays gets zeros.  The caller sums the rows of a table it passed with stride 0.  With n_dist 8 the gradient of K
 * passes through the inverse of the distortion Jacobian at the solution (0 where |det J| < eps); with the fisheye lens
 * grad_K must be NULL.  The distortion parameters get no gradient.  n_rays == 0 returns at once and writes nothing. */
int nfa_generate_rays_bwd(const void *x, const void *y, int32_t pixel_dtype, const int64_t *camera_ids, const int64_t *order,
                          int64_t n_rays, int64_t n_cameras, const float *K, int64_t k_stride, const float *camtoworlds,
                          int64_t pose_stride, const float *distortion, int32_t n_dist, int64_t dist_stride, int32_t fisheye,
                          int32_t opengl, float pixel_center, int32_t normalize, float eps, int32_t iters,
                          const float *g_origins, const float *g_viewdirs, float *partials, int64_t n_partial_rows,
                          int32_t pose_floats, float *grad_camtoworlds, float *grad_K, nfa_stream_t stream);
int nfa_generate_rays_chunk(void);   /* rays per chunk of the backward's reduction (a constant of the build) */

/* ------------------------------------------------------------------ fused MLP */

/* The field's network as fused half-precision MFMA passes: tiny-cuda-nn's FullyFusedMLP with ReLU hidden layers, no biases
 * and no output activation (ref: examples/radiance_fields/ngp.py:131-135, 150-154, 255-259).  n_hidden + 1 matrices W_l
 * [out_l, in_l] (torch's Linear layout), in_0 = n_in, out_last = n_out, every other side `width`:
 *   H_0 = relu(x W_0^T), H_l = relu(H_{l-1} W_l^T), y = H_last W_L^T.
 * Shapes: elem NFA_ELEM_F16 or NFA_ELEM_BF16 (the network's type: weights, hidden activations, dZ), width 64 or 128,
 * n_hidden 1..4, n_in 1..256, n_out 1..32; and the packed images below must fit the 160 KiB of LDS of a compute unit
 * beside 16,896 B of store staging (the message gives the sizes).  All five entries check, in this order: elem, width,
 * n_hidden, n_in, n_out, n_points >= 0, the LDS budget, the other element codes; then n_points == 0 returns NFA_OK
 * whatever the pointers are; then null pointers and alignment.  Nothing reaches the GPU before every check passed.
 * Rounding (always to nearest even): x, v and the masters to `elem`, every hidden activation after its ReLU, every dZ_l and
 * T_l after its mask, y / grad_x / u once as stored; float32 outputs are the float32 accumulators unrounded.
 *
 * nfa_mlp_pack_weights: params = the float32 masters, W_0 .. W_L flat in that order, to the two images the passes read
 * (one launch).  A packed matrix A [rows, k] is a run of 1 KiB blocks (m, q), m < ceil(rows / 32) major, q < ceil(k / 16):
 * element ((m KQ + q) 64 + lane) 8 + j = A[32 m + (lane & 31)][16 q + kpos], zero outside A, with kpos = 8 (lane >> 5) + j for
 * the layer whose other operand comes from memory (layer 0 forward, the last layer backward) and 8 (j >> 2) + 4 (lane >> 5) +
 * (j & 3) elsewhere (the order in which an accumulator tile presents its rows as the next operand).  fwd_image: A = W_l;
 * bwd_image: A = W_l^T; layers in order.  fwd_elems / bwd_elems: the images' sizes in elements, which must be exactly
 * sum_l ceil(out_l / 32) ceil(in_l / 16) 512 and sum_l ceil(in_l / 32) ceil(out_l / 16) 512.  Images are 16-byte aligned. */
int nfa_mlp_pack_weights(int32_t elem, const float *params, int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden,
                         void *fwd_image, int64_t fwd_elems, void *bwd_image, int64_t bwd_elems, nfa_stream_t stream);
/* One launch for the whole network.  x [n_points, n_in] of x_elem (NFA_ELEM_F32: rounded on load; or elem), rows of a
 * multiple of 8 elements from a 16-byte aligned base load as 16-byte pieces, any other shape element by element.
 * y [n_points, n_out] of y_elem (elem, or NFA_ELEM_F32).  save_hidden != 0: hidden [n_hidden, n_points, width] (elem,
 * 8-byte aligned) receives the rounded post-ReLU activations; otherwise nothing but y is written. */
int nfa_mlp_fwd(int32_t elem, const void *x, int32_t x_elem, const void *fwd_image, int64_t n_points, int32_t n_in, int32_t n_out,
                int32_t width, int32_t n_hidden, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream);
/* One launch for the gradient chain: dZ_L = grad_y rounded to elem (g_elem: NFA_ELEM_F32 or elem), dH_{l-1} = dZ_l W_l,
 * dZ_{l-1} = dH_{l-1} * (H_{l-1} > 0) with H from `hidden` as nfa_mlp_fwd saved it.  Writes dz [n_hidden, n_points, width]
 * (elem; dZ_0 .. dZ_{L-1}), dz_out [n_points, n_out] (elem; dZ_L, optional: a caller whose grad_y is of type elem
 * already passes grad_y to nfa_mlp_bwd_weights instead) and grad_x [n_points, n_in] of x_elem (optional). */
int nfa_mlp_bwd_data(int32_t elem, const void *grad_y, int32_t g_elem, const void *hidden, const void *bwd_image, int64_t n_points,
                     int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, void *dz, void *dz_out, void *grad_x,
                     int32_t x_elem, nfa_stream_t stream);
/* grad_params (the masters' layout, float32, overwritten) = dW_l = dZ_l^T H_{l-1}, H_{-1} = x rounded as the forward rounds
 * it: split-K MFMA over the points and an ordered sum, two launches, no atomics, bitwise reproducible.  The points are
 * cut into n_slices = ceil(n_points / slice) slices, slice = ceil(n_points / s) rounded up to a multiple of 64 with
 * s = clamp(ceil(n_points / NFA_MLP_WGRAD_MIN_SLICE), 1, NFA_MLP_WGRAD_MAX_SLICES): a function of n_points alone.  A
 * workgroup per (slice, layer) writes its float32 partial to partials [n_slices, n_params] (scratch of partial_floats floats,
 * need not be initialised; too small is NFA_EINVAL), the second launch adds the slices in ascending order.  hidden, dz:
 * as above, 16-byte aligned; dz_out [n_points, n_out] of elem.
 * The second order reuses this entry as it stands: called with x := v and hidden := tangent of nfa_mlp_tangent (and dz, dz_out
 * of the first backward) it returns ds/dW_l = dZ_l^T T_{l-1}. */
#define NFA_MLP_WGRAD_MIN_SLICE 256
#define NFA_MLP_WGRAD_MAX_SLICES 256
int nfa_mlp_bwd_weights(int32_t elem, const void *x, int32_t x_elem, const void *hidden, const void *dz, const void *dz_out,
                        int64_t n_points, int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, float *partials,
                        int64_t partial_floats, float *grad_params, nfa_stream_t stream);
/* The second order (double backward), one launch for the whole network.  With v [n_points, n_in] the cotangent of grad_x and
 * s = <v, grad_x>: T_{-1} = v rounded to elem (v_elem: NFA_ELEM_F32 or elem; loaded as nfa_mlp_fwd loads x),
 * T_l = (T_{l-1} W_l^T) * (H_l > 0) rounded to elem, l < n_hidden, with H from `hidden` as nfa_mlp_fwd saved it (the saved
 * mask, not a ReLU of the tangent), and u = T_last W_L^T = ds/dgrad_y.  The backward is linear in grad_y and the masks are
 * piecewise constant, so this is exact; ds/dx is zero.  Writes u [n_points, n_out] of u_elem (elem: rounded once; NFA_ELEM_F32:
 * the accumulators) and tangent [n_hidden, n_points, width] (elem, 8-byte aligned; T_0 .. T_{L-1}; optional: NULL when no
 * weight gradient is wanted), laid out as `hidden`: ds/dW_l = dZ_l^T T_{l-1} is nfa_mlp_bwd_weights on (v, tangent). */
int nfa_mlp_tangent(int32_t elem, const void *v, int32_t v_elem, const void *hidden, const void *fwd_image, int64_t n_points,
                    int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, void *tangent, void *u, int32_t u_elem,
                    nfa_stream_t stream);

/* The same five passes for the reference's MLP class (ref: examples/radiance_fields/mlp.py, MLP), restricted to what the
 * kernels hold: biases and skip connections on top of the network above.  The five entries above are these with bias = 0 and
 * skip_mask = 0, bit for bit.
 *   bias != 0: every layer has a float32 bias b_l [out_l], z_l = b_l + W_l in_l.  A bias is never rounded: it is the float32
 *     value the layer's accumulator starts from.
 *   skip_mask: bit l set (2 <= l <= n_hidden) makes layer l a "cat layer" whose input is [H_{l-1}, x], in this column order, x
 *     rounded as layer 0 sees it; its matrix is [out_l, width + n_in].  The reference's skip_layer = s sets bit i + 1 for every
 *     hidden layer 0 < i < n_hidden with i % s == 0; bit n_hidden is the output layer.
 * Parameters (params, grad_params, each slice of partials): all matrices W_0 .. W_L in layer order, row-major [out_l, in_l] with
 * in_l = width + n_in at a cat layer, then (bias != 0) all biases b_0 .. b_L in layer order: n_params = sum out_l in_l + sum out_l.
 * Limits, checked by every entry after n_points >= 0 and before the LDS budget (a null descriptor first of all): bias is 0
 * or 1; skip_mask has no bit outside 2 .. n_hidden; with a skip, n_in + width <= 256 (what the weight gradient stages for one
 * layer).  The LDS budget counts the longer images and, for the forward pass, (n_hidden width + 32) 4 bytes of biases.  The
 * other checks and their order are those of the entries above.
 * Images: the forward image of a cat layer has width / 16 + ceil(n_in / 16) k-steps, the H part in the permuted k order and
 * behind it the x part in the natural order 8 (lane >> 5) + j (its operand comes from memory, as layer 0's does); the backward
 * image of a cat layer has width + n_in rows, rows >= width feed grad_x only; a cat OUTPUT layer's backward image is in natural
 * k order throughout.  fwd_elems / bwd_elems follow the formulas of nfa_mlp_pack_weights with these in_l and k-step counts.
 * The biases are not part of the images: nfa_mlp_net_fwd reads them as float32. */
typedef struct nfa_mlp_desc {
    int32_t n_in, n_out, width, n_hidden;
    int32_t bias;        /* 0 or 1 */
    int32_t skip_mask;   /* bit l: layer l takes [H_{l-1}, x] */
} nfa_mlp_desc;
/* params: the matrices of the layout above (the biases behind them are not read). */
int nfa_mlp_net_pack_weights(int32_t elem, const nfa_mlp_desc *net, const float *params, void *fwd_image, int64_t fwd_elems,
                             void *bwd_image, int64_t bwd_elems, nfa_stream_t stream);
/* As nfa_mlp_fwd.  bias: b_0 .. b_L, float32, sum out_l of them in layer order (params + sum out_l in_l); read only when
 * net->bias != 0, staged once per workgroup beside the image. */
int nfa_mlp_net_fwd(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *fwd_image, const float *bias,
                    int64_t n_points, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream);
/* As nfa_mlp_bwd_data; grad_x = dZ_0 W_0 + sum over the cat layers of dZ_l W_l[:, width:], summed in float32 in one accumulator
 * and rounded once as stored.  The biases do not enter. */
int nfa_mlp_net_bwd_data(int32_t elem, const nfa_mlp_desc *net, const void *grad_y, int32_t g_elem, const void *hidden,
                         const void *bwd_image, int64_t n_points, void *dz, void *dz_out, void *grad_x, int32_t x_elem,
                         nfa_stream_t stream);
/* As nfa_mlp_bwd_weights, n_params as above: dW_l = dZ_l^T [H_{l-1}, x] at a cat layer, and db_l = sum_p dZ_l[p, :] in float32
 * over the same slices, the points of a slice in a fixed order and the slices in ascending order: no atomics, bitwise
 * reproducible.  zero_bias != 0 writes zeros into the bias segment instead: the second-order call (x := v, hidden := tangent)
 * sets it, since the masks are piecewise constant and d<v, grad_x>/db is zero. */
int nfa_mlp_net_bwd_weights(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *hidden, const void *dz,
                            const void *dz_out, int64_t n_points, float *partials, int64_t partial_floats, float *grad_params,
                            int32_t zero_bias, nfa_stream_t stream);
/* As nfa_mlp_tangent: every accumulator starts at zero (a bias has no tangent) and a cat layer sees [T_{l-1}, v], the output
 * layer included: u = W_L [T_{L-1}(, v)].  ds/dW_l = dZ_l^T [T_{l-1}(, v)] is nfa_mlp_net_bwd_weights on (v, tangent). */
int nfa_mlp_net_tangent(int32_t elem, const nfa_mlp_desc *net, const void *v, int32_t v_elem, const void *hidden, const void *fwd_image,
                        int64_t n_points, void *tangent, void *u, int32_t u_elem, nfa_stream_t stream);

/* The same network with tiny-cuda-nn's activation set: ONE hidden activation f for all hidden layers and one output activation
 * f_out, each an NFA_MLP_ACT_* code.  With y_l = f(z_l) as stored (rounded to elem), f' and rho = f'' / f' are formed from y:
 *   NONE         z                                  f' = 1                        rho = 0
 *   RELU         max(z, 0)                          select y > 0                  0
 *   LEAKY_RELU   z > 0 ? z : 0.01f z                y > 0 ? 1 : 0.01f (select)    0
 *   SIGMOID      1 / (1 + e^-z)                     y (1 - y)                     1 - 2 y
 *   TANH         tanh z                             1 - y^2                       -2 y
 *   SOFTPLUS     max(z, 0) + log1p(e^(-beta |z|)) / beta   1 - e^(-beta y)        beta e^(-beta y)
 *   EXPONENTIAL  e^z                                y                             1
 * Transcendentals are float32 with the accurate device functions; the result is rounded once where ReLU's is.  Forward:
 * H_l = f(z_l), y = f_out(z_L).  Data gradient: dZ_L = rnd(grad_y * f_out'(y)), dZ_l = rnd(dH_l * f'(H_l)); y is the
 * forward's output as stored (y_elem: elem or NFA_ELEM_F32), read only when f_out is not NONE, and then dz_out is required.
 * Tangent, A_l = W_l [T_{l-1}(, v)]: T_l = rnd(A_l * f'(H_l)), u = f_out'(y) * A_L, and, when r and r_out are given (both or
 * neither; then dz and dz_out of the first backward are read), R_l = rnd((rho(H_l) dZ_l) A_l) to r [n_hidden, n_points, width]
 * and R_L = rnd((rho_out(y) dZ_L) A_L) to r_out [n_points, n_out], exact zeros where rho is identically zero.
 * Curvature pass (the data gradient's chain with an injected cotangent): E_L = r_out, E_{l-1} = rnd((W_l^T E_l)[:width] *
 * f'(H_{l-1}) + R_{l-1}) with R from `inject` (laid out as `hidden`, 8-byte aligned), written to e [n_hidden, n_points, width];
 * grad_x = ds/dx = W_0^T E_0 + sum over the cat layers W_l[:, width:]^T E_l.  The second-order parameter gradient is
 * nfa_mlp_net_bwd_weights twice, on (v, tangent, dz, dz_out) with zero_bias = 1 and on (x, hidden, e, r_out) with zero_bias = 0,
 * and the sum of the two.  Images, descriptor, nfa_mlp_net_pack_weights and nfa_mlp_net_bwd_weights are shared unchanged.
 * Checks: those of the nfa_mlp_net_* twins in their order, with the activation checked right after the shape: null `act`, a
 * code outside NFA_MLP_ACT_NONE .. NFA_MLP_ACT_EXPONENTIAL, beta <= 0 (or NaN).  With hidden = NFA_MLP_ACT_RELU and output = NFA_MLP_ACT_NONE
 * every pass gives the bits of its twin. */
#define NFA_MLP_ACT_NONE 0
#define NFA_MLP_ACT_RELU 1
#define NFA_MLP_ACT_LEAKY_RELU 2
#define NFA_MLP_ACT_SIGMOID 3
#define NFA_MLP_ACT_TANH 4
#define NFA_MLP_ACT_SOFTPLUS 5
#define NFA_MLP_ACT_EXPONENTIAL 6
typedef struct nfa_mlp_act { int32_t hidden, output; float beta; } nfa_mlp_act;
int nfa_mlp_act_fwd(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *x, int32_t x_elem,
                    const void *fwd_image, const float *bias, int64_t n_points, void *y, int32_t y_elem, void *hidden,
                    int32_t save_hidden, nfa_stream_t stream);
int nfa_mlp_act_bwd_data(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *grad_y, int32_t g_elem,
                         const void *y, int32_t y_elem, const void *hidden, const void *bwd_image, int64_t n_points, void *dz,
                         void *dz_out, void *grad_x, int32_t x_elem, nfa_stream_t stream);
int nfa_mlp_act_tangent(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *v, int32_t v_elem,
                        const void *y, int32_t y_elem, const void *hidden, const void *dz, const void *dz_out,
                        const void *fwd_image, int64_t n_points, void *tangent, void *r, void *r_out, void *u, int32_t u_elem,
                        nfa_stream_t stream);
int nfa_mlp_act_curvature(int32_t elem, const nfa_mlp_desc *net, const nfa_mlp_act *act, const void *r_out, const void *hidden,
                          const void *inject, const void *bwd_image, int64_t n_points, void *e, void *grad_x, int32_t x_elem,
                          nfa_stream_t stream);

/* The same network with STREAMED weights (csrc/mlp_stream.hip), for what the entries above refuse: NeRF's 63 -> 8 x 256 trunk
 * (ref: examples/radiance_fields/mlp.py, NerfMLP).  Descriptor, parameter layout, images (nfa_mlp_stream_pack_weights writes
 * exactly what nfa_mlp_net_pack_weights would), buffers, arithmetic and rounding points are those of the nfa_mlp_net_* entries,
 * and so are the argument lists and the null-pointer, alignment, negative-n_points and n_points = 0 checks.  The images stay in
 * global memory and pass through the LDS one row tile of one layer at a time (a "piece": 32 rows x all k-steps of the layer),
 * through a ring of two slots, while a workgroup's NFA_MLP_STREAM_POINTS points wait in registers; the fused passes launch
 * min(ceil(n_points / NFA_MLP_STREAM_POINTS), NFA_MLP_STREAM_GROUPS) workgroups, each sweeping the points with that stride.
 * Limits, checked by every entry in this order after the null descriptor and elem: width 128 or 256; n_hidden 1 .. 8; n_in
 * 1 .. 320; n_out 1 .. 288; n_points >= 0; bias 0 or 1; skip_mask with bits 2 .. n_hidden only (no limit on n_in + width);
 * the ring: 2 slots of the largest piece (at most (width / 16 + 20) KiB) + 16896 B of store staging + 1280 B of piece table +
 * (n_hidden width + 32 ceil(n_out / 32)) 4 B of biases (bias != 0; the forward pass stages them once per workgroup) against
 * 160 KiB of LDS, which holds for every shape inside the other limits (101248 B at most).
 * There is no tangent entry: the second order is not implemented for the streamed network.
 * nfa_mlp_stream_bwd_weights: partials holds s slices of n_params floats, s = clamp(ceil(n_points / NFA_MLP_STREAM_WGRAD_MIN_SLICE),
 * 1, NFA_MLP_STREAM_WGRAD_MAX_SLICES) cut as in nfa_mlp_bwd_weights (slice length rounded up to 64 points, s the slices that
 * are not empty): a function of n_points alone, at most 16 (the trunk has 0.6 M parameters: 38 MB of partials).  Grid (slice,
 * layer, 128 x 128 macro tile of dW_l); the slices are summed in ascending order: no atomics, bitwise reproducible. */
#define NFA_MLP_STREAM_POINTS 128
#define NFA_MLP_STREAM_GROUPS 256
#define NFA_MLP_STREAM_WGRAD_MIN_SLICE 256
#define NFA_MLP_STREAM_WGRAD_MAX_SLICES 16
int nfa_mlp_stream_pack_weights(int32_t elem, const nfa_mlp_desc *net, const float *params, void *fwd_image, int64_t fwd_elems,
                                void *bwd_image, int64_t bwd_elems, nfa_stream_t stream);
int nfa_mlp_stream_fwd(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *fwd_image, const float *bias,
                       int64_t n_points, void *y, int32_t y_elem, void *hidden, int32_t save_hidden, nfa_stream_t stream);
int nfa_mlp_stream_bwd_data(int32_t elem, const nfa_mlp_desc *net, const void *grad_y, int32_t g_elem, const void *hidden,
                            const void *bwd_image, int64_t n_points, void *dz, void *dz_out, void *grad_x, int32_t x_elem,
                            nfa_stream_t stream);
int nfa_mlp_stream_bwd_weights(int32_t elem, const nfa_mlp_desc *net, const void *x, int32_t x_elem, const void *hidden, const void *dz,
                               const void *dz_out, int64_t n_points, float *partials, int64_t partial_floats, float *grad_params,
                               int32_t zero_bias, nfa_stream_t stream);

/* ------------------------------------------------------------------ fused optimiser (csrc/optim.hip)
 * One Adam / AdamW step (torch's, non-amsgrad) over a LIST of float32 tensors in at most three launches, whatever the length
 * of the list, with the loss scale, its overflow policy (torch's GradScaler) and a warm-up + multi-step LR schedule held and
 * advanced on the device: no host read, so a whole training step captures into one graph.  The launches are cut at the
 * all-to-all seams (no grid-wide barrier): nfa_optim_scan (only with a scaler), nfa_optim_decide (one wave), nfa_optim_update.
 *
 * The list is two device arrays the caller builds once per set of pointers and sizes: `table` (one nfa_optim_tensor per
 * tensor) and `work` (one nfa_optim_chunk per NFA_OPTIM_CHUNK elements of a tensor, the last chunk of a tensor shorter: no
 * chunk crosses a tensor, every element is in exactly one chunk).  A workgroup takes chunks in a grid-stride loop.  Where the
 * four pointers of a tensor are 16-byte aligned a lane moves 16-byte pieces and the tail (n % 4 elements) goes element by
 * element; otherwise the whole tensor does.  Both paths run the same per-element function: the same bits.  No atomics.
 *
 * Per element, float32, every operation rounded on its own, in this order (G: the group's scalars, below):
 *     g = grad * inv_scale
 *     skip_zero_grad and g == 0:  p, m, v stay as they are (no decay either)
 *     L2 decay (weight_decay != 0, not decoupled):  g = g + weight_decay * p
 *     decoupled decay:                              p = p * decay
 *     m = m + one_minus_beta1 * (g - m)
 *     v = beta2 * v + one_minus_beta2 * (g * g)
 *     p = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 * zero_grad: grad = 0 afterwards, on a skipped step too.  On a skipped step nothing else is written. */
#define NFA_OPTIM_CHUNK 4096       /* elements per work-list entry (a multiple of 4) */
#define NFA_OPTIM_MAX_GROUPS 16
#define NFA_OPTIM_MAX_MILESTONES 8
#define NFA_OPTIM_DECOUPLED 1      /* nfa_optim_group.flags: weight decay is AdamW's */
#define NFA_OPTIM_SKIP_ZERO_GRAD 2 /* an element whose unscaled gradient is exactly 0 is left alone (tiny-cuda-nn's rule) */
typedef struct nfa_optim_tensor {   /* 48 bytes */
    float *p, *grad, *exp_avg, *exp_avg_sq;
    int64_t n;
    int32_t group;                  /* index into the groups of nfa_optim_args */
    int32_t reserved;
} nfa_optim_tensor;
typedef struct nfa_optim_chunk {    /* elements [chunk * NFA_OPTIM_CHUNK, min(n, (chunk + 1) * NFA_OPTIM_CHUNK)) of table[tensor] */
    int32_t tensor, chunk;
} nfa_optim_chunk;
/* The scaler's state, device memory owned by the caller (32 bytes).  found: set to 1 by nfa_optim_scan, read and cleared by
 * nfa_optim_decide.  Policy (torch.amp.GradScaler): found -> scale *= backoff_factor, tracker = 0, skipped += 1 and the step
 * is skipped; else tracker += 1 and at growth_interval scale *= growth_factor (kept if finite), tracker = 0. */
typedef struct nfa_optim_scaler {
    float scale;
    int32_t tracker, found, reserved;
    int64_t skipped, reserved2;
} nfa_optim_scaler;
typedef struct nfa_optim_group {    /* a param group's settings as the host has them now (48 bytes) */
    double lr, beta1, beta2, eps, weight_decay;
    int32_t flags, reserved;
} nfa_optim_group;
/* HOST struct, passed by value into the decide launch (a captured graph keeps the values it was captured with).
 * Schedule: factor(t) = (start_factor + (1 - start_factor) * min(t, warmup_iters) / warmup_iters) * gamma^(milestones <= t),
 * t = nfa_optim_state.calls, the power by repeated multiplication, all in double; warmup_iters = 0 and n_milestones = 0: 1. */
typedef struct nfa_optim_args {
    int32_t n_groups, n_milestones;
    nfa_optim_group groups[NFA_OPTIM_MAX_GROUPS];
    double start_factor, gamma;
    int64_t warmup_iters;
    int64_t milestones[NFA_OPTIM_MAX_MILESTONES];
    float growth_factor, backoff_factor;   /* of the scaler */
    int32_t growth_interval, reserved;     /* <= 0: the scale stays fixed on clean steps */
} nfa_optim_args;
typedef struct nfa_optim_group_scalars {   /* 48 bytes; what nfa_optim_update reads, each a double expression rounded once */
    float step_size;        /* lr * factor / (1 - beta1^step) */
    float bc2_sqrt;         /* sqrt(1 - beta2^step) */
    float decay;            /* 1 - lr * factor * weight_decay */
    float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
    int32_t flags, reserved[3];
} nfa_optim_group_scalars;
/* Device memory owned by the caller; calls = step = 0 and every power 1.0 at the start.  step counts PERFORMED updates (bias
 * correction), calls counts nfa_optim_decide launches (the schedule).  beta^step are running products in double. */
typedef struct nfa_optim_state {
    int64_t calls, step;
    double beta1_pow[NFA_OPTIM_MAX_GROUPS], beta2_pow[NFA_OPTIM_MAX_GROUPS];
    float inv_scale;   /* this step's: float(1 / scale) of the scale the gradients were made with; 1 without a scaler */
    int32_t skip;      /* this step's: the scan found a non-finite gradient */
    float factor;      /* this step's schedule factor (for inspection) */
    int32_t reserved;
    nfa_optim_group_scalars group[NFA_OPTIM_MAX_GROUPS];
} nfa_optim_state;
int nfa_optim_chunk_elems(void);   /* NFA_OPTIM_CHUNK */
/* scaler->found = 1 if any gradient of the list is not finite (left alone otherwise).  dtype: NFA_ELEM_F32, anything else is
 * NFA_EINVAL.  n_tensors = 0 or n_chunks = 0: nothing to do. */
int nfa_optim_scan(int32_t dtype, const nfa_optim_tensor *table, int32_t n_tensors, const nfa_optim_chunk *work, int64_t n_chunks,
                   nfa_optim_scaler *scaler, nfa_stream_t stream);
/* This step's scalars into *state, the counters, the powers and the scaler advanced.  scaler NULL: no loss scaling. */
int nfa_optim_decide(const nfa_optim_args *args_host, nfa_optim_state *state, nfa_optim_scaler *scaler, nfa_stream_t stream);
int nfa_optim_update(int32_t dtype, const nfa_optim_tensor *table, int32_t n_tensors, const nfa_optim_chunk *work, int64_t n_chunks,
                     const nfa_optim_state *state, int32_t zero_grad, nfa_stream_t stream);

/* ------------------------------------------------------------------ photometric loss (csrc/photo.hip)
 * The target side of a training step: the pixel gather, the background blend, the loss, its gradient and the MSE.  The
 * per-element terms (P = param; s(d) = 1, -1 or d itself for d > 0, d < 0, otherwise), float32, each operation rounded:
 *     NFA_PHOTO_L1           |d|                                               dterm/dd = s(d)
 *     NFA_PHOTO_L2           d * d                                             2 * d
 *     NFA_PHOTO_SMOOTH_L1    |d| < P ? ((0.5 * d) * d) / P : |d| - 0.5 * P     |d| < P ? d / P : s(d)        (P > 0)
 *     NFA_PHOTO_HUBER        |d| <= P ? (0.5 * d) * d : P * (|d| - 0.5 * P)    |d| <= P ? d : P * s(d)
 *     NFA_PHOTO_RELATIVE_L2  (d * d) / (rgb * rgb + 0.01)                      (2 * d) / (rgb * rgb + 0.01)  (instant-ngp's)
 *     NFA_PHOTO_CHARBONNIER  sqrt(d * d + P * P)                               d / sqrt(d * d + P * P) */
#define NFA_PHOTO_L1 0
#define NFA_PHOTO_L2 1
#define NFA_PHOTO_SMOOTH_L1 2
#define NFA_PHOTO_HUBER 3
#define NFA_PHOTO_RELATIVE_L2 4
#define NFA_PHOTO_CHARBONNIER 5
/* Targets, loss and MSE of n_rays rays in two launches (one when rgb is NULL).  Replaces, ref: examples/datasets/
 * nerf_synthetic.py:195 (`rgba = images[image_id, y, x] / 255.0`) and :153 (`pixels = rgba[:, :3] * alpha + color_bkgd *
 * (1 - alpha)`), dnerf_synthetic.py:155,197 (the same), nerf_360_v2.py:327 (the RGB-only gather), and the trainers'
 * `F.smooth_l1_loss(rgb, pixels)` and `F.mse_loss(rgb, pixels)` (examples/train_ngp_nerf_occ.py:198,208,245,
 * train_ngp_nerf_prop.py:243,253,295, train_mlp_nerf.py:170,179,226, train_mlp_tnerf.py:163,172,211).
 * Source, exactly one of: images, a uint8 stack [n_images, height, width, n_channels] read at (image_ids, y, x) [n_rays]
 * (index_dtype 1: int32, 2: int64, one type for the three; image_ids NULL: image 0; x and y NULL: ray i reads pixel i of
 * the stack in memory order), every index clamped into the stack, the byte offset formed in 64 bits, a channel float(byte) /
 * 255.0f; or pixels_in, float32 [n_rays, n_channels].  n_channels 3 or 4.  With 4 channels and bkgd ([3]: bkgd_stride 0, or
 * [n_rays, 3]: 3) target = (p * a) + (b * (1.0f - a)); bkgd NULL: the three colour channels as they are.
 * rgb [n_rays, 3] of type elem (NFA_ELEM_*), computed in float32; d = rgb - target.  weights [n_rays] or NULL.
 * Writes pixels [n_rays, 3] (the target), loss[0] = sum w * term / (3 n_rays), mse[0] = sum d * d / (3 n_rays) and, if not
 * NULL, per_ray [n_rays] = (w * ((t_0 + t_1) + t_2)) / 3.0f.  The sums are float64 without atomics: a workgroup adds the
 * nfa_photometric_chunk() rays of a chunk in a fixed order into partials [n_partials >= ceil(n_rays / chunk), 2] (scratch,
 * 8-byte aligned, need not be initialised), a second launch of one wave adds those (lane t: t, t + 64, .. in order; then
 * the lanes in order), divides by 3 n_rays and rounds to float32 once.  rgb NULL: only pixels is written (kind, weights,
 * partials, loss, mse, per_ray are not looked at).  n_rays == 0 returns at once and writes nothing.  No host read. */
int nfa_photometric_fwd(const void *rgb, int32_t elem, int64_t n_rays, const uint8_t *images, int64_t n_images, int64_t height,
                        int64_t width, const void *image_ids, const void *x, const void *y, int32_t index_dtype,
                        const float *pixels_in, int32_t n_channels, const float *bkgd, int64_t bkgd_stride, const float *weights,
                        int32_t kind, float param, float *pixels, double *partials, int64_t n_partials, float *loss, float *mse,
                        float *per_ray, nfa_stream_t stream);
/* Its backward, ref: what `(loss * scale).backward()` delivers at rgb (examples/train_ngp_nerf_occ.py:202, train_ngp_nerf_prop.py:247), one launch:
 * g_rgb [n_rays, 3] of type elem = ((g * w) * inv) * dterm/dd, rounded once, with g = g_loss[0] read on the device (the
 * gradient that arrived at the loss: the loss scale), inv = 1.0f / (float)(3 n_rays) and d = rgb - pixels, pixels being the
 * forward's output.  per_ray and mse carry no gradient. */
int nfa_photometric_bwd(const void *rgb, int32_t elem, const float *pixels, const float *weights, const float *g_loss,
                        int64_t n_rays, int32_t kind, float param, void *g_rgb, nfa_stream_t stream);
int nfa_photometric_chunk(void);   /* rays per partial pair of the forward's reduction (a constant of the build) */

#ifdef __cplusplus
}
#endif
#endif /* NERFACC_HIP_H */

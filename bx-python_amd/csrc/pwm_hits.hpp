// pwm_hits.hpp -- the elements of pwm.hpp's score planes that reach a threshold, as one compact list in a fixed order, without
// the planes ever being written (bxmi_twobit_pwm_hits*).  Included by sequence.hip after pwm.hpp.  In the reference's terms, for
// matrix m and row i: numpy.nonzero(pwms[m].score_string(row i) >= threshold[m]) and the scores there (lib/bx/motif/pwm.py:141-149
// over _pwm.pyx:23-55).
//
// An element of plane m is a HIT when it is scored (pwm.hpp: every letter of its window has a column and lies in the row), its
// score is not a NaN, and score >= threshold[m] as a float32 comparison: an unscoreable element and an arithmetic NaN are never
// hits, a -inf score is one only under a -inf threshold.  The list holds the hits in ascending (matrix, row, offset in row):
// hit_row, hit_pos (as best_pos) and hit_score, parallel arrays; matrix m's part is [mat_hits[m], mat_hits[m + 1]).
//
//   pw_hits_kernel<FILL>   the cut of pw_scores_kernel: tiles of PW_TILE elements of the flat output axis, four consecutive
//                          elements per thread, a tile walked row segment by row segment, the columns of the segment and its halo
//                          staged in LDS by pw_stage_columns of pwm.hpp, every accumulator in ascending j from +0.0f.  (The
//                          window walk stands here a second time.)  A workgroup takes every gridDim.x-th tile of the launch's
//                          [tile_first, tile_first + tile_count).
//     FILL == false        counts: per (segment, matrix) the workgroup's hits are summed -- a wave prefix over the threads' 0 .. 4
//                          hits (PH_WAVE_PREFIX), the four waves' totals through LDS -- into a running count per matrix in LDS,
//                          and at the tile's end thread m stores counts[m * tiles + tile]: plain stores, no atomics.
//     (between the two)    an exclusive scan of counts[n_mats * tiles] gives int64 bases in (matrix, tile) order, the grand total
//                          behind them: mat_hits[m] is bases[m * tiles].
//     FILL == true         scores again -- but for the tiles, and in a tile the matrices, whose count is 0: under a threshold that
//                          few scores reach, the second pass is a fraction of the first -- and the same prefix is now the rank:
//                          hit k of a thread goes to bases[m * tiles + tile] + the running count of the tile's earlier segments
//                          + the earlier waves' totals + the wave's prefix before the thread + k.  Tiles ascend along the flat
//                          axis, segments along a tile, threads along a segment and the elements along a thread, so the
//                          placement IS the order; the same on every run.
// LDS: pw_scores_kernel's and 160 bytes (the running counts, two sets of wave totals so that one barrier per step is enough).
// Scratch: 12 bytes per (matrix, tile) and the scan's block sums; nothing per element.
#pragma once

#include "pwm.hpp"
#ifndef PH_WAVE_PREFIX
#include "primitives.hpp"  // wave_inclusive_sum_dpp
#endif

namespace bxmi {

#ifndef PH_TILES_PER_LAUNCH
#define PH_TILES_PER_LAUNCH ((int64_t)1 << 22)  // tiles a launch is given at most (a grid's threads are counted in 32 bits: 2^22 workgroups of 256)
#endif

struct PhThresholds {
    float t[PW_MATS_MAX];
};

// the inclusive prefix sum of `v` over the wave's 64 lanes; every lane of the workgroup calls it.  (The host build of
// tests/cpp/pwm_hits_kernel_host.cpp puts its own in its place: host threads have no lanes.)
#ifndef PH_WAVE_PREFIX
#define PH_WAVE_PREFIX(v) ((int)wave_inclusive_sum_dpp((unsigned)(v)))
#endif

// the launches of one pass over `tiles` tiles: launch(tile_first, tile_count, grid), at most `per_launch` tiles each, the grid at
// most `fill` workgroups
template <typename Launch>
inline int ph_each_launch(int64_t tiles, int64_t per_launch, int64_t fill, Launch launch)
{
    for (int64_t first = 0; first < tiles; first += per_launch) {
        const int64_t m = tiles - first < per_launch ? tiles - first : per_launch;
        const int rc = launch(first, m, (unsigned)(m < fill ? m : fill));
        if (rc != 0) return rc;
    }
    return 0;
}

// The text of pw_hits_kernel (STRAND == false: `strand` is not read) and of pw_hits_strand_kernel (STRAND == true: strand[n_rows],
// any non-zero entry a minus row).  The staging is pw_stage_columns of pwm.hpp; hit_pos is the offset in the strand's string.
template <bool STRAND, bool FILL>
__device__ __forceinline__ void pw_hits_body(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                             const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows, int width,
                                             const int64_t *__restrict__ row_off, int64_t total, int do_mask, PwSet pw, PhThresholds thr, int64_t tile_first,
                                             int64_t tile_count, int64_t tiles, int32_t *counts, const int64_t *__restrict__ bases,
                                             int32_t *__restrict__ hit_row, int32_t *__restrict__ hit_pos, float *__restrict__ hit_score)
{
    __shared__ int32_t l_st[TB_CHUNK], l_en[TB_CHUNK];
    __shared__ int8_t l_col[PW_STAGE] __attribute__((aligned(8)));
    __shared__ float l_val[PW_LDS_VALUES];
    __shared__ int32_t l_run[PW_MATS_MAX];  // the tile's hits so far, per matrix
    __shared__ int32_t l_wave[2][PW_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int32_t BX_GLOBAL *g_track = as_global(track_of), *g_start = as_global(start);
    const int8_t BX_GLOBAL *g_strand = as_global(strand);
    const int64_t BX_GLOBAL *g_off = as_global(row_off);
    const float BX_GLOBAL *g_val = as_global(pw.values);
    const int32_t BX_GLOBAL *g_mat = as_global(pw.mat_off);
    const int n_cols = pw.n_cols;
    const int all_values = g_mat[pw.n_mats] * n_cols;
    const bool resident = all_values <= PW_LDS_VALUES;  // the whole set stays in LDS
    if (resident) {
        for (int k = tid; k < all_values; k += PW_THREADS) l_val[k] = g_val[k];
    }
    unsigned turn = 0;  // the (segment, matrix) steps this workgroup has taken: which set of wave totals is in use
    const int64_t tile_end = tile_first + tile_count;
    for (int64_t tile = tile_first + blockIdx.x; tile < tile_end && tile * PW_TILE < total; tile += gridDim.x) {
        const int64_t t0 = tile * PW_TILE;
        const int64_t t1 = t0 + PW_TILE < total ? t0 + PW_TILE : total;
        const int64_t e0 = t0 + 4 * tid;  // this thread's elements: [e0, e0 + 4)
        if (FILL) {  // a tile without a hit has nothing to place: most tiles, under a threshold few scores reach
            int any = 0;
            for (int m = 0; m < pw.n_mats; m++) any |= as_global(counts)[(int64_t)m * tiles + tile];
            if (any == 0) continue;
        }
        if (tid < pw.n_mats) l_run[tid] = 0;  // (read after the first segment's barriers)
        for (int64_t o = t0; o < t1;) {  // the segment [o, seg1) of row r, whose elements are [r_lo, r_hi)
            int64_t r, r_lo, r_hi;
            if (row_off) {
                r = sa_row_of(g_off, n_rows, o);
                r_lo = g_off[r];
                r_hi = g_off[r + 1];
            } else {
                r = o / width;
                r_lo = r * width;
                r_hi = r_lo + width;
            }
            int64_t seg1 = r_hi < t1 ? r_hi : t1;
            if (seg1 <= o) seg1 = o + 1;  // (offsets that are not what they should be: the walk still ends)
            const int n_stage = pw_stage_columns<STRAND>(table, n_tracks, g_track[r], g_start[r], tb_minus<STRAND>(g_strand, r), r_lo, r_hi, o, seg1, do_mask,
                                                         pw, tid, l_st, l_en, l_col);
            // this thread's elements of the segment
            unsigned act = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (e0 + q >= o && e0 + q < seg1) act |= 1u << q;
            const int kb = (int)(e0 - o);  // the staged column under element e0 (meaningful where act != 0)
            for (int m = 0; m < pw.n_mats; m++) {
                if (FILL && as_global(counts)[(int64_t)m * tiles + tile] == 0) continue;  // (the same for every thread: no barrier is left out by some)
                const int row0 = g_mat[m], w_m = g_mat[m + 1] - row0;
                const float *val = l_val + row0 * n_cols;
                if (!resident) {
                    __syncthreads();  // the matrix before has been read
                    for (int k = tid; k < w_m * n_cols; k += PW_THREADS) l_val[k] = g_val[row0 * n_cols + k];
                    __syncthreads();
                    val = l_val;
                }
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                unsigned bad = 0;
                if (act) {
                    for (int jj = 0; jj < w_m + 3; jj++) {
                        const int idx = kb + jj;
                        if (idx < 0 || idx >= n_stage) continue;  // (under no window of an element of the segment)
                        const int c = l_col[idx];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int j = jj - q;
                            if (j < 0 || j >= w_m) continue;
                            if (c < 0) bad |= 1u << q;
                            else acc[q] += val[j * n_cols + c];
                        }
                    }
                }
                // this thread's hits (a NaN compares false), their rank among the workgroup's, the tile's count so far
                const float least = thr.t[m];
                unsigned hit = 0;
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (((act >> q) & 1u) && !((bad >> q) & 1u) && acc[q] >= least) hit |= 1u << q;
                const int mine = __builtin_popcount(hit);
                const int upto = PH_WAVE_PREFIX(mine);  // the wave's hits up to and including this thread's
                const int set = (int)(turn++ & 1u);     // (the set the step before used may still be being read)
                const int run = l_run[m];               // (written before this segment's barriers at the latest)
                if ((tid & 63) == 63) l_wave[set][tid >> 6] = upto;
                __syncthreads();
                int before = 0, all = 0;
#pragma unroll
                for (int w = 0; w < PW_THREADS / 64; w++) {
                    const int x = l_wave[set][w];
                    if (w < (tid >> 6)) before += x;
                    all += x;
                }
                if (tid == 0) l_run[m] = run + all;
                if (FILL && hit) {
                    int64_t at = as_global(bases)[(int64_t)m * tiles + tile] + run + before + (upto - mine);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (!((hit >> q) & 1u)) continue;
                        as_global(hit_row)[at] = (int32_t)r;
                        as_global(hit_pos)[at] = (int32_t)(e0 + q - r_lo);
                        reinterpret_cast<int32_t BX_GLOBAL *>(as_global(hit_score))[at] = (int)pw_bits(acc[q]);
                        at++;
                    }
                }
            }
            o = seg1;
        }
        __syncthreads();  // the last step's running counts are written; the next tile begins them anew
        if (!FILL && tid < pw.n_mats) as_global(counts)[(int64_t)tid * tiles + tile] = l_run[tid];
    }
}

// track_of, start, row_off, width: the whole batch, as pw_scores_kernel<true> is given it; `total` is exact.  tiles ==
// ceil(total / PW_TILE) is the stride of counts and bases.  FILL: counts is read; else it is written and bases and the hit arrays
// are not used.
template <bool FILL>
__global__ __launch_bounds__(PW_THREADS) void pw_hits_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                             const int32_t *__restrict__ start, int64_t n_rows, int width,
                                                             const int64_t *__restrict__ row_off, int64_t total, int do_mask, PwSet pw, PhThresholds thr,
                                                             int64_t tile_first, int64_t tile_count, int64_t tiles, int32_t *counts,
                                                             const int64_t *__restrict__ bases, int32_t *__restrict__ hit_row, int32_t *__restrict__ hit_pos,
                                                             float *__restrict__ hit_score)
{
    pw_hits_body<false, FILL>(table, n_tracks, track_of, start, nullptr, n_rows, width, row_off, total, do_mask, pw, thr, tile_first, tile_count, tiles, counts,
                              bases, hit_row, hit_pos, hit_score);
}

// the same with strand[n_rows] of the batch
template <bool FILL>
__global__ __launch_bounds__(PW_THREADS) void pw_hits_strand_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                    const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows,
                                                                    int width, const int64_t *__restrict__ row_off, int64_t total, int do_mask, PwSet pw,
                                                                    PhThresholds thr, int64_t tile_first, int64_t tile_count, int64_t tiles, int32_t *counts,
                                                                    const int64_t *__restrict__ bases, int32_t *__restrict__ hit_row,
                                                                    int32_t *__restrict__ hit_pos, float *__restrict__ hit_score)
{
    pw_hits_body<true, FILL>(table, n_tracks, track_of, start, strand, n_rows, width, row_off, total, do_mask, pw, thr, tile_first, tile_count, tiles, counts,
                             bases, hit_row, hit_pos, hit_score);
}

// heads[m] = bases[m * tiles], m in [0, count): where each matrix's part of the list begins, and (bases[n_mats * tiles]) where it ends
__global__ __launch_bounds__(64) void ph_heads_kernel(const int64_t *__restrict__ bases, int64_t tiles, int count, int64_t *__restrict__ heads)
{
    const int m = (int)threadIdx.x;
    if (m < count) as_global(heads)[m] = as_global(bases)[(int64_t)m * tiles];
}

}  // namespace bxmi

// profile.hpp -- site profiles over a batch of windows (the reference's scripts/bed_bigwig_profile.py:27-41): for every offset j
// of a window of `width` bases, the float64 sum of the scores the n windows have at that offset and the number of windows that
// have a score there.  Included by scores.hip (the entry points bxmi_scores_profile*).
//
// Window i reads positions win_start[i] + j (int64, so any int32 start is legal) of track track_of[i]; a position outside
// [0, size) of its track, a NaN there, a track_of of -1: no score.  Unlike the aggregation of scores.hpp, +-0 IS a score here.
//
// The total of column j is the reference's: a float64 accumulator that starts as +0.0 and takes (double)v_ij for i = 0 .. n-1
// IN INPUT ORDER, one rounding per add; a missing score adds +0.0 (an exact identity: an accumulator that starts as +0.0 never
// becomes -0.0 under round-to-nearest, x + (-x) gives +0 and +0 + -0 = +0).  That chain is as long as the batch.  It is run in
// parallel whenever that provably gives the same bits:
//
//   Write a finite, non-zero float32 x as an integer multiple of 2^u(x), u(x) = max(exponent field, 1) - 150 (the unbiased
//   exponent minus 23; -149 for denormals).  For one column let q = min u(x) over its finite non-zero scores and S = sum |x|
//   over all its scores, in real arithmetic.  Every sum of any subset of the column is an integer multiple of 2^q of magnitude
//   <= S.  If S < 2^(q+53) it is k * 2^q with |k| < 2^53, which float64 holds exactly (q >= -149 and q + 53 <= 157: no
//   underflow, no overflow).  Then every partial sum of every order and grouping is exact, every add rounds nothing, and the
//   chunked sum below IS the ordered chain, bit for bit.  (Partial sums start as +0.0 too, so no -0.0 appears anywhere.)
//   S itself is computed in float64 in whatever order the chunks give: for m non-negative terms any order of rounded adds
//   returns S' >= S * (1 - g), g = (m-1) * 2^-53 / (1 - (m-1) * 2^-53) < 2^-21 for m <= 2^31, so S < S' * (1 + 2^-20).  The
//   test is therefore  S' * (1 + 2^-20) < 2^(q+53) : conservative, never wrong.  An inf makes S' inf and fails it; a column
//   without a finite non-zero score passes (its sum is +0.0, or there is an inf and S' fails it first).
//   (A bound by count and largest exponent, n * 2^(E+1), is up to two bits looser: a million three-decimal scores of [0, 1]
//   would miss it by one bit, S' passes with room.)
//
//   track_table_kernel (track_batch.hpp, 16 tracks per launch) writes the table PfTrack[n_tracks + 1] the others read.
//   pf_partial_kernel  a wave owns 64 adjacent columns (lane = column) and one chunk of PF_CHUNK consecutive windows.  The
//                      window's track and start are wave-uniform; the 64 lanes read 64 consecutive floats with one coalesced,
//                      generally unaligned load, PF_AHEAD windows' loads in flight (pf_meta / pf_fetch).  Per lane: the float64
//                      sum (even and odd windows in two accumulators, added at the end), S', the count of scores and q,
//                      stored to scratch [chunks][width].  No floating-point atomics.
//   pf_combine_kernel  a lane per column folds the chunks in chunk order, writes totals[j] and valid[j] (exact either way) and
//                      tests the column; a wave that holds a column failing the test appends its 64-column group to a list.
//   pf_chain_kernel    a wave per listed group walks ALL n windows in input order, PF_CHAIN_AHEAD coalesced loads ahead of
//                      the adds, and every lane runs t += (double)v; the listed columns' totals are overwritten.  PROVIDED the
//                      file is built without fast-math and without flushing denormals (csrc/build.sh: plain -O3).  A chain
//                      costs n dependent float64 adds however many CUs there are.
#pragma once

namespace bxmi {

constexpr int PF_CHUNK = 2048;        // windows per chunk of the partial pass
constexpr int PF_AHEAD = 8;           // windows whose loads a wave of the partial pass keeps in flight
constexpr int PF_CHAIN_AHEAD = 16;    // the same for the chain, which has nothing else to hide its loads behind
constexpr int PF_THREADS = 256;       // partial pass and combine: 4 waves
constexpr int PF_Q_NONE = 1 << 20;    // q of a column (chunk) without a finite non-zero score

struct PfTrack {
    const float *values;
    int64_t size;
};

// What a wave needs of 64 consecutive windows, window base + l in lane l: its track's array and size (0 where the window has
// no track or lies beyond `end`) and its start.  Three vector loads per 64 windows; pf_fetch hands a window's triple to the
// whole wave through v_readlane, so no load of the walk depends on a scalar load issued just before it.
struct PfMeta {
    int ptr_lo, ptr_hi;
    int size;
    int start;
};

__device__ __forceinline__ PfMeta pf_meta(const PfTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                          const int32_t *__restrict__ win_start, int64_t base, int64_t end)
{
    const int64_t i = base + lane_id();
    const bool in = i < end;
    const int t = in ? track_of[i] : -1;
    const int s = in ? win_start[i] : 0;
    const bool has = t >= 0 && t < n_tracks;
    const PfTrack tr = table[has ? t : n_tracks];  // (the spare entry: size 0, valid memory)
    const unsigned long long p = (unsigned long long)reinterpret_cast<uintptr_t>(tr.values);
    return PfMeta{(int)(unsigned)(p & 0xffffffffull), (int)(unsigned)(p >> 32), has ? (int)tr.size : 0, s};
}

// Lane `col`'s score in window r (wave-uniform, 0 .. 63) of the 64 that `m` describes, NaN where it has none.  The load is
// unconditional so that several are in flight: a lane with nothing to fetch reads word 0 of the window's track.
__device__ __forceinline__ float pf_fetch(const PfMeta &m, int r, int64_t col, bool col_ok)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane(m.ptr_lo, r), hi = (unsigned)__builtin_amdgcn_readlane(m.ptr_hi, r);
    const int64_t size = __builtin_amdgcn_readlane(m.size, r);
    const int64_t p = (int64_t)__builtin_amdgcn_readlane(m.start, r) + col;
    const float *values = reinterpret_cast<const float *>((uintptr_t)(((unsigned long long)hi << 32) | lo));
    const bool ok = col_ok && p >= 0 && p < size;
    const float x = as_global(values)[ok ? p : 0];
    return ok ? x : __builtin_nanf("");
}

// One wave per (chunk, 64-column group); adjacent waves take adjacent groups of the same chunk.
__global__ __launch_bounds__(PF_THREADS) void pf_partial_kernel(const PfTrack *__restrict__ table, int n_tracks,
                                                                const int32_t *__restrict__ track_of, const int32_t *__restrict__ win_start,
                                                                int64_t n, int64_t width, int64_t groups, int64_t items,
                                                                double *__restrict__ p_sum, double *__restrict__ p_abs,
                                                                int32_t *__restrict__ p_valid, int32_t *__restrict__ p_q)
{
    const int lane = lane_id();
    const int64_t item = (int64_t)blockIdx.x * (PF_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= items) return;
    const int64_t chunk = item / groups, group = item - chunk * groups;
    const int64_t col = group * 64 + lane;
    const bool col_ok = col < width;
    const int64_t first = chunk * PF_CHUNK, end = first + PF_CHUNK < n ? first + PF_CHUNK : n;
    double sum[2] = {0.0, 0.0}, sabs = 0.0;  // even and odd windows apart: two dependent-add chains of half the length
    int valid = 0, q = PF_Q_NONE;
    for (int64_t base = first; base < end; base += 64) {
        const PfMeta m = pf_meta(table, n_tracks, track_of, win_start, base, end);
        for (int r = 0; r < 64 && base + r < end; r += PF_AHEAD) {
            float v[PF_AHEAD];
#pragma unroll
            for (int k = 0; k < PF_AHEAD; k++) v[k] = pf_fetch(m, r + k, col, col_ok);
#pragma unroll
            for (int k = 0; k < PF_AHEAD; k++) {
                const float x = v[k];
                const bool ok = x == x;
                const double d = ok ? (double)x : 0.0;
                sum[k & 1] += d;
                sabs += __builtin_fabs(d);
                valid += ok ? 1 : 0;
                const int ef = (__float_as_int(x) >> 23) & 0xff;
                const int u = (ef > 1 ? ef : 1) - 150;
                q = ok && x != 0.0f && u < q ? u : q;
            }
        }
    }
    if (col_ok) {
        const int64_t at = chunk * width + col;
        p_sum[at] = sum[0] + sum[1];
        p_abs[at] = sabs;
        p_valid[at] = valid;
        p_q[at] = q;
    }
}

// A lane per column.  chain_mode (scores.profile_chain): 0 = the columns that fail the test go to the chain, 1 = all of them,
// -1 = none.  A wave's columns are one group; *n_listed and *chain_columns are zeroed by the host.
__global__ __launch_bounds__(PF_THREADS) void pf_combine_kernel(const double *__restrict__ p_sum, const double *__restrict__ p_abs,
                                                                const int32_t *__restrict__ p_valid, const int32_t *__restrict__ p_q,
                                                                int64_t chunks, int64_t width, int chain_mode, double *__restrict__ totals,
                                                                int32_t *__restrict__ valid, int32_t *__restrict__ col_flag,
                                                                int32_t *__restrict__ group_list, int32_t *__restrict__ n_listed,
                                                                unsigned long long *__restrict__ chain_columns)
{
    const int64_t col = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x;
    const bool col_ok = col < width;
    double t = 0.0, a = 0.0;
    int v = 0, q = PF_Q_NONE;
    if (col_ok)
        for (int64_t c = 0; c < chunks; c++) {
            const int64_t at = c * width + col;
            t += p_sum[at];
            a += p_abs[at];
            v += p_valid[at];
            const int cq = p_q[at];
            q = cq < q ? cq : q;
        }
    const bool exact = q == PF_Q_NONE ? a == 0.0 : a * (1.0 + 0x1p-20) < __builtin_ldexp(1.0, q + 53);
    const bool take = col_ok && (chain_mode > 0 || (chain_mode == 0 && !exact));
    if (col_ok) {
        totals[col] = t;
        valid[col] = v;
        col_flag[col] = take ? 1 : 0;
    }
    const unsigned long long takers = __ballot(take);
    if (takers && lane_id() == 0) {
        atomicAdd(chain_columns, (unsigned long long)__popcll(takers));
        group_list[atomicAdd(n_listed, 1)] = (int32_t)(col >> 6);
    }
}

// One wave (== one workgroup) per listed group; the grid is sized for "every group is listed".
__global__ __launch_bounds__(64) void pf_chain_kernel(const PfTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                      const int32_t *__restrict__ win_start, int64_t n, int64_t width,
                                                      const int32_t *__restrict__ col_flag, const int32_t *__restrict__ group_list,
                                                      const int32_t *__restrict__ n_listed, double *__restrict__ totals)
{
    if ((int)blockIdx.x >= *n_listed) return;
    const int64_t col = (int64_t)group_list[blockIdx.x] * 64 + lane_id();
    const bool col_ok = col < width;
    double t = 0.0;
    PfMeta m = pf_meta(table, n_tracks, track_of, win_start, 0, n);
    float cur[PF_CHAIN_AHEAD];
#pragma unroll
    for (int k = 0; k < PF_CHAIN_AHEAD; k++) cur[k] = pf_fetch(m, k, col, col_ok);
    for (int64_t base = 0; base < n; base += 64) {
        // the next 64 windows' triples and the next PF_CHAIN_AHEAD windows' scores are on their way while this stretch of the
        // chain runs; windows beyond n have no score and add +0.0
        const PfMeta m_next = pf_meta(table, n_tracks, track_of, win_start, base + 64, n);
#pragma unroll
        for (int r = 0; r < 64; r += PF_CHAIN_AHEAD) {
            float next[PF_CHAIN_AHEAD];
#pragma unroll
            for (int k = 0; k < PF_CHAIN_AHEAD; k++)
                next[k] = r + PF_CHAIN_AHEAD < 64 ? pf_fetch(m, r + PF_CHAIN_AHEAD + k, col, col_ok) : pf_fetch(m_next, k, col, col_ok);
#pragma unroll
            for (int k = 0; k < PF_CHAIN_AHEAD; k++) {
                const float x = cur[k];
                t += x == x ? (double)x : 0.0;  // the ordered chain: exactly one float64 add per window
                cur[k] = next[k];
            }
        }
        m = m_next;
    }
    if (col_ok && col_flag[col]) totals[col] = t;
}

}  // namespace bxmi

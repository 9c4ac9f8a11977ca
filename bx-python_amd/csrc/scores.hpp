// scores.hpp -- per-base score tracks and their aggregation over intervals (the reference's
// scripts/aggregate_scores_in_intervals.py:107-134 over lib/bx/binned_array.py): count, sum, minimum and maximum of the
// valid scores of every interval of a batch in one device pass.  Included by scores.hip (the entry points bxmi_scores_*).
//
// A track is a dense float32 array [0, size), NaN = no score.  A base is VALID when its score is neither NaN nor +-0 and its
// bit in the optional mask (the LSB-first words of a bxmi_bits_t) is clear; positions outside the track have no score, positions
// at or beyond the mask's size are not masked.
//
// The sum is the reference's: a float32 accumulator that takes the valid scores IN POSITION ORDER, one rounding per add
// (`total += score` on numpy.float32, :123).  No tree, no wider accumulator, no reassociation -- any of them changes the
// last bits on most intervals.  So the sum of one interval is a serial chain of v_add_f32; the parallelism is across
// intervals (row path) and between a chain and the loads that feed it.  The chain is branch-free: a skipped base adds
// +0.0f, which is an exact identity because the accumulator starts as +0.0f and can never become -0.0f (x + (-x) rounds
// to +0 in round-to-nearest, -0 is never added), PROVIDED float32 denormals are not flushed and the file is not built with
// fast-math (csrc/build.sh: plain -O3).  Minimum and maximum are plain comparisons on valid scores.
//
//   sc_bucket_*      rows of one wave should be of similar length (a wave walks until its longest row is done): the short
//                    intervals are ordered by their number of 64-base steps, longest first, with a counting sort that never
//                    comes back to the host -- per-workgroup LDS histograms into 512 buckets, a one-workgroup scan, a scatter
//                    that reserves a workgroup's places with one atomic per bucket.  Results go to the caller's order.  The
//                    count pass also lists the intervals of at least `wave_min_len` bases inside the track for the wave kernel.
//   sc_rows_kernel   a wave owns 64 neighbours of that order ("rows"), one per lane.  Per step the wave loads the next 64 floats
//                    of each unfinished row with one coalesced 256-byte load per row into an LDS tile of 64 x 65 words (the
//                    pad makes lane r's walk along row r hit 64 different banks), then lane r runs its own row's chain over
//                    the 64 words.  Lane r fetches the two mask words of its 64 bases itself.
//   sc_wave_kernel   a wave per listed interval: coalesced 64-float loads, the count by ballot, minimum and maximum per lane
//                    and a wave reduction at the end, the sum chain fed lane by lane through v_readlane.
//   sc_fill_kernel   values[start[i] .. end[i]) = value[i] for ascending, disjoint spans (one launch per such run).
#pragma once

namespace bxmi {

constexpr int SC_ROWS = 64;          // rows of a wave == lanes
constexpr int SC_PITCH = 65;         // words per LDS row: 64 + 1 pad
constexpr int SC_WAVE_THREADS = 256; // sc_wave_kernel: 4 waves, an interval each
constexpr int SC_FILL_THREADS = 256;
constexpr int SC_BUCKETS = 512;      // by steps of 64 bases, longest first; the last step count stands for "that many or more"
constexpr int SC_ORD_THREADS = 256;
constexpr int SC_ORD_ITEMS = 8;      // intervals per thread of the scatter
// the ordering's counters, int32: [0, SC_BUCKETS) the histogram, then each bucket's cursor, then the number of rows
constexpr int SC_WORK_INTS = 2 * SC_BUCKETS + 1;

struct ScMask {
    const unsigned long long *words;  // NULL = no mask
    int64_t nwords;
    int64_t size;                     // bits at or beyond it read as clear
};

// The 64 mask bits of positions p .. p + 63 (bit j = position p + j), p >= 0.
__device__ __forceinline__ unsigned long long sc_mask_bits(const ScMask &M, int64_t p)
{
    if (!M.words) return 0ull;
    const int64_t left = M.size - p;
    if (left <= 0) return 0ull;
    const int64_t w = p >> 6;
    const int sh = (int)(p & 63);
    unsigned long long m = w < M.nwords ? M.words[w] >> sh : 0ull;
    if (sh && w + 1 < M.nwords) m |= M.words[w + 1] << (64 - sh);
    if (left < 64) m &= (1ull << left) - 1ull;
    return m;
}

// [s, e) clipped to the track; an empty or inverted interval comes back with e <= s.
__device__ __forceinline__ void sc_clip(int s, int e, int64_t size, int64_t *cs, int64_t *ce)
{
    *cs = s > 0 ? (int64_t)s : 0;
    *ce = (int64_t)e < size ? (int64_t)e : size;
}

// lane l's value as a wave-uniform one (l is a constant after unrolling: v_readlane_b32, no LDS crossbar)
__device__ __forceinline__ float sc_readlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int64_t sc_readlane(int64_t v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
    return ((int64_t)hi << 32) | (int64_t)lo;
}

__device__ __forceinline__ int sc_bucket(int64_t len)
{
    const int64_t steps = (len + 63) >> 6;
    return SC_BUCKETS - 1 - (steps < SC_BUCKETS - 1 ? (int)steps : SC_BUCKETS - 1);
}

// Histogram of the short intervals' buckets; the others go to long_list (long_list[0] counts them, long_list[1 ..] are their
// indices; both it and `work` are zeroed by the host).
__global__ __launch_bounds__(SC_ORD_THREADS) void sc_bucket_count_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ end, int64_t n,
                                                                         int64_t size, int64_t wave_min_len, int32_t *__restrict__ work,
                                                                         int32_t *__restrict__ long_list)
{
    __shared__ int h[SC_BUCKETS];
    for (int t = threadIdx.x; t < SC_BUCKETS; t += SC_ORD_THREADS) h[t] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * SC_ORD_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SC_ORD_THREADS) {
        int64_t cs, ce;
        sc_clip(start[i], end[i], size, &cs, &ce);
        const int64_t len = ce > cs ? ce - cs : 0;
        if (len >= wave_min_len) long_list[1 + atomicAdd(long_list, 1)] = (int32_t)i;
        else atomicAdd(&h[sc_bucket(len)], 1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < SC_BUCKETS; t += SC_ORD_THREADS)
        if (h[t]) atomicAdd(&work[t], h[t]);
}

// One workgroup: cursor[b] = the rows of the buckets before b, and their total.
__global__ __launch_bounds__(SC_BUCKETS) void sc_bucket_scan_kernel(int32_t *__restrict__ work)
{
    __shared__ int a[SC_BUCKETS];
    const int t = threadIdx.x, v = work[t];
    a[t] = v;
    __syncthreads();
    for (int off = 1; off < SC_BUCKETS; off <<= 1) {
        const int x = t >= off ? a[t - off] : 0;
        __syncthreads();
        a[t] += x;
        __syncthreads();
    }
    work[SC_BUCKETS + t] = a[t] - v;
    if (t == SC_BUCKETS - 1) work[2 * SC_BUCKETS] = a[t];
}

// order[] = the short intervals, bucket by bucket.  A workgroup takes SC_ORD_THREADS * SC_ORD_ITEMS consecutive intervals,
// reserves its places in every bucket with one atomic on the bucket's cursor and hands them out through an LDS counter.
__global__ __launch_bounds__(SC_ORD_THREADS) void sc_bucket_scatter_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ end, int64_t n,
                                                                           int64_t size, int64_t wave_min_len, int32_t *__restrict__ work,
                                                                           int32_t *__restrict__ order)
{
    __shared__ int h[SC_BUCKETS], base[SC_BUCKETS];
    for (int t = threadIdx.x; t < SC_BUCKETS; t += SC_ORD_THREADS) h[t] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * (SC_ORD_THREADS * SC_ORD_ITEMS);
    int bucket[SC_ORD_ITEMS];
#pragma unroll
    for (int k = 0; k < SC_ORD_ITEMS; k++) {
        const int64_t i = first + k * SC_ORD_THREADS + threadIdx.x;
        bucket[k] = -1;
        if (i < n) {
            int64_t cs, ce;
            sc_clip(start[i], end[i], size, &cs, &ce);
            const int64_t len = ce > cs ? ce - cs : 0;
            if (len < wave_min_len) {
                bucket[k] = sc_bucket(len);
                atomicAdd(&h[bucket[k]], 1);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < SC_BUCKETS; t += SC_ORD_THREADS) {
        base[t] = h[t] ? atomicAdd(&work[SC_BUCKETS + t], h[t]) : 0;
        h[t] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SC_ORD_ITEMS; k++)
        if (bucket[k] >= 0) order[base[bucket[k]] + atomicAdd(&h[bucket[k]], 1)] = (int32_t)(first + k * SC_ORD_THREADS + threadIdx.x);
}

// One wave (== one workgroup) per 64 rows of the order.
__global__ __launch_bounds__(SC_ROWS) void sc_rows_kernel(const float *__restrict__ values, int64_t size, ScMask M,
                                                          const int32_t *__restrict__ start, const int32_t *__restrict__ end,
                                                          const int32_t *__restrict__ work, const int32_t *__restrict__ order,
                                                          int32_t *__restrict__ count, float *__restrict__ sum, float *__restrict__ vmin,
                                                          float *__restrict__ vmax)
{
    __shared__ float tile[SC_ROWS * SC_PITCH];
    const int lane = (int)threadIdx.x;
    const int64_t n_rows = work[2 * SC_BUCKETS];
    if ((int64_t)blockIdx.x * SC_ROWS >= n_rows) return;  // (the grid is sized for "every interval is a row")
    const int64_t row = (int64_t)blockIdx.x * SC_ROWS + lane;
    int64_t pos = 0, ce = 0, i = -1;
    if (row < n_rows) {
        i = order[row];
        sc_clip(start[i], end[i], size, &pos, &ce);
    }
    float total = 0.0f, mn = INFINITY, mx = -INFINITY;
    int cnt = 0;
    while (__any(pos < ce)) {
        // the tile: row r = the next 64 floats of lane r's interval, 0.0f beyond its end.  The loads are unconditional (a lane with
        // nothing to fetch reads values[0]) so that eight of them are in flight before the first one is waited for.
#pragma unroll
        for (int r0 = 0; r0 < SC_ROWS; r0 += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int64_t rp = sc_readlane(pos, r0 + k), re = sc_readlane(ce, r0 + k);  // wave-uniform
                const int64_t p = rp + lane;
                const float x = values[p < re ? p : 0];
                v[k] = p < re ? x : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) tile[(r0 + k) * SC_PITCH + lane] = v[k];
        }
        __syncthreads();
        if (pos < ce) {
            const unsigned long long mbits = sc_mask_bits(M, pos);
            const int left = ce - pos < 64 ? (int)(ce - pos) : 64;
            const float *row = tile + lane * SC_PITCH;
#pragma unroll 16
            for (int j = 0; j < 64; j++) {
                const float v = row[j];
                const bool ok = j < left && v == v && v != 0.0f && !((mbits >> j) & 1ull);
                total += ok ? v : 0.0f;  // the ordered chain: exactly one float32 add per valid base
                cnt += ok ? 1 : 0;
                mn = ok && v < mn ? v : mn;
                mx = ok && v > mx ? v : mx;
            }
            pos += 64;
        }
        __syncthreads();
    }
    if (i >= 0) {
        count[i] = cnt;
        sum[i] = total;
        vmin[i] = mn;
        vmax[i] = mx;
    }
}

// A wave per listed interval.
__global__ __launch_bounds__(SC_WAVE_THREADS) void sc_wave_kernel(const float *__restrict__ values, int64_t size, ScMask M,
                                                                  const int32_t *__restrict__ start, const int32_t *__restrict__ end,
                                                                  int32_t *__restrict__ count, float *__restrict__ sum, float *__restrict__ vmin,
                                                                  float *__restrict__ vmax, const int32_t *__restrict__ long_list)
{
    const int lane = lane_id();
    const int waves = SC_WAVE_THREADS / 64;
    const int n_long = long_list[0];
    for (int w = blockIdx.x * waves + (threadIdx.x >> 6); w < n_long; w += gridDim.x * waves) {
        const int64_t i = long_list[1 + w];
        int64_t cs, ce;
        sc_clip(start[i], end[i], size, &cs, &ce);
        float total = 0.0f, mn = INFINITY, mx = -INFINITY;
        int cnt = 0;
        float next = values[cs + lane < ce ? cs + lane : 0];  // (a lane beyond the end reads values[0] and drops it)
        for (int64_t p = cs; p < ce; p += 64) {
            const int64_t q = p + lane;
            const float v = next;
            next = values[q + 64 < ce ? q + 64 : 0];              // the next 64 floats are on their way while this chain runs
            const unsigned long long mbits = sc_mask_bits(M, p);  // wave-uniform
            const bool ok = q < ce && v == v && v != 0.0f && !((mbits >> lane) & 1ull);
            cnt += __popcll(__ballot(ok));
            mn = ok && v < mn ? v : mn;
            mx = ok && v > mx ? v : mx;
            const float x = ok ? v : 0.0f;
#pragma unroll
            for (int j = 0; j < 64; j++) total += sc_readlane(x, j);  // position order, every lane runs the same chain
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if (lane == 0) {
            count[i] = cnt;
            sum[i] = total;
            vmin[i] = mn;
            vmax[i] = mx;
        }
    }
}

// values[start[i] .. end[i]) = value[i], spans clipped to the track.  The spans of one launch are disjoint, so the order of the
// stores between them does not matter.  A lane takes a short span by itself; spans of 64 bases or more are then stored by
// the whole wave, one after the other.
__global__ __launch_bounds__(SC_FILL_THREADS) void sc_fill_kernel(float *__restrict__ values, int64_t size, const int32_t *__restrict__ start,
                                                                  const int32_t *__restrict__ end, const float *__restrict__ value, int64_t n)
{
    const int lane = lane_id();
    const int64_t stride = (int64_t)gridDim.x * SC_FILL_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * SC_FILL_THREADS + (threadIdx.x - lane); base < n; base += stride) {
        const int64_t i = base + lane;
        int64_t cs = 0, ce = 0;
        float v = 0.0f;
        if (i < n) {
            sc_clip(start[i], end[i], size, &cs, &ce);
            v = value[i];
        }
        const bool wide = ce - cs >= 64;
        if (!wide)
            for (int64_t p = cs; p < ce; p++) values[p] = v;
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t ws = __shfl(cs, src, 64), we = __shfl(ce, src, 64);
            const float wv = __shfl(v, src, 64);
            for (int64_t p = ws + lane; p < we; p += 64) values[p] = wv;
        }
    }
}

// values[0 .. n) = NaN (a new track)
__global__ __launch_bounds__(SC_FILL_THREADS) void sc_nan_kernel(float *__restrict__ values, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * SC_FILL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SC_FILL_THREADS)
        values[i] = __builtin_nanf("");
}

}  // namespace bxmi

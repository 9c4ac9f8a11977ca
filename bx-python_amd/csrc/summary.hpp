// summary.hpp -- binned summaries of span tracks over a batch of regions (the reference's BigWigFile.summarize_from_full:
// lib/bx/bbi/bbi_file.pyx:80-111 under bigwig_file.pyx:93-108, 176-185).  Included by summary.hip (bxmi_spans_*).
//
// A span track is one chromosome's bigWig items (start, end, value) as three arrays in HBM, IN FILE ORDER.  For region i =
// [start[i], end[i]) of tracks[track_of[i]] and `size` bins, step = (end - start) / size (integer), bin j = [start + step * j,
// start + step * (j + 1)); the last (end - start) % size bases belong to no bin, and step == 0 leaves every bin empty.  Every item
// is clipped to the region (dropped when nothing is left) and then, for every bin it overlaps, in item order:
//     n = clipped length, w = (double)n * ((double)overlap / n)      -- NOT always the integer overlap: 22 * (15.0 / 22) != 15
//     valid += w;  sum += (double)val * w;  sumsq += (double)(val * val) * w   (the square in float32, as the reference takes it)
//     if (max < val) max = val;  if (min > val) min = val                      (in double; a NaN value changes neither)
// from valid = sum = sumsq = 0, min = +inf, max = -inf; at the end valid = rint(valid) (Python's round: half to even).  Each bin is
// therefore an ordered float64 chain over its items, and the five planes come out bit for bit as the reference's.
//
// FLOATING-POINT CONTRACTION IS OFF for these kernels (`#pragma clang fp contract(off)` at the top of summary.hip, before this
// header): hipcc would otherwise fuse sum += val * w into one fused multiply-add with a single rounding, and the reference's
// x86-64 build rounds the product and the sum separately.  Float64 division on gfx950 is correctly rounded (its expansion uses
// fused operations internally; that is the division's own algorithm, not a contraction of the chain).
//
//   track_table_kernel (track_batch.hpp, 8 tracks per launch) writes the table SmTrack[n_tracks + 1] that sm_summary_kernel reads.
//   sm_summary_kernel  one wave (== one workgroup) per region.  Bins are taken 64 at a time, lane = bin; the lane keeps its bin's
//                      five accumulators in registers across all chunks of items and writes them once, so the five [n, size]
//                      planes are written coalesced along the bin axis.
//     ordered tracks   (starts AND ends non-decreasing -- every real bigWig): the items that overlap any range are ONE contiguous
//                      run, already in file order.  One binary search pair finds the region's run, one more (inside that run)
//                      the run of each group of 64 bins; the run is streamed through LDS SM_CHUNK items at a time by coalesced
//                      loads, and every lane walks, in order, only the items of the chunk that overlap ITS bin (a binary search
//                      in LDS for the first one): bin-major, so a track of one-base spans keeps all 64 lanes busy.
//     other tracks     (overlapping or out-of-order items): the general path.  The wave walks ALL items of the track in file order
//                      through the same LDS staging, every lane testing every item against its bin, once per group of 64 bins.
//                      CORRECT AND SLOW: a region costs the whole track.  It exists so that no track is refused.
//   A row without a track (track_of outside [0, n_tracks)), with start >= end or with a negative coordinate is an EMPTY ROW:
//   (0, +inf, -inf, 0, 0) in every bin.
#pragma once

namespace bxmi {

constexpr int SM_CHUNK = 256;        // items staged in LDS at a time (3 KiB per workgroup)
constexpr int SM_THREADS = 64;       // one wave per region

struct SmTrack {
    const int32_t *start;
    const int32_t *end;
    const float *value;
    int64_t n;
    int64_t ordered;
};

struct SmAcc {
    double valid, mn, mx, sum, sumsq;
};

// A kernel's row: region [s, e) of the track whose table entry is `tr`; `has`: the row names a track and a region, else it is an
// EMPTY ROW and `tr` the spare entry (nothing in it); step: bases per bin.
template <typename Entry>
struct SmRow {
    Entry tr;
    int s, e;
    bool has;
    int step;
};
template <typename Entry>
__device__ __forceinline__ SmRow<Entry> sm_row(const Entry *table, int n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                                               int64_t row, int size)
{
    const int t = track_of[row], s = start[row], e = end[row];
    const bool has = t >= 0 && t < n_tracks && s >= 0 && s < e;
    const Entry tr = table[has ? t : n_tracks];
    return SmRow<Entry>{tr, s, e, has, has ? (e - s) / size : 0};
}

// Bins [g0, g1) of a row, 64 at a time, lane = bin: this lane's bin is [b0, b1) where `ok`.  (g0 is 64-bit in the kernels' loops:
// g0 + 64 may pass 2^31 for a size near it; s + step * bin <= e for bin <= size, so the bases fit an int.)
struct SmGroup {
    int64_t g1, bin;
    bool ok;
    int b0, b1;
};
__device__ __forceinline__ SmGroup sm_group(int64_t g0, int size, int lane, int s, int step)
{
    const int64_t g1 = g0 + 64 < size ? g0 + 64 : size;
    const int64_t bin = g0 + lane;
    const bool ok = bin < g1;
    const int b0 = ok ? (int)(s + (int64_t)step * bin) : 0;
    return SmGroup{g1, bin, ok, b0, ok ? b0 + step : 0};
}

// The weight w of the item [st, en) in the bin [b0, b1) of the region [s, e); false when the item, clipped to the region, does not
// overlap the bin.  The one place where a weight is computed: bigWig items (sm_item) and bigBed records (bd_item) share its bits.
__device__ __forceinline__ bool sm_weight(double &w, int st, int en, int s, int e, int b0, int b1)
{
    const int cs = st > s ? st : s, ce = en < e ? en : e;
    if (cs >= ce) return false;
    const int ov = (ce < b1 ? ce : b1) - (cs > b0 ? cs : b0);
    if (ov <= 0) return false;
    const int n = ce - cs;
    // (x / x == 1.0 exactly, so an item inside the bin weighs (double)n without the division: the same bits)
    w = ov == n ? (double)n : (double)n * ((double)ov / (double)n);
    return true;
}

// One item against one bin [b0, b1) of the region [s, e): the body of accumulate_interval_value (bbi_file.pyx:90-111).
__device__ __forceinline__ void sm_item(SmAcc &a, int st, int en, float val, int s, int e, int b0, int b1)
{
    double w;
    if (!sm_weight(w, st, en, s, e, b0, b1)) return;
    const double v = (double)val;
    a.valid += w;
    a.sum += v * w;
    a.sumsq += (double)(val * val) * w;
    if (a.mx < v) a.mx = v;
    if (a.mn > v) a.mn = v;
}

// first index in [lo, hi) whose key is > x (keys non-decreasing)
__device__ __forceinline__ int64_t sm_first_above(const int32_t BX_GLOBAL *keys, int64_t lo, int64_t hi, int x)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// first index in [lo, hi) whose key is >= x (keys non-decreasing)
__device__ __forceinline__ int64_t zm_first_at_least(const int32_t BX_GLOBAL *keys, int64_t lo, int64_t hi, int x)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] >= x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(SM_THREADS) void sm_summary_kernel(const SmTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                const int32_t *__restrict__ start, const int32_t *__restrict__ end, int size,
                                                                double *__restrict__ o_valid, double *__restrict__ o_min, double *__restrict__ o_max,
                                                                double *__restrict__ o_sum, double *__restrict__ o_sumsq)
{
    __shared__ int32_t l_st[SM_CHUNK], l_en[SM_CHUNK];
    __shared__ float l_val[SM_CHUNK];
    const int64_t row = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const auto [tr, s, e, has, step] = sm_row(table, n_tracks, track_of, start, end, row, size);
    const int32_t BX_GLOBAL *t_st = as_global(tr.start), *t_en = as_global(tr.end);
    const float BX_GLOBAL *t_val = as_global(tr.value);
    const bool ordered = tr.ordered != 0;
    // the region's items: [lo, hi)
    int64_t lo = 0, hi = 0;
    if (step > 0 && tr.n > 0) {
        hi = tr.n;
        if (ordered) {
            lo = sm_first_above(t_en, 0, tr.n, s);       // the first item that ends after the region starts
            hi = sm_first_above(t_st, lo, tr.n, e - 1);  // the first item that starts at or after its end
        }
    }
    const int64_t out0 = row * (int64_t)size;
    for (int64_t g0 = 0; g0 < size; g0 += 64) {
        const auto [g1, bin, ok, b0, b1] = sm_group(g0, size, lane, s, step);  // bins [g0, g1), this lane's [b0, b1)
        SmAcc a{0.0, __builtin_inf(), -__builtin_inf(), 0.0, 0.0};
        if (hi > lo) {
            int64_t glo = lo, ghi = hi;
            if (ordered) {
                glo = sm_first_above(t_en, lo, hi, (int)(s + (int64_t)step * g0));
                ghi = sm_first_above(t_st, glo, hi, (int)(s + (int64_t)step * g1 - 1));
            }
            for (int64_t pos = glo; pos < ghi; pos += SM_CHUNK) {
                const int cnt = ghi - pos < SM_CHUNK ? (int)(ghi - pos) : SM_CHUNK;
                __syncthreads();  // the previous chunk has been walked
                for (int k = lane; k < cnt; k += SM_THREADS) {
                    l_st[k] = t_st[pos + k];
                    l_en[k] = t_en[pos + k];
                    l_val[k] = t_val[pos + k];
                }
                __syncthreads();
                if (ok) {
                    int k = 0, last = cnt;
                    if (ordered) {
                        // this lane's items of the chunk: from the first that ends after b0, while they start before b1
                        int a0 = 0, a1 = cnt;
                        while (a0 < a1) {
                            const int mid = (a0 + a1) >> 1;
                            if (l_en[mid] > b0) a1 = mid;
                            else a0 = mid + 1;
                        }
                        k = a0;
                    }
                    for (; k < last; k++) {
                        const int st = l_st[k];
                        if (ordered && st >= b1) break;
                        sm_item(a, st, l_en[k], l_val[k], s, e, b0, b1);
                    }
                }
            }
        }
        if (ok) {
            o_valid[out0 + bin] = __builtin_rint(a.valid);
            o_min[out0 + bin] = a.mn;
            o_max[out0 + bin] = a.mx;
            o_sum[out0 + bin] = a.sum;
            o_sumsq[out0 + bin] = a.sumsq;
        }
    }
}

}  // namespace bxmi

// zoom_summary.hpp -- binned summaries FROM A ZOOM LEVEL over a batch of regions (the reference's ZoomLevel._summarize and
// _get_summary_slice: lib/bx/bbi/bbi_file.pyx:296-432 over cirtree_file.pyx:5-20, 49-105).  Included by summary.hip (bxmi_zoom_*),
// after summary.hpp and under the same `#pragma clang fp contract(off)`.
//
// A zoom track is one chromosome's part of one zoom level (bxmi.bigwig.read_zoom_file): its 32-byte summary records as seven
// arrays in HBM, IN LOAD ORDER, and the level's leaf entries for that chromosome -- leaf k covers bases (leaf_lo[k], leaf_hi[k])
// as the reference's overlap test sees them and holds records [leaf_first[k], leaf_first[k + 1]).  For a region [s, e) the
// reference loads, whole, every leaf with  s < leaf_hi && e > leaf_lo; then, for bin j = [b0, b1) = [s + step * j, s + step *
// (j + 1)), step = (e - s) / size, it drops records from the FRONT of that list while they end at or before b0 and
//     list empty:  valid = sum = sumsq = 0, min = max = NaN
//     else:        min, max = the front record's (whether or not it overlaps the bin); then over the records in order, until one
//                  starts at or after b1, for every one with overlap = min(b1, end) - max(b0, start) > 0:
//                      f = (float)((double)overlap / (double)(end - start))
//                      valid = (float)((double)valid + (double)rec.valid * (double)f)      likewise sum and sumsq
//                      if (max < rec.max) max = rec.max;  if (min > rec.min) min = rec.min   (a NaN changes neither)
// The accumulators are floats, but every product and every sum is ROUNDED IN DOUBLE and only the sum is then rounded to float: the
// reference's loop variable is an untyped object, so its build multiplies and adds Python floats and converts the result to its
// C float (recorded by tools/record_zoom_golden.py).  (double)float * (double)float is exact; (double)uint32 *
// (double)float is not once valid_count passes 2^29, which is why contraction must stay off here too.
//
// Only ORDERED tracks exist on the device (bxmi_zoom_create refuses others): record starts and ends both non-decreasing, leaf_lo
// and leaf_hi both non-decreasing.  Then the leaves a region loads are one run of leaves, its list one run of records [lo, hi),
// the front record of a bin is the first record of that run that ends after b0 -- a binary search, so every bin is independent of
// the others -- and the records a bin walks are contiguous from there.
//
//   zm_summary_kernel  one wave (== one workgroup) per region, lane = bin, 64 bins at a time, as sm_summary_kernel.  Every lane
//                      finds its front record in global memory and takes min and max from it; the records of the 64 bins -- from
//                      the first lane's front record to the first record that starts at or after the last lane's bin end -- are
//                      streamed through LDS ZM_CHUNK records at a time by coalesced loads, and every lane walks, in order, its
//                      own part of the chunk.  Runs of any length: the accumulators stay in registers across chunks.
//   A row without a track (track_of outside [0, n_tracks)), with start >= end or with a negative coordinate is the EMPTY ROW of
//   the full-data path, (0, +inf, -inf, 0, 0): those are the rows where the reference answers None.  A row whose list is empty
//   is (0, NaN, NaN, 0, 0) in every bin.
#pragma once

namespace bxmi {

constexpr int ZM_CHUNK = 256;   // records staged in LDS at a time (7 KiB per workgroup)
constexpr int ZM_THREADS = 64;  // one wave per region

struct ZmTrack {
    const int32_t *start;
    const int32_t *end;
    const uint32_t *valid;
    const float *mn;
    const float *mx;
    const float *sum;
    const float *sumsq;
    const int32_t *leaf_lo;
    const int32_t *leaf_hi;
    const int64_t *leaf_first;
    int64_t n;
    int64_t n_leaves;
};

// acc += field * factor as the reference's build rounds it
__device__ __forceinline__ float zm_add(float acc, double field, float factor)
{
    const double product = field * (double)factor;
    return (float)((double)acc + product);
}

__global__ __launch_bounds__(ZM_THREADS) void zm_summary_kernel(const ZmTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                const int32_t *__restrict__ start, const int32_t *__restrict__ end, int size,
                                                                double *__restrict__ o_valid, double *__restrict__ o_min, double *__restrict__ o_max,
                                                                double *__restrict__ o_sum, double *__restrict__ o_sumsq)
{
    __shared__ int32_t l_st[ZM_CHUNK], l_en[ZM_CHUNK];
    __shared__ uint32_t l_valid[ZM_CHUNK];
    __shared__ float l_mn[ZM_CHUNK], l_mx[ZM_CHUNK], l_sum[ZM_CHUNK], l_sumsq[ZM_CHUNK];
    const int64_t row = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const auto [tr, s, e, has, step] = sm_row(table, n_tracks, track_of, start, end, row, size);
    const int32_t BX_GLOBAL *t_st = as_global(tr.start), *t_en = as_global(tr.end);
    const uint32_t BX_GLOBAL *t_valid = as_global(tr.valid);
    const float BX_GLOBAL *t_mn = as_global(tr.mn), *t_mx = as_global(tr.mx), *t_sum = as_global(tr.sum), *t_sumsq = as_global(tr.sumsq);
    // the records the region loads: [lo, hi), those of the leaves with s < leaf_hi and e > leaf_lo
    int64_t lo = 0, hi = 0;
    if (has && tr.n_leaves > 0) {
        const int32_t BX_GLOBAL *leaf_lo = as_global(tr.leaf_lo), *leaf_hi = as_global(tr.leaf_hi);
        const int64_t BX_GLOBAL *leaf_first = as_global(tr.leaf_first);
        const int64_t a = sm_first_above(leaf_hi, 0, tr.n_leaves, s);      // the first leaf that reaches beyond the region's start
        const int64_t b = zm_first_at_least(leaf_lo, a, tr.n_leaves, e);  // the first leaf, from there on, that begins at or after its end
        if (b > a) {
            lo = leaf_first[a];
            hi = leaf_first[b];
        }
    }
    const double nan = __builtin_nan("");
    const int64_t out0 = row * (int64_t)size;
    for (int64_t g0 = 0; g0 < size; g0 += 64) {
        const auto [g1, bin, ok, b0, b1] = sm_group(g0, size, lane, s, step);  // bins [g0, g1), this lane's [b0, b1)
        float valid = 0.0f, sum = 0.0f, sumsq = 0.0f, mn = 0.0f, mx = 0.0f;
        bool any = false;
        int64_t front = hi;
        if (hi > lo) {
            // the group's records: from the front record of its first bin to the first record that starts at or after its last bin's end
            const int64_t glo = sm_first_above(t_en, lo, hi, (int)(s + (int64_t)step * g0));
            const int64_t ghi = zm_first_at_least(t_st, glo, hi, (int)(s + (int64_t)step * g1));
            if (ok) {
                front = sm_first_above(t_en, glo, hi, b0);  // (b0 is not below the first bin's: the search may begin at glo)
                any = front < hi;
                if (any) {
                    mn = t_mn[front];
                    mx = t_mx[front];
                }
            }
            for (int64_t pos = glo; pos < ghi; pos += ZM_CHUNK) {
                const int cnt = ghi - pos < ZM_CHUNK ? (int)(ghi - pos) : ZM_CHUNK;
                __syncthreads();  // the previous chunk has been walked
                for (int k = lane; k < cnt; k += ZM_THREADS) {
                    l_st[k] = t_st[pos + k];
                    l_en[k] = t_en[pos + k];
                    l_valid[k] = t_valid[pos + k];
                    l_mn[k] = t_mn[pos + k];
                    l_mx[k] = t_mx[pos + k];
                    l_sum[k] = t_sum[pos + k];
                    l_sumsq[k] = t_sumsq[pos + k];
                }
                __syncthreads();
                if (any) {
                    // this lane's records of the chunk: from its front record on, while they start before b1
                    for (int64_t k = front > pos ? front - pos : 0; k < cnt; k++) {
                        const int st = l_st[k], en = l_en[k];
                        if (st >= b1) break;
                        const int ov = (en < b1 ? en : b1) - (st > b0 ? st : b0);
                        if (ov <= 0) continue;
                        const float f = (float)((double)ov / (double)(en - st));
                        valid = zm_add(valid, (double)l_valid[k], f);
                        sum = zm_add(sum, (double)l_sum[k], f);
                        sumsq = zm_add(sumsq, (double)l_sumsq[k], f);
                        if (mx < l_mx[k]) mx = l_mx[k];
                        if (mn > l_mn[k]) mn = l_mn[k];
                    }
                }
            }
        }
        if (ok) {
            o_valid[out0 + bin] = (double)valid;
            o_min[out0 + bin] = !has ? __builtin_inf() : any ? (double)mn : nan;
            o_max[out0 + bin] = !has ? -__builtin_inf() : any ? (double)mx : nan;
            o_sum[out0 + bin] = (double)sum;
            o_sumsq[out0 + bin] = (double)sumsq;
        }
    }
}

}  // namespace bxmi

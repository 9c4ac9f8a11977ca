// bed_summary.hpp -- binned COVERAGE summaries of bigBed tracks over a batch of regions (the reference's
// BigBedFile._summarize_from_full: lib/bx/bbi/bigbed_file.pyx:57-76, 104-113 over bbi_file.pyx:80-111).  Included by summary.hip
// (bxmi_beds_*), after summary.hpp and under the same `#pragma clang fp contract(off)`.
//
// A bed track is one chromosome's bigBed records (start, end) as two arrays in HBM, IN FILE ORDER; there is NO VALUE ARRAY: the
// reference accumulates every record with the value 1.0f.  The bins of a region are those of summary.hpp, and so is the weight of
// a record in a bin -- the record clipped to the region, n = clipped length, w = (double)n * ((double)overlap / n) -- but with a
// value of 1 the five chains of summary.hpp collapse into ONE: 1.0 * w and (double)(1f * 1f) * w are w exactly, so
//     sum = sumsq = the ordered float64 chain of w over the bin's records in file order,  valid = rint(that chain),
//     min = max = 1.0 where at least one record has a positive overlap (the chain is then > 0), else +inf / -inf.
// The order of the chain is observable (22 * (15.0 / 22) != 15): every bin is the chain over its records IN FILE ORDER; records may
// be skipped only when their overlap with the bin is not positive.
//
// bigBed records are sorted by start, but their ENDS descend wherever features nest or overlap, so the ordered path of summary.hpp
// (starts AND ends non-decreasing) never applies.  What a search needs instead is built once per track, on the host:
//     reach[i]  = max(end[0 .. i])                    -- never descends: the first index with reach > x is the first record that
//                                                        ends after x, and nothing before it does
//     creach[i] = max(end[c .. i]), c = i - i % BD_CHUNK  -- the same, restarted at every aligned chunk of BD_CHUNK records: it
//                                                        never descends INSIDE a chunk, and at a chunk's last record it is that
//                                                        chunk's own furthest end
// (bd_build_reach below: plain C++, tests/cpp/bed_summary_kernel_host.cpp checks it against a direct computation).
//
//   bd_summary_kernel  one wave (== one workgroup) per region, bins 64 at a time, lane = bin, as sm_summary_kernel; one float64
//                      accumulator per lane, carried from chunk to chunk, five coalesced stores per bin at the end.
//     sorted tracks    (starts non-decreasing -- every real bigBed): the region's records lie in [lo, hi), lo = the first index
//                      with reach > s, hi = the first with start >= e; the same pair of searches inside it gives the run [glo, ghi)
//                      of each group of 64 bins.  The run goes through LDS in chunks ALIGNED to multiples of BD_CHUNK (glo is
//                      rounded down, the records before it are masked).  A chunk whose own furthest end does not pass the group's
//                      first base is SKIPPED WITHOUT BEING STAGED: the wave tests 64 chunks at a time, lane = chunk, one load of
//                      creach each, and a ballot names the chunks to stage.  So one chromosome-long record at the head of the
//                      file pulls lo to 0 for every region, but each region then pays one test per chunk up to its own records --
//                      one wave-wide load per 64 chunks -- not a walk over them.  In a staged chunk a lane finds its first record
//                      with creach > b0 by binary search in LDS, walks while start < b1 and tests each record's own end.
//     other tracks     the general walk: every chunk of the track (still skipped when its furthest end does not reach the group),
//                      every lane testing every record from its first with creach > b0 on, without the break on start.  CORRECT
//                      AND SLOW, as in summary.hpp; it exists so that no track is refused.
//   A row without a track (track_of outside [0, n_tracks)), with start >= end or with a negative coordinate is the EMPTY ROW of
//   summary.hpp: (0, +inf, -inf, 0, 0) in every bin.
#pragma once

namespace bxmi {

constexpr int BD_CHUNK = 256;   // records staged in LDS at a time (3 KiB per workgroup); chunks are aligned to multiples of it
constexpr int BD_THREADS = 64;  // one wave per region

// which lanes of the wave hold `p` (the host build of tests/cpp/kernel_host.hpp supplies its own)
#ifndef BD_BALLOT
#define BD_BALLOT(p) __ballot(p)
#endif

struct BdTrack {
    const int32_t *start;
    const int32_t *end;
    const int32_t *reach;
    const int32_t *creach;
    int64_t n;
    int64_t sorted;
};

// reach[] and creach[] of a track (see above); returns 1 when the starts never descend, else 0.  Host code.
inline int bd_build_reach(const int32_t *start, const int32_t *end, int64_t n, int32_t *reach, int32_t *creach)
{
    int sorted = 1;
    for (int64_t i = 0; i < n; i++) {
        if (i > 0 && start[i] < start[i - 1]) sorted = 0;
        reach[i] = i > 0 && reach[i - 1] > end[i] ? reach[i - 1] : end[i];
        creach[i] = i % BD_CHUNK != 0 && creach[i - 1] > end[i] ? creach[i - 1] : end[i];
    }
    return sorted;
}

// One record against one bin [b0, b1) of the region [s, e): an item of value 1, by the weight of summary.hpp.
__device__ __forceinline__ void bd_item(double &acc, int st, int en, int s, int e, int b0, int b1)
{
    double w;
    if (sm_weight(w, st, en, s, e, b0, b1)) acc += w;
}

__global__ __launch_bounds__(BD_THREADS) void bd_summary_kernel(const BdTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                const int32_t *__restrict__ start, const int32_t *__restrict__ end, int size,
                                                                double *__restrict__ o_valid, double *__restrict__ o_min, double *__restrict__ o_max,
                                                                double *__restrict__ o_sum, double *__restrict__ o_sumsq)
{
    __shared__ int32_t l_st[BD_CHUNK], l_en[BD_CHUNK], l_creach[BD_CHUNK];
    const int64_t row = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const auto [tr, s, e, has, step] = sm_row(table, n_tracks, track_of, start, end, row, size);
    const int32_t BX_GLOBAL *t_st = as_global(tr.start), *t_en = as_global(tr.end);
    const int32_t BX_GLOBAL *t_reach = as_global(tr.reach), *t_creach = as_global(tr.creach);
    const bool sorted = tr.sorted != 0;
    // the region's records: [lo, hi)
    int64_t lo = 0, hi = 0;
    if (step > 0 && tr.n > 0) {
        hi = tr.n;
        if (sorted) {
            lo = sm_first_above(t_reach, 0, tr.n, s);    // the first record that ends after the region starts
            hi = sm_first_above(t_st, lo, tr.n, e - 1);  // the first record, from there on, that starts at or after its end
        }
    }
    const int64_t out0 = row * (int64_t)size;
    for (int64_t g0 = 0; g0 < size; g0 += 64) {
        const auto [g1, bin, ok, b0, b1] = sm_group(g0, size, lane, s, step);  // bins [g0, g1), this lane's [b0, b1)
        double acc = 0.0;
        if (hi > lo) {
            const int gb0 = (int)(s + (int64_t)step * g0);  // the group's first base
            int64_t glo = lo, ghi = hi;
            if (sorted) {
                glo = sm_first_above(t_reach, lo, hi, gb0);
                ghi = sm_first_above(t_st, glo, hi, (int)(s + (int64_t)step * g1 - 1));
            }
            // chunks [c_first, c_end), 64 at a time: lane = chunk, one load of the chunk's own furthest end per lane; the wave
            // then stages, in order, only the chunks that reach the group (the ballot is the same for every lane)
            const int64_t c_first = glo / BD_CHUNK, c_end = (ghi + BD_CHUNK - 1) / BD_CHUNK;
            for (int64_t cb = c_first; cb < c_end; cb += 64) {
                const int64_t c = cb + lane;
                bool reaches = false;
                if (c < c_end) {
                    const int64_t last = (c + 1) * BD_CHUNK < ghi ? (c + 1) * BD_CHUNK - 1 : ghi - 1;  // of the chunk, inside the run
                    reaches = t_creach[last] > gb0;
                }
                unsigned long long todo = BD_BALLOT(reaches);
                while (todo) {
                    const int64_t pos = (cb + __builtin_ctzll(todo)) * BD_CHUNK;
                    todo &= todo - 1;
                    const int cnt = ghi - pos < BD_CHUNK ? (int)(ghi - pos) : BD_CHUNK;
                    const int first = glo > pos ? (int)(glo - pos) : 0;  // the records before glo are not the group's
                    __syncthreads();  // the previous chunk has been walked
                    for (int k = lane; k < cnt; k += BD_THREADS) {
                        l_st[k] = t_st[pos + k];
                        l_en[k] = t_en[pos + k];
                        l_creach[k] = t_creach[pos + k];
                    }
                    __syncthreads();
                    if (ok) {
                        // this lane's records of the chunk: from the first one at or behind which something ends after b0
                        int a0 = first, a1 = cnt;
                        while (a0 < a1) {
                            const int mid = (a0 + a1) >> 1;
                            if (l_creach[mid] > b0) a1 = mid;
                            else a0 = mid + 1;
                        }
                        for (int k = a0; k < cnt; k++) {
                            const int st = l_st[k];
                            if (sorted && st >= b1) break;
                            bd_item(acc, st, l_en[k], s, e, b0, b1);
                        }
                    }
                }
            }
        }
        if (ok) {
            const bool any = acc > 0.0;
            o_valid[out0 + bin] = __builtin_rint(acc);
            o_min[out0 + bin] = any ? 1.0 : __builtin_inf();
            o_max[out0 + bin] = any ? 1.0 : -__builtin_inf();
            o_sum[out0 + bin] = acc;
            o_sumsq[out0 + bin] = acc;
        }
    }
}

}  // namespace bxmi

// span_arrays.hpp -- per-base values of span tracks over a batch of rows (the reference's BigWigFile.get_as_array:
// lib/bx/bbi/bigwig_file.pyx:122-137, 200-211, its ArrayAccumulatingBlockHandler).  Included by summary.hip (bxmi_spans_arrays*).
//
// Row i has L_i output elements; element j is position p = start[i] + j (in int64) of tracks[track_of[i]] and holds value[k] of the
// LARGEST k in file order with start[k] <= p < end[k] -- the reference assigns item after item, so the later item wins -- or NaN
// (0x7FC00000, numpy's) where no item covers p, where p is outside [0, 2^31-1), where the row names no track and where the track is
// empty.  An item's own value is copied as its 32 bits (a NaN value keeps its payload); zero-length and inverted items cover
// nothing.  No arithmetic at all: nothing here depends on the contraction setting of the unit.
//
//   sa_arrays_kernel   the work is cut on the flat OUTPUT axis: workgroup t owns output elements [t * SA_TILE, (t + 1) * SA_TILE)
//                      whatever rows they belong to, thread k of it the 4 consecutive elements from 4 k, which it keeps in registers
//                      and writes once, with one 16-byte store.  A tile is walked ROW SEGMENT by row segment (the part of one row
//                      inside the tile: the tail of a row, whole short rows, the head of another); a thread's 4 elements may lie in
//                      up to 4 segments.  The row of an element is o / width in a matrix, the last row with row_off <= o in a ragged
//                      batch (empty rows are passed over).  Everything about a segment is uniform over the workgroup.
//     ordered tracks   (starts AND ends non-decreasing -- every real bigWig): the items that cover any position of the segment
//                      [p0, p1) are one contiguous run: from the first item with end > p0 to the first with start >= p1, two binary
//                      searches in HBM per SEGMENT.  The run is streamed through LDS SA_CHUNK items at a time by coalesced loads;
//                      every thread binary-searches the staged starts for each of its positions: the winner is the last item
//                      with start <= p if its end > p, and if its end <= p nothing before it covers p either (ends never
//                      descend).  A later chunk overwrites an earlier one.  A base costs LDS work and its 4 bytes of store.
//     other tracks     the general path: every segment walks ALL the track's items in file order through the same staging, every
//                      thread testing every item against its positions and overwriting.  CORRECT AND SLOW, as summary.hpp's
//                      general path: it exists so that no track is refused.
//   Cost to know: a segment costs two searches and, where it meets items, two barriers per chunk whatever its length, so a batch of
//   one-base rows pays them per base; rows of a tile's length or more pay them once or twice per tile.
//   `out` is the element o_first's address.  When it is 16-byte aligned (vec != 0; o_first is a multiple of SA_TILE) full groups of
//   4 are written by one 16-byte store; else, and in the last group of the output, element by element.  Nothing outside
//   [o_first, o_first + count) is written.
#pragma once

#include "summary.hpp"

namespace bxmi {

constexpr int SA_THREADS = 256;           // 4 waves; with 3 KiB of LDS the 32-wave limit of a CU binds, not the LDS
constexpr int SA_TILE = 4 * SA_THREADS;   // output elements per workgroup: 4 per thread, one 16-byte store
constexpr int SA_CHUNK = 256;             // items staged in LDS at a time (3 KiB per workgroup)
constexpr int SA_NAN = 0x7FC00000;        // the fill: numpy's float32 NaN
constexpr int64_t SA_POS_END = 2147483647LL;  // positions lie in [0, 2^31-1)

// The last row r of [0, n) with row_off[r] <= o: with row_off non-decreasing and o < row_off[n] that is the row holding output
// element o, empty rows before it passed over.  Always inside [0, n), whatever row_off holds.  Plain code for the device and the
// host (Offsets: a pointer to int64 in either address space): the kernel and the slab cutting of bxmi_spans_arrays share it.
template <typename Offsets>
__host__ __device__ inline int64_t sa_row_of(Offsets row_off, int64_t n, int64_t o)
{
    int64_t lo = 1, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (row_off[mid] > o) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

// The rows [r0, r0 + m) that hold output elements [o0, o0 + count), count >= 1: what a launch over those elements is given
// (row_off == nullptr: rows of `width` elements).  The host form of bxmi_spans_arrays cuts its slabs with it.
struct SaRows {
    int64_t r0, m;
};
inline SaRows sa_rows_of(const int64_t *row_off, int64_t n, int64_t width, int64_t o0, int64_t count)
{
    const int64_t r0 = row_off ? sa_row_of(row_off, n, o0) : o0 / width;
    const int64_t r1 = row_off ? sa_row_of(row_off, n, o0 + count - 1) : (o0 + count - 1) / width;
    return SaRows{r0, r1 - r0 + 1};
}

// track_of, start: rows [row_base, row_base + n_rows) of the batch; row_off (ragged; else nullptr and `width` >= 1): the n_rows + 1
// offsets of those rows, absolute.  The launch covers output elements [o_first, o_first + count), SA_TILE per workgroup.
__global__ __launch_bounds__(SA_THREADS) void sa_arrays_kernel(const SmTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                               const int32_t *__restrict__ start, int64_t n_rows, int64_t row_base, int width,
                                                               const int64_t *__restrict__ row_off, int64_t o_first, int64_t count,
                                                               float *__restrict__ out, int vec)
{
    __shared__ int32_t l_st[SA_CHUNK], l_en[SA_CHUNK], l_val[SA_CHUNK];
    const int tid = (int)threadIdx.x;
    const int64_t t0 = o_first + (int64_t)blockIdx.x * SA_TILE;
    const int64_t t1 = t0 + SA_TILE < o_first + count ? t0 + SA_TILE : o_first + count;
    const int64_t e0 = t0 + 4 * tid;  // this thread's elements: [e0, e0 + 4)
    const int32_t BX_GLOBAL *g_track = as_global(track_of), *g_start = as_global(start);
    const int64_t BX_GLOBAL *g_off = as_global(row_off);
    int v[4] = {SA_NAN, SA_NAN, SA_NAN, SA_NAN};
    for (int64_t o = t0; o < t1;) {  // the segment [o, seg1) of row r, whose elements are [r_lo, r_hi)
        int64_t r, r_lo, r_hi;
        if (row_off) {
            r = sa_row_of(g_off, n_rows, o);
            r_lo = g_off[r];
            r_hi = g_off[r + 1];
        } else {
            const int64_t row = o / width;
            r = row - row_base;
            r_lo = row * width;
            r_hi = r_lo + width;
        }
        int64_t seg1 = r_hi < t1 ? r_hi : t1;
        if (seg1 <= o) seg1 = o + 1;  // (offsets that are not what they should be: the walk still ends)
        const int t = g_track[r];
        const int64_t p0 = (int64_t)g_start[r] + (o - r_lo), p1 = p0 + (seg1 - o);  // the segment's positions
        const int64_t c0 = p0 > 0 ? p0 : 0, c1 = p1 < SA_POS_END ? p1 : SA_POS_END;  // those that can hold data
        const bool has = t >= 0 && t < n_tracks && c0 < c1;
        const SmTrack tr = table[has ? t : n_tracks];  // (the spare entry: no items)
        if (tr.n > 0) {
            const int32_t BX_GLOBAL *t_st = as_global(tr.start), *t_en = as_global(tr.end);
            const int32_t BX_GLOBAL *t_val = as_global(reinterpret_cast<const int32_t *>(tr.value));
            const bool ordered = tr.ordered != 0;
            int64_t lo = 0, hi = tr.n;
            if (ordered) {
                lo = sm_first_above(t_en, 0, tr.n, (int)c0);        // the first item that ends after the segment starts
                hi = sm_first_above(t_st, lo, tr.n, (int)(c1 - 1));  // the first item that starts at or after its end
            }
            // this thread's positions in the segment: -1 where an element is not in it or cannot hold data
            int pos[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t p = p0 + (e0 + q - o);
                pos[q] = e0 + q >= o && e0 + q < seg1 && p >= c0 && p < c1 ? (int)p : -1;
            }
            for (int64_t at = lo; at < hi; at += SA_CHUNK) {
                const int cnt = hi - at < SA_CHUNK ? (int)(hi - at) : SA_CHUNK;
                __syncthreads();  // the previous chunk has been searched
                for (int k = tid; k < cnt; k += SA_THREADS) {
                    l_st[k] = t_st[at + k];
                    l_en[k] = t_en[at + k];
                    l_val[k] = t_val[at + k];
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int p = pos[q];
                    if (p < 0) continue;
                    if (ordered) {
                        int a0 = 0, a1 = cnt;  // the first staged item that starts after p
                        while (a0 < a1) {
                            const int mid = (a0 + a1) >> 1;
                            if (l_st[mid] > p) a1 = mid;
                            else a0 = mid + 1;
                        }
                        if (a0 > 0 && l_en[a0 - 1] > p) v[q] = l_val[a0 - 1];
                    } else {
                        for (int k = 0; k < cnt; k++)
                            if (l_st[k] <= p && p < l_en[k]) v[q] = l_val[k];
                    }
                }
            }
        }
        o = seg1;
    }
    int32_t BX_GLOBAL *g_out = as_global(reinterpret_cast<int32_t *>(out)) + (e0 - o_first);
    if (vec && e0 + 4 <= t1) {
        store_int4(g_out, v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (e0 + q < t1) g_out[q] = v[q];
    }
}

}  // namespace bxmi

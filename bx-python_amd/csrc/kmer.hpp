// kmer.hpp -- the k-mer spectrum of 2bit tracks over a batch of rows: counts[row][word] of every word of k letters (the reference's
// bx.intseq.ngramcount.count_ngrams, lib/bx/intseq/ngramcount.pyx:34-85, over bx.seqmapping's translate, lib/bx/seqmapping.py:36-48
// and lib/bx/_seqmapping.pyx:24-67).  Included by sequence.hip after twobit.hpp (bxmi_twobit_kmer_counts*).  Integers only, like
// twobit.hpp: the counts do not depend on the order the atomics land in.
//
// Row i is the string of letters tb_bases_kernel would write.  A letter is one of eight classes, 4 * lower_case + code (codes T=0
// C=1 A=2 G=3; nothing is lower case without do_mask); digits[8] gives the digit of each class in [0, radix) or -1.  'N', a position
// outside [0, size) and every position of a row that names no track have no digit.  The window at offset j of a row counts iff its k
// letters j .. j + k - 1 lie in the row and all have a digit; its word is sum(digit[j + t] * radix^t), the first letter least
// significant (ngramcount.pyx:73-82).  EVERY window of a row counts, the last one included: the reference's loop stops one window
// early (ngramcount.pyx:71), which the Python layer reproduces by shortening the rows, not this kernel.
//
//   km_counts_kernel   the work is cut on the flat axis of the rows' bases as in tb_bases_kernel: tile t is window starts [t * KM_TILE,
//                      (t + 1) * KM_TILE) whatever rows they belong to, thread i of the workgroup the KM_RUN consecutive starts from
//                      KM_RUN * i.  A grid smaller than the tiles loops.  A tile is walked ROW SEGMENT by row segment; everything
//                      about a segment is uniform over the workgroup.  A thread's windows in a segment need its KM_RUN letters and a
//                      halo of k - 1 more (k - 1 <= 6 at radix 4, <= 13 at radix 2): at most 21 letters from at most three aligned
//                      32-bit words of packed bytes (tb_word).  The segment, its track and the N and mask blocks over a thread's
//                      letters come from twobit.hpp's row-segment layer: tb_segment (sa_row_of), tb_letters with the halo, and
//                      tb_block_bits (two sm_first_above searches per list, the run staged TB_CHUNK at a time, tb_covered), which gives
//                      the thread a bit per letter; from the bits and the codes it builds `bad`, a bit per position without a digit
//                      (positions past the row's end or outside the sequence included: a -1 digit is nothing special), and `dig`,
//                      two bits per position.  Window j is bad where any of bits j .. j + k - 1 of `bad` is set.
//   accumulation       per segment, one of two ways (km_use_lds):
//                        (a) an LDS histogram of `bins` counters is zeroed, every window adds to it with an LDS atomic, and the
//                            non-zero counters are added to counts[row] with global atomics (a row may span workgroups);
//                        (b) every window adds straight to counts[row] with a global atomic; LDS is not touched.
//                      (a) costs a zeroing and a flush of `bins` and three barriers, (b) a global atomic per window.  An operation
//                      count (zero + flush of `bins` against the windows) suggested a cut-off that grows with `bins`; measured
//                      (tools/bench_kmers.py) the two ways cross at 330 .. 450 window starts for every `bins` from
//                      64 to 4096: the flush is a few coalesced rounds, the atomics of (b) are scattered and collide.  km_use_lds
//                      takes (a) where the segment has at least KM_CUT window starts, and (b) always where bins > KM_LDS_BINS,
//                      the counters a workgroup keeps in LDS (16 KiB; with the 2 KiB of staged blocks 8 workgroups fit a CU's
//                      160 KiB, which is also what 256 threads each allow).  `force` overrides the cut-off for measurements and tests.
//   strand             km_counts_strand_kernel takes a strand per row and counts a minus row over its reverse complement, without
//                      mirroring the flat axis: described at km_counts_body.  km_counts_kernel is the STRAND == false instantiation.
//   `counts` must be zero before the launch (the library zeroes it on the stream).  Nothing outside counts[0 .. n_rows * bins) is
//   written: a word is below bins by construction (every digit is below radix).
#pragma once

#include "twobit.hpp"

namespace bxmi {

constexpr int KM_THREADS = 256;                // 4 waves
constexpr int KM_RUN = 8;                      // window starts per thread
constexpr int KM_TILE = KM_RUN * KM_THREADS;   // window starts per tile
constexpr int KM_BINS_MAX = 16384;             // k = 7 at radix 4, k = 14 at radix 2
constexpr int KM_K_MAX = 14;                   // so a thread's letters are at most KM_RUN + KM_K_MAX - 1 = 21: 21 bits, 42 bits of digits
constexpr int KM_LDS_BINS = 4096;              // the largest histogram kept in LDS (k = 6 at radix 4): 16 KiB
constexpr int KM_CUT = 384;                    // (a) for a segment of at least this many window starts (measured: DESIGN.md 3.16)
constexpr int KM_PLAN = 0, KM_FORCE_LDS = 1, KM_FORCE_DIRECT = 2;  // `force`

static_assert(KM_RUN + KM_K_MAX - 1 <= 32, "a bit per letter of a thread");
static_assert(15 + KM_RUN + KM_K_MAX - 1 <= 48, "a thread's letters lie in three words");

struct KmSpec {
    int k, radix, bins;
    unsigned digits;  // 4 bits per letter class 4 * lower_case + code: digit + 1, 0 for none
    int force;
};

// radix^k, or KM_BINS_MAX + 1 where that is beyond KM_BINS_MAX (k >= 1, radix >= 2)
__host__ __device__ inline int km_bins(int k, int radix)
{
    int64_t bins = 1;
    for (int t = 0; t < k && bins <= KM_BINS_MAX; t++) bins *= radix;
    return bins <= KM_BINS_MAX ? (int)bins : KM_BINS_MAX + 1;
}

// the digits table as it travels: -1 <= digits[c] < 15
__host__ __device__ inline unsigned km_pack_digits(const int8_t *digits)
{
    unsigned packed = 0;
    for (int c = 0; c < 8; c++) packed |= (unsigned)(digits[c] + 1) << (4 * c);
    return packed;
}

// whether a segment of `windows` window starts goes through the LDS histogram (a) or straight to HBM (b)
__host__ __device__ inline bool km_use_lds(int bins, int64_t windows, int force)
{
    if (bins > KM_LDS_BINS || force == KM_FORCE_DIRECT) return false;
    if (force == KM_FORCE_LDS) return true;
    return windows >= KM_CUT;
}

// the k two-bit digits of x, 2 k <= 16 bits, in reverse order
__host__ __device__ inline unsigned km_reverse4(unsigned x, int k)
{
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0F0Fu) << 4) | ((x >> 4) & 0x0F0Fu);
    x = ((x & 0x00FFu) << 8) | ((x >> 8) & 0x00FFu);
    return x >> (16 - 2 * k);
}

// The text of km_counts_kernel (STRAND == false: `strand` is not read) and of km_counts_strand_kernel.  The string of a minus row is
// the reverse complement of the plus row's (twobit.hpp, strand in the row-segment layer), and its windows are the plus string's
// windows one to one: the window at offset j of the plus string is the one at offset len - k - j of the minus string, over the same
// positions, so it counts under the same condition.  Only its word differs: the digits are those of the COMPLEMENTED letters (the
// table need not be closed under complement: a letter's complement may have no digit, and then the window does not count), taken in
// reverse order.  So a minus row walks the flat axis as a plus row does; strand is uniform over a segment, rows of either strand
// share a tile, and both ways of accumulating are untouched.
template <bool STRAND>
__device__ __forceinline__ void km_counts_body(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                               const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows, int64_t row_base,
                                               int width, const int64_t *__restrict__ row_off, int64_t o_first, int64_t count, int do_mask,
                                               const KmSpec &spec, int32_t *__restrict__ counts, int32_t *l_st, int32_t *l_en, int32_t *l_hist)
{
    const int tid = (int)threadIdx.x;
    const int32_t BX_GLOBAL *g_track = as_global(track_of), *g_start = as_global(start);
    const int64_t BX_GLOBAL *g_off = as_global(row_off);
    const int8_t BX_GLOBAL *g_strand = as_global(strand);
    const int k = spec.k, radix = spec.radix, bins = spec.bins;
    const unsigned k_bits = (1u << k) - 1u;
    int64_t o_end = o_first + count;
    if (row_off && g_off[n_rows] < o_end) o_end = g_off[n_rows];  // (`count` may be a bound: the offsets say where the rows end)
    // the tiles of this workgroup: one when the grid has a workgroup per tile, else every gridDim.x-th
    for (int64_t tile = blockIdx.x; o_first + tile * KM_TILE < o_end; tile += gridDim.x) {
        const int64_t t0 = o_first + tile * KM_TILE;
        const int64_t t1 = t0 + KM_TILE < o_end ? t0 + KM_TILE : o_end;
        const int64_t e0 = t0 + KM_RUN * tid;  // this thread's window starts: [e0, e0 + KM_RUN)
        for (int64_t o = t0; o < t1;) {  // the segment [o, seg1) of row r, whose elements are [r_lo, r_hi)
            const TbSegment sg = tb_segment(g_off, n_rows, row_base, width, o, t1);
            const int64_t r = sg.r, seg1 = sg.seg1;
            const int seg_len = (int)(seg1 - o);
            const bool minus = tb_minus<STRAND>(g_strand, r);
            // p0: the position of the segment's first window start; [c0, c1): the positions under the segment's windows that are
            // letters of the row
            const TbLetters lt = tb_letters(table, n_tracks, g_track[r], g_start[r], sg.r_lo, sg.r_hi, o, seg_len + k - 1);
            const int64_t p0 = lt.p0, c0 = lt.c0, c1 = lt.c1;
            // this thread's window starts of the segment: [lo_el, lo_el + n_win), the positions under them [first, first + span)
            const int64_t lo_el = e0 > o ? e0 : o, hi_el = e0 + KM_RUN < seg1 ? e0 + KM_RUN : seg1;
            const int n_win = lo_el < hi_el ? (int)(hi_el - lo_el) : 0;
            const int span = n_win ? n_win + k - 1 : 0;
            const int64_t first = p0 + (lo_el - o);
            unsigned bad = span ? (1u << span) - 1u : 0u;  // a bit per position without a digit
            uint64_t dig = 0;                              // the digit of position first + i at bits 2 i, 2 i + 1
            if (c0 < c1) {
                // those of its positions that are letters: [pf, pf + cnt), its positions qa .. qa + cnt - 1
                const int64_t lo_p = first > c0 ? first : c0, hi_p = first + span < c1 ? first + span : c1;
                const int cnt = n_win && lo_p < hi_p ? (int)(hi_p - lo_p) : 0;
                const int qa = cnt ? (int)(lo_p - first) : 0, pf = cnt ? (int)lo_p : 0;
                const int b = pf & 15;
                uint32_t w0 = 0, w1 = 0, w2 = 0;  // base pf + i at bits 31 - 2 ((b + i) & 15) .. of word (b + i) >> 4
                if (cnt) {
                    const uint32_t BX_GLOBAL *packed = as_global(lt.tr.packed);
                    const int64_t w = pf >> 4, last = (pf + cnt - 1) >> 4;
                    w0 = tb_word(packed, w);
                    if (last > w) w1 = tb_word(packed, w + 1);
                    if (last > w + 1) w2 = tb_word(packed, w + 2);
                }
                const TbBits bits = tb_block_bits<KM_THREADS>(lt.tr, do_mask, c0, c1, pf, cnt, tid, l_st, l_en);
                for (int i = 0; i < cnt; i++) {
                    const int at = b + i;
                    const uint32_t word = at < 16 ? w0 : at < 32 ? w1 : w2;
                    const unsigned code = tb_complement((word >> (30 - 2 * (at & 15))) & 3u, minus);
                    const unsigned cls = code + ((bits.is_m >> i) & 1u ? 4u : 0u);
                    const unsigned d1 = (bits.is_n >> i) & 1u ? 0u : (spec.digits >> (4 * cls)) & 15u;  // digit + 1
                    if (d1 == 0) continue;
                    bad &= ~(1u << (qa + i));
                    dig |= (uint64_t)(d1 - 1u) << (2 * (qa + i));
                }
            }
            const bool lds = km_use_lds(bins, seg_len, spec.force);
            int32_t *row_counts = counts + r * (int64_t)bins;
            if (lds) {
                __syncthreads();  // the previous segment's histogram has been flushed
                for (int q = tid; q < bins; q += KM_THREADS) l_hist[q] = 0;
                __syncthreads();
            }
            for (int j = 0; j < n_win; j++) {
                if ((bad >> j) & k_bits) continue;
                int word;
                if (radix == 4) {
                    word = (int)(dig >> (2 * j)) & (bins - 1);  // the digits as they lie
                    if (minus) word = (int)km_reverse4((unsigned)word, k);
                } else if (minus) {
                    word = 0;
                    for (int q = 0; q < k; q++) word = word * radix + (int)((dig >> (2 * (j + q))) & 3u);  // the last letter least significant
                } else {
                    word = 0;
                    int factor = 1;
                    for (int q = 0; q < k; q++) {
                        word += (int)((dig >> (2 * (j + q))) & 3u) * factor;
                        factor *= radix;
                    }
                }
                if (lds) atomicAdd(&l_hist[word], 1);
                else atomicAdd(&row_counts[word], 1);
            }
            if (lds) {
                __syncthreads();
                for (int q = tid; q < bins; q += KM_THREADS) {
                    const int v = l_hist[q];
                    if (v) atomicAdd(&row_counts[q], v);
                }
            }
            o = seg1;
        }
    }
}

// track_of, start, row_off, row_base, width, o_first, count: as tb_bases_kernel; with row_off the walk ends at row_off[n_rows] where
// that is below o_first + count (`count` may be a bound).  counts is [n_rows][bins], row r of the rows given is entry r.
__global__ __launch_bounds__(KM_THREADS) void km_counts_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                               const int32_t *__restrict__ start, int64_t n_rows, int64_t row_base, int width,
                                                               const int64_t *__restrict__ row_off, int64_t o_first, int64_t count, int do_mask,
                                                               KmSpec spec, int32_t *__restrict__ counts)
{
    __shared__ int32_t l_st[TB_CHUNK], l_en[TB_CHUNK];
    __shared__ int32_t l_hist[KM_LDS_BINS];
    km_counts_body<false>(table, n_tracks, track_of, start, nullptr, n_rows, row_base, width, row_off, o_first, count, do_mask, spec, counts, l_st, l_en, l_hist);
}

// the same with strand[n_rows] of the rows given: any non-zero entry is a minus row, counted as its reverse complement
__global__ __launch_bounds__(KM_THREADS) void km_counts_strand_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                      const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows,
                                                                      int64_t row_base, int width, const int64_t *__restrict__ row_off, int64_t o_first,
                                                                      int64_t count, int do_mask, KmSpec spec, int32_t *__restrict__ counts)
{
    __shared__ int32_t l_st[TB_CHUNK], l_en[TB_CHUNK];
    __shared__ int32_t l_hist[KM_LDS_BINS];
    km_counts_body<true>(table, n_tracks, track_of, start, strand, n_rows, row_base, width, row_off, o_first, count, do_mask, spec, counts, l_st, l_en, l_hist);
}

}  // namespace bxmi

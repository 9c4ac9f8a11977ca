// twobit.hpp -- the sequence of 2bit tracks over a batch of rows, as letters and as base counts (the reference's
// bx.seq._twobit.read: lib/bx/seq/_twobit.pyx:22-137 under TwoBitSequence.get / __getitem__, twobit.py:34-56).  Included by
// sequence.hip (bxmi_twobit_*).
//
// A 2bit track is ONE sequence in HBM: its packed bytes (4 bases per byte, the first base in the two most significant bits, codes
// T=0 C=1 A=2 G=3), its N blocks and its mask blocks as starts and ENDS.  Within each list the blocks are sorted, non-empty, disjoint
// and inside [0, size] (bxmi_twobit_create refuses anything else), so the reference's bisect-and-walk is plain coverage: position p
// is 'N' where an N block covers it, else the letter of its code, and lower case where a mask block covers it and do_mask is set.
// Integers only: no arithmetic that could round, nothing depends on a contraction setting.
//
//   tb_bases_kernel    the work is cut on the flat OUTPUT axis as in sa_arrays_kernel (span_arrays.hpp): workgroup t owns output
//                      bytes [t * TB_TILE, (t + 1) * TB_TILE) whatever rows they belong to, thread k of it the 16 consecutive bytes
//                      from 16 k, which it keeps in four registers and writes once, with one 16-byte store.  A tile is walked ROW
//                      SEGMENT by row segment; everything about a segment is uniform over the workgroup.  A thread's bases within a
//                      segment are contiguous in the sequence: at most 16 bases from two aligned 32-bit words of packed bytes, byte
//                      swapped so that base k of a word lies at bits 31-2k..30-2k, and shifted.  The letter of a code is a byte of the
//                      packed constant TB_LETTERS.  Per list of blocks, two searches per segment find the contiguous run of blocks
//                      that meet it; the run is streamed through LDS TB_CHUNK blocks at a time, every thread searching the staged
//                      ends for the first block that ends after its first position and walking on while blocks start before its
//                      last: a 16-bit mask of its positions.  A segment that meets no block of a list runs no chunk loop for it.
//   the row-segment layer   tb_segment, tb_letters, tb_block_bits, tb_codes: the walk above as this kernel and km_counts_kernel
//                      (kmer.hpp) share it; the latter's `want` positions per segment hold a halo beyond the segment.  Described
//                      once, at the helpers.  (pw_scores_kernel and pw_hits_kernel share one staging of their own, pw_stage_columns
//                      of pwm.hpp, which carries the same walk as its own text: on the helpers they measured 1 - 3 % slower at
//                      unchanged register counts; it takes tb_minus, tb_complement, tb_code and tb_covered.)
//   strand             tb_bases_strand_kernel, tb_composition_strand_kernel (and km_counts_strand_kernel of kmer.hpp) take a strand
//                      per row: a minus row is the reverse complement of the plus row (the reference's SeqFile.reverse_complement,
//                      lib/bx/seq/seq.py:108-109), the pad mirrored with it and not complemented.  Strand sits in the row-segment layer
//                      (tb_minus, tb_letters_minus, tb_complement; described there); each kernel's text is a body templated on
//                      STRAND with two thin wrappers, and the unstranded kernels are the STRAND == false instantiations.
//   tb_count_kernel    (creation) the four code counts of every checkpoint block of TB_CKPT bases, one wave per block, as four
//                      planes; a device scan per plane (primitives.hpp) and tb_interleave_kernel turn them into the running totals
//                      ckpt[k] = counts of bases [0, TB_CKPT * k) as one 16-byte entry (T, C, A, G).
//   tb_under_kernel    (creation) the code counts UNDER every N block (a file may pack anything there), one wave per block, from
//                      the checkpoints themselves (tb_raw); scanned and interleaved in the same way into n_codes.
//   tb_composition_kernel   one wave per row, and a row's cost does not depend on its length:
//                        raw(s, e)  = ckpt difference + at most two edge pieces, each inside ONE checkpoint block (64 aligned words,
//                                     a word per lane: a mask of the selected bases on the two bit planes, four popcounts);
//                        under N    = the n_codes difference of the blocks wholly inside the row + raw of at most two clipped ones;
//                        N, masked  = differences of the running block sizes, less the clipped ends.  Two searches per list.
//                      A, C, G, T = raw - under N.  Nothing outside [0, size) is counted: every piece is clipped to the row, the row to
//                      the sequence, so neither the padding bits of the last byte nor the rest of the last checkpoint block count.
//   `out` of tb_bases_kernel is byte o_first's address.  When it is 16-byte aligned (vec != 0; o_first is a multiple of TB_TILE) full
//   groups of 16 are written by one 16-byte store; else, and in the last group of the output, byte by byte.  Nothing outside
//   [o_first, o_first + count) is written.
#pragma once

#include "summary.hpp"
#include "span_arrays.hpp"

namespace bxmi {

constexpr int TB_THREADS = 256;             // 4 waves; 2 KiB of LDS
constexpr int TB_TILE = 16 * TB_THREADS;    // output bytes per workgroup: 16 per thread, one 16-byte store
constexpr int TB_CHUNK = 256;               // blocks staged in LDS at a time
constexpr int TB_CKPT = 1024;               // bases per checkpoint block: 256 packed bytes, 64 aligned words
constexpr int TB_WAVE = 64;                 // threads of the creation kernels and of tb_composition_kernel: one wave
constexpr unsigned TB_LETTERS = 0x47414354u;  // "TCAG": the letter of code c is byte c
constexpr int64_t TB_SIZE_MAX = 2147483647LL;

struct TbTrack {
    const uint32_t *packed;   // the packed bytes as aligned words, zero-filled to a whole checkpoint block
    const int32_t *n_start, *n_end, *m_start, *m_end;
    const int32_t *ckpt;      // [ceil(size / TB_CKPT) + 1][4]: entry k = the code counts of bases [0, min(TB_CKPT * k, size))
    const int32_t *n_cum;     // [n_blocks + 1]: running sizes of the N blocks
    const int32_t *n_codes;   // [n_blocks + 1][4]: running code counts under the N blocks
    const int32_t *m_cum;     // [m_blocks + 1]
    int64_t size, n_blocks, m_blocks;
};

// bases [k * 16, k * 16 + 16) of the sequence, base j of them at bits 31 - 2 j .. 30 - 2 j
__device__ __forceinline__ uint32_t tb_word(const uint32_t BX_GLOBAL *packed, int64_t k)
{
    return __builtin_bswap32(packed[k]);
}

// the low bit of every base [qa, qb) of such a word, 0 <= qa <= qb <= 16
__device__ __forceinline__ uint32_t tb_select(int qa, int qb)
{
    const uint32_t from = qa < 16 ? 0xFFFFFFFFu >> (2 * qa) : 0u, past = qb < 16 ? 0xFFFFFFFFu >> (2 * qb) : 0u;
    return from & ~past & 0x55555555u;
}

// acc[c] += sign * (the bases of code c among those `sel` selects in `w`)
__device__ __forceinline__ void tb_count_word(int acc[4], uint32_t w, uint32_t sel, int sign)
{
    const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
    acc[0] += sign * __builtin_popcount(~hi & ~lo & sel);
    acc[1] += sign * __builtin_popcount(~hi & lo & sel);
    acc[2] += sign * __builtin_popcount(hi & ~lo & sel);
    acc[3] += sign * __builtin_popcount(hi & lo & sel);
}

// v[c] = the wave's sum of v[c], in every lane.  (TB_WAVE_SUM4: the host build of tests/cpp/twobit_kernel_host.cpp puts its own in its
// place, as BD_BALLOT of bed_summary.hpp: a workgroup of host threads has no shuffle.)
#ifndef TB_WAVE_SUM4
__device__ __forceinline__ void tb_wave_sum4(int v[4])
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] += __shfl_xor(v[c], m, 64);
    }
}
#define TB_WAVE_SUM4(v) tb_wave_sum4(v)
#endif

// acc (this LANE's share; the wave's sum is the answer) += sign * code counts of bases [a, b), which lie inside ONE checkpoint block
__device__ __forceinline__ void tb_edge(int acc[4], const uint32_t BX_GLOBAL *packed, int lane, int64_t a, int64_t b, int sign)
{
    if (a >= b) return;
    const int64_t first = (a / TB_CKPT) * TB_CKPT + 16 * lane;  // this lane's word: bases [first, first + 16)
    const int64_t qa = a - first, qb = b - first;
    if (qb <= 0 || qa >= 16) return;
    tb_count_word(acc, tb_word(packed, first >> 4), tb_select(qa > 0 ? (int)qa : 0, qb < 16 ? (int)qb : 16), sign);
}

// acc += sign * code counts of bases [s, e), 0 <= s <= e <= size, whatever covers them: the checkpoint difference in lane 0's share,
// the edges in every lane's
__device__ __forceinline__ void tb_raw(int acc[4], const uint32_t BX_GLOBAL *packed, const int32_t BX_GLOBAL *ckpt, int lane, int64_t s, int64_t e,
                                       int sign)
{
    if (s >= e) return;
    const int64_t k0 = (s + TB_CKPT - 1) / TB_CKPT, k1 = e / TB_CKPT;  // the checkpoints inside [s, e] are k0 .. k1
    if (k0 > k1) {
        tb_edge(acc, packed, lane, s, e, sign);
        return;
    }
    tb_edge(acc, packed, lane, s, k0 * TB_CKPT, sign);
    tb_edge(acc, packed, lane, k1 * TB_CKPT, e, sign);
    if (lane == 0 && k0 < k1) {
        const int4 lo = load_int4(ckpt + 4 * k0), hi = load_int4(ckpt + 4 * k1);
        acc[0] += sign * (hi.x - lo.x);
        acc[1] += sign * (hi.y - lo.y);
        acc[2] += sign * (hi.z - lo.z);
        acc[3] += sign * (hi.w - lo.w);
    }
}

// ---- creation ----
// planes[c * stride + k] = the bases of code c in checkpoint block k, clipped to the sequence; one wave per block
__global__ __launch_bounds__(TB_WAVE) void tb_count_kernel(const uint32_t *__restrict__ packed, int64_t size, int64_t stride, int32_t *__restrict__ planes)
{
    const int lane = (int)threadIdx.x;
    const int64_t k = blockIdx.x, a = k * TB_CKPT, b = a + TB_CKPT < size ? a + TB_CKPT : size;
    int acc[4] = {0, 0, 0, 0};
    tb_edge(acc, as_global(packed), lane, a, b, 1);
    TB_WAVE_SUM4(acc);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) as_global(planes)[c * stride + k] = acc[c];
    }
}

// planes[c * stride + i] = the bases of code c under N block [start[i], end[i]); one wave per block
__global__ __launch_bounds__(TB_WAVE) void tb_under_kernel(const uint32_t *__restrict__ packed, const int32_t *__restrict__ ckpt,
                                                           const int32_t *__restrict__ start, const int32_t *__restrict__ end, int64_t stride,
                                                           int32_t *__restrict__ planes)
{
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    int acc[4] = {0, 0, 0, 0};
    tb_raw(acc, as_global(packed), as_global(ckpt), lane, as_global(start)[i], as_global(end)[i], 1);
    TB_WAVE_SUM4(acc);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) as_global(planes)[c * stride + i] = acc[c];
    }
}

// table[i] = (planes[0][i], planes[1][i], planes[2][i], planes[3][i]) for i in [0, n): the scanned planes as 16-byte entries
__global__ __launch_bounds__(TB_THREADS) void tb_interleave_kernel(const int32_t *__restrict__ planes, int64_t stride, int64_t n, int32_t *__restrict__ table)
{
    const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t BX_GLOBAL *p = as_global(planes);
    store_int4(as_global(table) + 4 * i, p[i], p[stride + i], p[2 * stride + i], p[3 * stride + i]);
}

// ---- letters ----
// the bits [a - pf, b - pf) of a thread's positions [pf, pf + cnt) that the staged blocks cover
__device__ __forceinline__ unsigned tb_covered(const int32_t *l_st, const int32_t *l_en, int staged, int pf, int cnt)
{
    int a0 = 0, a1 = staged;  // the first staged block that ends after pf
    while (a0 < a1) {
        const int mid = (a0 + a1) >> 1;
        if (l_en[mid] > pf) a1 = mid;
        else a0 = mid + 1;
    }
    unsigned bits = 0;
    for (int k = a0; k < staged && l_st[k] < pf + cnt; k++) {  // (at most 16 rounds: the blocks are disjoint and not empty)
        const int a = l_st[k] > pf ? l_st[k] - pf : 0, b = l_en[k] < pf + cnt ? l_en[k] - pf : cnt;
        bits |= ((1u << (b - a)) - 1u) << a;
    }
    return bits;
}

// ---- the row-segment layer ----
// What tb_bases_kernel and km_counts_kernel (kmer.hpp) share, and what a further kernel over 2bit rows starts from: a tile of the
// flat axis is walked row segment by row segment, and per segment -- everything here is uniform over the workgroup but pf, cnt and
// tid -- tb_segment finds the row, tb_letters its track and the positions that are letters, tb_block_bits the N and mask blocks
// over a thread's letters, tb_codes the letters' codes.

// The segment [o, seg1) of the tile that ends at t1: it lies in row r of the rows given, whose elements are [r_lo, r_hi).
struct TbSegment {
    int64_t r, r_lo, r_hi, seg1;
};
__device__ __forceinline__ TbSegment tb_segment(const int64_t BX_GLOBAL *g_off, int64_t n_rows, int64_t row_base, int width, int64_t o, int64_t t1)
{
    TbSegment s;
    if (g_off) {
        s.r = sa_row_of(g_off, n_rows, o);
        s.r_lo = g_off[s.r];
        s.r_hi = g_off[s.r + 1];
    } else {
        const int64_t row = o / width;
        s.r = row - row_base;
        s.r_lo = row * width;
        s.r_hi = s.r_lo + width;
    }
    s.seg1 = s.r_hi < t1 ? s.r_hi : t1;
    if (s.seg1 <= o) s.seg1 = o + 1;  // (offsets that are not what they should be: the walk still ends)
    return s;
}

// The track of a row that names track `t` and starts at `start`, and of the `want` positions from p0, the position of element o,
// those that are letters: [c0, c1), inside the sequence and before the position of element r_end -- the row's end r_hi for a caller
// whose `want` holds a halo, seg1 for one that wants the segment alone.  A row that names no track gets the spare entry behind the
// table, of size 0: c0 >= c1.
struct TbLetters {
    TbTrack tr;
    int64_t p0, c0, c1;
};
__device__ __forceinline__ TbLetters tb_letters(const TbTrack *table, int n_tracks, int t, int start, int64_t r_lo, int64_t r_end, int64_t o, int64_t want)
{
    const bool named = t >= 0 && t < n_tracks;
    TbLetters s{table[named ? t : n_tracks], 0, 0, 0};
    s.p0 = (int64_t)start + (o - r_lo);
    s.c1 = s.p0 + want;
    if (s.c1 > (int64_t)start + (r_end - r_lo)) s.c1 = (int64_t)start + (r_end - r_lo);
    if (s.c1 > s.tr.size) s.c1 = s.tr.size;
    s.c0 = s.p0 > 0 ? s.p0 : 0;
    return s;
}

// A bit per position of this thread's letters [pf, pf + cnt) that an N block covers, and one that a mask block covers (0 without
// do_mask), of the letters [c0, c1), c0 < c1, of a segment.  Per list two searches find the run of blocks that meets [c0, c1); the run
// goes through l_st / l_en TB_CHUNK blocks at a time, between two barriers.  So EVERY thread of the workgroup of THREADS calls this,
// and with the same tr, do_mask, c0 and c1 -- a thread without letters (cnt == 0) too; the callers skip the call where a segment has
// no letter (c0 >= c1), which is the same for the whole workgroup.  A list that does not meet [c0, c1) takes no barrier.
struct TbBits {
    unsigned is_n, is_m;
};
template <int THREADS>
__device__ __forceinline__ TbBits tb_block_bits(const TbTrack &tr, int do_mask, int64_t c0, int64_t c1, int pf, int cnt, int tid, int32_t *l_st, int32_t *l_en)
{
    TbBits s{0, 0};
    for (int list = 0; list < (do_mask ? 2 : 1); list++) {
        const int64_t blocks = list ? tr.m_blocks : tr.n_blocks;
        if (blocks == 0) continue;
        const int32_t BX_GLOBAL *b_st = as_global(list ? tr.m_start : tr.n_start), *b_en = as_global(list ? tr.m_end : tr.n_end);
        const int64_t lo = sm_first_above(b_en, 0, blocks, (int)c0);        // the first block that ends after the letters start
        const int64_t hi = sm_first_above(b_st, lo, blocks, (int)(c1 - 1));  // the first that starts at or after their end
        unsigned bits = 0;
        for (int64_t at = lo; at < hi; at += TB_CHUNK) {
            const int staged = hi - at < TB_CHUNK ? (int)(hi - at) : TB_CHUNK;
            __syncthreads();  // the previous chunk has been searched
            for (int k = tid; k < staged; k += THREADS) {
                l_st[k] = b_st[at + k];
                l_en[k] = b_en[at + k];
            }
            __syncthreads();
            if (cnt) bits |= tb_covered(l_st, l_en, staged, pf, cnt);
        }
        if (list) s.is_m = bits;
        else s.is_n = bits;
    }
    return s;
}

// The codes of letters [pf, pf + cnt), cnt <= 17, from at most two words: letter pf + i at bits 63 - 2 (b + i) .. 62 - 2 (b + i),
// b = pf & 15, which tb_code takes out.  Nothing is read for cnt == 0.
__device__ __forceinline__ uint64_t tb_codes(const TbTrack &tr, int pf, int cnt)
{
    if (cnt == 0) return 0;
    const uint32_t BX_GLOBAL *packed = as_global(tr.packed);
    const int64_t w = pf >> 4;
    uint64_t codes = (uint64_t)tb_word(packed, w) << 32;
    if (((pf + cnt - 1) >> 4) > w) codes |= tb_word(packed, w + 1);
    return codes;
}
__device__ __forceinline__ unsigned tb_code(uint64_t codes, int at) { return (unsigned)(codes >> (62 - 2 * at)) & 3u; }

// ---- strand in the row-segment layer ----
// A batch may carry a strand per row (int8; 0: as stored, anything else: the reverse complement, the reference's
// SeqFile.reverse_complement, lib/bx/seq/seq.py:108-109 over DNA_COMP, seq.py:9-14).  Element j of a minus row of len elements is the
// COMPLEMENT of the letter at position start + (len - 1 - j); pad stays pad.  Strand is uniform over a segment like everything else
// about it, and a segment of a minus row is still one ascending run of positions, so the loads, the searches and the chunk walk
// (tb_block_bits, tb_codes) are what they are for a plus row: tb_minus says whether the segment's row is a minus row,
// tb_letters_minus gives its positions (the mirror of tb_letters without a halo), tb_complement the code (T=0 C=1 A=2 G=3: code ^ 2;
// 'N' and the case bit are their own complements).  A kernel that only counts what lies under a row (km_counts_kernel) keeps
// tb_letters: the positions of a minus row are those of the plus row.  STRAND == false folds all of it away.
template <bool STRAND>
__device__ __forceinline__ bool tb_minus(const int8_t BX_GLOBAL *g_strand, int64_t r)
{
    if constexpr (STRAND) return g_strand[r] != 0;
    else return false;
}
// The segment [o, seg1) of a minus row whose elements end at r_hi: element e of it is position p0 + (seg1 - 1 - e), in 64 bits; of
// those positions [c0, c1) are letters.
__device__ __forceinline__ TbLetters tb_letters_minus(const TbTrack *table, int n_tracks, int t, int start, int64_t r_hi, int64_t o, int64_t seg1)
{
    const bool named = t >= 0 && t < n_tracks;
    TbLetters s{table[named ? t : n_tracks], 0, 0, 0};
    s.p0 = (int64_t)start + (r_hi - seg1);
    s.c1 = s.p0 + (seg1 - o);
    if (s.c1 > s.tr.size) s.c1 = s.tr.size;
    s.c0 = s.p0 > 0 ? s.p0 : 0;
    return s;
}
__device__ __forceinline__ unsigned tb_complement(unsigned code, bool minus) { return minus ? code ^ 2u : code; }

// The text of tb_bases_kernel (STRAND == false: `strand` is not read) and of tb_bases_strand_kernel (STRAND == true: strand[r] of
// the rows given).  In a segment of a minus row a thread's bytes are still one ascending run of positions [pf, pf + cnt); letter i of
// them goes to place cnt - 1 - i of the thread's bytes of the segment, complemented.
template <bool STRAND>
__device__ __forceinline__ void tb_bases_body(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                              const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows, int64_t row_base,
                                              int width, const int64_t *__restrict__ row_off, int64_t o_first, int64_t count, int do_mask, int pad,
                                              uint8_t *__restrict__ out, int vec, int32_t *l_st, int32_t *l_en)
{
    const int tid = (int)threadIdx.x;
    const int64_t t0 = o_first + (int64_t)blockIdx.x * TB_TILE;
    const int64_t t1 = t0 + TB_TILE < o_first + count ? t0 + TB_TILE : o_first + count;
    const int64_t e0 = t0 + 16 * tid;  // this thread's bytes: [e0, e0 + 16)
    const int32_t BX_GLOBAL *g_track = as_global(track_of), *g_start = as_global(start);
    const int64_t BX_GLOBAL *g_off = as_global(row_off);
    const int8_t BX_GLOBAL *g_strand = as_global(strand);
    const uint32_t pad4 = (uint32_t)(pad & 0xFF) * 0x01010101u;
    uint32_t v[4] = {pad4, pad4, pad4, pad4};
    for (int64_t o = t0; o < t1;) {  // the segment [o, seg1) of row r, whose bytes are [r_lo, r_hi)
        const TbSegment sg = tb_segment(g_off, n_rows, row_base, width, o, t1);
        const int64_t seg1 = sg.seg1;
        const bool minus = tb_minus<STRAND>(g_strand, sg.r);
        const TbLetters lt = minus ? tb_letters_minus(table, n_tracks, g_track[sg.r], g_start[sg.r], sg.r_hi, o, seg1)
                                   : tb_letters(table, n_tracks, g_track[sg.r], g_start[sg.r], sg.r_lo, seg1, o, seg1 - o);  // the segment's positions
        const int64_t p0 = lt.p0, c0 = lt.c0, c1 = lt.c1;
        if (c0 < c1) {
            // this thread's bytes that are bases of the segment: [lo_el, hi_el), positions [pf, pf + cnt), bits [qa, qa + cnt) of 16
            int64_t lo_el = e0 > o ? e0 : o, hi_el = e0 + 16 < seg1 ? e0 + 16 : seg1;
            if (minus) {  // (position p is element seg1 - 1 - (p - p0))
                if (lo_el < seg1 - (c1 - p0)) lo_el = seg1 - (c1 - p0);
                if (hi_el > seg1 - (c0 - p0)) hi_el = seg1 - (c0 - p0);
            } else {
                if (lo_el < o + (c0 - p0)) lo_el = o + (c0 - p0);
                if (hi_el > o + (c1 - p0)) hi_el = o + (c1 - p0);
            }
            const int cnt = lo_el < hi_el ? (int)(hi_el - lo_el) : 0;
            const int qa = cnt ? (int)(lo_el - e0) : 0, pf = cnt ? (int)(minus ? p0 + (seg1 - hi_el) : p0 + (lo_el - o)) : 0;
            const uint64_t codes = tb_codes(lt.tr, pf, cnt);
            const TbBits bits = tb_block_bits<TB_THREADS>(lt.tr, do_mask, c0, c1, pf, cnt, tid, l_st, l_en);
            const int b = pf & 15;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                int i = q - qa;  // the base's place among this thread's
                if (i < 0 || i >= cnt) continue;
                if (minus) i = cnt - 1 - i;
                unsigned letter = (bits.is_n >> i) & 1u ? (unsigned)'N' : (TB_LETTERS >> (8 * tb_complement(tb_code(codes, b + i), minus))) & 0xFFu;
                if ((bits.is_m >> i) & 1u) letter |= 0x20u;
                v[q >> 2] = (v[q >> 2] & ~(0xFFu << (8 * (q & 3)))) | (letter << (8 * (q & 3)));
            }
        }
        o = seg1;
    }
    uint8_t BX_GLOBAL *g_out = as_global(out) + (e0 - o_first);
    if (e0 >= t1) return;
    if (vec && e0 + 16 <= t1) {
        store_int4(reinterpret_cast<int32_t BX_GLOBAL *>(g_out), (int)v[0], (int)v[1], (int)v[2], (int)v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (e0 + q < t1) g_out[q] = (uint8_t)(v[q >> 2] >> (8 * (q & 3)));
    }
}

// track_of, start: rows [row_base, row_base + n_rows) of the batch; row_off (ragged; else nullptr and `width` >= 1): the n_rows + 1
// offsets of those rows, absolute.  The launch covers output bytes [o_first, o_first + count), TB_TILE per workgroup.
__global__ __launch_bounds__(TB_THREADS) void tb_bases_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                              const int32_t *__restrict__ start, int64_t n_rows, int64_t row_base, int width,
                                                              const int64_t *__restrict__ row_off, int64_t o_first, int64_t count, int do_mask,
                                                              int pad, uint8_t *__restrict__ out, int vec)
{
    __shared__ int32_t l_st[TB_CHUNK], l_en[TB_CHUNK];
    tb_bases_body<false>(table, n_tracks, track_of, start, nullptr, n_rows, row_base, width, row_off, o_first, count, do_mask, pad, out, vec, l_st, l_en);
}

// the same with strand[n_rows] of the rows given: any non-zero entry is a minus row
__global__ __launch_bounds__(TB_THREADS) void tb_bases_strand_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                     const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows,
                                                                     int64_t row_base, int width, const int64_t *__restrict__ row_off, int64_t o_first,
                                                                     int64_t count, int do_mask, int pad, uint8_t *__restrict__ out, int vec)
{
    __shared__ int32_t l_st[TB_CHUNK], l_en[TB_CHUNK];
    tb_bases_body<true>(table, n_tracks, track_of, start, strand, n_rows, row_base, width, row_off, o_first, count, do_mask, pad, out, vec, l_st, l_en);
}

// ---- base counts ----
// The blocks [i0, i1) of a sorted disjoint list that meet [s, e), s < e, and the bases of [s, e) they cover.
struct TbMeet {
    int64_t i0, i1;
    int covered;
};
__device__ __forceinline__ TbMeet tb_meet(const int32_t BX_GLOBAL *b_st, const int32_t BX_GLOBAL *b_en, const int32_t BX_GLOBAL *cum, int64_t blocks,
                                          int s, int e)
{
    TbMeet m{0, 0, 0};
    if (blocks == 0) return m;
    m.i0 = sm_first_above(b_en, 0, blocks, s);
    m.i1 = sm_first_above(b_st, m.i0, blocks, e - 1);
    if (m.i0 >= m.i1) return m;
    const int first = b_st[m.i0], last = b_en[m.i1 - 1];
    m.covered = cum[m.i1] - cum[m.i0] - (first < s ? s - first : 0) - (last > e ? last - e : 0);
    return m;
}

// The text of tb_composition_kernel and of tb_composition_strand_kernel: the strand of a row is a swap at the final store.
template <bool STRAND>
__device__ __forceinline__ void tb_composition_body(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                    const int32_t *__restrict__ start, const int32_t *__restrict__ end, const int8_t *__restrict__ strand,
                                                    int do_mask, int32_t *__restrict__ counts)
{
    const int lane = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int t = as_global(track_of)[row];
    const bool named = t >= 0 && t < n_tracks;
    const TbTrack tr = table[named ? t : n_tracks];  // (the spare entry: size 0)
    const int64_t s64 = as_global(start)[row], e64 = as_global(end)[row];
    const int s = s64 > 0 ? (int)s64 : 0, e = e64 < tr.size ? (int)e64 : (int)tr.size;
    int acc[4] = {0, 0, 0, 0};
    int n_count = 0, m_count = 0;
    if (s < e) {
        const uint32_t BX_GLOBAL *packed = as_global(tr.packed);
        const int32_t BX_GLOBAL *ckpt = as_global(tr.ckpt);
        tb_raw(acc, packed, ckpt, lane, s, e, 1);
        const int32_t BX_GLOBAL *n_st = as_global(tr.n_start), *n_en = as_global(tr.n_end);
        const TbMeet n = tb_meet(n_st, n_en, as_global(tr.n_cum), tr.n_blocks, s, e);
        n_count = n.covered;
        if (n.i0 < n.i1) {  // less what lies under the N blocks: the clipped ones at the ends, the table for the rest
            const bool cut_first = n_st[n.i0] < s, cut_last = n_en[n.i1 - 1] > e;
            const int64_t j0 = n.i0 + (cut_first ? 1 : 0), j1 = n.i1 - (cut_last ? 1 : 0);
            if (cut_first) tb_raw(acc, packed, ckpt, lane, s, n_en[n.i0] < e ? n_en[n.i0] : e, -1);
            if (cut_last && !(cut_first && n.i1 - n.i0 == 1)) tb_raw(acc, packed, ckpt, lane, n_st[n.i1 - 1], e, -1);
            if (lane == 0 && j0 < j1) {
                const int32_t BX_GLOBAL *codes = as_global(tr.n_codes);
                const int4 lo = load_int4(codes + 4 * j0), hi = load_int4(codes + 4 * j1);
                acc[0] -= hi.x - lo.x;
                acc[1] -= hi.y - lo.y;
                acc[2] -= hi.z - lo.z;
                acc[3] -= hi.w - lo.w;
            }
        }
        if (do_mask) m_count = tb_meet(as_global(tr.m_start), as_global(tr.m_end), as_global(tr.m_cum), tr.m_blocks, s, e).covered;
    }
    TB_WAVE_SUM4(acc);
    if (lane == 0) {
        int32_t BX_GLOBAL *o = as_global(counts) + 6 * row;
        if (tb_minus<STRAND>(as_global(strand), row)) o[0] = acc[0], o[1] = acc[3], o[2] = acc[1], o[3] = acc[2];  // the complements' counts
        else o[0] = acc[2], o[1] = acc[1], o[2] = acc[3], o[3] = acc[0];  // A, C, G, T of codes T=0 C=1 A=2 G=3
        o[4] = n_count, o[5] = m_count;
    }
}

// counts[row] = A, C, G, T, N, masked of [start[row], end[row]) clipped to the sequence; one wave per row
__global__ __launch_bounds__(TB_WAVE) void tb_composition_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                 const int32_t *__restrict__ start, const int32_t *__restrict__ end, int do_mask,
                                                                 int32_t *__restrict__ counts)
{
    tb_composition_body<false>(table, n_tracks, track_of, start, end, nullptr, do_mask, counts);
}

// the same of the reverse complement where strand[row] is not zero: A, C, G, T of a minus row are T, G, C, A of the plus row
__global__ __launch_bounds__(TB_WAVE) void tb_composition_strand_kernel(const TbTrack *__restrict__ table, int n_tracks,
                                                                        const int32_t *__restrict__ track_of, const int32_t *__restrict__ start,
                                                                        const int32_t *__restrict__ end, const int8_t *__restrict__ strand, int do_mask,
                                                                        int32_t *__restrict__ counts)
{
    tb_composition_body<true>(table, n_tracks, track_of, start, end, strand, do_mask, counts);
}

}  // namespace bxmi

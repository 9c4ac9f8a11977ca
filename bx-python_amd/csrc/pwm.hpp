// pwm.hpp -- position weight matrices scored over 2bit tracks for a batch of rows (the reference's ScoringMatrix.score_string:
// lib/bx/motif/pwm.py:141-149 over _pwm.score_string, lib/bx/motif/_pwm.pyx:23-55).  Included by sequence.hip after twobit.hpp
// (bxmi_pwm_*, bxmi_twobit_pwm_*).  twobit.hpp stays integers only: every float of the 2bit unit is here.
//
// Row i is a string of L_i letters, the ones tb_bases_kernel would write: TCAG by code, 'N' inside an N block, | 0x20 inside a mask
// block when do_mask is set.  For a matrix of W rows, element j of row i of its plane is
//     ((0.0f + v[0][c(j)]) + v[1][c(j + 1)]) + ... + v[W - 1][c(j + W - 1)]
// in float32, in that order, where c(k) >= 0 is the column of letter k of the row, and NaN (0x7FC00000, numpy's) where a letter of the
// window has no column, where the window passes the row's end (the last W - 1 elements; every element of a row shorter than W) and
// where a position is outside [0, size) or the row names no track.  Only additions: nothing to contract, nothing reassociated.
//
//   letter classes     a base is one of ten letters, in the order T C A G N t c a g n: class = (N ? 4 : code) + (masked ? 5 : 0).
//                      The handle's letter_col[10] (the column of each, or -1) travels as one 64-bit kernel argument, 5 bits per
//                      class holding column + 1.
//   pw_scores_kernel   the work is cut on the flat OUTPUT axis as in tb_bases_kernel: workgroup t owns elements [t * PW_TILE,
//                      (t + 1) * PW_TILE) of every plane, thread k of it the 4 consecutive elements from 4 k.  A tile is walked ROW
//                      SEGMENT by row segment; everything about a segment is uniform over the workgroup.  Per segment the workgroup
//                      stages (pw_stage_columns) the column (int8, -1: unscoreable) of the segment's positions and of a halo of max width - 1 positions
//                      beyond its end into LDS, 8 positions per thread from at most two packed words and the staged block runs
//                      (tb_covered), one 8-byte LDS store each; positions past the row's end or outside the sequence are -1, so a
//                      window that leaves the row meets a -1.  Then, matrix after matrix, every thread walks the W + 3 columns under
//                      its four windows once, each feeding up to four accumulators, each accumulator in ascending j from +0.0f.
//                      A matrix set of at most PW_LDS_VALUES values stays in LDS for the whole tile; a larger one is staged matrix
//                      by matrix.  A thread whose four elements lie in the segment and whose address in the plane is 16-byte aligned
//                      writes them by one 16-byte store; otherwise element by element.  Nothing outside the planes is written.
//   BEST               the same walk storing no score: a thread folds its scored elements into a 64-bit key -- high word the float's
//                      order-preserving image bits ^ (sign ? 0xFFFFFFFF : 0x80000000), low word 0xFFFFFFFF - offset in row, so the
//                      greatest key is the greatest score at its FIRST offset -- the wave takes the maximum (PW_WAVE_MAX64) and one
//                      lane sends it to keys[m * n_rows + row] by a 64-bit atomic maximum (PW_ATOMIC_MAX64), at most one per wave
//                      per (segment, matrix).  A NaN score is never a candidate; every candidate's key is above 0, the value the keys
//                      start from.  A chain started from +0.0f never gives -0.0f (x + y is -0 only when both are), so equal scores
//                      have equal bits.  pw_unpack_kernel turns keys into best_score / best_pos: NaN and -1 for a key of 0.
//   strand             pw_scores_strand_kernel<BEST> (and pw_hits_strand_kernel<FILL> of pwm_hits.hpp) take a strand per row: a minus
//                      row is scored on its reverse complement (the reference's matrix.score_string(text.translate(DNA_COMP)[::-1]),
//                      lib/bx/seq/seq.py:108-109), offsets, ties and the order of hits being those of that string.  Strand sits in
//                      pw_stage_columns<STRAND>, the one staging of both headers, and nowhere else: it decides which column lands
//                      where in l_col.  Everything behind the staging barrier -- the window walk, the order of every accumulator's
//                      additions, the 16-byte store rule, the keys, the ranks -- is the same text for both strands, so a minus row's
//                      chain is ascending in the matrix's rows over the strand's letters, NOT the reverse-complement matrix's chain
//                      on the plus string read backwards.  Each kernel's text is a body templated on STRAND with two thin wrappers;
//                      the unstranded kernels are the STRAND == false instantiations.  Rows of both strands share a tile.
#pragma once

#include "twobit.hpp"

namespace bxmi {

constexpr int PW_THREADS = 256;             // 4 waves
constexpr int PW_TILE = 4 * PW_THREADS;     // output elements per workgroup and plane: 4 per thread, one 16-byte store
constexpr int PW_WIDTH_MAX = 256;           // rows of a matrix
constexpr int PW_COLS_MAX = 16;             // columns of a matrix: the largest is 16 KiB of LDS
constexpr int PW_MATS_MAX = 32;             // matrices of a handle
constexpr int PW_LDS_VALUES = PW_WIDTH_MAX * PW_COLS_MAX;  // values staged at a time
constexpr int PW_STAGE = PW_TILE + PW_WIDTH_MAX;           // columns staged per segment: the segment and its halo, 8 per thread
constexpr int PW_LETTERS = 10;              // T C A G N t c a g n
constexpr unsigned PW_NAN = 0x7FC00000u;    // numpy's float32 NaN

static_assert(PW_STAGE <= 8 * PW_THREADS && PW_STAGE % 8 == 0, "8 staged columns per thread");

struct PwSet {
    const float *values;      // [mat_off[n_mats]][n_cols]
    const int32_t *mat_off;   // [n_mats + 1]: matrix m is rows [mat_off[m], mat_off[m + 1])
    int n_mats, n_cols, max_width;
    unsigned long long letters;  // 5 bits per letter class: column + 1
};

__device__ __forceinline__ unsigned pw_bits(float x)
{
    unsigned u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}

// the wave's maximum of `key`, in lane 0 at least.  (The host build of tests/cpp/pwm_kernel_host.cpp puts its own in the place of
// both macros, as it does for TB_WAVE_SUM4: host threads have no shuffle.)
#ifndef PW_WAVE_MAX64
__device__ __forceinline__ unsigned long long pw_wave_max64(unsigned long long key)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long other = __shfl_xor(key, m, 64);
        key = other > key ? other : key;
    }
    return key;
}
#define PW_WAVE_MAX64(key) pw_wave_max64(key)
#endif
#ifndef PW_ATOMIC_MAX64
#define PW_ATOMIC_MAX64(at, key) atomicMax(at, key)
#endif

// The int8 columns (-1: unscoreable) of the segment [o, seg1) of a row [r_lo, r_hi) and of a halo of max width - 1 letters behind it, in
// the order of the row's strand, into l_col; n_stage, the number of columns staged, is returned.  The row names track `t` and starts at
// `start`.  Staged column k is offset (o - r_lo) + k of the strand's string:
//   plus    position start + (o - r_lo) + k: the halo lies beyond the segment and ends at the row's end;
//   minus   position start + (r_hi - r_lo) - 1 - (o - r_lo) - k, in 64 bits, its class complemented (tb_complement: N and the case
//           are their own complements) BEFORE the `letters` lookup: the halo lies at lower positions and ends at the row's start.
// Either way the staged positions are one ascending run [p0, p0 + n_stage) of which [c0, c1) are letters of the row inside the
// sequence, a thread owns 8 consecutive ascending positions from `mine` in at most two packed words, the two searches per block list
// go over [c0, c1), and the thread makes one 8-byte LDS store: on a minus row its columns byte-reversed, at the mirrored place.
// The loads, the searches and the chunk walk are the text this kernel always had (on tb_block_bits and tb_codes of twobit.hpp the
// unstranded kernels measured 1 - 3 % slower); tb_minus, tb_complement, tb_code and tb_covered are twobit.hpp's.
// Every thread of the workgroup calls this with the same arguments but tid: it holds barriers, the last of them after the stores.
template <bool STRAND>
__device__ __forceinline__ int pw_stage_columns(const TbTrack *__restrict__ table, int n_tracks, int t, int start, bool minus, int64_t r_lo, int64_t r_hi,
                                                int64_t o, int64_t seg1, int do_mask, const PwSet &pw, int tid, int32_t *l_st, int32_t *l_en, int8_t *l_col)
{
    const int seg_len = (int)(seg1 - o);
    const int n_stage = seg_len + pw.max_width - 1;  // the segment and its halo: at most PW_STAGE - 1
    const bool named = t >= 0 && t < n_tracks;
    const TbTrack tr = table[named ? t : n_tracks];  // (the spare entry: size 0)
    const bool mirror = STRAND && minus;
    // the staged positions that are letters of the row: inside the row, inside the sequence
    int64_t p0, c0, c1, mine;  // mine: the first of this thread's 8 positions
    if (mirror) {
        c1 = (int64_t)start + (r_hi - r_lo) - (o - r_lo);  // one past the position of staged column 0
        p0 = c1 - n_stage;
        mine = c1 - 8 - 8 * tid;
        c0 = p0 > (int64_t)start ? p0 : (int64_t)start;
        if (c0 < 0) c0 = 0;
        if (c1 > tr.size) c1 = tr.size;
    } else {
        p0 = (int64_t)start + (o - r_lo);  // the position of staged column 0
        mine = p0 + 8 * tid;
        c1 = p0 + n_stage;
        if (c1 > (int64_t)start + (r_hi - r_lo)) c1 = (int64_t)start + (r_hi - r_lo);
        if (c1 > tr.size) c1 = tr.size;
        c0 = p0 > 0 ? p0 : 0;
    }
    unsigned long long cols = ~0ull;  // this thread's 8 staged columns, -1 each
    const bool stages = 8 * tid < n_stage;
    if (c0 < c1) {
        // this thread's staged positions that are letters: [pf, pf + cnt), places [qa, qa + cnt) of its 8 ascending positions
        const int64_t lo_p = mine > c0 ? mine : c0, hi_p = mine + 8 < c1 ? mine + 8 : c1;
        const int cnt = stages && lo_p < hi_p ? (int)(hi_p - lo_p) : 0;
        const int qa = cnt ? (int)(lo_p - mine) : 0, pf = cnt ? (int)lo_p : 0;
        uint64_t codes = 0;  // base pf + i at bits 63 - 2 (b + i) .. 62 - 2 (b + i), b = pf & 15
        if (cnt) {
            const uint32_t BX_GLOBAL *packed = as_global(tr.packed);
            const int64_t w = pf >> 4;
            codes = (uint64_t)tb_word(packed, w) << 32;
            if (((pf + cnt - 1) >> 4) > w) codes |= tb_word(packed, w + 1);
        }
        unsigned is_n = 0, is_m = 0;
        for (int list = 0; list < (do_mask ? 2 : 1); list++) {
            const int64_t blocks = list ? tr.m_blocks : tr.n_blocks;
            if (blocks == 0) continue;
            const int32_t BX_GLOBAL *b_st = as_global(list ? tr.m_start : tr.n_start), *b_en = as_global(list ? tr.m_end : tr.n_end);
            const int64_t lo = sm_first_above(b_en, 0, blocks, (int)c0);        // the first block that ends after the staged letters start
            const int64_t hi = sm_first_above(b_st, lo, blocks, (int)(c1 - 1));  // the first that starts at or after their end
            unsigned bits = 0;
            for (int64_t at = lo; at < hi; at += TB_CHUNK) {
                const int staged = hi - at < TB_CHUNK ? (int)(hi - at) : TB_CHUNK;
                __syncthreads();  // the previous chunk has been searched
                for (int k = tid; k < staged; k += PW_THREADS) {
                    l_st[k] = b_st[at + k];
                    l_en[k] = b_en[at + k];
                }
                __syncthreads();
                if (cnt) bits |= tb_covered(l_st, l_en, staged, pf, cnt);
            }
            if (list) is_m = bits;
            else is_n = bits;
        }
        const int b = pf & 15;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = q - qa;  // the letter's place among this thread's
            if (i < 0 || i >= cnt) continue;
            const unsigned code = tb_complement(tb_code(codes, b + i), mirror);
            const unsigned cls = ((is_n >> i) & 1u ? 4u : code) + ((is_m >> i) & 1u ? 5u : 0u);
            const unsigned long long col = ((pw.letters >> (5 * cls)) & 31ull) - 1ull;  // (-1: all ones)
            const int at = mirror ? 7 - q : q;  // the staged column among this thread's 8
            cols = (cols & ~(0xFFull << (8 * at))) | ((col & 0xFFull) << (8 * at));
        }
    }
    __syncthreads();  // the previous segment's windows have been read (and, the first time, the resident values are staged)
    if (stages) __builtin_memcpy(l_col + 8 * tid, &cols, 8);
    __syncthreads();
    return n_stage;
}

// The text of pw_scores_kernel (STRAND == false: `strand` is not read) and of pw_scores_strand_kernel (STRAND == true: strand[r] of
// the rows given).  Strand changes which column lands where in l_col, and nothing after the staging barrier: an element's offset
// e - r_lo is its offset in the strand's string.
template <bool STRAND, bool BEST>
__device__ __forceinline__ void pw_scores_body(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                               const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows, int64_t row_base,
                                               int width, const int64_t *__restrict__ row_off, int64_t o_first, int64_t count, int do_mask, PwSet pw,
                                               float *__restrict__ out, int64_t plane_stride, unsigned long long *__restrict__ keys, int64_t key_rows)
{
    __shared__ int32_t l_st[TB_CHUNK], l_en[TB_CHUNK];
    __shared__ int8_t l_col[PW_STAGE] __attribute__((aligned(8)));
    __shared__ float l_val[PW_LDS_VALUES];
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
    int64_t o_end = o_first + count;
    if (BEST && row_off && g_off[n_rows] < o_end) o_end = g_off[n_rows];  // (`count` may be a bound: the offsets say where the rows end)
    // the tiles of this workgroup: one when the grid has a workgroup per tile, else every gridDim.x-th
    for (int64_t tile = blockIdx.x; o_first + tile * PW_TILE < o_end; tile += gridDim.x) {
        const int64_t t0 = o_first + tile * PW_TILE;
        const int64_t t1 = t0 + PW_TILE < o_end ? t0 + PW_TILE : o_end;
        const int64_t e0 = t0 + 4 * tid;  // this thread's elements: [e0, e0 + 4)
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
            const int n_stage = pw_stage_columns<STRAND>(table, n_tracks, g_track[r], g_start[r], tb_minus<STRAND>(g_strand, r), r_lo, r_hi, o, seg1, do_mask,
                                                         pw, tid, l_st, l_en, l_col);
            // this thread's elements of the segment
            unsigned act = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (e0 + q >= o && e0 + q < seg1) act |= 1u << q;
            const int kb = (int)(e0 - o);  // the staged column under element e0 (meaningful where act != 0)
            for (int m = 0; m < pw.n_mats; m++) {
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
                if (BEST) {
                    unsigned long long key = 0;
#pragma unroll
                    for (int q = 3; q >= 0; q--) {
                        if (!((act >> q) & 1u) || ((bad >> q) & 1u) || !(acc[q] == acc[q])) continue;
                        const unsigned u = pw_bits(acc[q]);
                        const unsigned long long k =
                            ((unsigned long long)(u ^ (u & 0x80000000u ? 0xFFFFFFFFu : 0x80000000u)) << 32) | (0xFFFFFFFFu - (unsigned)(e0 + q - r_lo));
                        key = k > key ? k : key;
                    }
                    key = PW_WAVE_MAX64(key);
                    if ((tid & 63) == 0 && key != 0) PW_ATOMIC_MAX64(keys + (int64_t)m * key_rows + r, key);
                } else if (act) {
                    unsigned v[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) v[q] = (bad >> q) & 1u ? PW_NAN : pw_bits(acc[q]);
                    float BX_GLOBAL *g_out = as_global(out) + (int64_t)m * plane_stride + (e0 - o_first);
                    if (act == 15u && (reinterpret_cast<uintptr_t>(g_out) & 15) == 0) {
                        store_int4(reinterpret_cast<int32_t BX_GLOBAL *>(g_out), (int)v[0], (int)v[1], (int)v[2], (int)v[3]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if ((act >> q) & 1u) reinterpret_cast<int32_t BX_GLOBAL *>(g_out)[q] = (int)v[q];
                    }
                }
            }
            o = seg1;
        }
    }
}

// track_of, start, row_off, row_base, width, o_first, count: as tb_bases_kernel.  `out` is the address of element o_first of plane
// 0, plane m lies plane_stride elements after plane m - 1.  BEST: nothing is stored; keys is [n_mats][key_rows], row r of the rows
// given is entry r (the launch is given the whole batch: row_base == 0).
template <bool BEST>
__global__ __launch_bounds__(PW_THREADS) void pw_scores_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                               const int32_t *__restrict__ start, int64_t n_rows, int64_t row_base, int width,
                                                               const int64_t *__restrict__ row_off, int64_t o_first, int64_t count, int do_mask,
                                                               PwSet pw, float *__restrict__ out, int64_t plane_stride,
                                                               unsigned long long *__restrict__ keys, int64_t key_rows)
{
    pw_scores_body<false, BEST>(table, n_tracks, track_of, start, nullptr, n_rows, row_base, width, row_off, o_first, count, do_mask, pw, out, plane_stride,
                                keys, key_rows);
}

// the same with strand[n_rows] of the rows given: any non-zero entry is a minus row, whose string is the reverse complement
template <bool BEST>
__global__ __launch_bounds__(PW_THREADS) void pw_scores_strand_kernel(const TbTrack *__restrict__ table, int n_tracks, const int32_t *__restrict__ track_of,
                                                                      const int32_t *__restrict__ start, const int8_t *__restrict__ strand, int64_t n_rows,
                                                                      int64_t row_base, int width, const int64_t *__restrict__ row_off, int64_t o_first,
                                                                      int64_t count, int do_mask, PwSet pw, float *__restrict__ out, int64_t plane_stride,
                                                                      unsigned long long *__restrict__ keys, int64_t key_rows)
{
    pw_scores_body<true, BEST>(table, n_tracks, track_of, start, strand, n_rows, row_base, width, row_off, o_first, count, do_mask, pw, out, plane_stride,
                               keys, key_rows);
}

// best_score[i], best_pos[i] of keys[i], i in [0, count): NaN and -1 where no element of the row was scored
__global__ __launch_bounds__(PW_THREADS) void pw_unpack_kernel(const unsigned long long *__restrict__ keys, int64_t count, float *__restrict__ best_score,
                                                               int32_t *__restrict__ best_pos)
{
    const int64_t i = (int64_t)blockIdx.x * PW_THREADS + threadIdx.x;
    if (i >= count) return;
    const unsigned long long key = as_global(keys)[i];
    const unsigned image = (unsigned)(key >> 32);
    const unsigned u = key == 0 ? PW_NAN : image ^ (image & 0x80000000u ? 0x80000000u : 0xFFFFFFFFu);
    reinterpret_cast<int32_t BX_GLOBAL *>(as_global(best_score))[i] = (int)u;
    as_global(best_pos)[i] = key == 0 ? -1 : (int32_t)(0xFFFFFFFFu - (unsigned)key);
}

}  // namespace bxmi

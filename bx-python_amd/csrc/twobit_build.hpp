// twobit_build.hpp -- a 2bit track built on the device from its LETTERS: the inverse of tb_bases_kernel (twobit.hpp).  Included by
// sequence.hip after twobit.hpp (bxmi_twobit_create_letters, _create_letters_dev, _create_nib).  What the reference reads through
// the same SeqFile.get as 2bit -- FASTA (lib/bx/seq/fasta.py) and nib (nib.py, _nib.pyx) -- and letters already in HBM become what
// a bxmi_twobit holds, so that every kernel over 2bit rows runs on them unchanged.
//
// Input: `size` symbols of one of two sources (the template parameter SRC):
//   BL_ASCII   a byte per symbol.
//   BL_NIB     a nibble per symbol, the first of a byte in its high half: codes 0-3 = T C A G, 4 = N, 5-7 = the reference's 'X'
//              (_nib.pyx:20-21), bit 3 = lower case.
// Every symbol is one of the ten letters TCAGNtcagn or "other" (anything else; nib codes 5-7).  An other symbol counts as N, and as
// masked if it is lower case (ASCII a-z, the nib's bit 3); whether the call is refused over it is the host's decision from
// first_other, the lowest position of an other symbol with its value: an atomic minimum of (position << 8 | value), whose result
// does not depend on the order of the updates.
//
// Output: packed bytes in file order (first base in the two most significant bits, T=0 C=1 A=2 G=3, 0 under N and past `size` up to
// the end of the last whole checkpoint block), and the N blocks and the mask blocks as MAXIMAL runs -- the rule every real file
// follows: a block never touches the next, a lower-case n lies in both lists.
//
//   bl_build_kernel<SRC, FILL>   the sequence axis is cut into tiles of BL_TILE positions, one workgroup per tile, 16 consecutive
//                          positions per thread: at most 16 input bytes by one 16-byte load (8 by two 32-bit loads from a nib) when the
//                          input is aligned and the thread's positions all exist (vec != 0), byte by byte else.  A thread's flags are a
//                          16-bit mask per list; a run STARTS at p where flag[p] && !flag[p - 1] and ENDS after p where flag[p] &&
//                          !flag[p + 1], so a thread needs one symbol before and one after its own, which it reads itself (two byte
//                          loads that hit the lines its neighbours load): nothing about the flags crosses threads, and a run that
//                          straddles a tile boundary has its start and its end found by different workgroups.
//     FILL == false        packs (one aligned 32-bit store per thread), finds the lowest other symbol, and counts per tile the
//                          starts and the ends of either list -- a wave prefix over the threads' 0 .. 8 (BL_WAVE_PREFIX), the four
//                          waves' totals through LDS -- into counts[list * tiles + tile]: plain stores, no atomics.
//     (between the two)    ONE exclusive scan of counts[4 * tiles] (device_scan of primitives.hpp) gives int64 bases in (list, tile)
//                          order and the grand total behind them: list l's entries begin at bases[l * tiles], so the N blocks number
//                          bases[tiles] and the mask blocks bases[2 * tiles] - bases[tiles].
//     FILL == true         skips a tile whose four counts are zero (most tiles of a genome); else reads the letters again and the
//                          same prefix is now the rank: entry k of a thread goes to bases[l * tiles + tile] - bases[l * tiles] + the
//                          earlier waves' totals + the wave's prefix before the thread + k.  Tiles ascend along the sequence, threads
//                          along a tile and positions along a thread, so the placement IS the order, the same on every run; and the
//                          k-th start and the k-th end belong to the same block because both lists are in that order.
//   bl_sizes_kernel        cum[0] = 0, cum[i + 1] = end[i] - start[i]; an inclusive scan in place makes them the running sizes.
// LDS: 64 bytes.  Traffic: a byte per base read by the first pass (half a byte from a nib), a quarter written, and the letters of the
// tiles that hold a block boundary read once more.  Integers only.
#pragma once

#ifndef BL_WAVE_PREFIX
#include "primitives.hpp"  // wave_inclusive_sum_dpp
#endif

namespace bxmi {

constexpr int BL_THREADS = 256;            // 4 waves
constexpr int BL_TILE = 16 * BL_THREADS;   // positions per workgroup: 16 per thread, one packed word
constexpr int BL_LISTS = 4;                // N starts, mask starts, N ends, mask ends
constexpr int BL_ASCII = 0, BL_NIB = 1;
constexpr unsigned long long BL_NO_OTHER = ~0ull;

// the inclusive prefix sum of `v` over the wave's 64 lanes; every lane of the workgroup calls it.  (The host build of
// tests/cpp/build_kernel_host.cpp puts its own in its place, and its own minimum: host threads have no lanes.)
#ifndef BL_WAVE_PREFIX
#define BL_WAVE_PREFIX(v) ((int)wave_inclusive_sum_dpp((unsigned)(v)))
#endif
#ifndef BL_ATOMIC_MIN64
#define BL_ATOMIC_MIN64(at, key) atomicMin(at, key)
#endif

// what a symbol is: bits 0-1 its code (0 under N), bit 2 N, bit 3 lower case, bit 4 other (then N as well)
template <int SRC>
__device__ __forceinline__ unsigned bl_classify(unsigned v)
{
    if (SRC == BL_NIB) {
        const unsigned c = v & 7u;
        return (c < 4u ? c : 4u) | (v & 8u) | (c > 4u ? 16u : 0u);
    }
    const unsigned u = v & 0xDFu;  // (the letter's upper case; no other byte becomes one of the five)
    const unsigned lower = v >= (unsigned)'a' && v <= (unsigned)'z' ? 8u : 0u;
    if (u == (unsigned)'T') return 0u | lower;
    if (u == (unsigned)'C') return 1u | lower;
    if (u == (unsigned)'A') return 2u | lower;
    if (u == (unsigned)'G') return 3u | lower;
    if (u == (unsigned)'N') return 4u | lower;
    return 4u | 16u | lower;
}

// symbol p of the input
template <int SRC>
__device__ __forceinline__ unsigned bl_symbol(const uint8_t BX_GLOBAL *src, int64_t p)
{
    if (SRC == BL_NIB) {
        const unsigned b = src[p >> 1];
        return (p & 1) ? b & 15u : b >> 4;
    }
    return src[p];
}

// symbol i of a thread's 16, whose input bytes lie in raw[] in memory order (16 bytes; 8 of a nib)
template <int SRC>
__device__ __forceinline__ unsigned bl_at(const uint32_t raw[4], int i)
{
    if (SRC == BL_NIB) {
        const unsigned b = (raw[i >> 3] >> (8 * ((i >> 1) & 3))) & 0xFFu;
        return (i & 1) ? b & 15u : b >> 4;
    }
    return (raw[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

// src: the symbols (size bytes, or (size + 1) / 2 of a nib); vec: src is 16-byte aligned (4-byte for a nib).  tiles ==
// ceil(size / BL_TILE) is the grid and the stride of counts and bases; room_words: the words of `packed`, whole checkpoint blocks.
// FILL == false writes packed, counts and (with want_other) first_other; FILL == true reads counts and bases and writes the blocks.
template <int SRC, bool FILL>
__global__ __launch_bounds__(BL_THREADS) void bl_build_kernel(const uint8_t *__restrict__ src, int64_t size, int vec, int64_t tiles, int64_t room_words,
                                                              uint32_t *__restrict__ packed, int32_t *counts, int want_other,
                                                              unsigned long long *first_other, const int64_t *__restrict__ bases,
                                                              int32_t *__restrict__ n_start, int32_t *__restrict__ n_end, int32_t *__restrict__ m_start,
                                                              int32_t *__restrict__ m_end)
{
    __shared__ int32_t l_wave[BL_LISTS][BL_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    if (FILL) {  // a tile without a block boundary has nothing to place (the same for every thread: no barrier is left out by some)
        int any = 0;
#pragma unroll
        for (int l = 0; l < BL_LISTS; l++) any |= as_global(counts)[(int64_t)l * tiles + tile];
        if (any == 0) return;
    }
    const uint8_t BX_GLOBAL *g_src = as_global(src);
    const int64_t e0 = tile * BL_TILE + 16 * tid;  // this thread's positions: [e0, e0 + cnt)
    const int cnt = e0 >= size ? 0 : (size - e0 < 16 ? (int)(size - e0) : 16);
    uint32_t raw[4] = {0u, 0u, 0u, 0u};
    if (cnt == 16 && vec) {
        if (SRC == BL_NIB) {
            const uint32_t BX_GLOBAL *w = reinterpret_cast<const uint32_t BX_GLOBAL *>(g_src + (e0 >> 1));
            raw[0] = w[0], raw[1] = w[1];
        } else {
            const int4 w = load_int4(reinterpret_cast<const int32_t BX_GLOBAL *>(g_src + e0));
            raw[0] = (uint32_t)w.x, raw[1] = (uint32_t)w.y, raw[2] = (uint32_t)w.z, raw[3] = (uint32_t)w.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i >= cnt) continue;
            const unsigned s = bl_symbol<SRC>(g_src, e0 + i);
            if (SRC == BL_NIB) raw[i >> 3] |= s << (8 * ((i >> 1) & 3) + ((i & 1) ? 0 : 4));
            else raw[i >> 2] |= s << (8 * (i & 3));
        }
    }
    unsigned word = 0, is_n = 0, is_m = 0, is_other = 0;  // base i at bits 31 - 2 i .. 30 - 2 i; a bit per position
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const unsigned c = bl_classify<SRC>(bl_at<SRC>(raw, i));
        word |= (c & 3u) << (30 - 2 * i);
        is_n |= ((c >> 2) & 1u) << i;
        is_m |= ((c >> 3) & 1u) << i;
        is_other |= ((c >> 4) & 1u) << i;
    }
    const unsigned valid = (1u << cnt) - 1u;  // (what lies past the sequence is nothing: code 0, in no block)
    is_n &= valid, is_m &= valid, is_other &= valid;
    if (cnt < 16) word &= cnt ? ~(0xFFFFFFFFu >> (2 * cnt)) : 0u;
    if (!FILL) {
        const int64_t w = tile * BL_THREADS + tid;
        if (w < room_words) as_global(packed)[w] = __builtin_bswap32(word);
        if (want_other && is_other) {
            const int i = __builtin_ctz(is_other);
            BL_ATOMIC_MIN64(first_other, ((unsigned long long)(e0 + i) << 8) | bl_at<SRC>(raw, i));
        }
    }
    // the symbol before and the symbol after this thread's: where runs go on
    const unsigned before = cnt && e0 > 0 ? bl_classify<SRC>(bl_symbol<SRC>(g_src, e0 - 1)) : 0u;
    const unsigned after = cnt == 16 && e0 + 16 < size ? bl_classify<SRC>(bl_symbol<SRC>(g_src, e0 + 16)) : 0u;
    unsigned bits[BL_LISTS];
    bits[0] = is_n & ~((is_n << 1) | ((before >> 2) & 1u)) & 0xFFFFu;
    bits[1] = is_m & ~((is_m << 1) | ((before >> 3) & 1u)) & 0xFFFFu;
    bits[2] = is_n & ~((is_n >> 1) | (((after >> 2) & 1u) << 15));
    bits[3] = is_m & ~((is_m >> 1) | (((after >> 3) & 1u) << 15));
    int mine[BL_LISTS], upto[BL_LISTS];
#pragma unroll
    for (int l = 0; l < BL_LISTS; l++) {
        mine[l] = __builtin_popcount(bits[l]);
        upto[l] = BL_WAVE_PREFIX(mine[l]);  // the wave's entries up to and including this thread's
        if ((tid & 63) == 63) l_wave[l][tid >> 6] = upto[l];
    }
    __syncthreads();
    if (!FILL) {
        if (tid < BL_LISTS) {
            int all = 0;
#pragma unroll
            for (int w = 0; w < BL_THREADS / 64; w++) all += l_wave[tid][w];
            as_global(counts)[(int64_t)tid * tiles + tile] = all;
        }
        return;
    }
#pragma unroll
    for (int l = 0; l < BL_LISTS; l++) {
        if (bits[l] == 0) continue;
        int earlier = 0;
#pragma unroll
        for (int w = 0; w < BL_THREADS / 64; w++)
            if (w < (tid >> 6)) earlier += l_wave[l][w];
        int64_t at = as_global(bases)[(int64_t)l * tiles + tile] - as_global(bases)[(int64_t)l * tiles] + earlier + (upto[l] - mine[l]);
        int32_t BX_GLOBAL *to = as_global(l == 0 ? n_start : l == 1 ? m_start : l == 2 ? n_end : m_end);
        const int64_t first = e0 + (l >= 2 ? 1 : 0);  // (an end is the position after the run's last)
#pragma unroll
        for (int i = 0; i < 16; i++)
            if ((bits[l] >> i) & 1u) to[at++] = (int32_t)(first + i);
    }
}

// cum[0] = 0, cum[i + 1] = end[i] - start[i] for i in [0, n): the block sizes, for the scan that makes them running sizes
__global__ __launch_bounds__(BL_THREADS) void bl_sizes_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ end, int64_t n,
                                                              int32_t *__restrict__ cum)
{
    const int64_t i = (int64_t)blockIdx.x * BL_THREADS + threadIdx.x;
    if (i > n) return;
    as_global(cum)[i] = i == 0 ? 0 : as_global(end)[i - 1] - as_global(start)[i - 1];
}

}  // namespace bxmi

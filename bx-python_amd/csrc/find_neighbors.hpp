// find_neighbors.hpp -- batched before()/after(): IntervalNode.left / right for a whole array of positions, with the
// reference's "sort, keep n" rule applied on the device.  intersection.pyx:192-260.
// Included by intervals.hip (one translation unit; the kernels share its constants and device helpers).
//
// after  (dir > 0): the candidates are one contiguous run of the in-order sequence (start sorted), so two ranks on the
//                   start tree and a copy of the first min(k, count) of them is the whole answer.
// before (dir < 0): the candidates are filtered from the window [first j with pm[j] >= vlo, #{start <= p}) and listed in
//                   REVERSE in-order; the answer is their top k by (end desc, in-order position desc), or the list itself
//                   when it holds exactly k (intersection.pyx:242-245).  One wave per query keeps a sorted top 64 in
//                   registers (one 64-bit key per lane); a query whose window is longer than NB_BIG is moved to a list that
//                   whole workgroups take afterwards, so a pile of long targets does not hold the ordinary queries up.
#pragma once

namespace bxmi {

constexpr int NB_MAX_K = 64;          // the cap on k (one key per lane of a wave)
constexpr int NB_BIG = 2048;          // windows longer than this go to the workgroup kernel
constexpr int NB_WAVE_THREADS = 256;  // wave-per-query kernel: four independent waves per workgroup
constexpr int NB_BLOCK_THREADS = 1024;  // workgroup-per-query kernel: 16 waves share one window

// #{a[i] < x} for a 64-bit threshold: everything below INT_MIN ranks 0, everything above INT_MAX ranks n (the tree's
// keys are int32 and its padding is INT_MAX, so INT_MAX itself is answered by the tree).
__device__ __forceinline__ int nb_clamp_key(long long x) { return x < INT_MIN ? INT_MIN : x > INT_MAX ? INT_MAX : (int)x; }

// 64-bit ordering key of a candidate: biased end in the high word, in-order position + 1 in the low word.  Larger = earlier
// in the reference's sorted list; 0 = no candidate.
__device__ __forceinline__ unsigned long long nb_key(int32_t end, int j)
{
    return ((unsigned long long)((uint32_t)end ^ 0x80000000u) << 32) | (unsigned long long)(uint32_t)(j + 1);
}

__device__ __forceinline__ unsigned long long nb_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long nb_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// Bitonic sort of one key per lane across the wave, descending (lane 0 = largest).
__device__ __forceinline__ unsigned long long nb_wave_sort_desc(unsigned long long v)
{
    const int lane = lane_id();
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            unsigned long long o = __shfl_xor(v, j, 64);
            bool desc = (lane & k) == 0, low = (lane & j) == 0;
            v = (low == desc) ? nb_max(v, o) : nb_min(v, o);
        }
    }
    return v;
}

// top (descending across lanes) := the 64 largest of top and c (c descending too): the lane-wise max of top and reversed c
// is a bitonic sequence holding them, and six exchange steps sort it.
__device__ __forceinline__ unsigned long long nb_wave_merge_desc(unsigned long long top, unsigned long long c_rev)
{
    const int lane = lane_id();
    unsigned long long v = nb_max(top, c_rev);
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        unsigned long long o = __shfl_xor(v, j, 64);
        v = (lane & j) == 0 ? nb_max(v, o) : nb_min(v, o);
    }
    return v;
}

// One wave folds reverse-in-order steps [t_from, t_to) of a window ending at hi (step t = position hi - 1 - t) into its top
// list and candidate count.  Keys that cannot beat the current k-th do not pay for a sort.
__device__ __forceinline__ void nb_wave_scan(const int32_t *__restrict__ e_ord, int hi, int t_from, int t_to, long long vlo,
                                             long long vhi, int k, unsigned long long &top, int &cnt)
{
    const int lane = lane_id();
    for (int t0 = t_from; t0 < t_to; t0 += 64) {
        const int t = t0 + lane, j = hi - 1 - t;
        unsigned long long key = 0;
        if (t < t_to) {
            const long long v = e_ord[j];
            if (v >= vlo && v < vhi) key = nb_key((int32_t)v, j);
        }
        const unsigned long long m = __ballot(key != 0);
        if (m == 0) continue;
        cnt += __popcll(m);
        const unsigned long long kth = __shfl(top, k - 1, 64);
        if (!__any(key > kth)) continue;
        key = nb_wave_sort_desc(key);
        top = nb_wave_merge_desc(top, __shfl(key, 63 - lane, 64));
    }
}

// The answer of one query from its top list and candidate count (whole wave): out[q*k + i] for i < k, entries past
// min(k, cnt) are -1.  cnt == k: the candidates themselves in reverse in-order (all of them are in the list).
__device__ __forceinline__ void nb_wave_finish(unsigned long long top, int cnt, int k, const int32_t *__restrict__ idx, int64_t q,
                                               int32_t *__restrict__ out, int32_t *__restrict__ n_out, int64_t *__restrict__ n_cand)
{
    const int lane = lane_id();
    if (cnt == k) top = nb_wave_sort_desc(top & 0xffffffffull);  // position desc
    const int m = cnt < k ? cnt : k;
    if (lane < k) out[q * k + lane] = lane < m ? idx[(int)(uint32_t)top - 1] : -1;
    if (lane == 0) {
        n_out[q] = m;
        if (n_cand) n_cand[q] = cnt;
    }
}

// after(): two ranks on the start tree per query (8-lane groups, FIND_Q queries each), then the first min(k, count) of the
// run [lo, hi) in in-order -- already the reference's order, sorted by start or not.
template <bool DPP>
__global__ __launch_bounds__(FIND_THREADS) void nb_after_kernel(TreeDev S, IndexDev ix, const int32_t *__restrict__ pos_arr, int64_t nq,
                                                               int k, int max_dist, int32_t *__restrict__ out,
                                                               int32_t *__restrict__ n_out, int64_t *__restrict__ n_cand)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    stage_tree(S, lds);
    __syncthreads();
    const int sub = threadIdx.x & 7;
    const int64_t group = (int64_t)blockIdx.x * (FIND_THREADS / 8) + (threadIdx.x >> 3);
    const int64_t ngroups = (int64_t)gridDim.x * (FIND_THREADS / 8);
    for (int64_t q0 = group * FIND_Q; q0 < nq; q0 += ngroups * FIND_Q) {
        long long vlo[FIND_Q], vhi[FIND_Q];
        int klo[FIND_Q], khi[FIND_Q], rlo[FIND_Q], rhi[FIND_Q];
#pragma unroll
        for (int j = 0; j < FIND_Q; j++) {
            const long long p = (q0 + j < nq ? (long long)pos_arr[q0 + j] : 0ll) + 1;  // intersection.pyx:255
            vlo[j] = p, vhi[j] = p + max_dist;                                         // keep 0 <= start - p < max_dist
            klo[j] = nb_clamp_key(vlo[j]), khi[j] = nb_clamp_key(vhi[j]);
        }
        tree_rank_lt<DPP, FIND_Q>(S, lds, klo, rlo, sub);
        tree_rank_lt<DPP, FIND_Q>(S, lds, khi, rhi, sub);
#pragma unroll
        for (int j = 0; j < FIND_Q; j++) {
            const int64_t q = q0 + j;
            if (q >= nq) break;
            const int lo = vlo[j] > INT_MAX ? ix.n : rlo[j];
            const int hi = vhi[j] > INT_MAX ? ix.n : rhi[j];
            const int cnt = hi > lo ? hi - lo : 0;
            const int m = cnt < k ? cnt : k;
            for (int i = sub; i < k; i += 8) out[q * k + i] = i < m ? ix.idx[lo + i] : -1;
            if (sub == 0) {
                n_out[q] = m;
                if (n_cand) n_cand[q] = cnt;
            }
        }
    }
}

// before(), pass 1: the candidate window of every query (start tree: #{start <= p}; prefix-max tree: first pm >= vlo).
// Windows longer than NB_BIG are listed in big[1..] (big[0] = how many; zeroed by the host).
template <bool DPP>
__global__ __launch_bounds__(FIND_THREADS) void nb_before_window_kernel(TreeDev S, TreeDev P, IndexDev ix, const int32_t *__restrict__ pos_arr,
                                                                       int64_t nq, int max_dist, int2 *__restrict__ win,
                                                                       int32_t *__restrict__ big)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    int32_t *ldsS = lds, *ldsP = lds + S.lds_ints;
    stage_tree(S, ldsS);
    stage_tree(P, ldsP);
    __syncthreads();
    const int sub = threadIdx.x & 7;
    const int64_t group = (int64_t)blockIdx.x * (FIND_THREADS / 8) + (threadIdx.x >> 3);
    const int64_t ngroups = (int64_t)gridDim.x * (FIND_THREADS / 8);
    for (int64_t q0 = group * FIND_Q; q0 < nq; q0 += ngroups * FIND_Q) {
        long long vlo[FIND_Q], vhi[FIND_Q];
        int klo[FIND_Q], khi[FIND_Q], rlo[FIND_Q], rhi[FIND_Q];
#pragma unroll
        for (int j = 0; j < FIND_Q; j++) {
            const long long p = (q0 + j < nq ? (long long)pos_arr[q0 + j] : 0ll) - 1;  // intersection.pyx:240
            vlo[j] = p - max_dist + 1, vhi[j] = p + 1;                                  // keep 0 <= p - end < max_dist
            klo[j] = nb_clamp_key(vlo[j]), khi[j] = nb_clamp_key(vhi[j]);
        }
        tree_rank_lt<DPP, FIND_Q>(P, ldsP, klo, rlo, sub);
        tree_rank_lt<DPP, FIND_Q>(S, ldsS, khi, rhi, sub);
#pragma unroll
        for (int j = 0; j < FIND_Q; j++) {
            const int64_t q = q0 + j;
            if (q >= nq || sub != 0) continue;
            const int lo = vlo[j] > INT_MAX ? ix.n : rlo[j];
            int hi = ix.has_reversed ? ix.n : (vhi[j] > INT_MAX ? ix.n : rhi[j]);  // (reversed targets: the superset, see bxmi_ivl_neighbors)
            if (hi < lo) hi = lo;
            win[q] = make_int2(lo, hi);
            if (hi - lo > NB_BIG) big[1 + atomicAdd(big, 1)] = (int32_t)q;
        }
    }
}

// before(), pass 2: one wave per query with a window of at most NB_BIG.
__global__ __launch_bounds__(NB_WAVE_THREADS) void nb_before_wave_kernel(IndexDev ix, const int32_t *__restrict__ pos_arr, int64_t nq, int k,
                                                                        int max_dist, const int2 *__restrict__ win,
                                                                        int32_t *__restrict__ out, int32_t *__restrict__ n_out,
                                                                        int64_t *__restrict__ n_cand)
{
    const int64_t wave = (int64_t)blockIdx.x * (NB_WAVE_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (NB_WAVE_THREADS / 64);
    for (int64_t q = wave; q < nq; q += nwaves) {
        const int2 w = win[q];
        if (w.y - w.x > NB_BIG) continue;
        const long long p = (long long)pos_arr[q] - 1;
        unsigned long long top = 0;
        int cnt = 0;
        nb_wave_scan(ix.e_ord, w.y, 0, w.y - w.x, p - max_dist + 1, p + 1, k, top, cnt);
        nb_wave_finish(top, cnt, k, ix.idx, q, out, n_out, n_cand);
    }
}

// before(), pass 3: the long windows, one workgroup each; every wave folds a slice, wave 0 merges the 16 lists.
__global__ __launch_bounds__(NB_BLOCK_THREADS) void nb_before_block_kernel(IndexDev ix, const int32_t *__restrict__ pos_arr, int k,
                                                                          int max_dist, const int2 *__restrict__ win,
                                                                          const int32_t *__restrict__ big, int32_t *__restrict__ out,
                                                                          int32_t *__restrict__ n_out, int64_t *__restrict__ n_cand)
{
    constexpr int NW = NB_BLOCK_THREADS / 64;
    __shared__ unsigned long long tops[NW][64];
    __shared__ int cnts[NW];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int nbig = big[0];
    for (int b = blockIdx.x; b < nbig; b += gridDim.x) {
        const int64_t q = big[1 + b];
        const int2 w = win[q];
        const long long p = (long long)pos_arr[q] - 1;
        const int len = w.y - w.x;
        const int slice = ((len + NW - 1) / NW + 63) & ~63;
        const int t_from = wv * slice < len ? wv * slice : len;
        const int t_to = t_from + slice < len ? t_from + slice : len;
        unsigned long long top = 0;
        int cnt = 0;
        nb_wave_scan(ix.e_ord, w.y, t_from, t_to, p - max_dist + 1, p + 1, k, top, cnt);
        tops[wv][lane] = top;
        if (lane == 0) cnts[wv] = cnt;
        __syncthreads();
        if (wv == 0) {
            top = tops[0][lane];
            cnt = cnts[0];
            for (int i = 1; i < NW; i++) {
                top = nb_wave_merge_desc(top, tops[i][63 - lane]);
                cnt += cnts[i];
            }
            nb_wave_finish(top, cnt, k, ix.idx, q, out, n_out, n_cand);
        }
        __syncthreads();
    }
}

}  // namespace bxmi

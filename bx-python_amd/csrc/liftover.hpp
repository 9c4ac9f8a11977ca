// liftover.hpp -- mapping features through chain alignments (the reference's scripts/bnMapper.py) for a whole array of
// features in one device pass.  Included by liftover.hip (the entry points bxmi_chainmap_*).
//
// Resident per source chromosome (bxmi_chainmap): a sealed interval index over the chain spans [tStart, tEnd) in file order,
// the block tables of all chains concatenated (coordinates relative to their chain's start, bnMapper.py:293-308,
// lib/bx/align/epo.py:19-43) and per chain tStart, tEnd, qStart, Sz = qEnd - qStart and the query strand.
//
// Passes of one batch:
//   1. the chains each feature meets, as CSR in IntervalTree.find order (bnMapper.py:154)           -- bxmi_ivl_find_dev
//   2. lo_select_kernel, a thread per feature: for each of its chains transform() up to the slice list (bnMapper.py:83-112:
//      two binary searches in that chain's block table, the gap rule, to_start / to_end, mapped bases, the keep_split
//      measure), then the choice between chains (:157-183), the threshold (:187) and the number of rows the union leaves
//   3. exclusive scan of the row counts -> offsets                                                  -- device_scan
//   4. lo_emit_kernel (a thread per feature) and lo_emit_wave_kernel (a wave per feature whose rows come from more than
//      LO_BIG runs of blocks): slices, strand flip, offset, union, ascending order (:114-142, _epo.pyx:128-164)
//
// What keeps every step O(1) or O(log) per (feature, chain): the tables are validated on creation (no block and no gap of
// negative length; EMPTY blocks are legal -- chains made from EPO alignments have them), so inside a chain t_start, t_end, q_start
// and q_end never descend.  Then
//   * np.where(CT[:,1] > start)[0][0] and np.where(CT[:,0] < end)[0][-1] (:95-96) are binary searches;
//   * the slices of a chain never descend on the + strand and never ascend on the - strand, in starts AND ends, so sorting the
//     starts and the ends independently (elem_u, _epo.pyx:138) only reverses the - strand list, and the sweep "join while
//     next.start <= current end" cuts exactly at the block junctions whose query-side gap is positive -- whatever the clipping of
//     the first and the last slice did, their inner edges are block edges.  The blocks between two such junctions are a RUN: one
//     row of the output unless it is empty (the s < e filter of bnMapper.py:139: a run of empty blocks only).  run_of[] numbers
//     the runs of all chains, run_first[] gives a run's first block and rne[] the prefix count of non-empty runs, so a
//     feature's rows are counted from its two end runs plus a difference of rne[], and each run finds its row without a sweep;
//   * a single slice is returned as it is, zero-length included (:131);
//   * the gap rule (:102-107) asks whether ANY junction of si .. ei-2 is wider than max_gap: gapc[] is the prefix count of
//     such junctions for the batch's max_gap (one pass over the blocks per new value, kept until max_gap changes);
//   * the mapped bases (:187) are the clipped first and last slice plus cum[] (a prefix sum of block sizes) between them.
#pragma once

namespace bxmi {

constexpr int LO_THREADS = 256;
constexpr int LO_BIG = 64;  // features whose chosen chain contributes more runs than this are emitted a wave each

// per-feature status (bxmi.h: BXMI_LIFT_*)
constexpr int LO_MAPPED = 0, LO_NOCHAIN = 1, LO_SPLIT = 2, LO_BELOW = 3, LO_EMPTY = 4;

struct LoDev {
    const int32_t *t_start, *t_end, *q_start;  // per block, relative to the chain's tStart / forward qStart
    const int32_t *cum;                        // per block: sum of the sizes of the chain's earlier blocks
    const int32_t *run_of;                     // per block: its run (runs of all chains numbered in block order)
    const int32_t *run_first;                  // per run: its first block; [n_runs] = number of blocks
    const int32_t *rne;                        // per run r: #{r' < r : run r' holds a non-empty block}
    const int32_t *gapc;                       // per block j: #{i < j : the gap i -> i + 1 exceeds max_gap on either side} (max_gap >= 0 only)
    const int4 *c_meta;                        // per chain: tStart, tEnd, qStart, Sz
    const int32_t *c_off;                      // per chain: first block; [n_chains] = number of blocks
    const int32_t *c_minus;                    // per chain: 1 = query strand '-'
    int32_t n_chains;
};

// fs <= fe for every feature?  *bad (host-visible memory) is set otherwise.
__global__ __launch_bounds__(LO_THREADS) void lo_check_kernel(const int32_t *__restrict__ fs, const int32_t *__restrict__ fe, int64_t nf,
                                                             unsigned *__restrict__ bad)
{
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * LO_THREADS + threadIdx.x; i < nf; i += (int64_t)gridDim.x * LO_THREADS) b |= fs[i] > fe[i];
    if (__any(b) && lane_id() == 0) *bad = 1u;
}

// flag[j] = 1 when block j + 1 belongs to the same chain and either gap between the two exceeds max_gap (scanned into gapc).
__global__ __launch_bounds__(LO_THREADS) void lo_gap_flag_kernel(LoDev L, const int32_t *__restrict__ blk_chain, int64_t nb, int max_gap,
                                                                int32_t *__restrict__ flag)
{
    for (int64_t j = (int64_t)blockIdx.x * LO_THREADS + threadIdx.x; j < nb; j += (int64_t)gridDim.x * LO_THREADS) {
        int f = 0;
        if (j + 1 < nb && blk_chain[j + 1] == blk_chain[j]) {
            const int te = L.t_end[j], qe = L.q_start[j] + (te - L.t_start[j]);
            f = (L.t_start[j + 1] - te > max_gap) || (L.q_start[j + 1] - qe > max_gap);
        }
        flag[j] = f;
    }
}

// Pass 2 + 3a: transform() per (feature, chain) up to the slice list, the choice, the threshold, the row count.
// sel[f] = (first run, last run, to_start, to_end) of the chosen chain; big[1..] lists the features for
// the wave kernel (big[0] = how many; zeroed by the host).
__global__ __launch_bounds__(LO_THREADS) void lo_select_kernel(LoDev L, const int32_t *__restrict__ fs, const int32_t *__restrict__ fe,
                                                              int64_t nf, const int64_t *__restrict__ hoff, const int32_t *__restrict__ hits,
                                                              int max_gap, int select, double threshold, int4 *__restrict__ sel,
                                                              int32_t *__restrict__ chain_out, int32_t *__restrict__ status_out,
                                                              int32_t *__restrict__ rows_out, int32_t *__restrict__ big)
{
    for (int64_t f = (int64_t)blockIdx.x * LO_THREADS + threadIdx.x; f < nf; f += (int64_t)gridDim.x * LO_THREADS) {
        const int s = fs[f], e = fe[f];
        int n = 0, pick_chain = -1, pick_rows = 0;
        long long best = 0, pick_bases = 0;
        int4 pick = make_int4(0, 0, 0, 0);
        for (int64_t h = hoff[f], h_end = hoff[f + 1]; h < h_end; h++) {
            const int c = hits[h];
            const int4 m = L.c_meta[c];  // tStart, tEnd, qStart, Sz
            const int off = L.c_off[c], nb = L.c_off[c + 1] - off;
            const int a = (int)((long long)(s > m.x ? s : m.x) - m.x);  // bnMapper.py:89
            const int b = (int)((long long)(e < m.y ? e : m.y) - m.x);
            const int32_t *ts_ = L.t_start + off, *te_ = L.t_end + off, *qs_ = L.q_start + off;
            // si = first block with T.end > a                                                          (:95)
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (te_[mid] > a) hi = mid;
                else lo = mid + 1;
            }
            const int si = lo;
            if (si >= nb) continue;
            // ei = last block with T.start < b; it is at least si - 1: gallop from si, then halve          (:96)
            int p = si, step = 1;
            while (p < nb && ts_[p] < b) {
                lo = p + 1;
                p += step;
                step <<= 1;
            }
            hi = p < nb ? p : nb;
            if (lo > hi) lo = hi;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ts_[mid] < b) lo = mid + 1;
                else hi = mid;
            }
            const int ei = lo - 1;
            if (si > ei) continue;                                                                       // (:98)
            if (max_gap >= 0 && si < ei - 1 && L.gapc[off + ei - 1] - L.gapc[off + si] > 0) continue;      // (:102-107)
            const int t_si = ts_[si], q_si = qs_[si], qe_si = q_si + (te_[si] - t_si);
            const int t_ei = ts_[ei], q_ei = qs_[ei], te_ei = te_[ei], qe_ei = q_ei + (te_ei - t_ei);
            const int to_start = q_si + (a > t_si ? a - t_si : 0);                                      // (:111)
            const int to_end = qe_ei - (te_ei > b ? te_ei - b : 0);                                     // (:112)
            long long bases, measure;
            int rows, r0, r1;
            if (si == ei) {
                bases = (long long)to_end - to_start, measure = 0, rows = 1;
                r0 = r1 = L.run_of[off + si];
            } else {
                bases = ((long long)qe_si - to_start) + ((long long)L.cum[off + ei] - L.cum[off + si + 1]) + ((long long)to_end - q_ei);
                // last slice's end minus first slice's END (:176), after the strand flip (:120-122)
                measure = L.c_minus[c] ? (long long)to_start - q_ei : (long long)to_end - qe_si;
                r0 = L.run_of[off + si], r1 = L.run_of[off + ei];
                if (r0 == r1) {
                    rows = to_end > to_start ? 1 : 0;
                } else {  // the two end runs as clipped, the complete runs between them from the prefix count
                    const int kb = L.run_first[r0 + 1] - 1;
                    const int y0 = L.q_start[kb] + (L.t_end[kb] - L.t_start[kb]), x1 = L.q_start[L.run_first[r1]];
                    rows = (y0 > to_start) + (L.rne[r1] - L.rne[r0 + 1]) + (to_end > x1);
                }
            }
            n++;
            if (n == 1 || (select == 1 && measure > best)) {                                             // (:168-183)
                pick = make_int4(r0, r1, to_start, to_end);
                pick_chain = c, pick_rows = rows, pick_bases = bases;
                if (n == 1) best = measure > 0 ? measure : 0;
                else best = measure;
            }
        }
        int status = LO_MAPPED;
        if (n == 0) status = LO_NOCHAIN;
        else if (n > 1 && select == 0) status = LO_SPLIT;
        else if ((double)((long long)e - s) * threshold > (double)pick_bases) status = LO_BELOW;           // (:187)
        else if (pick_rows == 0) status = LO_EMPTY;                                                      // (:193)
        if (status != LO_MAPPED) pick_chain = -1, pick_rows = 0;
        sel[f] = pick;
        chain_out[f] = pick_chain;
        status_out[f] = status;
        rows_out[f] = pick_rows;
        if (pick_rows > 0 && pick.y - pick.x + 1 > LO_BIG) big[1 + atomicAdd(big, 1)] = (int32_t)f;
    }
}

// Run r of a chosen chain as its feature's row: (x, y) from the run's first and last block, the feature's end runs clipped to
// to_start / to_end; on the - strand (x, y) becomes (Sz - y, Sz - x) and the rows are reversed (see the head).  ne0 = the first
// run is not empty.  A feature of one run (r0 == r1) has one row or none, as counted: a single slice is kept even when empty.
__device__ __forceinline__ void lo_emit_run(const LoDev &L, int r, int4 pk, int ne0, int4 m, bool minus, int rows, int64_t base,
                                            int32_t *__restrict__ out_start, int32_t *__restrict__ out_end)
{
    int x = pk.z, y = pk.w;
    if (r != pk.x) x = L.q_start[L.run_first[r]];
    if (r != pk.y) {
        const int kb = L.run_first[r + 1] - 1;
        y = L.q_start[kb] + (L.t_end[kb] - L.t_start[kb]);
    }
    if (pk.x != pk.y && x >= y) return;
    const int row = r == pk.x ? 0 : ne0 + (L.rne[r] - L.rne[pk.x + 1]);
    if (!minus) {
        out_start[base + row] = m.z + x;
        out_end[base + row] = m.z + y;
    } else {
        const int64_t o = base + (rows - 1 - row);
        out_start[o] = m.z + (m.w - y);
        out_end[o] = m.z + (m.w - x);
    }
}

__device__ __forceinline__ int lo_first_run_nonempty(const LoDev &L, int4 pk)
{
    if (pk.x == pk.y) return 1;
    const int kb = L.run_first[pk.x + 1] - 1;
    return L.q_start[kb] + (L.t_end[kb] - L.t_start[kb]) > pk.z;
}

// Pass 4, a thread per feature (features of more than LO_BIG runs are left to the wave kernel).  Nothing is written when
// the rows do not fit `cap` (BXMI_ERANGE: offsets and total valid, slices untouched).
__global__ __launch_bounds__(LO_THREADS) void lo_emit_kernel(LoDev L, int64_t nf, const int4 *__restrict__ sel, const int32_t *__restrict__ chain,
                                                            const int64_t *__restrict__ offsets, int64_t cap, int32_t *__restrict__ out_start,
                                                            int32_t *__restrict__ out_end)
{
    if (offsets[nf] > cap) return;
    for (int64_t f = (int64_t)blockIdx.x * LO_THREADS + threadIdx.x; f < nf; f += (int64_t)gridDim.x * LO_THREADS) {
        const int c = chain[f];
        if (c < 0) continue;
        const int4 pk = sel[f];
        if (pk.y - pk.x + 1 > LO_BIG) continue;
        const int64_t base = offsets[f];
        const int rows = (int)(offsets[f + 1] - base);
        if (rows == 0) continue;
        const int4 m = L.c_meta[c];
        const bool minus = L.c_minus[c] != 0;
        const int ne0 = lo_first_run_nonempty(L, pk);
        for (int r = pk.x; r <= pk.y; r++) lo_emit_run(L, r, pk, ne0, m, minus, rows, base, out_start, out_end);
    }
}

// Pass 4 for the long features: a wave each, a run per lane and step.
__global__ __launch_bounds__(LO_THREADS) void lo_emit_wave_kernel(LoDev L, int64_t nf, const int4 *__restrict__ sel,
                                                                 const int32_t *__restrict__ chain, const int32_t *__restrict__ big,
                                                                 const int64_t *__restrict__ offsets, int64_t cap, int32_t *__restrict__ out_start,
                                                                 int32_t *__restrict__ out_end)
{
    if (offsets[nf] > cap) return;
    const int nbig = big[0];
    const int lane = lane_id();
    for (int w = blockIdx.x * (LO_THREADS / 64) + (threadIdx.x >> 6); w < nbig; w += gridDim.x * (LO_THREADS / 64)) {
        const int64_t f = big[1 + w];
        const int c = chain[f];
        const int4 pk = sel[f];
        const int64_t base = offsets[f];
        const int rows = (int)(offsets[f + 1] - base);
        const int4 m = L.c_meta[c];
        const bool minus = L.c_minus[c] != 0;
        const int ne0 = lo_first_run_nonempty(L, pk);
        for (int r = pk.x + lane; r <= pk.y; r += 64) lo_emit_run(L, r, pk, ne0, m, minus, rows, base, out_start, out_end);
    }
}

}  // namespace bxmi

// liftover.hip -- liftover through chain alignments (bxmi_chainmap_*): the chains' tables in HBM, a batch of features mapped in
// four passes.  Kernels and what the tables promise them: liftover.hpp.  The chain spans live in an interval index that is
// used through its public entry points only.
#include <climits>
#include <new>
#include <vector>

#include "primitives.hpp"
#include "liftover.hpp"

namespace bxmi {

int ivl_host_stream(bxmi_ivl_t *h, hipStream_t *out);  // intervals.hip: the stream the index's host-pointer entry points run on

}  // namespace bxmi

using namespace bxmi;

struct bxmi_chainmap {
    bxmi_ivl_t *ivl = nullptr;  // the chain spans, in the order given
    int64_t n_chains = 0, n_blocks = 0, max_chain_blocks = 0;
    DevBuf t_start, t_end, q_start, cum, run_of, run_first, rne, blk_chain, c_meta, c_off, c_minus;
    DevBuf gapc;              // the gap rule's prefix counts for gap_for
    int64_t gap_for = -1;     // the max_gap gapc was made for (-1 = none yet)
    // scratch of one batch
    DevBuf hoff, hits, sel, rows, big, scan_scratch;
    unsigned *bad_host = nullptr;  // host-visible word lo_check_kernel writes
    // device staging of the host-pointer entry point
    DevBuf d_fs, d_fe, d_chain, d_status, d_off, d_os, d_oe;
};

static LoDev lo_dev(const bxmi_chainmap *m)
{
    LoDev L;
    L.t_start = m->t_start.as<int32_t>(), L.t_end = m->t_end.as<int32_t>(), L.q_start = m->q_start.as<int32_t>();
    L.cum = m->cum.as<int32_t>(), L.gapc = m->gapc.as<int32_t>();
    L.run_of = m->run_of.as<int32_t>(), L.run_first = m->run_first.as<int32_t>(), L.rne = m->rne.as<int32_t>();
    L.c_meta = m->c_meta.as<int4>(), L.c_off = m->c_off.as<int32_t>(), L.c_minus = m->c_minus.as<int32_t>();
    L.n_chains = (int32_t)m->n_chains;
    return L;
}

template <typename T>
static int lo_upload(DevBuf &b, const std::vector<T> &v)
{
    BXMI_TRY(b.reserve(v.size() * sizeof(T) + 16));
    if (!v.empty()) BXMI_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return BXMI_OK;
}

extern "C" int bxmi_chainmap_destroy(bxmi_chainmap_t *m)
{
    if (!m) return BXMI_OK;
    if (m->ivl) (void)bxmi_ivl_destroy(m->ivl);
    if (m->bad_host) (void)hipHostFree(m->bad_host);
    delete m;
    return BXMI_OK;
}

extern "C" int bxmi_chainmap_create(bxmi_chainmap_t **out, int64_t n_chains, const int32_t *t_start, const int32_t *t_end,
                                    const int32_t *q_start, const int32_t *q_span, const uint8_t *q_minus, const int64_t *block_off,
                                    const int32_t *blk_t_start, const int32_t *blk_t_end, const int32_t *blk_q_start)
{
    if (!out || n_chains < 0 || n_chains > INT_MAX ||
        (n_chains > 0 && (!t_start || !t_end || !q_start || !q_span || !q_minus || !block_off || !blk_t_start || !blk_t_end || !blk_q_start)))
        return fail(BXMI_EINVAL, "bxmi_chainmap_create: bad arguments");
    *out = nullptr;
    const int64_t nb = n_chains > 0 ? block_off[n_chains] : 0;
    if (n_chains > 0 && (block_off[0] != 0 || nb > INT_MAX)) return fail(BXMI_EINVAL, "bxmi_chainmap_create: block_off must run from 0 to at most 2^31-1");
    // the tables as the kernels read them, validated on the way (see the head of liftover.hpp for what rests on this)
    std::vector<int32_t> cum((size_t)nb), run_of((size_t)nb), run_first, rne, blk_chain((size_t)nb), c_off((size_t)n_chains + 1, 0), c_minus((size_t)n_chains);
    std::vector<int4> c_meta((size_t)n_chains);
    int64_t longest = 0;
    int32_t run_nonempty = 0;  // the run being walked holds a non-empty block
    for (int64_t c = 0; c < n_chains; c++) {
        const int64_t b0 = block_off[c], b1 = block_off[c + 1];
        if (b1 <= b0 || b1 > nb) return fail(BXMI_EINVAL, "bxmi_chainmap_create: chain %lld has no blocks", (long long)c);
        const long long t_span = (long long)t_end[c] - t_start[c];
        if (t_span < 0 || t_span > INT_MAX || q_span[c] < 0 || q_start[c] < 0 || (long long)q_start[c] + q_span[c] > INT_MAX)
            return fail(BXMI_EINVAL, "bxmi_chainmap_create: chain %lld: a span is negative or reaches beyond 2^31-1", (long long)c);
        long long sum = 0;
        for (int64_t j = b0; j < b1; j++) {
            const long long len = (long long)blk_t_end[j] - blk_t_start[j], qe = (long long)blk_q_start[j] + len;
            bool ok = len >= 0 && blk_t_start[j] >= 0 && blk_q_start[j] >= 0 && blk_t_end[j] <= t_span && qe <= q_span[c];
            if (ok && j > b0)
                ok = blk_t_start[j] >= blk_t_end[j - 1] && (long long)blk_q_start[j] >= (long long)blk_q_start[j - 1] + (blk_t_end[j - 1] - blk_t_start[j - 1]);
            if (!ok)
                return fail(BXMI_EINVAL, "bxmi_chainmap_create: chain %lld, block %lld: negative length, outside its chain's span, or before the end of the block before it",
                            (long long)c, (long long)(j - b0));
            cum[(size_t)j] = (int32_t)sum;
            sum += len;
            // a run begins with its chain and after every junction with a gap on the query side
            if (j == b0 || (long long)blk_q_start[j] > (long long)blk_q_start[j - 1] + (blk_t_end[j - 1] - blk_t_start[j - 1])) {
                run_first.push_back((int32_t)j);
                rne.push_back(rne.empty() ? 0 : rne.back() + run_nonempty);
                run_nonempty = 0;
            }
            if (len > 0) run_nonempty = 1;
            run_of[(size_t)j] = (int32_t)run_first.size() - 1;
            blk_chain[(size_t)j] = (int32_t)c;
        }
        c_off[(size_t)c] = (int32_t)b0;
        c_minus[(size_t)c] = q_minus[c] ? 1 : 0;
        c_meta[(size_t)c] = make_int4(t_start[c], t_end[c], q_start[c], q_span[c]);
        if (b1 - b0 > longest) longest = b1 - b0;
    }
    c_off[(size_t)n_chains] = (int32_t)nb;
    run_first.push_back((int32_t)nb);  // [n_runs]: what ends the last run
    rne.push_back(rne.empty() ? 0 : rne.back() + run_nonempty);
    bxmi_chainmap *m = new (std::nothrow) bxmi_chainmap();
    if (!m) return fail(BXMI_ENOMEM, "bxmi_chainmap_create: out of host memory");
    m->n_chains = n_chains, m->n_blocks = nb, m->max_chain_blocks = longest;
    auto build = [&]() -> int {
        BXMI_TRY(bxmi_ivl_create(&m->ivl));
        if (n_chains > 0) BXMI_TRY(bxmi_ivl_append(m->ivl, t_start, t_end, n_chains));
        BXMI_TRY(bxmi_ivl_seal(m->ivl, nullptr));
        BXMI_TRY(lo_upload(m->cum, cum));
        BXMI_TRY(lo_upload(m->run_of, run_of));
        BXMI_TRY(lo_upload(m->run_first, run_first));
        BXMI_TRY(lo_upload(m->rne, rne));
        BXMI_TRY(lo_upload(m->blk_chain, blk_chain));
        BXMI_TRY(lo_upload(m->c_meta, c_meta));
        BXMI_TRY(lo_upload(m->c_off, c_off));
        BXMI_TRY(lo_upload(m->c_minus, c_minus));
        DevBuf *dst[3] = {&m->t_start, &m->t_end, &m->q_start};
        const int32_t *src[3] = {blk_t_start, blk_t_end, blk_q_start};
        for (int i = 0; i < 3; i++) {
            BXMI_TRY(dst[i]->reserve((size_t)nb * 4 + 16));
            if (nb > 0) BXMI_HIP(hipMemcpy(dst[i]->p, src[i], (size_t)nb * 4, hipMemcpyHostToDevice));
        }
        BXMI_HIP(hipHostMalloc(reinterpret_cast<void **>(&m->bad_host), 64, hipHostMallocDefault));
        *m->bad_host = 0;
        return BXMI_OK;
    };
    const int rc = build();
    if (rc != BXMI_OK) {
        (void)bxmi_chainmap_destroy(m);
        return rc;
    }
    *out = m;
    return BXMI_OK;
}

extern "C" int bxmi_chainmap_info(const bxmi_chainmap_t *m, int64_t *n_chains, int64_t *n_blocks, int64_t *max_chain_blocks)
{
    if (!m) return fail(BXMI_EINVAL, "bxmi_chainmap_info: NULL handle");
    if (n_chains) *n_chains = m->n_chains;
    if (n_blocks) *n_blocks = m->n_blocks;
    if (max_chain_blocks) *max_chain_blocks = m->max_chain_blocks;
    return BXMI_OK;
}

// gapc for this max_gap: one pass over the blocks and a scan, kept until another value is asked for
static int lo_ensure_gapc(bxmi_chainmap *m, int max_gap, hipStream_t st)
{
    if (max_gap < 0 || m->gap_for == (int64_t)max_gap || m->n_blocks == 0) return BXMI_OK;
    BXMI_TRY(m->gapc.reserve((size_t)m->n_blocks * 4 + 16));
    m->gap_for = -1;
    int32_t *g = m->gapc.as<int32_t>();
    hipLaunchKernelGGL(lo_gap_flag_kernel, dim3(stream_grid(m->n_blocks, LO_THREADS)), dim3(LO_THREADS), 0, st, lo_dev(m),
                       m->blk_chain.as<int32_t>(), m->n_blocks, max_gap, g);
    BXMI_LAUNCH_CHECK();
    BXMI_TRY((device_scan<int32_t, int32_t, OpSum, false>(g, g, m->n_blocks, 0, nullptr, m->scan_scratch, st)));
    m->gap_for = max_gap;
    return BXMI_OK;
}

extern "C" int bxmi_chainmap_map_dev(bxmi_chainmap_t *m, const int32_t *fs, const int32_t *fe, int64_t nf, int32_t max_gap, int select,
                                     double threshold, int32_t *chain, int32_t *status, int64_t *offsets, int32_t *out_start,
                                     int32_t *out_end, int64_t cap, int64_t *total_host, void *stream)
{
    if (!m) return fail(BXMI_EINVAL, "bxmi_chainmap_map_dev: NULL handle");
    if (nf < 0 || nf > INT_MAX || !offsets || (nf > 0 && (!fs || !fe || !chain || !status)) || cap < 0 || (cap > 0 && (!out_start || !out_end)) ||
        select < 0 || select > 2 || threshold != threshold)
        return fail(BXMI_EINVAL, "bxmi_chainmap_map_dev: bad arguments");
    hipStream_t st = as_stream(stream);
    if (total_host) *total_host = 0;
    if (nf == 0) {
        BXMI_HIP(hipMemsetAsync(offsets, 0, 8, st));
        return BXMI_OK;
    }
    // fs <= fe everywhere?  The answer lies in host memory by the time the find below has waited for the stream.
    *m->bad_host = 0;
    hipLaunchKernelGGL(lo_check_kernel, dim3(stream_grid(nf, LO_THREADS)), dim3(LO_THREADS), 0, st, fs, fe, nf, m->bad_host);
    BXMI_LAUNCH_CHECK();
    // pass 1: the chains every feature meets, in find order
    BXMI_TRY(m->hoff.reserve((size_t)(nf + 2) * 8));
    int64_t pairs = 0;
    if (m->n_chains == 0) {
        BXMI_HIP(hipMemsetAsync(m->hoff.p, 0, (size_t)(nf + 1) * 8, st));
        BXMI_HIP(hipStreamSynchronize(st));
    } else {
        BXMI_TRY(m->hits.reserve((size_t)(2 * nf + 1024) * 4));  // (overlapping chains: room for two per feature before the find has to run twice)
        for (int attempt = 0;; attempt++) {
            const int64_t hcap = (int64_t)(m->hits.cap / 4) - 4;
            const int rc = bxmi_ivl_find_dev(m->ivl, fs, fe, nf, m->hoff.as<int64_t>(), m->hits.as<int32_t>(), hcap, &pairs, st);
            if (rc == BXMI_OK) break;
            if (rc != BXMI_ERANGE || attempt > 0) return rc;
            BXMI_TRY(m->hits.reserve((size_t)(pairs + 4) * 4));  // (the list did not fit the scratch: once more with room for it)
        }
    }
    if (*m->bad_host) return fail(BXMI_EINVAL, "bxmi_chainmap_map_dev: a feature has start > end");
    BXMI_TRY(lo_ensure_gapc(m, max_gap, st));
    BXMI_TRY(m->sel.reserve((size_t)nf * 16));
    BXMI_TRY(m->rows.reserve((size_t)(nf + 4) * 4));
    BXMI_TRY(m->big.reserve((size_t)(nf + 1) * 4));
    const LoDev L = lo_dev(m);
    int4 *sel = m->sel.as<int4>();
    int32_t *rows = m->rows.as<int32_t>(), *big = m->big.as<int32_t>();
    BXMI_HIP(hipMemsetAsync(big, 0, 4, st));
    const int grid = stream_grid(nf, LO_THREADS);
    // passes 2 and 3
    hipLaunchKernelGGL(lo_select_kernel, dim3(grid), dim3(LO_THREADS), 0, st, L, fs, fe, nf, m->hoff.as<int64_t>(), m->hits.as<int32_t>(),
                       (int)max_gap, select, threshold, sel, chain, status, rows, big);
    BXMI_LAUNCH_CHECK();
    BXMI_TRY((device_scan<int32_t, long long, OpSum, false>(rows, reinterpret_cast<long long *>(offsets), nf, 0ll,
                                                           reinterpret_cast<long long *>(offsets) + nf, m->scan_scratch, st)));
    // pass 4: both kernels stand down on the device when the rows do not fit cap
    hipLaunchKernelGGL(lo_emit_kernel, dim3(grid), dim3(LO_THREADS), 0, st, L, nf, sel, chain, offsets, cap, out_start, out_end);
    BXMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(lo_emit_wave_kernel, dim3(device_props().cus * 4), dim3(LO_THREADS), 0, st, L, nf, sel, chain, big, offsets, cap,
                       out_start, out_end);
    BXMI_LAUNCH_CHECK();
    int64_t total = 0;  // (copied behind the launches: nothing returns between this copy and the wait for it)
    BXMI_HIP(hipMemcpyAsync(&total, offsets + nf, 8, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipStreamSynchronize(st));
    if (total_host) *total_host = total;
    if (total > cap) return fail(BXMI_ERANGE, "bxmi_chainmap_map: %lld rows need larger buffers than cap=%lld", (long long)total, (long long)cap);
    return BXMI_OK;
}

extern "C" int bxmi_chainmap_map(bxmi_chainmap_t *m, const int32_t *fs, const int32_t *fe, int64_t nf, int32_t max_gap, int select,
                                 double threshold, int32_t *chain, int32_t *status, int64_t *offsets, int32_t *out_start, int32_t *out_end,
                                 int64_t cap, int64_t *total)
{
    if (!m) return fail(BXMI_EINVAL, "bxmi_chainmap_map: NULL handle");
    if (nf < 0 || nf > INT_MAX || !offsets || (nf > 0 && (!fs || !fe || !chain || !status)) || cap < 0 || (cap > 0 && (!out_start || !out_end)))
        return fail(BXMI_EINVAL, "bxmi_chainmap_map: bad arguments");
    if (total) *total = 0;
    if (nf == 0) {
        offsets[0] = 0;
        return BXMI_OK;
    }
    hipStream_t st = nullptr;
    BXMI_TRY(ivl_host_stream(m->ivl, &st));
    BXMI_TRY(m->d_fs.reserve((size_t)(nf + 4) * 4));
    BXMI_TRY(m->d_fe.reserve((size_t)(nf + 4) * 4));
    BXMI_TRY(m->d_chain.reserve((size_t)(nf + 4) * 4));
    BXMI_TRY(m->d_status.reserve((size_t)(nf + 4) * 4));
    BXMI_TRY(m->d_off.reserve((size_t)(nf + 2) * 8));
    BXMI_TRY(m->d_os.reserve((size_t)(cap + 4) * 4));
    BXMI_TRY(m->d_oe.reserve((size_t)(cap + 4) * 4));
    BXMI_HIP(hipMemcpyAsync(m->d_fs.p, fs, (size_t)nf * 4, hipMemcpyHostToDevice, st));
    BXMI_HIP(hipMemcpyAsync(m->d_fe.p, fe, (size_t)nf * 4, hipMemcpyHostToDevice, st));
    int64_t tot = 0;
    const int rc = bxmi_chainmap_map_dev(m, m->d_fs.as<int32_t>(), m->d_fe.as<int32_t>(), nf, max_gap, select, threshold, m->d_chain.as<int32_t>(),
                                         m->d_status.as<int32_t>(), m->d_off.as<int64_t>(), m->d_os.as<int32_t>(), m->d_oe.as<int32_t>(), cap,
                                         &tot, st);
    if (total) *total = tot;
    if (rc != BXMI_OK && rc != BXMI_ERANGE) return rc;
    BXMI_HIP(hipMemcpyAsync(chain, m->d_chain.p, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipMemcpyAsync(status, m->d_status.p, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipMemcpyAsync(offsets, m->d_off.p, (size_t)(nf + 1) * 8, hipMemcpyDeviceToHost, st));
    if (rc == BXMI_OK && tot > 0) {
        BXMI_HIP(hipMemcpyAsync(out_start, m->d_os.p, (size_t)tot * 4, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipMemcpyAsync(out_end, m->d_oe.p, (size_t)tot * 4, hipMemcpyDeviceToHost, st));
    }
    BXMI_HIP(hipStreamSynchronize(st));
    return rc;
}

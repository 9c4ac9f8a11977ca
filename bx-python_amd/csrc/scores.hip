// scores.hip -- per-base score tracks (bxmi_scores_*): dense float32 arrays in HBM, filled from spans, aggregated over
// batches of intervals (kernels and the exactness argument: scores.hpp) and summed column by column over batches of windows
// (site profiles: profile.hpp).
#include <mutex>
#include <new>
#include <vector>

#include "common.hpp"
#include "scores.hpp"
#include "profile.hpp"
#include "track_batch.hpp"

namespace bxmi {

static int64_t g_opt_wave_min_len = 8192;  // scores.wave_min_len: intervals of at least this many bases take a wave each
static int64_t g_opt_profile_chain = 0;    // scores.profile_chain: 0 = the ordered chain where it is needed, 1 = everywhere, -1 = nowhere (WRONG)

int scores_set_option(const char *key, int64_t value)
{
    if (!strcmp(key, "scores.wave_min_len")) {
        g_opt_wave_min_len = value < 0 ? 0 : value;
        return 1;
    }
    if (!strcmp(key, "scores.profile_chain")) {
        g_opt_profile_chain = value > 0 ? 1 : value < 0 ? -1 : 0;
        return 1;
    }
    return 0;
}

int64_t scores_get_wave_min_len() { return g_opt_wave_min_len; }
int64_t scores_get_profile_chain() { return g_opt_profile_chain; }

}  // namespace bxmi

using namespace bxmi;

struct bxmi_scores {
    int64_t size = 0;
    DevBuf values;
    DevBuf long_list;                            // int32[1 + n]: the intervals of the current batch left to the wave kernel
    DevBuf order, work;                          // int32[n]: the others ordered by length; the ordering's counters (scores.hpp)
    DevBuf q_start, q_end, q_value;              // staging of the host forms
    DevBuf r_count, r_sum, r_min, r_max;
    hipStream_t stream = nullptr;
};

static int scores_stream(bxmi_scores *h)
{
    if (!h->stream) BXMI_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    return BXMI_OK;
}

extern "C" int bxmi_scores_create(int64_t size, bxmi_scores_t **out)
{
    if (!out) return fail(BXMI_EINVAL, "bxmi_scores_create: out is NULL");
    *out = nullptr;
    if (size < 0 || size > 2147483647LL) return fail(BXMI_EINVAL, "bxmi_scores_create: size %lld outside [0, 2^31-1]", (long long)size);
    bxmi_scores *h = new (std::nothrow) bxmi_scores();
    if (!h) return fail(BXMI_ENOMEM, "bxmi_scores_create: host allocation failed");
    h->size = size;
    int rc = scores_stream(h);
    if (rc == BXMI_OK) rc = h->values.reserve((size_t)(size > 0 ? size : 1) * sizeof(float));
    if (rc == BXMI_OK && size > 0) {
        hipLaunchKernelGGL(sc_nan_kernel, dim3(stream_grid(size, SC_FILL_THREADS * 8)), dim3(SC_FILL_THREADS), 0, h->stream, h->values.as<float>(), size);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(BXMI_EHIP, "bxmi_scores_create: %s", hipGetErrorString(e));
    }
    if (rc != BXMI_OK) {
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return rc;
    }
    *out = h;
    return BXMI_OK;
}

extern "C" int bxmi_scores_destroy(bxmi_scores_t *h)
{
    if (!h) return BXMI_OK;
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return BXMI_OK;
}

extern "C" int bxmi_scores_info(const bxmi_scores_t *h, int64_t *size)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_scores_info: NULL handle");
    if (size) *size = h->size;
    return BXMI_OK;
}

extern "C" int bxmi_scores_values_dev(bxmi_scores_t *h, float **values_dev, int64_t *n)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_scores_values_dev: NULL handle");
    if (values_dev) *values_dev = h->values.as<float>();
    if (n) *n = h->size;
    return BXMI_OK;
}

static int scores_check_window(const bxmi_scores *h, int64_t offset, const void *p, int64_t n, const char *who)
{
    if (!h) return fail(BXMI_EINVAL, "%s: NULL handle", who);
    if (n < 0 || offset < 0 || offset > h->size || n > h->size - offset)
        return fail(BXMI_EINVAL, "%s: [%lld, %lld + %lld) outside the track [0, %lld)", who, (long long)offset, (long long)offset, (long long)n,
                    (long long)h->size);
    if (n > 0 && !p) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

extern "C" int bxmi_scores_write(bxmi_scores_t *h, int64_t offset, const float *values, int64_t n)
{
    BXMI_TRY(scores_check_window(h, offset, values, n, "bxmi_scores_write"));
    if (n) BXMI_HIP(hipMemcpy(h->values.as<float>() + offset, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return BXMI_OK;
}

extern "C" int bxmi_scores_read(bxmi_scores_t *h, int64_t offset, float *out, int64_t n)
{
    BXMI_TRY(scores_check_window(h, offset, out, n, "bxmi_scores_read"));
    if (n) BXMI_HIP(hipMemcpy(out, h->values.as<float>() + offset, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return BXMI_OK;
}

// "As if applied in order": the list is cut into maximal runs of ascending, disjoint spans (after clipping; spans clipped to
// nothing belong to any run), each run is one launch, the launches follow each other on one stream.  A wiggle file in
// position order is a single run; a list in descending order costs a launch per span.
extern "C" int bxmi_scores_set_spans(bxmi_scores_t *h, const int32_t *start, const int32_t *end, const float *value, int64_t n)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_scores_set_spans: NULL handle");
    if (n < 0 || (n > 0 && (!start || !end || !value))) return fail(BXMI_EINVAL, "bxmi_scores_set_spans: bad arguments");
    if (n == 0 || h->size == 0) return BXMI_OK;
    std::vector<int64_t> cuts;  // first span of every run
    cuts.push_back(0);
    int64_t reach = 0;          // end of the last non-empty span of the current run
    for (int64_t i = 0; i < n; i++) {
        const int64_t s = start[i] > 0 ? start[i] : 0, e = end[i] < h->size ? end[i] : h->size;
        if (s >= e) continue;
        if (s < reach) cuts.push_back(i);
        reach = e;
    }
    cuts.push_back(n);
    BXMI_TRY(scores_stream(h));
    BXMI_TRY(h->q_start.reserve((size_t)n * 4));
    BXMI_TRY(h->q_end.reserve((size_t)n * 4));
    BXMI_TRY(h->q_value.reserve((size_t)n * 4));
    BXMI_HIP(hipMemcpyAsync(h->q_start.p, start, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    BXMI_HIP(hipMemcpyAsync(h->q_end.p, end, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    BXMI_HIP(hipMemcpyAsync(h->q_value.p, value, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    for (size_t r = 0; r + 1 < cuts.size(); r++) {
        const int64_t a = cuts[r], m = cuts[r + 1] - a;
        if (m <= 0) continue;
        hipLaunchKernelGGL(sc_fill_kernel, dim3(stream_grid(m, SC_FILL_THREADS)), dim3(SC_FILL_THREADS), 0, h->stream, h->values.as<float>(), h->size,
                           h->q_start.as<int32_t>() + a, h->q_end.as<int32_t>() + a, h->q_value.as<float>() + a, m);
        BXMI_LAUNCH_CHECK();
    }
    BXMI_HIP(hipStreamSynchronize(h->stream));
    return BXMI_OK;
}

extern "C" int bxmi_scores_aggregate_dev(bxmi_scores_t *h, const bxmi_bits_t *mask_or_null, const int32_t *start, const int32_t *end, int64_t n,
                                         int32_t *count, float *sum, float *min, float *max, void *stream)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_scores_aggregate_dev: NULL handle");
    if (n < 0 || n > 2147483647LL) return fail(BXMI_EINVAL, "bxmi_scores_aggregate_dev: n = %lld outside [0, 2^31-1]", (long long)n);
    if (n == 0) return BXMI_OK;
    if (!start || !end || !count || !sum || !min || !max) return fail(BXMI_EINVAL, "bxmi_scores_aggregate_dev: NULL array");
    ScMask M{nullptr, 0, 0};
    if (mask_or_null) {
        uint64_t *words = nullptr;
        int32_t msize = 0;
        // (the view makes the mask allocate the bins it has not touched yet; its bits do not change)
        BXMI_TRY(bxmi_bits_words_dev(const_cast<bxmi_bits_t *>(mask_or_null), &words, &M.nwords));
        BXMI_TRY(bxmi_bits_info(mask_or_null, &msize, nullptr, nullptr));
        M.words = reinterpret_cast<const unsigned long long *>(words);
        M.size = msize;
    }
    hipStream_t st = as_stream(stream);
    BXMI_TRY(h->long_list.reserve((size_t)(n + 1) * sizeof(int32_t)));
    int32_t *long_list = h->long_list.as<int32_t>();
    BXMI_TRY(h->order.reserve((size_t)n * sizeof(int32_t)));
    BXMI_TRY(h->work.reserve(SC_WORK_INTS * sizeof(int32_t)));
    int32_t *order = h->order.as<int32_t>(), *work = h->work.as<int32_t>();
    BXMI_HIP(hipMemsetAsync(long_list, 0, sizeof(int32_t), st));
    BXMI_HIP(hipMemsetAsync(work, 0, SC_WORK_INTS * sizeof(int32_t), st));
    const float *values = h->values.as<float>();
    const int64_t wave_min_len = g_opt_wave_min_len;
    hipLaunchKernelGGL(sc_bucket_count_kernel, dim3(stream_grid(n, SC_ORD_THREADS * 4)), dim3(SC_ORD_THREADS), 0, st, start, end, n, h->size,
                       wave_min_len, work, long_list);
    BXMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sc_bucket_scan_kernel, dim3(1), dim3(SC_BUCKETS), 0, st, work);
    BXMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sc_bucket_scatter_kernel, dim3((unsigned)div_up(n, SC_ORD_THREADS * SC_ORD_ITEMS)), dim3(SC_ORD_THREADS), 0, st, start, end, n,
                       h->size, wave_min_len, work, order);
    BXMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sc_rows_kernel, dim3((unsigned)div_up(n, SC_ROWS)), dim3(SC_ROWS), 0, st, values, h->size, M, start, end, work, order, count, sum,
                       min, max);
    BXMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sc_wave_kernel, dim3(stream_grid(n, SC_WAVE_THREADS / 64)), dim3(SC_WAVE_THREADS), 0, st, values, h->size, M, start, end, count,
                       sum, min, max, long_list);
    BXMI_LAUNCH_CHECK();
    return BXMI_OK;
}

extern "C" int bxmi_scores_aggregate(bxmi_scores_t *h, const bxmi_bits_t *mask_or_null, const int32_t *start, const int32_t *end, int64_t n, int32_t *count,
                                     float *sum, float *min, float *max)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_scores_aggregate: NULL handle");
    if (n < 0 || n > 2147483647LL) return fail(BXMI_EINVAL, "bxmi_scores_aggregate: n = %lld outside [0, 2^31-1]", (long long)n);
    if (n == 0) return BXMI_OK;
    if (!start || !end || !count || !sum || !min || !max) return fail(BXMI_EINVAL, "bxmi_scores_aggregate: NULL array");
    BXMI_TRY(scores_stream(h));
    const size_t bytes = (size_t)n * 4;
    BXMI_TRY(h->q_start.reserve(bytes));
    BXMI_TRY(h->q_end.reserve(bytes));
    BXMI_TRY(h->r_count.reserve(bytes));
    BXMI_TRY(h->r_sum.reserve(bytes));
    BXMI_TRY(h->r_min.reserve(bytes));
    BXMI_TRY(h->r_max.reserve(bytes));
    BXMI_HIP(hipMemcpyAsync(h->q_start.p, start, bytes, hipMemcpyHostToDevice, h->stream));
    BXMI_HIP(hipMemcpyAsync(h->q_end.p, end, bytes, hipMemcpyHostToDevice, h->stream));
    BXMI_TRY(bxmi_scores_aggregate_dev(h, mask_or_null, h->q_start.as<int32_t>(), h->q_end.as<int32_t>(), n, h->r_count.as<int32_t>(),
                                       h->r_sum.as<float>(), h->r_min.as<float>(), h->r_max.as<float>(), h->stream));
    BXMI_HIP(hipMemcpyAsync(count, h->r_count.p, bytes, hipMemcpyDeviceToHost, h->stream));
    BXMI_HIP(hipMemcpyAsync(sum, h->r_sum.p, bytes, hipMemcpyDeviceToHost, h->stream));
    BXMI_HIP(hipMemcpyAsync(min, h->r_min.p, bytes, hipMemcpyDeviceToHost, h->stream));
    BXMI_HIP(hipMemcpyAsync(max, h->r_max.p, bytes, hipMemcpyDeviceToHost, h->stream));
    BXMI_HIP(hipStreamSynchronize(h->stream));
    return BXMI_OK;
}

// ---- site profiles (profile.hpp) ----------------------------------------------
// The scratch of the profile pass belongs to the library, not to a track (a call may name no track at all): one profile call
// at a time per process may be in flight.
namespace {
struct ProfileBufs {
    DevBuf table;                        // PfTrack[n_tracks + 1], the last one the spare entry
    DevBuf p_sum, p_abs, p_valid, p_q;   // [chunks][width]
    DevBuf col_flag, group_list;         // int32[width], int32[groups]
    DevBuf ctl;                          // 8 bytes chain_columns, 4 bytes listed groups, 4 bytes the spare entry's "track"
    DevBuf q_track, q_start, r_totals, r_valid;  // staging of the host form
};
LibraryScratch<ProfileBufs> &g_profile = LibraryScratch<ProfileBufs>::leaked();
}  // namespace

static int profile_check(const char *who, bxmi_scores_t *const *tracks, int32_t n_tracks, const void *track_of, const void *win_start, int64_t n,
                         int32_t width, const void *totals, const void *valid)
{
    BXMI_TRY(track_batch_check(who, "width", width, tracks, n_tracks, n));
    if (!totals || !valid || (n > 0 && (!track_of || !win_start))) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

static int profile_dev_locked(const char *who, bxmi_scores_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *win_start,
                              int64_t n, int32_t width, double *totals, int32_t *valid, int64_t *chain_columns_or_null, hipStream_t st)
{
    ProfileBufs &S = g_profile.bufs;
    BXMI_HIP(hipMemsetAsync(totals, 0, (size_t)width * sizeof(double), st));
    BXMI_HIP(hipMemsetAsync(valid, 0, (size_t)width * sizeof(int32_t), st));
    if (chain_columns_or_null) BXMI_HIP(hipMemsetAsync(chain_columns_or_null, 0, sizeof(int64_t), st));
    if (n == 0) return BXMI_OK;
    const int64_t groups = div_up(width, 64), chunks = div_up(n, PF_CHUNK), items = groups * chunks;
    const int64_t blocks = div_up(items, PF_THREADS / 64);
    if (blocks > 2147483647LL) return fail(BXMI_EINVAL, "%s: %lld windows of %d bases are more than one call takes", who, (long long)n, (int)width);
    const size_t cells = (size_t)chunks * (size_t)width;
    BXMI_TRY(S.p_sum.reserve(cells * sizeof(double)));
    BXMI_TRY(S.p_abs.reserve(cells * sizeof(double)));
    BXMI_TRY(S.p_valid.reserve(cells * sizeof(int32_t)));
    BXMI_TRY(S.p_q.reserve(cells * sizeof(int32_t)));
    BXMI_TRY(S.col_flag.reserve((size_t)width * sizeof(int32_t)));
    BXMI_TRY(S.group_list.reserve((size_t)groups * sizeof(int32_t)));
    BXMI_TRY(S.ctl.reserve(16));
    BXMI_HIP(hipMemsetAsync(S.ctl.p, 0, 16, st));
    unsigned long long *chain_columns = S.ctl.as<unsigned long long>();
    int32_t *n_listed = S.ctl.as<int32_t>() + 2;
    const PfTrack spare{reinterpret_cast<const float *>(S.ctl.as<int32_t>() + 3), 0};
    BXMI_TRY((fill_track_table<PfTrack, 16>(S.table, n_tracks, [&](int k) { return PfTrack{tracks[k]->values.as<float>(), tracks[k]->size}; }, spare, st)));
    const PfTrack *table = S.table.as<PfTrack>();
    hipLaunchKernelGGL(pf_partial_kernel, dim3((unsigned)blocks), dim3(PF_THREADS), 0, st, table, (int)n_tracks, track_of, win_start, n, (int64_t)width,
                       groups, items, S.p_sum.as<double>(), S.p_abs.as<double>(), S.p_valid.as<int32_t>(), S.p_q.as<int32_t>());
    BXMI_LAUNCH_CHECK();
    const int chain_mode = (int)g_opt_profile_chain;
    hipLaunchKernelGGL(pf_combine_kernel, dim3((unsigned)div_up(width, PF_THREADS)), dim3(PF_THREADS), 0, st, S.p_sum.as<double>(), S.p_abs.as<double>(),
                       S.p_valid.as<int32_t>(), S.p_q.as<int32_t>(), chunks, (int64_t)width, chain_mode, totals, valid, S.col_flag.as<int32_t>(),
                       S.group_list.as<int32_t>(), n_listed, chain_columns);
    BXMI_LAUNCH_CHECK();
    if (chain_mode >= 0) {
        hipLaunchKernelGGL(pf_chain_kernel, dim3((unsigned)groups), dim3(64), 0, st, table, (int)n_tracks, track_of, win_start, n, (int64_t)width,
                           S.col_flag.as<int32_t>(), S.group_list.as<int32_t>(), n_listed, totals);
        BXMI_LAUNCH_CHECK();
    }
    if (chain_columns_or_null) BXMI_HIP(hipMemcpyAsync(chain_columns_or_null, chain_columns, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return BXMI_OK;
}

extern "C" int bxmi_scores_profile_dev(bxmi_scores_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *win_start, int64_t n,
                                       int32_t width, double *totals, int32_t *valid, int64_t *chain_columns_or_null, void *stream)
{
    BXMI_TRY(profile_check("bxmi_scores_profile_dev", tracks, n_tracks, track_of, win_start, n, width, totals, valid));
    std::lock_guard<std::mutex> hold(g_profile.lock);
    BXMI_TRY(g_profile.enter());
    return profile_dev_locked("bxmi_scores_profile_dev", tracks, n_tracks, track_of, win_start, n, width, totals, valid, chain_columns_or_null,
                              as_stream(stream));
}

extern "C" int bxmi_scores_profile(bxmi_scores_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *win_start, int64_t n,
                                   int32_t width, double *totals, int32_t *valid, int64_t *chain_columns_or_null)
{
    const char *who = "bxmi_scores_profile";
    BXMI_TRY(profile_check(who, tracks, n_tracks, track_of, win_start, n, width, totals, valid));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    std::lock_guard<std::mutex> hold(g_profile.lock);
    BXMI_TRY(g_profile.enter(true));
    ProfileBufs &S = g_profile.bufs;
    const hipStream_t stream = g_profile.stream;
    const size_t rows = (size_t)(n > 0 ? n : 1) * sizeof(int32_t);
    BXMI_TRY(S.q_track.reserve(rows));
    BXMI_TRY(S.q_start.reserve(rows));
    BXMI_TRY(S.r_totals.reserve((size_t)width * sizeof(double) + sizeof(int64_t)));  // (the count of chain columns rides behind the totals)
    BXMI_TRY(S.r_valid.reserve((size_t)width * sizeof(int32_t)));
    if (n > 0) {
        BXMI_HIP(hipMemcpyAsync(S.q_track.p, track_of, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        BXMI_HIP(hipMemcpyAsync(S.q_start.p, win_start, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    int64_t *r_chain = reinterpret_cast<int64_t *>(S.r_totals.as<double>() + width);
    BXMI_TRY(profile_dev_locked(who, tracks, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), n, width, S.r_totals.as<double>(),
                                S.r_valid.as<int32_t>(), r_chain, stream));
    BXMI_HIP(hipMemcpyAsync(totals, S.r_totals.p, (size_t)width * sizeof(double), hipMemcpyDeviceToHost, stream));
    BXMI_HIP(hipMemcpyAsync(valid, S.r_valid.p, (size_t)width * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (chain_columns_or_null) BXMI_HIP(hipMemcpyAsync(chain_columns_or_null, r_chain, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    BXMI_HIP(hipStreamSynchronize(stream));
    return BXMI_OK;
}

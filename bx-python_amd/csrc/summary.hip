// summary.hip -- span tracks (bxmi_spans_*): one chromosome's bigWig items in HBM, in file order, their binned summaries over
// batches of regions (kernels and semantics: summary.hpp) and their per-base values over batches of rows (span_arrays.hpp); zoom
// tracks (bxmi_zoom_*): one chromosome's part of one zoom level and the same summaries answered from its records
// (zoom_summary.hpp); bed tracks (bxmi_beds_*): one chromosome's bigBed records and their coverage summaries (bed_summary.hpp).
//
// No floating-point contraction anywhere in this unit: the chains of summary.hpp round every product and every sum separately,
// as the reference's x86-64 build does (hipcc's default would fuse them into multiply-adds).  The pragma, not __dmul_rn /
// __dadd_rn, is what guarantees it: it covers every expression below, including the ones added later.
#pragma clang fp contract(off)

#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>

#include "common.hpp"
#include "summary.hpp"
#include "bed_summary.hpp"
#include "span_arrays.hpp"
#include "track_batch.hpp"
#include "zoom_summary.hpp"

using namespace bxmi;

// Every kind of handle names what its summaries run on: Entry (what the kernel reads for a track; entry() makes it, and an empty
// handle's entry() is the SPARE entry of the table), the kernel and its thread count.  The code below the creates is written once
// for all kinds and takes everything from the handle type.
struct bxmi_spans {
    using Entry = SmTrack;
    static constexpr auto kernel = sm_summary_kernel;
    static constexpr int THREADS = SM_THREADS;
    int64_t n = 0;
    int ordered = 1;
    DevBuf start, end, value;
    Entry entry() const { return SmTrack{start.as<int32_t>(), end.as<int32_t>(), value.as<float>(), n, ordered}; }
};

// One chromosome's part of one zoom level (zoom_summary.hpp): seven record arrays and three leaf arrays.
struct bxmi_zoom {
    using Entry = ZmTrack;
    static constexpr auto kernel = zm_summary_kernel;
    static constexpr int THREADS = ZM_THREADS;
    int64_t n = 0, n_leaves = 0;
    DevBuf start, end, valid, mn, mx, sum, sumsq, leaf_lo, leaf_hi, leaf_first;
    Entry entry() const
    {
        return ZmTrack{start.as<int32_t>(), end.as<int32_t>(), valid.as<uint32_t>(), mn.as<float>(), mx.as<float>(), sum.as<float>(), sumsq.as<float>(),
                       leaf_lo.as<int32_t>(), leaf_hi.as<int32_t>(), leaf_first.as<int64_t>(), n, n_leaves};
    }
};

// One chromosome's bigBed records (bed_summary.hpp): starts and ends in file order, and the two running maxima of the ends.
struct bxmi_beds {
    using Entry = BdTrack;
    static constexpr auto kernel = bd_summary_kernel;
    static constexpr int THREADS = BD_THREADS;
    int64_t n = 0;
    int sorted = 1;
    DevBuf start, end, reach, creach;
    Entry entry() const { return BdTrack{start.as<int32_t>(), end.as<int32_t>(), reach.as<int32_t>(), creach.as<int32_t>(), n, sorted}; }
};

// `what` ("item", "record", "region") i = [start[i], end[i]): none may have a negative coordinate
static int no_negative(const char *who, const char *what, const int32_t *start, const int32_t *end, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (start[i] < 0 || end[i] < 0)
            return fail(BXMI_EINVAL, "%s: %s %lld = [%d, %d) has a negative coordinate", who, what, (long long)i, (int)start[i], (int)end[i]);
    return BXMI_OK;
}

// A new handle's arrays: every buffer is reserved (never zero bytes) and filled from the host; the first failure ends it.
struct Upload {
    DevBuf *to;
    const void *from;
    size_t bytes;
};
static int upload(const char *who, std::initializer_list<Upload> copies)
{
    for (const Upload &c : copies) {
        BXMI_TRY(c.to->reserve(c.bytes ? c.bytes : 8));
        if (c.bytes == 0) continue;
        const hipError_t e = hipMemcpy(c.to->p, c.from, c.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(BXMI_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    return BXMI_OK;
}

extern "C" int bxmi_spans_create(const int32_t *start, const int32_t *end, const float *value, int64_t n, bxmi_spans_t **out)
{
    const char *who = "bxmi_spans_create";
    if (!out) return fail(BXMI_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (n < 0 || (n > 0 && (!start || !end || !value))) return fail(BXMI_EINVAL, "%s: bad arguments", who);
    BXMI_TRY(no_negative(who, "item", start, end, n));
    std::unique_ptr<bxmi_spans> h(new (std::nothrow) bxmi_spans());
    if (!h) return fail(BXMI_ENOMEM, "%s: host allocation failed", who);
    h->n = n;
    for (int64_t i = 1; i < n; i++)
        if (start[i] < start[i - 1] || end[i] < end[i - 1]) h->ordered = 0;
    const size_t bytes = (size_t)n * 4;
    BXMI_TRY(upload(who, {{&h->start, start, bytes}, {&h->end, end, bytes}, {&h->value, value, bytes}}));
    *out = h.release();
    return BXMI_OK;
}

extern "C" int bxmi_spans_destroy(bxmi_spans_t *h)
{
    delete h;
    return BXMI_OK;
}

extern "C" int bxmi_spans_info(const bxmi_spans_t *h, int64_t *n, int *ordered)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_spans_info: NULL handle");
    if (n) *n = h->n;
    if (ordered) *ordered = h->ordered;
    return BXMI_OK;
}

extern "C" int bxmi_zoom_create(const int32_t *start, const int32_t *end, const uint32_t *valid, const float *min, const float *max, const float *sum,
                                const float *sumsq, int64_t n, const int32_t *leaf_lo, const int32_t *leaf_hi, const int64_t *leaf_first,
                                int64_t n_leaves, bxmi_zoom_t **out)
{
    const char *who = "bxmi_zoom_create";
    if (!out) return fail(BXMI_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (n < 0 || n_leaves < 0 || !leaf_first || (n > 0 && (!start || !end || !valid || !min || !max || !sum || !sumsq)) ||
        (n_leaves > 0 && (!leaf_lo || !leaf_hi)))
        return fail(BXMI_EINVAL, "%s: bad arguments", who);
    BXMI_TRY(no_negative(who, "record", start, end, n));
    // an ORDERED level, and leaves that partition the records: what the kernel's searches and its indexes rest on
    for (int64_t i = 0; i < n; i++) {
        if (start[i] > end[i]) return fail(BXMI_EINVAL, "%s: record %lld = [%d, %d) has start > end", who, (long long)i, (int)start[i], (int)end[i]);
        if (i > 0 && start[i] < start[i - 1])
            return fail(BXMI_EINVAL, "%s: record starts are not non-decreasing (record %lld: %d after %d)", who, (long long)i, (int)start[i], (int)start[i - 1]);
        if (i > 0 && end[i] < end[i - 1])
            return fail(BXMI_EINVAL, "%s: record ends are not non-decreasing (record %lld: %d after %d)", who, (long long)i, (int)end[i], (int)end[i - 1]);
    }
    if (leaf_first[0] != 0 || leaf_first[n_leaves] != n)
        return fail(BXMI_EINVAL, "%s: leaf_first runs from %lld to %lld, not from 0 to n = %lld", who, (long long)leaf_first[0], (long long)leaf_first[n_leaves],
                    (long long)n);
    for (int64_t k = 0; k < n_leaves; k++) {
        if (leaf_first[k + 1] < leaf_first[k]) return fail(BXMI_EINVAL, "%s: leaf_first is not non-decreasing at leaf %lld", who, (long long)k);
        if (leaf_lo[k] < -1 || leaf_hi[k] < 0)
            return fail(BXMI_EINVAL, "%s: leaf %lld = (%d, %d) has a negative coordinate", who, (long long)k, (int)leaf_lo[k], (int)leaf_hi[k]);
        if (k > 0 && leaf_lo[k] < leaf_lo[k - 1])
            return fail(BXMI_EINVAL, "%s: leaf_lo is not non-decreasing (leaf %lld: %d after %d)", who, (long long)k, (int)leaf_lo[k], (int)leaf_lo[k - 1]);
        if (k > 0 && leaf_hi[k] < leaf_hi[k - 1])
            return fail(BXMI_EINVAL, "%s: leaf_hi is not non-decreasing (leaf %lld: %d after %d)", who, (long long)k, (int)leaf_hi[k], (int)leaf_hi[k - 1]);
    }
    std::unique_ptr<bxmi_zoom> h(new (std::nothrow) bxmi_zoom());
    if (!h) return fail(BXMI_ENOMEM, "%s: host allocation failed", who);
    h->n = n;
    h->n_leaves = n_leaves;
    const size_t rec = (size_t)n * 4, leaf = (size_t)n_leaves * 4;
    BXMI_TRY(upload(who, {{&h->start, start, rec}, {&h->end, end, rec}, {&h->valid, valid, rec}, {&h->mn, min, rec}, {&h->mx, max, rec},
                          {&h->sum, sum, rec}, {&h->sumsq, sumsq, rec}, {&h->leaf_lo, leaf_lo, leaf}, {&h->leaf_hi, leaf_hi, leaf},
                          {&h->leaf_first, leaf_first, (size_t)(n_leaves + 1) * 8}}));
    *out = h.release();
    return BXMI_OK;
}

extern "C" int bxmi_zoom_destroy(bxmi_zoom_t *h)
{
    delete h;
    return BXMI_OK;
}

extern "C" int bxmi_zoom_info(const bxmi_zoom_t *h, int64_t *n, int64_t *n_leaves)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_zoom_info: NULL handle");
    if (n) *n = h->n;
    if (n_leaves) *n_leaves = h->n_leaves;
    return BXMI_OK;
}

extern "C" int bxmi_beds_create(const int32_t *start, const int32_t *end, int64_t n, bxmi_beds_t **out)
{
    const char *who = "bxmi_beds_create";
    if (!out) return fail(BXMI_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (n < 0 || (n > 0 && (!start || !end))) return fail(BXMI_EINVAL, "%s: bad arguments", who);
    BXMI_TRY(no_negative(who, "record", start, end, n));
    std::unique_ptr<int32_t[]> reach(new (std::nothrow) int32_t[(size_t)(n > 0 ? 2 * n : 1)]);
    std::unique_ptr<bxmi_beds> h(new (std::nothrow) bxmi_beds());
    if (!h || !reach) return fail(BXMI_ENOMEM, "%s: host allocation failed", who);
    h->n = n;
    h->sorted = bd_build_reach(start, end, n, reach.get(), reach.get() + n);
    const size_t bytes = (size_t)n * 4;
    BXMI_TRY(upload(who, {{&h->start, start, bytes}, {&h->end, end, bytes}, {&h->reach, reach.get(), bytes}, {&h->creach, reach.get() + n, bytes}}));
    *out = h.release();
    return BXMI_OK;
}

extern "C" int bxmi_beds_destroy(bxmi_beds_t *h)
{
    delete h;
    return BXMI_OK;
}

extern "C" int bxmi_beds_info(const bxmi_beds_t *h, int64_t *n, int *sorted)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_beds_info: NULL handle");
    if (n) *n = h->n;
    if (sorted) *sorted = h->sorted;
    return BXMI_OK;
}

// The track table and the staging of the host form belong to the library, not to a track (a call may name no track at all): one
// summary call at a time per process may be in flight.
namespace {
constexpr int64_t SM_SLAB_CELLS = 1 << 23;  // the host form goes through the device in slabs of about this many (row, bin) cells

struct SummaryBufs {
    DevBuf table;                      // SmTrack, ZmTrack or BdTrack [n_tracks + 1] (the call's kind), the last one the spare entry
    DevBuf q_track, q_start, q_end;    // staging of the host form
    DevBuf r[5];
};
LibraryScratch<SummaryBufs> &g_summary = LibraryScratch<SummaryBufs>::leaked();

struct Planes {  // the five outputs of a summary, in the order of include/bxmi.h
    double *p[5];
};
}  // namespace

template <typename Handle>
static int summary_check(const char *who, Handle *const *tracks, int32_t n_tracks, const void *track_of, const void *start, const void *end,
                         int64_t n, int32_t size, const Planes &out)
{
    BXMI_TRY(track_batch_check(who, "size", size, tracks, n_tracks, n));
    if (n > 0) {
        if (!track_of || !start || !end) return fail(BXMI_EINVAL, "%s: NULL array", who);
        for (int k = 0; k < 5; k++)
            if (!out.p[k]) return fail(BXMI_EINVAL, "%s: NULL output array", who);
    }
    return BXMI_OK;
}

// S.table for this call's tracks, 8 per launch; the spare entry (an empty handle's) has no items
template <typename Handle>
static int summary_fill_table(SummaryBufs &S, Handle *const *tracks, int32_t n_tracks, hipStream_t st)
{
    return fill_track_table<typename Handle::Entry, 8>(S.table, n_tracks, [&](int k) { return tracks[k]->entry(); }, Handle().entry(), st);
}

// Handle: the kind of track S.table was filled for
template <typename Handle>
static int summary_launch(SummaryBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end, int64_t n,
                          int32_t size, const Planes &out, hipStream_t st)
{
    constexpr int64_t ROWS_PER_LAUNCH = 1 << 25;  // (a grid's threads are counted in 32 bits: 2^25 workgroups of 64)
    for (int64_t first = 0; first < n; first += ROWS_PER_LAUNCH) {
        const int64_t m = n - first < ROWS_PER_LAUNCH ? n - first : ROWS_PER_LAUNCH, cell = first * (int64_t)size;
        hipLaunchKernelGGL(Handle::kernel, dim3((unsigned)m), dim3(Handle::THREADS), 0, st, S.table.as<typename Handle::Entry>(), (int)n_tracks,
                           track_of + first, start + first, end + first, (int)size, out.p[0] + cell, out.p[1] + cell, out.p[2] + cell, out.p[3] + cell,
                           out.p[4] + cell);
        BXMI_LAUNCH_CHECK();
    }
    return BXMI_OK;
}

// The device form of every kind of track.
template <typename Handle>
static int summarize_dev(const char *who, Handle *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                         int64_t n, int32_t size, const Planes &out, void *stream)
{
    BXMI_TRY(summary_check(who, tracks, n_tracks, track_of, start, end, n, size, out));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_summary.lock);
    BXMI_TRY(g_summary.enter());
    BXMI_TRY(summary_fill_table(g_summary.bufs, tracks, n_tracks, as_stream(stream)));
    return summary_launch<Handle>(g_summary.bufs, n_tracks, track_of, start, end, n, size, out, as_stream(stream));
}

// The host form of every kind: through the device in slabs.
template <typename Handle>
static int summarize_host(const char *who, Handle *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                          int64_t n, int32_t size, const Planes &out)
{
    BXMI_TRY(summary_check(who, tracks, n_tracks, track_of, start, end, n, size, out));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(no_negative(who, "region", start, end, n));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_summary.lock);
    BXMI_TRY(g_summary.enter(true));
    SummaryBufs &S = g_summary.bufs;
    const hipStream_t st = g_summary.stream;
    int64_t slab = SM_SLAB_CELLS / size;  // rows per slab
    if (slab < 1) slab = 1;
    if (slab > n) slab = n;
    const size_t rows = (size_t)slab * sizeof(int32_t), cells = (size_t)slab * (size_t)size * sizeof(double);
    BXMI_TRY(S.q_track.reserve(rows));
    BXMI_TRY(S.q_start.reserve(rows));
    BXMI_TRY(S.q_end.reserve(rows));
    Planes dev_out;
    for (int k = 0; k < 5; k++) {
        BXMI_TRY(S.r[k].reserve(cells));
        dev_out.p[k] = S.r[k].as<double>();
    }
    BXMI_TRY(summary_fill_table(S, tracks, n_tracks, st));
    for (int64_t first = 0; first < n; first += slab) {
        const int64_t m = n - first < slab ? n - first : slab;
        const size_t in_bytes = (size_t)m * sizeof(int32_t), out_bytes = (size_t)m * (size_t)size * sizeof(double);
        BXMI_HIP(hipMemcpyAsync(S.q_track.p, track_of + first, in_bytes, hipMemcpyHostToDevice, st));
        BXMI_HIP(hipMemcpyAsync(S.q_start.p, start + first, in_bytes, hipMemcpyHostToDevice, st));
        BXMI_HIP(hipMemcpyAsync(S.q_end.p, end + first, in_bytes, hipMemcpyHostToDevice, st));
        BXMI_TRY(summary_launch<Handle>(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), S.q_end.as<int32_t>(), m, size, dev_out, st));
        for (int k = 0; k < 5; k++)
            BXMI_HIP(hipMemcpyAsync(out.p[k] + first * (int64_t)size, dev_out.p[k], out_bytes, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));  // the staging is reused by the next slab
    }
    return BXMI_OK;
}

extern "C" int bxmi_spans_summarize_dev(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                        const int32_t *end, int64_t n, int32_t size, double *valid, double *min, double *max, double *sum,
                                        double *sumsq, void *stream)
{
    return summarize_dev("bxmi_spans_summarize_dev", tracks, n_tracks, track_of, start, end, n, size, {{valid, min, max, sum, sumsq}}, stream);
}

extern "C" int bxmi_spans_summarize(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                                    int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq)
{
    return summarize_host("bxmi_spans_summarize", tracks, n_tracks, track_of, start, end, n, size, {{valid, min, max, sum, sumsq}});
}

extern "C" int bxmi_zoom_summarize_dev(bxmi_zoom_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                       const int32_t *end, int64_t n, int32_t size, double *valid, double *min, double *max, double *sum,
                                       double *sumsq, void *stream)
{
    return summarize_dev("bxmi_zoom_summarize_dev", tracks, n_tracks, track_of, start, end, n, size, {{valid, min, max, sum, sumsq}}, stream);
}

extern "C" int bxmi_zoom_summarize(bxmi_zoom_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                                   int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq)
{
    return summarize_host("bxmi_zoom_summarize", tracks, n_tracks, track_of, start, end, n, size, {{valid, min, max, sum, sumsq}});
}

extern "C" int bxmi_beds_summarize_dev(bxmi_beds_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                       const int32_t *end, int64_t n, int32_t size, double *valid, double *min, double *max, double *sum,
                                       double *sumsq, void *stream)
{
    return summarize_dev("bxmi_beds_summarize_dev", tracks, n_tracks, track_of, start, end, n, size, {{valid, min, max, sum, sumsq}}, stream);
}

extern "C" int bxmi_beds_summarize(bxmi_beds_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                                   int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq)
{
    return summarize_host("bxmi_beds_summarize", tracks, n_tracks, track_of, start, end, n, size, {{valid, min, max, sum, sumsq}});
}

// ---- per-base arrays (span_arrays.hpp): BigWigFile.get_as_array for a batch of rows ----
namespace {
constexpr int64_t SA_SLAB = (int64_t)SA_TILE << 14;      // output elements per slab of the host form (64 MiB), whole tiles
constexpr int64_t SA_TILES_PER_LAUNCH = 1 << 22;         // (a grid's threads are counted in 32 bits: 2^22 workgroups of 256)
}  // namespace

// what both forms check; `row_off` is only tested for being there
static int arrays_check(const char *who, bxmi_spans_t *const *tracks, int32_t n_tracks, const void *track_of, const void *start, int64_t n,
                        int32_t width, const void *row_off, int64_t total, const void *out)
{
    if (!row_off) {
        BXMI_TRY(track_batch_check(who, "width", width, tracks, n_tracks, n));
        if (total != n * (int64_t)width)
            return fail(BXMI_EINVAL, "%s: total = %lld, but n * width = %lld", who, (long long)total, (long long)(n * (int64_t)width));
    } else {
        if (width != 0) return fail(BXMI_EINVAL, "%s: width = %d with row offsets, must be 0", who, (int)width);
        BXMI_TRY(track_batch_check(who, "width", 1, tracks, n_tracks, n));
        if (total < 0) return fail(BXMI_EINVAL, "%s: total = %lld is negative", who, (long long)total);
    }
    if ((n > 0 && (!track_of || !start)) || (n > 0 && total > 0 && !out)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

// output elements [o_first, o_first + count) of rows [row_base, row_base + n_rows); `out` is element o_first's address
static int arrays_launch(SummaryBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n_rows, int64_t row_base,
                         int32_t width, const int64_t *row_off, int64_t o_first, int64_t count, float *out, hipStream_t st)
{
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;  // else the kernel stores element by element
    constexpr int64_t PER_LAUNCH = SA_TILES_PER_LAUNCH * SA_TILE;
    for (int64_t done = 0; done < count; done += PER_LAUNCH) {
        const int64_t m = count - done < PER_LAUNCH ? count - done : PER_LAUNCH;
        hipLaunchKernelGGL(sa_arrays_kernel, dim3((unsigned)div_up(m, SA_TILE)), dim3(SA_THREADS), 0, st, S.table.as<SmTrack>(), (int)n_tracks,
                           track_of, start, n_rows, row_base, (int)width, row_off, o_first + done, m, out + done, vec);
        BXMI_LAUNCH_CHECK();
    }
    return BXMI_OK;
}

extern "C" int bxmi_spans_arrays_dev(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                     int32_t width, const int64_t *row_off_or_null, int64_t total, float *out, void *stream)
{
    const char *who = "bxmi_spans_arrays_dev";
    BXMI_TRY(arrays_check(who, tracks, n_tracks, track_of, start, n, width, row_off_or_null, total, out));
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_summary.lock);
    BXMI_TRY(g_summary.enter());
    BXMI_TRY(summary_fill_table(g_summary.bufs, tracks, n_tracks, as_stream(stream)));
    return arrays_launch(g_summary.bufs, n_tracks, track_of, start, n, 0, width, row_off_or_null, 0, total, out, as_stream(stream));
}

extern "C" int bxmi_spans_arrays(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                 int32_t width, const int64_t *row_off_or_null, int64_t total, float *out)
{
    const char *who = "bxmi_spans_arrays";
    const int64_t *row_off = row_off_or_null;
    BXMI_TRY(arrays_check(who, tracks, n_tracks, track_of, start, n, width, row_off, total, out));
    if (row_off) {
        if (row_off[0] != 0) return fail(BXMI_EINVAL, "%s: row_off[0] = %lld, must be 0", who, (long long)row_off[0]);
        for (int64_t i = 0; i < n; i++) {
            if (row_off[i + 1] < row_off[i]) return fail(BXMI_EINVAL, "%s: row_off descends at row %lld", who, (long long)i);
            if (row_off[i + 1] - row_off[i] > 2147483647LL)
                return fail(BXMI_EINVAL, "%s: row %lld has %lld elements, more than 2^31-1", who, (long long)i, (long long)(row_off[i + 1] - row_off[i]));
        }
        if (row_off[n] != total)
            return fail(BXMI_EINVAL, "%s: row_off[n] = %lld, but total = %lld", who, (long long)row_off[n], (long long)total);
    }
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_summary.lock);
    BXMI_TRY(g_summary.enter(true));
    SummaryBufs &S = g_summary.bufs;
    const hipStream_t st = g_summary.stream;
    BXMI_TRY(summary_fill_table(S, tracks, n_tracks, st));
    for (int64_t o0 = 0; o0 < total; o0 += SA_SLAB) {  // slabs of whole tiles; a row may lie in several
        const int64_t count = total - o0 < SA_SLAB ? total - o0 : SA_SLAB;
        const SaRows rows = sa_rows_of(row_off, n, width, o0, count);  // the slab's rows
        const int64_t r0 = rows.r0, m = rows.m;
        const size_t in_bytes = (size_t)m * sizeof(int32_t), off_bytes = (size_t)(m + 1) * sizeof(int64_t), out_bytes = (size_t)count * sizeof(float);
        BXMI_TRY(S.q_track.reserve(in_bytes));
        BXMI_TRY(S.q_start.reserve(in_bytes));
        BXMI_TRY(S.r[0].reserve(out_bytes));
        BXMI_HIP(hipMemcpyAsync(S.q_track.p, track_of + r0, in_bytes, hipMemcpyHostToDevice, st));
        BXMI_HIP(hipMemcpyAsync(S.q_start.p, start + r0, in_bytes, hipMemcpyHostToDevice, st));
        if (row_off) {  // (q_end holds the slab's offsets)
            BXMI_TRY(S.q_end.reserve(off_bytes));
            BXMI_HIP(hipMemcpyAsync(S.q_end.p, row_off + r0, off_bytes, hipMemcpyHostToDevice, st));
        }
        BXMI_TRY(arrays_launch(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), m, r0, width, row_off ? S.q_end.as<int64_t>() : nullptr, o0,
                               count, S.r[0].as<float>(), st));
        BXMI_HIP(hipMemcpyAsync(out + o0, S.r[0].p, out_bytes, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));  // the staging is reused by the next slab
    }
    return BXMI_OK;
}

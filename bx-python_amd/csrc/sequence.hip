// sequence.hip -- 2bit tracks (bxmi_twobit_*): one sequence of a .2bit file in HBM -- its packed bytes, its N blocks and its mask
// blocks -- the letters under batches of rows (bxmi_twobit_bases*) and their base counts (bxmi_twobit_composition*).  Kernels and
// semantics: twobit.hpp.  The argument checks, the track table and the staging are track_batch.hpp's, as in summary.hip; the scratch
// is this unit's own, so these calls do not share the one-call-at-a-time rule with the summaries, only with each other.
// Position weight matrices scored over those rows (bxmi_pwm_*, bxmi_twobit_pwm_*): kernels and semantics in pwm.hpp, those of the
// thresholded hits (bxmi_twobit_pwm_hits*) in pwm_hits.hpp; they use the same table and scratch and so the same rule.
// The k-mer spectrum of those rows (bxmi_twobit_kmer_counts*): kernel and semantics in kmer.hpp; the same table, scratch and rule.
// Strand (bxmi_twobit_bases_strand*, bxmi_twobit_composition_strand*, bxmi_twobit_kmer_counts_strand*, bxmi_twobit_pwm_scores_strand*,
// bxmi_twobit_pwm_best_strand*, bxmi_twobit_pwm_hits_strand*): the unstranded entry points are the stranded ones with a NULL strand,
// which launch the kernels they always launched; a strand array launches the *_strand_kernel of twobit.hpp, kmer.hpp, pwm.hpp and
// pwm_hits.hpp.  The host forms check the entries (0 or 1) and slice the array with the rows of every slab (the best hits and the
// thresholded hits send the rows, and so the strands, whole).
// Tracks from letters (bxmi_twobit_create_letters, _create_letters_dev, _create_nib): kernels and semantics in twobit_build.hpp; they
// fill the buffers bxmi_twobit_create fills from a file's arrays and end with the same twobit_finish.  Their scratch is the call's own.
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "common.hpp"
#include "primitives.hpp"
// twobit.hpp takes sm_first_above, sa_row_of and sa_rows_of from summary.hpp and span_arrays.hpp, which also DEFINE their kernels
// wherever they are included.  summary.hip owns those; the copies this unit cannot avoid take other names and are never launched.
#define sm_summary_kernel sm_summary_kernel_unused_in_sequence
#define sa_arrays_kernel sa_arrays_kernel_unused_in_sequence
#include "summary.hpp"
#include "span_arrays.hpp"
#undef sm_summary_kernel
#undef sa_arrays_kernel
#include "twobit.hpp"
#include "twobit_build.hpp"
#include "pwm.hpp"
#include "pwm_hits.hpp"
#include "kmer.hpp"
#include "track_batch.hpp"

using namespace bxmi;

struct bxmi_twobit {
    int64_t size = 0, n_blocks = 0, m_blocks = 0;
    DevBuf packed, n_start, n_end, m_start, m_end, ckpt, n_cum, n_codes, m_cum;
    TbTrack entry() const
    {
        return TbTrack{packed.as<uint32_t>(), n_start.as<int32_t>(), n_end.as<int32_t>(), m_start.as<int32_t>(), m_end.as<int32_t>(), ckpt.as<int32_t>(),
                       n_cum.as<int32_t>(), n_codes.as<int32_t>(), m_cum.as<int32_t>(), size, n_blocks, m_blocks};
    }
};

namespace {
constexpr int64_t TB_SLAB = (int64_t)TB_TILE << 14;   // output bytes per slab of the host form (64 MiB), whole tiles
constexpr int64_t TB_TILES_PER_LAUNCH = 1 << 22;      // (a grid's threads are counted in 32 bits: 2^22 workgroups of 256)
constexpr int64_t TB_ROWS_PER_LAUNCH = 1 << 25;       // (2^25 workgroups of 64)
constexpr int64_t TB_COMP_SLAB = 1 << 22;             // rows per slab of the host form of the composition
constexpr int64_t PW_SLAB = (int64_t)PW_TILE << 12;   // output elements of ALL planes per slab of the host form of the scores (16 MiB): whole tiles per plane
constexpr int64_t PW_TILES_PER_LAUNCH = 1 << 22;      // (2^22 workgroups of 256)
constexpr int64_t PW_OUT_MAX = INT64_MAX / 8;         // elements of all planes: their byte offsets stay far inside int64
constexpr int64_t KM_SLAB_CELLS = 1 << 24;            // counters per slab of rows of the host form of the k-mer counts (64 MiB); at least one row
constexpr int64_t KM_OUT_MAX = INT64_MAX / 8;         // counters of all rows: their byte offsets stay far inside int64

struct SequenceBufs {
    DevBuf table;                         // TbTrack [n_tracks + 1], the last one the spare entry
    DevBuf q_track, q_start, q_end, r;    // staging of the host forms
    DevBuf q_strand;                      // int8 [rows of a slab] of the stranded host forms
    DevBuf keys;                          // uint64 [n_mats][n] of the best hits
    DevBuf hit_counts, hit_bases, hit_scan;  // of the thresholded hits: int32 [n_mats][tiles], int64 bases of them + total + heads, the scan's sums
};
LibraryScratch<SequenceBufs> &g_sequence = LibraryScratch<SequenceBufs>::leaked();

// `what` blocks [start[i], start[i] + size[i]): sorted, non-empty, disjoint, inside [0, size] -> ends[] and the running sizes cum[]
int check_blocks(const char *who, const char *what, const int32_t *start, const int32_t *sizes, int64_t blocks, int64_t size, std::vector<int32_t> &ends,
                 std::vector<int32_t> &cum)
{
    ends.resize((size_t)blocks);
    cum.assign((size_t)blocks + 1, 0);
    int64_t prev_end = 0;
    for (int64_t i = 0; i < blocks; i++) {
        const int64_t s = start[i], e = s + (int64_t)sizes[i];
        if (sizes[i] < 1) return fail(BXMI_EINVAL, "%s: %s block %lld at %lld is empty (size %d)", who, what, (long long)i, (long long)s, (int)sizes[i]);
        if (s < 0 || e > size)
            return fail(BXMI_EINVAL, "%s: %s block %lld = [%lld, %lld) is outside [0, size = %lld]", who, what, (long long)i, (long long)s, (long long)e,
                        (long long)size);
        if (i > 0 && s < prev_end)
            return fail(BXMI_EINVAL, "%s: %s blocks are not sorted and disjoint (block %lld starts at %lld, the one before ends at %lld)", who, what,
                        (long long)i, (long long)s, (long long)prev_end);
        prev_end = e;
        ends[(size_t)i] = (int32_t)e;
        cum[(size_t)i + 1] = cum[(size_t)i] + sizes[i];
    }
    return BXMI_OK;
}

int put(DevBuf &to, const void *from, size_t bytes)
{
    BXMI_TRY(to.reserve(bytes ? bytes : 8));
    if (bytes) BXMI_HIP(hipMemcpy(to.p, from, bytes, hipMemcpyHostToDevice));
    return BXMI_OK;
}

// table = the running totals, one 16-byte entry each, of planes[4][stride] (counts per item in [0, items), scanned in place into
// [1, items]; entry 0 is zero): items + 1 entries
int running_codes(DevBuf &planes, int64_t items, DevBuf &table, DevBuf &scratch, hipStream_t st)
{
    const int64_t stride = items + 1;
    int32_t *p = planes.as<int32_t>();
    for (int c = 0; c < 4; c++)  // the counts sit at [1, items] of every plane, a zero before them
        BXMI_TRY((device_scan<int32_t, int32_t, OpSum, true>(p + c * stride, p + c * stride, stride, 0, nullptr, scratch, st)));
    BXMI_TRY(table.reserve((size_t)stride * 16));
    hipLaunchKernelGGL(tb_interleave_kernel, dim3((unsigned)div_up(stride, TB_THREADS)), dim3(TB_THREADS), 0, st, p, stride, stride, table.as<int32_t>());
    BXMI_LAUNCH_CHECK();
    return BXMI_OK;
}
}  // namespace

// What every builder of a track ends with, its nine buffers but ckpt and n_codes filled: the checkpoints, then the counts under the
// N blocks from them.  Queued on st and waited for.
static int twobit_finish(bxmi_twobit &t, hipStream_t st)
{
    const int64_t size = t.size, n_blocks = t.n_blocks, ckpts = div_up(size, TB_CKPT);
    DevBuf planes, scratch;
    const int64_t most = ckpts > n_blocks ? ckpts : n_blocks;
    BXMI_TRY(planes.reserve((size_t)(most + 1) * 16));
    BXMI_HIP(hipMemsetAsync(planes.p, 0, (size_t)(ckpts + 1) * 16, st));
    if (ckpts > 0) {
        hipLaunchKernelGGL(tb_count_kernel, dim3((unsigned)ckpts), dim3(TB_WAVE), 0, st, t.packed.as<uint32_t>(), size, ckpts + 1, planes.as<int32_t>() + 1);
        BXMI_LAUNCH_CHECK();
    }
    BXMI_TRY(running_codes(planes, ckpts, t.ckpt, scratch, st));
    BXMI_HIP(hipMemsetAsync(planes.p, 0, (size_t)(n_blocks + 1) * 16, st));
    for (int64_t first = 0; first < n_blocks; first += TB_ROWS_PER_LAUNCH) {  // (one wave per block: a grid's threads are counted in 32 bits)
        const int64_t m = n_blocks - first < TB_ROWS_PER_LAUNCH ? n_blocks - first : TB_ROWS_PER_LAUNCH;
        hipLaunchKernelGGL(tb_under_kernel, dim3((unsigned)m), dim3(TB_WAVE), 0, st, t.packed.as<uint32_t>(), t.ckpt.as<int32_t>(),
                           t.n_start.as<int32_t>() + first, t.n_end.as<int32_t>() + first, n_blocks + 1, planes.as<int32_t>() + 1 + first);
        BXMI_LAUNCH_CHECK();
    }
    BXMI_TRY(running_codes(planes, n_blocks, t.n_codes, scratch, st));
    BXMI_HIP(hipStreamSynchronize(st));  // (planes and scratch go away)
    return BXMI_OK;
}

// the bytes of `packed` on the device: whole checkpoint blocks, which the kernels read as aligned words
static size_t packed_room(int64_t size)
{
    const int64_t ckpts = div_up(size, TB_CKPT);
    return (size_t)(ckpts > 0 ? ckpts : 1) * (TB_CKPT / 4);
}

extern "C" int bxmi_twobit_create(const uint8_t *packed, int64_t size, const int32_t *n_start, const int32_t *n_size, int64_t n_blocks,
                                  const int32_t *m_start, const int32_t *m_size, int64_t m_blocks, bxmi_twobit_t **out)
{
    const char *who = "bxmi_twobit_create";
    if (!out) return fail(BXMI_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (size < 0 || size > TB_SIZE_MAX) return fail(BXMI_EINVAL, "%s: size = %lld outside [0, 2^31-1]", who, (long long)size);
    if (n_blocks < 0 || m_blocks < 0 || (size > 0 && !packed) || (n_blocks > 0 && (!n_start || !n_size)) || (m_blocks > 0 && (!m_start || !m_size)))
        return fail(BXMI_EINVAL, "%s: bad arguments", who);
    std::vector<int32_t> n_end, n_cum, m_end, m_cum;
    BXMI_TRY(check_blocks(who, "N", n_start, n_size, n_blocks, size, n_end, n_cum));
    BXMI_TRY(check_blocks(who, "mask", m_start, m_size, m_blocks, size, m_end, m_cum));
    std::unique_ptr<bxmi_twobit> h(new (std::nothrow) bxmi_twobit());
    if (!h) return fail(BXMI_ENOMEM, "%s: host allocation failed", who);
    h->size = size;
    h->n_blocks = n_blocks;
    h->m_blocks = m_blocks;
    // the packed bytes, zero-filled to whole checkpoint blocks: the kernels read aligned words
    const size_t bytes = (size_t)((size + 3) / 4), room = packed_room(size);
    BXMI_TRY(h->packed.reserve(room));
    BXMI_HIP(hipMemset(h->packed.p, 0, room));
    if (bytes) BXMI_HIP(hipMemcpy(h->packed.p, packed, bytes, hipMemcpyHostToDevice));
    BXMI_TRY(put(h->n_start, n_start, (size_t)n_blocks * 4));
    BXMI_TRY(put(h->n_end, n_end.data(), (size_t)n_blocks * 4));
    BXMI_TRY(put(h->n_cum, n_cum.data(), (size_t)(n_blocks + 1) * 4));
    BXMI_TRY(put(h->m_start, m_start, (size_t)m_blocks * 4));
    BXMI_TRY(put(h->m_end, m_end.data(), (size_t)m_blocks * 4));
    BXMI_TRY(put(h->m_cum, m_cum.data(), (size_t)(m_blocks + 1) * 4));
    BXMI_TRY(twobit_finish(*h, nullptr));
    *out = h.release();
    return BXMI_OK;
}

// ---- a track from its letters (bl_build_kernel of twobit_build.hpp) ----
static int build_check(const char *who, const void *in, int64_t size, int32_t other, bxmi_twobit_t **out)
{
    if (!out) return fail(BXMI_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (other != BXMI_TB_OTHER_REFUSE && other != BXMI_TB_OTHER_N)
        return fail(BXMI_EINVAL, "%s: other = %d is neither BXMI_TB_OTHER_REFUSE (0) nor BXMI_TB_OTHER_N (1)", who, (int)other);
    if (size < 0 || size > TB_SIZE_MAX) return fail(BXMI_EINVAL, "%s: size = %lld outside [0, 2^31-1]", who, (long long)size);
    if (size > 0 && !in) return fail(BXMI_EINVAL, "%s: NULL input with size = %lld", who, (long long)size);
    return BXMI_OK;
}

// running sizes cum[blocks + 1] of the blocks [start[i], end[i])
static int build_running_sizes(const DevBuf &start, const DevBuf &end, int64_t blocks, DevBuf &cum, DevBuf &scratch, hipStream_t st)
{
    BXMI_TRY(cum.reserve((size_t)(blocks + 1) * 4));
    hipLaunchKernelGGL(bl_sizes_kernel, dim3((unsigned)div_up(blocks + 1, BL_THREADS)), dim3(BL_THREADS), 0, st, start.as<int32_t>(), end.as<int32_t>(), blocks,
                       cum.as<int32_t>());
    BXMI_LAUNCH_CHECK();
    return device_scan<int32_t, int32_t, OpSum, true>(cum.as<int32_t>(), cum.as<int32_t>(), blocks + 1, 0, nullptr, scratch, st);
}

// d_src: the symbols ON THE DEVICE (size bytes; (size + 1) / 2 of a nib).  Everything is queued on st; one synchronisation reads the
// two block counts and the lowest other symbol, the last one is twobit_finish's.
template <int SRC>
static int build_track(const char *who, const uint8_t *d_src, int64_t size, int32_t other, bxmi_twobit_t **out, hipStream_t st)
{
    std::unique_ptr<bxmi_twobit> h(new (std::nothrow) bxmi_twobit());
    if (!h) return fail(BXMI_ENOMEM, "%s: host allocation failed", who);
    h->size = size;
    const size_t room = packed_room(size);
    BXMI_TRY(h->packed.reserve(room));
    if (size == 0) BXMI_HIP(hipMemsetAsync(h->packed.p, 0, room, st));  // (else the kernel writes every word)
    const int64_t tiles = div_up(size, BL_TILE);  // at most 2^19: one launch
    const int vec = (reinterpret_cast<uintptr_t>(d_src) & (SRC == BL_NIB ? 3 : 15)) == 0;
    DevBuf counts, bases, scratch, lowest;
    int64_t head[2] = {0, 0};  // where the mask starts and the N ends begin in the scanned counts
    if (tiles > 0) {
        unsigned long long first_other = BL_NO_OTHER;
        BXMI_TRY(counts.reserve((size_t)tiles * BL_LISTS * 4));
        BXMI_TRY(bases.reserve((size_t)(tiles * BL_LISTS + 1) * 8));
        BXMI_TRY(lowest.reserve(8));
        BXMI_HIP(hipMemsetAsync(lowest.p, 0xFF, 8, st));
        hipLaunchKernelGGL((bl_build_kernel<SRC, false>), dim3((unsigned)tiles), dim3(BL_THREADS), 0, st, d_src, size, vec, tiles, (int64_t)(room / 4),
                           h->packed.as<uint32_t>(), counts.as<int32_t>(), (int)(other == BXMI_TB_OTHER_REFUSE), lowest.as<unsigned long long>(),
                           (const int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
        BXMI_LAUNCH_CHECK();
        BXMI_TRY((device_scan<int32_t, int64_t, OpSum, false>(counts.as<int32_t>(), bases.as<int64_t>(), tiles * BL_LISTS, (int64_t)0,
                                                              bases.as<int64_t>() + tiles * BL_LISTS, scratch, st)));
        BXMI_HIP(hipMemcpyAsync(&first_other, lowest.p, 8, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipMemcpyAsync(&head[0], bases.as<int64_t>() + tiles, 8, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipMemcpyAsync(&head[1], bases.as<int64_t>() + 2 * tiles, 8, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));
        if (other == BXMI_TB_OTHER_REFUSE && first_other != BL_NO_OTHER) {
            const long long at = (long long)(first_other >> 8);
            const unsigned v = (unsigned)(first_other & 0xFFu);
            if (SRC == BL_NIB) return fail(BXMI_EINVAL, "%s: position %lld holds nibble 0x%X (code %u), none of the codes 0 - 4 (T C A G N)", who, at, v, v & 7u);
            return fail(BXMI_EINVAL, "%s: position %lld holds byte 0x%02X, none of TCAGNtcagn", who, at, v);
        }
    }
    h->n_blocks = head[0];
    h->m_blocks = head[1] - head[0];
    BXMI_TRY(h->n_start.reserve((size_t)(h->n_blocks ? h->n_blocks * 4 : 8)));
    BXMI_TRY(h->n_end.reserve((size_t)(h->n_blocks ? h->n_blocks * 4 : 8)));
    BXMI_TRY(h->m_start.reserve((size_t)(h->m_blocks ? h->m_blocks * 4 : 8)));
    BXMI_TRY(h->m_end.reserve((size_t)(h->m_blocks ? h->m_blocks * 4 : 8)));
    if (h->n_blocks + h->m_blocks > 0) {
        hipLaunchKernelGGL((bl_build_kernel<SRC, true>), dim3((unsigned)tiles), dim3(BL_THREADS), 0, st, d_src, size, vec, tiles, (int64_t)(room / 4),
                           (uint32_t *)nullptr, counts.as<int32_t>(), 0, (unsigned long long *)nullptr, (const int64_t *)bases.as<int64_t>(),
                           h->n_start.as<int32_t>(), h->n_end.as<int32_t>(), h->m_start.as<int32_t>(), h->m_end.as<int32_t>());
        BXMI_LAUNCH_CHECK();
    }
    BXMI_TRY(build_running_sizes(h->n_start, h->n_end, h->n_blocks, h->n_cum, scratch, st));
    BXMI_TRY(build_running_sizes(h->m_start, h->m_end, h->m_blocks, h->m_cum, scratch, st));
    BXMI_TRY(twobit_finish(*h, st));  // (waits: counts, bases and scratch go away)
    *out = h.release();
    return BXMI_OK;
}

// the host forms: the whole input into a temporary on the device
template <int SRC>
static int build_from_host(const char *who, const uint8_t *in, int64_t size, int32_t other, bxmi_twobit_t **out)
{
    BXMI_TRY(build_check(who, in, size, other, out));
    const size_t bytes = (size_t)(SRC == BL_NIB ? (size + 1) / 2 : size);
    DevBuf tmp;
    BXMI_TRY(tmp.reserve(bytes ? bytes : 8));
    if (bytes) BXMI_HIP(hipMemcpy(tmp.p, in, bytes, hipMemcpyHostToDevice));
    return build_track<SRC>(who, tmp.as<uint8_t>(), size, other, out, nullptr);
}

extern "C" int bxmi_twobit_create_letters(const uint8_t *letters, int64_t size, int32_t other, bxmi_twobit_t **out)
{
    return build_from_host<BL_ASCII>("bxmi_twobit_create_letters", letters, size, other, out);
}

extern "C" int bxmi_twobit_create_nib(const uint8_t *nibbles, int64_t size, int32_t other, bxmi_twobit_t **out)
{
    return build_from_host<BL_NIB>("bxmi_twobit_create_nib", nibbles, size, other, out);
}

extern "C" int bxmi_twobit_create_letters_dev(const uint8_t *letters, int64_t size, int32_t other, bxmi_twobit_t **out, void *stream)
{
    const char *who = "bxmi_twobit_create_letters_dev";
    BXMI_TRY(build_check(who, letters, size, other, out));
    return build_track<BL_ASCII>(who, letters, size, other, out, as_stream(stream));
}

extern "C" int bxmi_twobit_arrays(const bxmi_twobit_t *h, uint8_t *packed, int32_t *n_start, int32_t *n_size, int32_t *m_start, int32_t *m_size)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_twobit_arrays: NULL handle");
    const size_t bytes = (size_t)((h->size + 3) / 4);
    if (packed && bytes) BXMI_HIP(hipMemcpy(packed, h->packed.p, bytes, hipMemcpyDeviceToHost));
    for (int list = 0; list < 2; list++) {
        const size_t blocks = (size_t)(list ? h->m_blocks : h->n_blocks);
        int32_t *start = list ? m_start : n_start, *size = list ? m_size : n_size;
        if (blocks == 0 || (!start && !size)) continue;
        std::vector<int32_t> s(blocks), e(blocks);
        BXMI_HIP(hipMemcpy(s.data(), (list ? h->m_start : h->n_start).p, blocks * 4, hipMemcpyDeviceToHost));
        if (size) BXMI_HIP(hipMemcpy(e.data(), (list ? h->m_end : h->n_end).p, blocks * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < blocks; i++) {
            if (start) start[i] = s[i];
            if (size) size[i] = e[i] - s[i];
        }
    }
    return BXMI_OK;
}

extern "C" int bxmi_twobit_destroy(bxmi_twobit_t *h)
{
    delete h;
    return BXMI_OK;
}

extern "C" int bxmi_twobit_info(const bxmi_twobit_t *h, int64_t *size, int64_t *n_blocks, int64_t *m_blocks)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_twobit_info: NULL handle");
    if (size) *size = h->size;
    if (n_blocks) *n_blocks = h->n_blocks;
    if (m_blocks) *m_blocks = h->m_blocks;
    return BXMI_OK;
}

static int sequence_fill_table(SequenceBufs &S, bxmi_twobit_t *const *tracks, int32_t n_tracks, hipStream_t st)
{
    return fill_track_table<TbTrack, 8>(S.table, n_tracks, [&](int k) { return tracks[k]->entry(); }, TbTrack{}, st);
}

// ---- letters (tb_bases_kernel) ----
// what both forms check; `row_off` is only tested for being there
static int rows_check(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, int64_t n, int32_t width, const void *row_off, int64_t total)
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
    return BXMI_OK;
}

static int bases_check(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const void *track_of, const void *start, int64_t n, int32_t width,
                       const void *row_off, int64_t total, int pad, const void *out)
{
    BXMI_TRY(rows_check(who, tracks, n_tracks, n, width, row_off, total));
    if (pad < 0 || pad > 255) return fail(BXMI_EINVAL, "%s: pad = %d is not a byte", who, pad);
    if ((n > 0 && (!track_of || !start)) || (n > 0 && total > 0 && !out)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

// what the host forms check of the offsets they can read (row_off == nullptr: nothing)
static int offsets_check(const char *who, const int64_t *row_off, int64_t n, int64_t total)
{
    if (!row_off) return BXMI_OK;
    if (row_off[0] != 0) return fail(BXMI_EINVAL, "%s: row_off[0] = %lld, must be 0", who, (long long)row_off[0]);
    for (int64_t i = 0; i < n; i++) {
        if (row_off[i + 1] < row_off[i]) return fail(BXMI_EINVAL, "%s: row_off descends at row %lld", who, (long long)i);
        if (row_off[i + 1] - row_off[i] > 2147483647LL)
            return fail(BXMI_EINVAL, "%s: row %lld has %lld elements, more than 2^31-1", who, (long long)i, (long long)(row_off[i + 1] - row_off[i]));
    }
    if (row_off[n] != total) return fail(BXMI_EINVAL, "%s: row_off[n] = %lld, but total = %lld", who, (long long)row_off[n], (long long)total);
    return BXMI_OK;
}

// what the host forms check of a strand array they can read (nullptr: all plus)
static int strand_check(const char *who, const int8_t *strand, int64_t n)
{
    if (!strand) return BXMI_OK;
    for (int64_t i = 0; i < n; i++)
        if (strand[i] != 0 && strand[i] != 1)
            return fail(BXMI_EINVAL, "%s: strand[%lld] = %d of row %lld is neither 0 (plus) nor 1 (minus)", who, (long long)i, (int)strand[i], (long long)i);
    return BXMI_OK;
}

// strand[r0 .. r0 + m) into S.q_strand -> *d_strand (nullptr without a strand array); queued on st
static int stage_strand(SequenceBufs &S, const int8_t *strand, int64_t r0, int64_t m, const int8_t **d_strand, hipStream_t st)
{
    *d_strand = nullptr;
    if (!strand) return BXMI_OK;
    BXMI_TRY(S.q_strand.reserve((size_t)(m > 0 ? m : 1)));
    if (m > 0) BXMI_HIP(hipMemcpyAsync(S.q_strand.p, strand + r0, (size_t)m, hipMemcpyHostToDevice, st));
    *d_strand = S.q_strand.as<int8_t>();
    return BXMI_OK;
}

// What the host forms put on the device of rows [r0, r0 + m): track and start into S.q_track and S.q_start and, with row_off, their
// m + 1 offsets into S.q_end -> *d_off, the offsets on the device (nullptr without).  Queued on st: the caller waits before the next use.
static int stage_rows(SequenceBufs &S, const int32_t *track_of, const int32_t *start, const int64_t *row_off, int64_t r0, int64_t m, const int64_t **d_off,
                      hipStream_t st)
{
    const size_t in_bytes = (size_t)m * sizeof(int32_t), off_bytes = (size_t)(m + 1) * sizeof(int64_t);
    BXMI_TRY(S.q_track.reserve(in_bytes));
    BXMI_TRY(S.q_start.reserve(in_bytes));
    BXMI_HIP(hipMemcpyAsync(S.q_track.p, track_of + r0, in_bytes, hipMemcpyHostToDevice, st));
    BXMI_HIP(hipMemcpyAsync(S.q_start.p, start + r0, in_bytes, hipMemcpyHostToDevice, st));
    *d_off = nullptr;
    if (row_off) {
        BXMI_TRY(S.q_end.reserve(off_bytes));
        BXMI_HIP(hipMemcpyAsync(S.q_end.p, row_off + r0, off_bytes, hipMemcpyHostToDevice, st));
        *d_off = S.q_end.as<int64_t>();
    }
    return BXMI_OK;
}

// the workgroups of a launch that strides over `tiles` tiles: at most a device's fill, 8 per compute unit
static unsigned fill_grid(int64_t tiles)
{
    const int64_t fill = (int64_t)device_props().cus * 8;
    return (unsigned)(tiles < fill ? tiles : fill);
}

// output bytes [o_first, o_first + count) of rows [row_base, row_base + n_rows); `out` is byte o_first's address
static int bases_launch(SequenceBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand, int64_t n_rows,
                        int64_t row_base, int32_t width, const int64_t *row_off, int64_t o_first, int64_t count, int do_mask, int pad, uint8_t *out,
                        hipStream_t st)
{
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;  // else the kernel stores byte by byte
    constexpr int64_t PER_LAUNCH = TB_TILES_PER_LAUNCH * TB_TILE;
    for (int64_t done = 0; done < count; done += PER_LAUNCH) {
        const int64_t m = count - done < PER_LAUNCH ? count - done : PER_LAUNCH;
        if (strand)
            hipLaunchKernelGGL(tb_bases_strand_kernel, dim3((unsigned)div_up(m, TB_TILE)), dim3(TB_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks,
                               track_of, start, strand, n_rows, row_base, (int)width, row_off, o_first + done, m, do_mask, pad, out + done, vec);
        else
            hipLaunchKernelGGL(tb_bases_kernel, dim3((unsigned)div_up(m, TB_TILE)), dim3(TB_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks, track_of,
                               start, n_rows, row_base, (int)width, row_off, o_first + done, m, do_mask, pad, out + done, vec);
        BXMI_LAUNCH_CHECK();
    }
    return BXMI_OK;
}

static int bases_dev(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                     int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out, void *stream)
{
    BXMI_TRY(bases_check(who, tracks, n_tracks, track_of, start, n, width, row_off_or_null, total, pad, out));
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter());
    BXMI_TRY(sequence_fill_table(g_sequence.bufs, tracks, n_tracks, as_stream(stream)));
    return bases_launch(g_sequence.bufs, n_tracks, track_of, start, strand, n, 0, width, row_off_or_null, 0, total, do_mask != 0, pad, out, as_stream(stream));
}

extern "C" int bxmi_twobit_bases_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                     int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out, void *stream)
{
    return bases_dev("bxmi_twobit_bases_dev", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pad, out, stream);
}

extern "C" int bxmi_twobit_bases_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                            const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                            int do_mask, int pad, uint8_t *out, void *stream)
{
    return bases_dev("bxmi_twobit_bases_strand_dev", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pad, out,
                     stream);
}

static int bases_host(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                      int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out)
{
    const int64_t *row_off = row_off_or_null;
    BXMI_TRY(bases_check(who, tracks, n_tracks, track_of, start, n, width, row_off, total, pad, out));
    BXMI_TRY(offsets_check(who, row_off, n, total));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(strand_check(who, strand, n));
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter(true));
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = g_sequence.stream;
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    for (int64_t o0 = 0; o0 < total; o0 += TB_SLAB) {  // slabs of whole tiles; a row may lie in several
        const int64_t count = total - o0 < TB_SLAB ? total - o0 : TB_SLAB;
        const SaRows rows = sa_rows_of(row_off, n, width, o0, count);  // the slab's rows
        const int64_t *d_off;
        const int8_t *d_strand;
        BXMI_TRY(stage_rows(S, track_of, start, row_off, rows.r0, rows.m, &d_off, st));
        BXMI_TRY(stage_strand(S, strand, rows.r0, rows.m, &d_strand, st));
        BXMI_TRY(S.r.reserve((size_t)count));
        BXMI_TRY(bases_launch(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), d_strand, rows.m, rows.r0, width, d_off, o0, count, do_mask != 0,
                              pad, S.r.as<uint8_t>(), st));
        BXMI_HIP(hipMemcpyAsync(out + o0, S.r.p, (size_t)count, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));  // the staging is reused by the next slab
    }
    return BXMI_OK;
}

extern "C" int bxmi_twobit_bases(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                                 const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out)
{
    return bases_host("bxmi_twobit_bases", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pad, out);
}

extern "C" int bxmi_twobit_bases_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                        const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask,
                                        int pad, uint8_t *out)
{
    return bases_host("bxmi_twobit_bases_strand", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pad, out);
}

// ---- base counts (tb_composition_kernel) ----
static int composition_check(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const void *track_of, const void *start, const void *end,
                             int64_t n, const void *counts)
{
    BXMI_TRY(track_batch_check(who, "width", 1, tracks, n_tracks, n));
    if (n > 0 && (!track_of || !start || !end || !counts)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

static int composition_launch(SequenceBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end, const int8_t *strand,
                              int64_t n, int do_mask, int32_t *counts, hipStream_t st)
{
    for (int64_t first = 0; first < n; first += TB_ROWS_PER_LAUNCH) {
        const int64_t m = n - first < TB_ROWS_PER_LAUNCH ? n - first : TB_ROWS_PER_LAUNCH;
        if (strand)
            hipLaunchKernelGGL(tb_composition_strand_kernel, dim3((unsigned)m), dim3(TB_WAVE), 0, st, S.table.as<TbTrack>(), (int)n_tracks, track_of + first,
                               start + first, end + first, strand + first, do_mask, counts + 6 * first);
        else
            hipLaunchKernelGGL(tb_composition_kernel, dim3((unsigned)m), dim3(TB_WAVE), 0, st, S.table.as<TbTrack>(), (int)n_tracks, track_of + first,
                               start + first, end + first, do_mask, counts + 6 * first);
        BXMI_LAUNCH_CHECK();
    }
    return BXMI_OK;
}

static int composition_dev(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                           const int8_t *strand, const int32_t *end, int64_t n, int do_mask, int32_t *counts, void *stream)
{
    BXMI_TRY(composition_check(who, tracks, n_tracks, track_of, start, end, n, counts));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter());
    BXMI_TRY(sequence_fill_table(g_sequence.bufs, tracks, n_tracks, as_stream(stream)));
    return composition_launch(g_sequence.bufs, n_tracks, track_of, start, end, strand, n, do_mask != 0, counts, as_stream(stream));
}

extern "C" int bxmi_twobit_composition_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                           const int32_t *end, int64_t n, int do_mask, int32_t *counts, void *stream)
{
    return composition_dev("bxmi_twobit_composition_dev", tracks, n_tracks, track_of, start, nullptr, end, n, do_mask, counts, stream);
}

extern "C" int bxmi_twobit_composition_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                                  const int8_t *strand_or_null, const int32_t *end, int64_t n, int do_mask, int32_t *counts, void *stream)
{
    return composition_dev("bxmi_twobit_composition_strand_dev", tracks, n_tracks, track_of, start, strand_or_null, end, n, do_mask, counts, stream);
}

static int composition_host(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                            const int8_t *strand, const int32_t *end, int64_t n, int do_mask, int32_t *counts)
{
    BXMI_TRY(composition_check(who, tracks, n_tracks, track_of, start, end, n, counts));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(strand_check(who, strand, n));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter(true));
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = g_sequence.stream;
    const int64_t slab = n < TB_COMP_SLAB ? n : TB_COMP_SLAB;
    const size_t rows = (size_t)slab * sizeof(int32_t);
    BXMI_TRY(S.q_track.reserve(rows));
    BXMI_TRY(S.q_start.reserve(rows));
    BXMI_TRY(S.q_end.reserve(rows));
    BXMI_TRY(S.r.reserve(rows * 6));
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    for (int64_t first = 0; first < n; first += slab) {
        const int64_t m = n - first < slab ? n - first : slab;
        const size_t in_bytes = (size_t)m * sizeof(int32_t);
        BXMI_HIP(hipMemcpyAsync(S.q_track.p, track_of + first, in_bytes, hipMemcpyHostToDevice, st));
        BXMI_HIP(hipMemcpyAsync(S.q_start.p, start + first, in_bytes, hipMemcpyHostToDevice, st));
        BXMI_HIP(hipMemcpyAsync(S.q_end.p, end + first, in_bytes, hipMemcpyHostToDevice, st));
        const int8_t *d_strand;
        BXMI_TRY(stage_strand(S, strand, first, m, &d_strand, st));
        BXMI_TRY(composition_launch(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), S.q_end.as<int32_t>(), d_strand, m, do_mask != 0,
                                    S.r.as<int32_t>(), st));
        BXMI_HIP(hipMemcpyAsync(counts + 6 * first, S.r.p, in_bytes * 6, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));  // the staging is reused by the next slab
    }
    return BXMI_OK;
}

extern "C" int bxmi_twobit_composition(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                                       int64_t n, int do_mask, int32_t *counts)
{
    return composition_host("bxmi_twobit_composition", tracks, n_tracks, track_of, start, nullptr, end, n, do_mask, counts);
}

extern "C" int bxmi_twobit_composition_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                              const int8_t *strand_or_null, const int32_t *end, int64_t n, int do_mask, int32_t *counts)
{
    return composition_host("bxmi_twobit_composition_strand", tracks, n_tracks, track_of, start, strand_or_null, end, n, do_mask, counts);
}

// ---- position weight matrices (pwm.hpp) ----
struct bxmi_pwm {
    int32_t n_mats = 0, n_cols = 0, max_width = 0;
    unsigned long long letters = 0;
    DevBuf values, mat_off;
    PwSet set() const { return PwSet{values.as<float>(), mat_off.as<int32_t>(), n_mats, n_cols, max_width, letters}; }
};

extern "C" int bxmi_pwm_create(const float *values, const int32_t *mat_off, int32_t n_mats, int32_t n_cols, const int8_t *letter_col, bxmi_pwm_t **out)
{
    const char *who = "bxmi_pwm_create";
    if (!out) return fail(BXMI_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (!values || !mat_off || !letter_col) return fail(BXMI_EINVAL, "%s: NULL array", who);
    if (n_mats < 1 || n_mats > PW_MATS_MAX) return fail(BXMI_EINVAL, "%s: n_mats = %d outside [1, %d]", who, (int)n_mats, PW_MATS_MAX);
    if (n_cols < 1 || n_cols > PW_COLS_MAX) return fail(BXMI_EINVAL, "%s: n_cols = %d outside [1, %d]", who, (int)n_cols, PW_COLS_MAX);
    if (mat_off[0] != 0) return fail(BXMI_EINVAL, "%s: mat_off[0] = %d, must be 0", who, (int)mat_off[0]);
    int32_t max_width = 0;
    for (int32_t m = 0; m < n_mats; m++) {
        const int64_t w = (int64_t)mat_off[m + 1] - mat_off[m];
        if (w < 0) return fail(BXMI_EINVAL, "%s: mat_off descends at matrix %d", who, (int)m);
        if (w < 1 || w > PW_WIDTH_MAX) return fail(BXMI_EINVAL, "%s: matrix %d has width %lld outside [1, %d]", who, (int)m, (long long)w, PW_WIDTH_MAX);
        if (w > max_width) max_width = (int32_t)w;
    }
    unsigned long long letters = 0;
    for (int k = 0; k < PW_LETTERS; k++) {
        if (letter_col[k] < -1 || letter_col[k] >= n_cols)
            return fail(BXMI_EINVAL, "%s: letter_col[%d] = %d outside [-1, n_cols = %d)", who, k, (int)letter_col[k], (int)n_cols);
        letters |= (unsigned long long)(letter_col[k] + 1) << (5 * k);
    }
    std::unique_ptr<bxmi_pwm> h(new (std::nothrow) bxmi_pwm());
    if (!h) return fail(BXMI_ENOMEM, "%s: host allocation failed", who);
    h->n_mats = n_mats;
    h->n_cols = n_cols;
    h->max_width = max_width;
    h->letters = letters;
    BXMI_TRY(put(h->values, values, (size_t)mat_off[n_mats] * (size_t)n_cols * sizeof(float)));
    BXMI_TRY(put(h->mat_off, mat_off, (size_t)(n_mats + 1) * sizeof(int32_t)));
    *out = h.release();
    return BXMI_OK;
}

extern "C" int bxmi_pwm_destroy(bxmi_pwm_t *h)
{
    delete h;
    return BXMI_OK;
}

extern "C" int bxmi_pwm_info(const bxmi_pwm_t *h, int32_t *n_mats, int32_t *n_cols, int32_t *max_width)
{
    if (!h) return fail(BXMI_EINVAL, "bxmi_pwm_info: NULL handle");
    if (n_mats) *n_mats = h->n_mats;
    if (n_cols) *n_cols = h->n_cols;
    if (max_width) *max_width = h->max_width;
    return BXMI_OK;
}

// what all four scoring calls check (`planes`: the call writes [n_mats][total] scores); `row_off` is only tested for being there
static int pwm_check(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const void *track_of, const void *start, int64_t n, int32_t width,
                     const void *row_off, int64_t total, const bxmi_pwm_t *pwm, bool planes)
{
    BXMI_TRY(rows_check(who, tracks, n_tracks, n, width, row_off, total));
    if (!pwm) return fail(BXMI_EINVAL, "%s: NULL matrix set", who);
    if (planes && total > PW_OUT_MAX / pwm->n_mats)
        return fail(BXMI_EINVAL, "%s: total = %lld elements in each of %d planes is more than the output index holds", who, (long long)total, (int)pwm->n_mats);
    if (n > 0 && (!track_of || !start)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

// elements [o_first, o_first + count) of every plane, of rows [row_base, row_base + n_rows); `out` is element o_first's address in
// plane 0.  keys != nullptr: the best hits instead (the whole batch: row_base == 0), nothing is stored to `out`.
static int pwm_launch(SequenceBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand, int64_t n_rows,
                      int64_t row_base, int32_t width, const int64_t *row_off, int64_t o_first, int64_t count, int do_mask, const bxmi_pwm_t *pwm, float *out, int64_t plane_stride,
                      unsigned long long *keys, hipStream_t st)
{
    if (keys) {  // one launch of at most a device's fill of workgroups, each walking every gridDim.x-th tile: `count` may be a bound
        if (strand)
            hipLaunchKernelGGL(pw_scores_strand_kernel<true>, dim3(fill_grid(div_up(count, PW_TILE))), dim3(PW_THREADS), 0, st, S.table.as<TbTrack>(),
                               (int)n_tracks, track_of, start, strand, n_rows, row_base, (int)width, row_off, o_first, count, do_mask, pwm->set(),
                               (float *)nullptr, (int64_t)0, keys, n_rows);
        else
            hipLaunchKernelGGL(pw_scores_kernel<true>, dim3(fill_grid(div_up(count, PW_TILE))), dim3(PW_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks,
                               track_of, start, n_rows, row_base, (int)width, row_off, o_first, count, do_mask, pwm->set(), (float *)nullptr, (int64_t)0, keys,
                               n_rows);
        BXMI_LAUNCH_CHECK();
        return BXMI_OK;
    }
    constexpr int64_t PER_LAUNCH = PW_TILES_PER_LAUNCH * PW_TILE;
    for (int64_t done = 0; done < count; done += PER_LAUNCH) {  // a workgroup per tile
        const int64_t m = count - done < PER_LAUNCH ? count - done : PER_LAUNCH;
        if (strand)
            hipLaunchKernelGGL(pw_scores_strand_kernel<false>, dim3((unsigned)div_up(m, PW_TILE)), dim3(PW_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks,
                               track_of, start, strand, n_rows, row_base, (int)width, row_off, o_first + done, m, do_mask, pwm->set(), out + done, plane_stride,
                               (unsigned long long *)nullptr, (int64_t)0);
        else
            hipLaunchKernelGGL(pw_scores_kernel<false>, dim3((unsigned)div_up(m, PW_TILE)), dim3(PW_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks,
                               track_of, start, n_rows, row_base, (int)width, row_off, o_first + done, m, do_mask, pwm->set(), out + done, plane_stride,
                               (unsigned long long *)nullptr, (int64_t)0);
        BXMI_LAUNCH_CHECK();
    }
    return BXMI_OK;
}

static int pwm_scores_dev(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                          int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out, void *stream)
{
    BXMI_TRY(pwm_check(who, tracks, n_tracks, track_of, start, n, width, row_off_or_null, total, pwm, true));
    if (n > 0 && total > 0 && !out) return fail(BXMI_EINVAL, "%s: NULL array", who);
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter());
    BXMI_TRY(sequence_fill_table(g_sequence.bufs, tracks, n_tracks, as_stream(stream)));
    return pwm_launch(g_sequence.bufs, n_tracks, track_of, start, strand, n, 0, width, row_off_or_null, 0, total, do_mask != 0, pwm, out, total, nullptr,
                      as_stream(stream));
}

extern "C" int bxmi_twobit_pwm_scores_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                          int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out,
                                          void *stream)
{
    return pwm_scores_dev("bxmi_twobit_pwm_scores_dev", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pwm, out, stream);
}

extern "C" int bxmi_twobit_pwm_scores_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                                 const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                                 int do_mask, const bxmi_pwm_t *pwm, float *out, void *stream)
{
    return pwm_scores_dev("bxmi_twobit_pwm_scores_strand_dev", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask,
                          pwm, out, stream);
}

static int pwm_scores_host(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                           int64_t n, int32_t width, const int64_t *row_off, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out)
{
    BXMI_TRY(pwm_check(who, tracks, n_tracks, track_of, start, n, width, row_off, total, pwm, true));
    if (n > 0 && total > 0 && !out) return fail(BXMI_EINVAL, "%s: NULL array", who);
    BXMI_TRY(offsets_check(who, row_off, n, total));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(strand_check(who, strand, n));
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter(true));
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = g_sequence.stream;
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    // slabs of whole tiles per plane, PW_SLAB elements over all planes (at least one tile each); a row may lie in several
    const int64_t slab = PW_SLAB / pwm->n_mats / PW_TILE > 0 ? PW_SLAB / pwm->n_mats / PW_TILE * PW_TILE : PW_TILE;
    for (int64_t o0 = 0; o0 < total; o0 += slab) {
        const int64_t count = total - o0 < slab ? total - o0 : slab;
        const SaRows rows = sa_rows_of(row_off, n, width, o0, count);  // the slab's rows
        const int64_t *d_off;
        const int8_t *d_strand;
        BXMI_TRY(stage_rows(S, track_of, start, row_off, rows.r0, rows.m, &d_off, st));
        BXMI_TRY(stage_strand(S, strand, rows.r0, rows.m, &d_strand, st));
        BXMI_TRY(S.r.reserve((size_t)count * sizeof(float) * (size_t)pwm->n_mats));
        BXMI_TRY(pwm_launch(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), d_strand, rows.m, rows.r0, width, d_off, o0, count, do_mask != 0,
                            pwm, S.r.as<float>(), count, nullptr, st));
        for (int32_t k = 0; k < pwm->n_mats; k++)  // each plane's part of the slab
            BXMI_HIP(hipMemcpyAsync(out + (int64_t)k * total + o0, S.r.as<float>() + (int64_t)k * count, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));  // the staging is reused by the next slab
    }
    return BXMI_OK;
}

extern "C" int bxmi_twobit_pwm_scores(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                                      const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out)
{
    return pwm_scores_host("bxmi_twobit_pwm_scores", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pwm, out);
}

extern "C" int bxmi_twobit_pwm_scores_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                             const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                             int do_mask, const bxmi_pwm_t *pwm, float *out)
{
    return pwm_scores_host("bxmi_twobit_pwm_scores_strand", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pwm,
                           out);
}

// keys = 0, the walk, the keys unpacked into best_score and best_pos [n_mats][n]
static int pwm_best_launch(SequenceBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand, int64_t n, int32_t width,
                           const int64_t *row_off, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos, hipStream_t st)
{
    const int64_t cells = (int64_t)pwm->n_mats * n;
    BXMI_TRY(S.keys.reserve((size_t)cells * sizeof(unsigned long long)));
    BXMI_HIP(hipMemsetAsync(S.keys.p, 0, (size_t)cells * sizeof(unsigned long long), st));
    if (total > 0)
        BXMI_TRY(pwm_launch(S, n_tracks, track_of, start, strand, n, 0, width, row_off, 0, total, do_mask, pwm, nullptr, 0, S.keys.as<unsigned long long>(), st));
    hipLaunchKernelGGL(pw_unpack_kernel, dim3((unsigned)div_up(cells, PW_THREADS)), dim3(PW_THREADS), 0, st, S.keys.as<unsigned long long>(), cells, best_score,
                       best_pos);
    BXMI_LAUNCH_CHECK();
    return BXMI_OK;
}

static int pwm_best_dev(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                        int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score,
                        int32_t *best_pos, void *stream)
{
    BXMI_TRY(pwm_check(who, tracks, n_tracks, track_of, start, n, width, row_off_or_null, total, pwm, false));
    if (n > 0 && (!best_score || !best_pos)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter());
    BXMI_TRY(sequence_fill_table(g_sequence.bufs, tracks, n_tracks, as_stream(stream)));
    return pwm_best_launch(g_sequence.bufs, n_tracks, track_of, start, strand, n, width, row_off_or_null, total, do_mask != 0, pwm, best_score, best_pos,
                           as_stream(stream));
}

extern "C" int bxmi_twobit_pwm_best_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                        int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score,
                                        int32_t *best_pos, void *stream)
{
    return pwm_best_dev("bxmi_twobit_pwm_best_dev", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pwm, best_score,
                        best_pos, stream);
}

extern "C" int bxmi_twobit_pwm_best_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                               const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                               int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos, void *stream)
{
    return pwm_best_dev("bxmi_twobit_pwm_best_strand_dev", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pwm,
                        best_score, best_pos, stream);
}

static int pwm_best_host(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                         int64_t n, int32_t width, const int64_t *row_off, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score,
                         int32_t *best_pos)
{
    BXMI_TRY(pwm_check(who, tracks, n_tracks, track_of, start, n, width, row_off, total, pwm, false));
    if (n > 0 && (!best_score || !best_pos)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    BXMI_TRY(offsets_check(who, row_off, n, total));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(strand_check(who, strand, n));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter(true));
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = g_sequence.stream;
    // nothing per base comes back: the rows go to the device whole and the walk is one launch
    const int64_t cells = (int64_t)pwm->n_mats * n;
    const size_t cell_bytes = (size_t)cells * 4;
    const int64_t *d_off;
    BXMI_TRY(S.r.reserve(2 * cell_bytes));
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    const int8_t *d_strand;
    BXMI_TRY(stage_rows(S, track_of, start, row_off, 0, n, &d_off, st));
    BXMI_TRY(stage_strand(S, strand, 0, n, &d_strand, st));
    float *d_score = S.r.as<float>();
    int32_t *d_pos = S.r.as<int32_t>() + cells;
    BXMI_TRY(pwm_best_launch(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), d_strand, n, width, d_off, total, do_mask != 0, pwm, d_score, d_pos,
                             st));
    BXMI_HIP(hipMemcpyAsync(best_score, d_score, cell_bytes, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipMemcpyAsync(best_pos, d_pos, cell_bytes, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipStreamSynchronize(st));
    return BXMI_OK;
}

extern "C" int bxmi_twobit_pwm_best(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                                    const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos)
{
    return pwm_best_host("bxmi_twobit_pwm_best", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pwm, best_score,
                         best_pos);
}

extern "C" int bxmi_twobit_pwm_best_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                           const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask,
                                           const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos)
{
    return pwm_best_host("bxmi_twobit_pwm_best_strand", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pwm,
                         best_score, best_pos);
}

// ---- thresholded hits (pwm_hits.hpp) ----
// what both forms check; `row_off` is only tested for being there
static int pwm_hits_check(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const void *track_of, const void *start, int64_t n, int32_t width,
                          const void *row_off, int64_t total, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap, const int64_t *mat_hits,
                          const void *hit_row, const void *hit_pos, const void *hit_score)
{
    BXMI_TRY(rows_check(who, tracks, n_tracks, n, width, row_off, total));  // (n above 2^31-1 is refused here: hit_row is int32)
    if (!threshold) return fail(BXMI_EINVAL, "%s: NULL threshold", who);
    if (!mat_hits) return fail(BXMI_EINVAL, "%s: NULL mat_hits", who);
    if (cap < 0) return fail(BXMI_EINVAL, "%s: cap = %lld is negative", who, (long long)cap);
    if (cap > 0 && (!hit_row || !hit_pos || !hit_score)) return fail(BXMI_EINVAL, "%s: NULL hit array with cap = %lld", who, (long long)cap);
    if (!pwm) return fail(BXMI_EINVAL, "%s: NULL matrix set", who);
    for (int32_t m = 0; m < pwm->n_mats; m++)
        if (threshold[m] != threshold[m]) return fail(BXMI_EINVAL, "%s: threshold[%d] is NaN", who, (int)m);
    if (total > PW_OUT_MAX / pwm->n_mats)
        return fail(BXMI_EINVAL, "%s: total = %lld elements under each of %d matrices is more than the hit index holds", who, (long long)total,
                    (int)pwm->n_mats);
    if (n > 0 && (!track_of || !start)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    return BXMI_OK;
}

// One pass of pw_hits_kernel over the whole batch, a workgroup per tile (measured against grids of 8 and of 16 workgroups per compute
// unit striding over the tiles: DESIGN.md 3.15), in launches of at most PH_TILES_PER_LAUNCH tiles.  FILL == false: S.hit_counts,
// their scan into S.hit_bases, and mat_hits[n_mats + 1] (host) from it -- BLOCKS on `st`.  FILL == true: the three hit arrays from
// S.hit_bases, queued.
template <bool FILL>
static int pwm_hits_pass(SequenceBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand, int64_t n, int32_t width,
                         const int64_t *row_off, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos,
                         float *hit_score, hipStream_t st)
{
    const int64_t tiles = div_up(total, PW_TILE), cells = tiles * pwm->n_mats;
    PhThresholds thr{};
    for (int32_t m = 0; m < pwm->n_mats; m++) thr.t[m] = threshold[m];
    if (!FILL) {
        BXMI_TRY(S.hit_counts.reserve((size_t)cells * sizeof(int32_t)));
        BXMI_TRY(S.hit_bases.reserve((size_t)(cells + 1 + pwm->n_mats + 1) * sizeof(int64_t)));
    }
    BXMI_TRY(ph_each_launch(tiles, PH_TILES_PER_LAUNCH, PH_TILES_PER_LAUNCH, [&](int64_t first, int64_t count, unsigned grid) {
        if (strand)
            hipLaunchKernelGGL(pw_hits_strand_kernel<FILL>, dim3(grid), dim3(PW_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks, track_of, start, strand, n,
                               (int)width, row_off, total, do_mask, pwm->set(), thr, first, count, tiles, S.hit_counts.as<int32_t>(), S.hit_bases.as<int64_t>(),
                               hit_row, hit_pos, hit_score);
        else
            hipLaunchKernelGGL(pw_hits_kernel<FILL>, dim3(grid), dim3(PW_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks, track_of, start, n, (int)width,
                               row_off, total, do_mask, pwm->set(), thr, first, count, tiles, S.hit_counts.as<int32_t>(), S.hit_bases.as<int64_t>(), hit_row,
                               hit_pos, hit_score);
        BXMI_LAUNCH_CHECK();
        return (int)BXMI_OK;
    }));
    if (FILL) return BXMI_OK;
    int64_t *bases = S.hit_bases.as<int64_t>(), *heads = bases + cells + 1;
    BXMI_TRY((device_scan<int32_t, int64_t, OpSum, false>(S.hit_counts.as<int32_t>(), bases, cells, (int64_t)0, bases + cells, S.hit_scan, st)));
    hipLaunchKernelGGL(ph_heads_kernel, dim3(1), dim3(64), 0, st, bases, tiles, (int)pwm->n_mats + 1, heads);
    BXMI_LAUNCH_CHECK();
    BXMI_HIP(hipMemcpyAsync(mat_hits, heads, (size_t)(pwm->n_mats + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipStreamSynchronize(st));
    return BXMI_OK;
}

static int pwm_hits_dev(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                        int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold,
                        int64_t cap, int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score, void *stream)
{
    BXMI_TRY(pwm_hits_check(who, tracks, n_tracks, track_of, start, n, width, row_off_or_null, total, pwm, threshold, cap, mat_hits, hit_row, hit_pos,
                            hit_score));
    for (int32_t m = 0; m <= pwm->n_mats; m++) mat_hits[m] = 0;
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter());
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = as_stream(stream);
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    BXMI_TRY(pwm_hits_pass<false>(S, n_tracks, track_of, start, strand, n, width, row_off_or_null, total, do_mask != 0, pwm, threshold, mat_hits, nullptr,
                                  nullptr, nullptr, st));
    const int64_t hits = mat_hits[pwm->n_mats];
    if (hits > cap) return fail(BXMI_ERANGE, "%s: %lld hits need larger arrays than cap=%lld", who, (long long)hits, (long long)cap);
    if (hits == 0) return BXMI_OK;
    return pwm_hits_pass<true>(S, n_tracks, track_of, start, strand, n, width, row_off_or_null, total, do_mask != 0, pwm, threshold, nullptr, hit_row, hit_pos,
                               hit_score, st);
}

extern "C" int bxmi_twobit_pwm_hits_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                        int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm,
                                        const float *threshold, int64_t cap, int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score,
                                        void *stream)
{
    return pwm_hits_dev("bxmi_twobit_pwm_hits_dev", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pwm, threshold, cap,
                        mat_hits, hit_row, hit_pos, hit_score, stream);
}

extern "C" int bxmi_twobit_pwm_hits_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                               const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                               int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap, int64_t *mat_hits, int32_t *hit_row,
                                               int32_t *hit_pos, float *hit_score, void *stream)
{
    return pwm_hits_dev("bxmi_twobit_pwm_hits_strand_dev", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pwm,
                        threshold, cap, mat_hits, hit_row, hit_pos, hit_score, stream);
}

static int pwm_hits_host(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                         int64_t n, int32_t width, const int64_t *row_off, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap,
                         int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score)
{
    BXMI_TRY(pwm_hits_check(who, tracks, n_tracks, track_of, start, n, width, row_off, total, pwm, threshold, cap, mat_hits, hit_row, hit_pos, hit_score));
    BXMI_TRY(offsets_check(who, row_off, n, total));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(strand_check(who, strand, n));
    for (int32_t m = 0; m <= pwm->n_mats; m++) mat_hits[m] = 0;
    if (n == 0 || total == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter(true));
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = g_sequence.stream;
    // nothing per base comes back: the rows go to the device whole, as for the best hits
    const int64_t *d_off;
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    const int8_t *d_strand;
    BXMI_TRY(stage_rows(S, track_of, start, row_off, 0, n, &d_off, st));
    BXMI_TRY(stage_strand(S, strand, 0, n, &d_strand, st));
    BXMI_TRY(pwm_hits_pass<false>(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), d_strand, n, width, d_off, total, do_mask != 0, pwm, threshold,
                                  mat_hits, nullptr, nullptr, nullptr, st));
    const int64_t hits = mat_hits[pwm->n_mats];
    if (hits > cap) return fail(BXMI_ERANGE, "%s: %lld hits need larger arrays than cap=%lld", who, (long long)hits, (long long)cap);
    if (hits == 0) return BXMI_OK;
    const size_t hit_bytes = (size_t)hits * 4;
    BXMI_TRY(S.r.reserve(3 * hit_bytes));
    int32_t *d_row = S.r.as<int32_t>(), *d_pos = d_row + hits;
    float *d_score = S.r.as<float>() + 2 * hits;
    BXMI_TRY(pwm_hits_pass<true>(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), d_strand, n, width, d_off, total, do_mask != 0, pwm, threshold,
                                 nullptr, d_row, d_pos, d_score, st));
    BXMI_HIP(hipMemcpyAsync(hit_row, d_row, hit_bytes, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipMemcpyAsync(hit_pos, d_pos, hit_bytes, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipMemcpyAsync(hit_score, d_score, hit_bytes, hipMemcpyDeviceToHost, st));
    BXMI_HIP(hipStreamSynchronize(st));
    return BXMI_OK;
}

extern "C" int bxmi_twobit_pwm_hits(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                                    const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap,
                                    int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score)
{
    return pwm_hits_host("bxmi_twobit_pwm_hits", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, pwm, threshold, cap,
                         mat_hits, hit_row, hit_pos, hit_score);
}

extern "C" int bxmi_twobit_pwm_hits_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                           const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask,
                                           const bxmi_pwm_t *pwm, const float *threshold, int64_t cap, int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos,
                                           float *hit_score)
{
    return pwm_hits_host("bxmi_twobit_pwm_hits_strand", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, pwm,
                         threshold, cap, mat_hits, hit_row, hit_pos, hit_score);
}

// ---- k-mer counts (kmer.hpp) ----
static std::atomic<int> g_km_force{KM_PLAN};

extern "C" int bxmi_twobit_kmer_force(int way)
{
    if (way != KM_PLAN && way != KM_FORCE_LDS && way != KM_FORCE_DIRECT)
        return fail(BXMI_EINVAL, "bxmi_twobit_kmer_force: way = %d is none of 0 (plan), 1 (LDS histogram), 2 (straight to HBM)", way);
    g_km_force.store(way);
    return BXMI_OK;
}

// what both forms check, and the kernel's description of the words; `row_off` is only tested for being there
static int kmer_check(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const void *track_of, const void *start, int64_t n, int32_t width,
                      const void *row_off, int64_t total, int k, int radix, const int8_t *digits, const void *counts, KmSpec &spec)
{
    BXMI_TRY(rows_check(who, tracks, n_tracks, n, width, row_off, total));
    if (k < 1) return fail(BXMI_EINVAL, "%s: k = %d, must be at least 1", who, k);
    if (radix < 2 || radix > 4) return fail(BXMI_EINVAL, "%s: radix = %d outside [2, 4]", who, radix);
    const int bins = km_bins(k, radix);
    if (bins > KM_BINS_MAX) return fail(BXMI_EINVAL, "%s: radix^k = %d^%d is more than KM_BINS_MAX = %d bins", who, radix, k, KM_BINS_MAX);
    if (!digits) return fail(BXMI_EINVAL, "%s: NULL digits", who);
    for (int c = 0; c < 8; c++)
        if (digits[c] < -1 || digits[c] >= radix)
            return fail(BXMI_EINVAL, "%s: digits[%d] = %d outside [-1, radix = %d)", who, c, (int)digits[c], radix);
    if (n > KM_OUT_MAX / bins)
        return fail(BXMI_EINVAL, "%s: n = %lld rows of %d bins are more than the output index holds", who, (long long)n, bins);
    if (n > 0 && !counts) return fail(BXMI_EINVAL, "%s: NULL counts", who);
    if (n > 0 && (!track_of || !start)) return fail(BXMI_EINVAL, "%s: NULL array", who);
    spec = KmSpec{k, radix, bins, km_pack_digits(digits), g_km_force.load()};
    return BXMI_OK;
}

// counts [n_rows][bins] = 0, then the windows that start at elements [o_first, o_first + count) of rows [row_base, row_base + n_rows):
// one launch of at most a device's fill of workgroups, each walking every gridDim.x-th tile (`count` may be a bound)
static int kmer_launch(SequenceBufs &S, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand, int64_t n_rows,
                       int64_t row_base, int32_t width, const int64_t *row_off, int64_t o_first, int64_t count, int do_mask, const KmSpec &spec,
                       int32_t *counts, hipStream_t st)
{
    BXMI_HIP(hipMemsetAsync(counts, 0, (size_t)n_rows * (size_t)spec.bins * sizeof(int32_t), st));
    if (count <= 0) return BXMI_OK;
    if (strand)
        hipLaunchKernelGGL(km_counts_strand_kernel, dim3(fill_grid(div_up(count, KM_TILE))), dim3(KM_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks,
                           track_of, start, strand, n_rows, row_base, (int)width, row_off, o_first, count, do_mask, spec, counts);
    else
        hipLaunchKernelGGL(km_counts_kernel, dim3(fill_grid(div_up(count, KM_TILE))), dim3(KM_THREADS), 0, st, S.table.as<TbTrack>(), (int)n_tracks, track_of,
                           start, n_rows, row_base, (int)width, row_off, o_first, count, do_mask, spec, counts);
    BXMI_LAUNCH_CHECK();
    return BXMI_OK;
}

static int kmer_dev(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                    int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits,
                    int32_t *counts, void *stream)
{
    KmSpec spec{};
    BXMI_TRY(kmer_check(who, tracks, n_tracks, track_of, start, n, width, row_off_or_null, total, k, radix, digits, counts, spec));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter());
    BXMI_TRY(sequence_fill_table(g_sequence.bufs, tracks, n_tracks, as_stream(stream)));
    return kmer_launch(g_sequence.bufs, n_tracks, track_of, start, strand, n, 0, width, row_off_or_null, 0, total, do_mask != 0, spec, counts,
                       as_stream(stream));
}

extern "C" int bxmi_twobit_kmer_counts_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n,
                                           int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix,
                                           const int8_t *digits, int32_t *counts, void *stream)
{
    return kmer_dev("bxmi_twobit_kmer_counts_dev", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, k, radix, digits,
                    counts, stream);
}

extern "C" int bxmi_twobit_kmer_counts_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                                  const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                                  int do_mask, int k, int radix, const int8_t *digits, int32_t *counts, void *stream)
{
    return kmer_dev("bxmi_twobit_kmer_counts_strand_dev", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, k,
                    radix, digits, counts, stream);
}

static int kmer_host(const char *who, bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int8_t *strand,
                     int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits,
                     int32_t *counts)
{
    const int64_t *row_off = row_off_or_null;
    KmSpec spec{};
    BXMI_TRY(kmer_check(who, tracks, n_tracks, track_of, start, n, width, row_off, total, k, radix, digits, counts, spec));
    BXMI_TRY(offsets_check(who, row_off, n, total));
    BXMI_TRY(track_of_check(who, track_of, n, n_tracks));
    BXMI_TRY(strand_check(who, strand, n));
    if (n == 0) return BXMI_OK;
    std::lock_guard<std::mutex> hold(g_sequence.lock);
    BXMI_TRY(g_sequence.enter(true));
    SequenceBufs &S = g_sequence.bufs;
    const hipStream_t st = g_sequence.stream;
    BXMI_TRY(sequence_fill_table(S, tracks, n_tracks, st));
    // slabs of whole rows, KM_SLAB_CELLS counters each (at least one row): the bases of a slab's rows are one stretch of the flat axis
    const int64_t slab = KM_SLAB_CELLS / spec.bins;
    for (int64_t r0 = 0; r0 < n; r0 += slab) {
        const int64_t m = n - r0 < slab ? n - r0 : slab;
        const int64_t o0 = row_off ? row_off[r0] : r0 * (int64_t)width, o1 = row_off ? row_off[r0 + m] : (r0 + m) * (int64_t)width;
        const size_t out_bytes = (size_t)m * (size_t)spec.bins * sizeof(int32_t);
        const int64_t *d_off;
        const int8_t *d_strand;
        BXMI_TRY(stage_rows(S, track_of, start, row_off, r0, m, &d_off, st));
        BXMI_TRY(stage_strand(S, strand, r0, m, &d_strand, st));
        BXMI_TRY(S.r.reserve(out_bytes));
        BXMI_TRY(kmer_launch(S, n_tracks, S.q_track.as<int32_t>(), S.q_start.as<int32_t>(), d_strand, m, r0, width, d_off, o0, o1 - o0, do_mask != 0, spec,
                             S.r.as<int32_t>(), st));
        BXMI_HIP(hipMemcpyAsync(counts + r0 * (int64_t)spec.bins, S.r.p, out_bytes, hipMemcpyDeviceToHost, st));
        BXMI_HIP(hipStreamSynchronize(st));  // the staging is reused by the next slab
    }
    return BXMI_OK;
}

extern "C" int bxmi_twobit_kmer_counts(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                                       const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits, int32_t *counts)
{
    return kmer_host("bxmi_twobit_kmer_counts", tracks, n_tracks, track_of, start, nullptr, n, width, row_off_or_null, total, do_mask, k, radix, digits, counts);
}

extern "C" int bxmi_twobit_kmer_counts_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                              const int8_t *strand_or_null, int64_t n, int32_t width, const int64_t *row_off_or_null, int64_t total,
                                              int do_mask, int k, int radix, const int8_t *digits, int32_t *counts)
{
    return kmer_host("bxmi_twobit_kmer_counts_strand", tracks, n_tracks, track_of, start, strand_or_null, n, width, row_off_or_null, total, do_mask, k,
                     radix, digits, counts);
}

// track_batch.hpp -- what the entry points over a BATCH OF ROWS ON A LIST OF TRACKS share (site profiles: profile.hpp + scores.hip;
// binned summaries: summary.hpp + summary.hip): the argument checks, the table of tracks the kernels read, the library's scratch.
// The table has n_tracks + 1 entries of the caller's Entry type: entry k < n_tracks describes tracks[k], entry n_tracks is the
// SPARE entry that rows without a track read (valid memory, nothing in it).  Every call rewrites it on its own stream; it travels
// in kernel arguments PACK entries at a time, so filling it is stream-ordered without a host buffer that would have to outlive
// the call.  The first half is plain C++ (tests/cpp/track_batch_test.cpp compiles it with g++); the device half needs hipcc.
#pragma once
#include <cstdint>

#include "../../include/bxmi.h"

namespace bxmi {

int fail(int code, const char *fmt, ...);  // (core.hip)

template <typename Entry, int PACK>
struct TrackPack { Entry t[PACK]; };

// Walks the table's entries [0, n_tracks] in packs of PACK: entry k < n_tracks is entry_of(k), entry n_tracks is `spare`;
// put(base, count, pack) takes pack.t[0 .. count) for entries [base, base + count).  Stops at put's first non-zero status.
template <typename Entry, int PACK, typename EntryOf, typename Put>
int for_each_track_pack(int32_t n_tracks, EntryOf entry_of, const Entry &spare, Put put)
{
    for (int32_t base = 0; base <= n_tracks; base += PACK) {
        TrackPack<Entry, PACK> pack{};
        const int count = n_tracks + 1 - base < PACK ? n_tracks + 1 - base : PACK;
        for (int k = 0; k < count; k++) pack.t[k] = base + k < n_tracks ? entry_of(base + k) : spare;
        if (const int rc = put((int)base, count, pack)) return rc;
    }
    return 0;
}

// The checks both forms of every such call begin with, in this order; `bin_name` is what the caller calls its `bin` parameter.
template <typename Handle>
int track_batch_check(const char *who, const char *bin_name, int32_t bin, Handle *const *tracks, int32_t n_tracks, int64_t n)
{
    if (bin < 1) return fail(BXMI_EINVAL, "%s: %s = %d, must be at least 1", who, bin_name, (int)bin);
    if (n < 0 || n > 2147483647LL) return fail(BXMI_EINVAL, "%s: n = %lld outside [0, 2^31-1]", who, (long long)n);
    if (n_tracks < 0) return fail(BXMI_EINVAL, "%s: n_tracks = %d is negative", who, (int)n_tracks);
    if (n_tracks > 0 && !tracks) return fail(BXMI_EINVAL, "%s: NULL track list", who);
    for (int32_t t = 0; t < n_tracks; t++)
        if (!tracks[t]) return fail(BXMI_EINVAL, "%s: track %d is a NULL handle", who, (int)t);
    return BXMI_OK;
}

// Host forms only (the device forms cannot look): a row may name no track (any negative entry), not one beyond the list.
inline int track_of_check(const char *who, const int32_t *track_of, int64_t n, int32_t n_tracks)
{
    for (int64_t i = 0; i < n; i++)
        if (track_of[i] >= n_tracks)
            return fail(BXMI_EINVAL, "%s: track_of[%lld] = %d, but there are %d tracks", who, (long long)i, (int)track_of[i], (int)n_tracks);
    return BXMI_OK;
}

}  // namespace bxmi

#if defined(__HIPCC__)
#include <mutex>
#include <new>

#include "common.hpp"

namespace bxmi {

// table[base .. base + count) = pack
template <typename Entry, int PACK>
__global__ __launch_bounds__(64) void track_table_kernel(Entry *__restrict__ table, int base, int count, TrackPack<Entry, PACK> pack)
{
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < PACK; k++)
        if (k < count) table[base + k] = pack.t[k];
}

// table = Entry[n_tracks + 1] as for_each_track_pack describes it, one launch per pack on `st`
template <typename Entry, int PACK, typename EntryOf>
int fill_track_table(DevBuf &table, int32_t n_tracks, EntryOf entry_of, const Entry &spare, hipStream_t st)
{
    BXMI_TRY(table.reserve((size_t)(n_tracks + 1) * sizeof(Entry)));
    return for_each_track_pack<Entry, PACK>(n_tracks, entry_of, spare, [&](int base, int count, const TrackPack<Entry, PACK> &pack) -> int {
        hipLaunchKernelGGL((track_table_kernel<Entry, PACK>), dim3(1), dim3(64), 0, st, table.as<Entry>(), base, count, pack);
        BXMI_LAUNCH_CHECK();
        return BXMI_OK;
    });
}

// Scratch that belongs to the library, not to a track (a call may name no track at all): one call at a time per process may be
// in flight on it, and `lock` is held for the length of a call.  Bufs is a plain struct of DevBuf members.  The scratch follows
// the current device: enter() (under the lock, first thing in a call; `own_stream`: the call is a host form and needs `stream`)
// drops the stream and ALL of Bufs when the device has changed since the last call -- Bufs is destroyed and constructed again
// in place, so no member can be left pointing at the previous device's memory.
template <typename Bufs>
struct LibraryScratch {
    std::mutex lock;
    int device = -1;
    hipStream_t stream = nullptr;  // of the host forms, non-blocking
    Bufs bufs;

    int enter(bool own_stream = false)
    {
        int dev = -1;
        BXMI_HIP(hipGetDevice(&dev));
        if (device != dev) {
            if (stream) (void)hipStreamDestroy(stream);
            stream = nullptr;
            bufs.~Bufs();
            new (&bufs) Bufs();
            device = dev;
        }
        if (own_stream && !stream) BXMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return BXMI_OK;
    }
    // (never destroyed: at process exit the runtime may be gone before a static destructor could free device memory)
    static LibraryScratch &leaked() { return *new LibraryScratch(); }
};

}  // namespace bxmi
#endif

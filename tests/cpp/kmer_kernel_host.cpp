// The kernel of bx-python_amd/csrc/kmer.hpp run on the host, its text compiled as it stands over kernel_host.hpp.  What this checks
// is everything in the kernel: the segments of a tile, the letters a thread decodes and from which words, the halo, the searches for
// the run of blocks, the chunks, the bits of the positions without a digit, the words, both ways of accumulating, every index and
// every atomic (build it with -fsanitize=address,undefined; the packed bytes are held in a buffer of exactly their whole words,
// every table in one of exactly its size, the counts between two guard bands).  km_use_lds, the plan, is called directly.
//
// usage: kmer_kernel_host IN OUT
//   IN:  int32 n_tracks, n, width, ragged, do_mask, k, radix, force, grid, slab_rows; int64 total; int8 digits[8];
//        per track int64 size, n_blocks, m_blocks, then packed[(size + 3) / 4] (uint8), n_start[], n_size[], m_start[], m_size[]
//        (int32); then track_of[n], start[n] (int32) and, when ragged, row_off[n + 1] (int64)
//        grid: the workgroups of a launch (0: one per tile), each walking every grid-th tile; `total` may be a bound beyond row_off[n]
//        slab_rows: > 0 cuts the batch into launches of that many rows, each given only its own rows and counts of exactly the slab's
//        size, as the host form of bxmi_twobit_kmer_counts does
//        n_tracks == -1: the plan instead -- n triples int64 (bins, windows, force) follow the head
//   OUT: int32 [GUARD + n * bins + GUARD], the guard bands as they were filled (0xEEEEEEEE); the counts are filled with 0x5A5A5A5A and
//        then zeroed as the library zeroes them, so a counter the zeroing misses shows; then int64 [2]: the atomic adds to LDS and to
//        the counts (the flushes of a histogram among the latter)
//        the plan: int32 [n], km_use_lds of every triple
#include "kernel_host.hpp"

#include "twobit_host.hpp"
// the integer atomic add, on LDS and on global memory alike: host threads share both
static std::atomic<long> g_lds_adds{0}, g_global_adds{0};
static int32_t *g_counts_lo = nullptr, *g_counts_hi = nullptr;
static int atomicAdd(int32_t *at, int v)
{
    if (at >= g_counts_lo && at < g_counts_hi) g_global_adds++;
    else g_lds_adds++;
    return __atomic_fetch_add(at, v, __ATOMIC_RELAXED);
}
#include "kmer.hpp"
using namespace bxmi;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<int64_t> total_in;
    std::vector<int8_t> digits;
    if (!read_n(f, head, 10) || !read_n(f, total_in, 1) || !read_n(f, digits, 8)) return 2;
    const int n_tracks = head[0], n = head[1], width = head[2], ragged = head[3], do_mask = head[4], k = head[5], radix = head[6], force = head[7];
    const int grid = head[8], slab_rows = head[9];
    const int64_t total = total_in[0];
    if (n_tracks == -1) {  // the plan
        std::vector<int64_t> triples;
        if (!read_n(f, triples, (size_t)n * 3)) return 2;
        fclose(f);
        std::vector<int32_t> answer(n);
        for (int i = 0; i < n; i++) answer[i] = km_use_lds((int)triples[3 * i], triples[3 * i + 1], (int)triples[3 * i + 2]) ? 1 : 0;
        f = fopen(argv[2], "wb");
        if (!f || fwrite(answer.data(), 4, answer.size(), f) != answer.size()) return 2;
        fclose(f);
        puts("kmer kernel host ok");
        return 0;
    }
    std::vector<Track> tracks(n_tracks);
    std::vector<TbTrack> table(n_tracks + 1);
    for (int t = 0; t < n_tracks; t++) {
        if (!read_track(f, tracks[t])) return 2;
        const Track &q = tracks[t];
        table[t] = TbTrack{q.packed.data(), q.n_start.data(), q.n_end.data(), q.m_start.data(), q.m_end.data(), nullptr, nullptr, nullptr, nullptr,
                           q.size, q.n_blocks, q.m_blocks};
    }
    table[n_tracks] = TbTrack{};
    std::vector<int32_t> track_of, start;
    std::vector<int64_t> row_off;
    if (!read_n(f, track_of, n) || !read_n(f, start, n) || (ragged && !read_n(f, row_off, (size_t)n + 1))) return 2;
    fclose(f);

    const int bins = km_bins(k, radix);
    if (k < 1 || bins > KM_BINS_MAX) return 3;
    const KmSpec spec{k, radix, bins, km_pack_digits(digits.data()), force};
    const size_t cells = (size_t)n * (size_t)bins;
    std::vector<uint32_t> out(2 * GUARD + cells, GUARD_BITS);
    int32_t *counts = reinterpret_cast<int32_t *>(out.data() + GUARD);

    auto launch = [&](const int32_t *s_track, const int32_t *s_start, int64_t m, int64_t r0, const int64_t *s_off, int64_t o0, int64_t count, int32_t *to) {
        memset(to, 0x5A, (size_t)m * bins * 4);
        memset(to, 0, (size_t)m * bins * 4);  // (hipMemsetAsync of the library)
        g_counts_lo = to, g_counts_hi = to + (size_t)m * bins;
        if (count <= 0) return;
        const int64_t tiles = (count + KM_TILE - 1) / KM_TILE;
        gridDim.x = (unsigned)(grid > 0 && grid < tiles ? grid : tiles);
        run_grid(KM_THREADS, gridDim.x, [&] { km_counts_kernel(table.data(), n_tracks, s_track, s_start, m, r0, width, s_off, o0, count, do_mask, spec, to); });
    };

    if (slab_rows <= 0) {
        if (n > 0) launch(track_of.data(), start.data(), n, 0, ragged ? row_off.data() : nullptr, 0, total, counts);
    } else {
        for (int64_t r0 = 0; r0 < n; r0 += slab_rows) {
            const int64_t m = n - r0 < slab_rows ? n - r0 : slab_rows;
            const int64_t o0 = ragged ? row_off[r0] : r0 * (int64_t)width, o1 = ragged ? row_off[r0 + m] : (r0 + m) * (int64_t)width;
            // (copies of exactly the slab's rows, counts of exactly the slab's size: an index outside them is an access outside an allocation)
            const std::vector<int32_t> s_track(track_of.begin() + r0, track_of.begin() + r0 + m), s_start(start.begin() + r0, start.begin() + r0 + m);
            std::vector<int64_t> s_off;
            if (ragged) s_off.assign(row_off.begin() + r0, row_off.begin() + r0 + m + 1);
            std::vector<int32_t> part((size_t)m * bins);
            launch(s_track.data(), s_start.data(), m, r0, ragged ? s_off.data() : nullptr, o0, o1 - o0, part.data());
            memcpy(counts + r0 * (int64_t)bins, part.data(), part.size() * 4);
        }
    }
    f = fopen(argv[2], "wb");
    const int64_t adds[2] = {g_lds_adds.load(), g_global_adds.load()};
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fwrite(adds, 8, 2, f) != 2) return 2;
    fclose(f);
    puts("kmer kernel host ok");
    return 0;
}

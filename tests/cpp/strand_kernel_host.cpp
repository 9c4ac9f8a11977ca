// The stranded kernels of bx-python_amd/csrc/twobit.hpp and kmer.hpp run on the host, their text compiled as it stands over
// kernel_host.hpp: tb_bases_strand_kernel, tb_composition_strand_kernel and km_counts_strand_kernel over a batch with a strand per
// row -- and, without a strand array, tb_bases_kernel, tb_composition_kernel and km_counts_kernel over the same batch, so that a
// strand array of zeros can be held against them byte for byte.  What this checks is everything strand touches: the positions of a
// segment of a minus row, the clipping of a thread's bytes to them, the place every letter goes to, the complement, the swap of
// the counts, the reversed words, every index and every store (build it with -fsanitize=address,undefined; the packed bytes are held
// in a buffer of exactly their whole words, every table and the strand array in one of exactly its size -- per slab, exactly the
// slab's rows -- and the output between two guard bands).
//
// usage: strand_kernel_host IN OUT
//   IN:  int32 mode (0 bases, 1 composition, 2 k-mer counts), n_tracks, n, width, ragged, misalign, slab, do_mask, pad, k, radix,
//        force, grid, has_strand; int64 total; int8 digits[8]; per track int64 size, n_blocks, m_blocks, then
//        packed[(size + 3) / 4] (uint8), n_start[], n_size[], m_start[], m_size[] (int32); then track_of[n], start[n] (int32), for
//        mode 1 end[n] (int32), with has_strand strand[n] (int8) and, when ragged, row_off[n + 1] (int64)
//        misalign: (mode 0) `out` starts this many bytes past a 16-byte boundary (not 0: the kernel stores byte by byte)
//        slab: > 0 cuts mode 0 into launches of that many tiles of output (sa_rows_of) and mode 2 into launches of that many rows,
//        each given only its own rows, as the host forms of the library do
//        grid: (mode 2) the workgroups of a launch (0: one per tile); `total` may be a bound beyond row_off[n]
//   OUT: mode 0: uint8 [GUARD + total + GUARD], the guard bands as they were filled (0xEE) unless the kernel wrote there
//        mode 1: int32 [GUARD + 6 n + GUARD], the guard bands 0x0EEEEEEE
//        mode 2: int32 [GUARD + n * bins + GUARD], the guard bands 0xEEEEEEEE
#include "kernel_host.hpp"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

// what the kernels use that kernel_host.hpp lacks
struct int4 {
    int x, y, z, w;
};
static int4 load_int4(const int32_t *p)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) abort();  // (the device would fault)
    return int4{p[0], p[1], p[2], p[3]};
}
static std::atomic<bool> g_aligned_store_seen{false}, g_misaligned_vector_store{false};
static bool g_watch_stores = false;  // (only the letters kernels' stores are the output's)
static void store_int4(int32_t *p, int a, int b, int c, int d)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) g_misaligned_vector_store = true;
    if (g_watch_stores) g_aligned_store_seen = true;
    p[0] = a, p[1] = b, p[2] = c, p[3] = d;
}
// TB_WAVE_SUM4 for a workgroup of one wave: everyone leaves its four values, meets at the barrier, adds up all 64, meets again
static int g_lane_values[64][4];
static void host_wave_sum4(int v[4])
{
    for (int c = 0; c < 4; c++) g_lane_values[threadIdx.x][c] = v[c];
    g_barrier.wait();
    for (int c = 0; c < 4; c++) {
        v[c] = 0;
        for (int lane = 0; lane < 64; lane++) v[c] += g_lane_values[lane][c];
    }
    g_barrier.wait();
}
#define TB_WAVE_SUM4(v) host_wave_sum4(v)
static Dim gridDim;
// the integer atomic add, on LDS and on global memory alike: host threads share both
static int atomicAdd(int32_t *at, int v) { return __atomic_fetch_add(at, v, __ATOMIC_RELAXED); }
#include "kmer.hpp"
using namespace bxmi;

constexpr size_t GUARD = 64;

// a 16-byte aligned array of exactly n int32 (ASan checks its ends)
struct AlignedDelete {
    void operator()(int32_t *p) const { ::operator delete[](p, std::align_val_t(16)); }
};
struct Aligned {
    std::unique_ptr<int32_t[], AlignedDelete> mem;
    explicit Aligned(size_t n) : mem(new (std::align_val_t(16)) int32_t[n ? n : 1]()) {}
    int32_t *get() const { return mem.get(); }
};

struct Track {
    int64_t size = 0, n_blocks = 0, m_blocks = 0;
    std::vector<uint32_t> packed;
    std::vector<int32_t> n_start, n_end, n_cum, m_start, m_end, m_cum;
    std::unique_ptr<Aligned> ckpt, n_codes;
};

// planes[4][items + 1], counts at [1, items] -> running totals, then the interleaved table of items + 1 entries
static std::unique_ptr<Aligned> running_codes(std::vector<int32_t> &planes, int64_t items)
{
    const int64_t stride = items + 1;
    for (int c = 0; c < 4; c++)
        for (int64_t i = 1; i < stride; i++) planes[c * stride + i] += planes[c * stride + i - 1];
    auto table = std::make_unique<Aligned>((size_t)stride * 4);
    run_grid(TB_THREADS, (unsigned)((stride + TB_THREADS - 1) / TB_THREADS), [&] { tb_interleave_kernel(planes.data(), stride, stride, table->get()); });
    return table;
}

static bool read_track(FILE *f, Track &t, bool tables)
{
    std::vector<int64_t> head;
    std::vector<uint8_t> bytes;
    std::vector<int32_t> n_size, m_size;
    if (!read_n(f, head, 3)) return false;
    t.size = head[0], t.n_blocks = head[1], t.m_blocks = head[2];
    if (!read_n(f, bytes, (size_t)(t.size + 3) / 4) || !read_n(f, t.n_start, t.n_blocks) || !read_n(f, n_size, t.n_blocks) ||
        !read_n(f, t.m_start, t.m_blocks) || !read_n(f, m_size, t.m_blocks))
        return false;
    t.packed.assign((bytes.size() + 3) / 4, 0u);  // whole words, the rest of the last one zero
    if (!bytes.empty()) memcpy(t.packed.data(), bytes.data(), bytes.size());
    auto ends = [](const std::vector<int32_t> &st, const std::vector<int32_t> &sz, std::vector<int32_t> &en, std::vector<int32_t> &cum) {
        en.resize(st.size());
        cum.assign(st.size() + 1, 0);
        for (size_t i = 0; i < st.size(); i++) en[i] = st[i] + sz[i], cum[i + 1] = cum[i] + sz[i];
    };
    ends(t.n_start, n_size, t.n_end, t.n_cum);
    ends(t.m_start, m_size, t.m_end, t.m_cum);
    if (!tables) return true;
    // creation, as bxmi_twobit_create runs it (the base counts need its tables)
    const int64_t ckpts = (t.size + TB_CKPT - 1) / TB_CKPT;
    std::vector<int32_t> planes((size_t)(ckpts + 1) * 4, 0);
    if (ckpts > 0) run_grid(TB_WAVE, (unsigned)ckpts, [&] { tb_count_kernel(t.packed.data(), t.size, ckpts + 1, planes.data() + 1); });
    t.ckpt = running_codes(planes, ckpts);
    planes.assign((size_t)(t.n_blocks + 1) * 4, 0);
    if (t.n_blocks > 0)
        run_grid(TB_WAVE, (unsigned)t.n_blocks,
                 [&] { tb_under_kernel(t.packed.data(), t.ckpt->get(), t.n_start.data(), t.n_end.data(), t.n_blocks + 1, planes.data() + 1); });
    t.n_codes = running_codes(planes, t.n_blocks);
    return true;
}

static int finish(const char *path, const void *data, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes) return 2;
    fclose(f);
    puts("strand kernel host ok");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<int64_t> total_in;
    std::vector<int8_t> digits;
    if (!read_n(f, head, 14) || !read_n(f, total_in, 1) || !read_n(f, digits, 8)) return 2;
    const int mode = head[0], n_tracks = head[1], n = head[2], width = head[3], ragged = head[4], misalign = head[5], slab = head[6];
    const int do_mask = head[7], pad = head[8], k = head[9], radix = head[10], force = head[11], grid = head[12], has_strand = head[13];
    const int64_t total = total_in[0];
    std::vector<Track> tracks(n_tracks);
    std::vector<TbTrack> table(n_tracks + 1);
    for (int t = 0; t < n_tracks; t++) {
        if (!read_track(f, tracks[t], mode == 1)) return 2;
        const Track &q = tracks[t];
        table[t] = TbTrack{q.packed.data(), q.n_start.data(), q.n_end.data(), q.m_start.data(), q.m_end.data(), mode == 1 ? q.ckpt->get() : nullptr,
                           q.n_cum.data(), mode == 1 ? q.n_codes->get() : nullptr, q.m_cum.data(), q.size, q.n_blocks, q.m_blocks};
    }
    table[n_tracks] = TbTrack{};
    std::vector<int32_t> track_of, start, end;
    std::vector<int8_t> strand;
    std::vector<int64_t> row_off;
    if (!read_n(f, track_of, n) || !read_n(f, start, n) || (mode == 1 && !read_n(f, end, n)) || (has_strand && !read_n(f, strand, n)) ||
        (ragged && !read_n(f, row_off, (size_t)n + 1)))
        return 2;
    fclose(f);

    if (mode == 1) {
        std::vector<int32_t> raw(2 * GUARD + (size_t)n * 6, 0x0EEEEEEE);
        if (n > 0)
            run_grid(TB_WAVE, (unsigned)n, [&] {
                if (has_strand)
                    tb_composition_strand_kernel(table.data(), n_tracks, track_of.data(), start.data(), end.data(), strand.data(), do_mask, raw.data() + GUARD);
                else tb_composition_kernel(table.data(), n_tracks, track_of.data(), start.data(), end.data(), do_mask, raw.data() + GUARD);
            });
        if (g_misaligned_vector_store) return 4;
        return finish(argv[2], raw.data(), raw.size() * 4);
    }

    if (mode == 2) {
        const int bins = km_bins(k, radix);
        if (k < 1 || bins > KM_BINS_MAX) return 3;
        const KmSpec spec{k, radix, bins, km_pack_digits(digits.data()), force};
        const size_t cells = (size_t)n * (size_t)bins;
        std::vector<uint32_t> out(2 * GUARD + cells, 0xEEEEEEEEu);
        int32_t *counts = reinterpret_cast<int32_t *>(out.data() + GUARD);
        auto launch = [&](const int32_t *s_track, const int32_t *s_start, const int8_t *s_strand, int64_t m, int64_t r0, const int64_t *s_off, int64_t o0,
                          int64_t count, int32_t *to) {
            memset(to, 0x5A, (size_t)m * bins * 4);
            memset(to, 0, (size_t)m * bins * 4);  // (hipMemsetAsync of the library)
            if (count <= 0) return;
            const int64_t tiles = (count + KM_TILE - 1) / KM_TILE;
            gridDim.x = (unsigned)(grid > 0 && grid < tiles ? grid : tiles);
            run_grid(KM_THREADS, gridDim.x, [&] {
                if (has_strand) km_counts_strand_kernel(table.data(), n_tracks, s_track, s_start, s_strand, m, r0, width, s_off, o0, count, do_mask, spec, to);
                else km_counts_kernel(table.data(), n_tracks, s_track, s_start, m, r0, width, s_off, o0, count, do_mask, spec, to);
            });
        };
        if (slab <= 0) {
            if (n > 0) launch(track_of.data(), start.data(), strand.data(), n, 0, ragged ? row_off.data() : nullptr, 0, total, counts);
        } else {
            for (int64_t r0 = 0; r0 < n; r0 += slab) {
                const int64_t m = n - r0 < slab ? n - r0 : slab;
                const int64_t o0 = ragged ? row_off[r0] : r0 * (int64_t)width, o1 = ragged ? row_off[r0 + m] : (r0 + m) * (int64_t)width;
                // (copies of exactly the slab's rows, counts of exactly the slab's size: an index outside them is an access outside an allocation)
                const std::vector<int32_t> s_track(track_of.begin() + r0, track_of.begin() + r0 + m), s_start(start.begin() + r0, start.begin() + r0 + m);
                std::vector<int8_t> s_strand;
                if (has_strand) s_strand.assign(strand.begin() + r0, strand.begin() + r0 + m);
                std::vector<int64_t> s_off;
                if (ragged) s_off.assign(row_off.begin() + r0, row_off.begin() + r0 + m + 1);
                std::vector<int32_t> part((size_t)m * bins);
                launch(s_track.data(), s_start.data(), s_strand.data(), m, r0, ragged ? s_off.data() : nullptr, o0, o1 - o0, part.data());
                memcpy(counts + r0 * (int64_t)bins, part.data(), part.size() * 4);
            }
        }
        return finish(argv[2], out.data(), out.size() * 4);
    }

    // [pad to the wanted alignment][GUARD][total][GUARD], the vector ending with the second guard band
    std::vector<uint8_t> raw(16 + misalign + 2 * GUARD + (size_t)total, 0xEE);
    size_t lead = 0;
    while ((reinterpret_cast<uintptr_t>(raw.data() + lead + GUARD) & 15) != 0) lead++;
    lead += misalign;
    raw.resize(lead + 2 * GUARD + (size_t)total);
    uint8_t *out = raw.data() + lead + GUARD;
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (vec != (misalign == 0)) return 3;
    g_watch_stores = true;
    const int64_t step = slab > 0 ? (int64_t)slab * TB_TILE : (total > 0 ? total : 1);
    for (int64_t o0 = 0; o0 < total; o0 += step) {
        const int64_t count = total - o0 < step ? total - o0 : step;
        const SaRows rows = slab > 0 ? sa_rows_of(ragged ? row_off.data() : nullptr, n, width, o0, count) : SaRows{0, n};
        const int64_t r0 = rows.r0, m = rows.m;
        // (copies of exactly the slab's rows: an index outside them is an access outside an allocation)
        const std::vector<int32_t> s_track(track_of.begin() + r0, track_of.begin() + r0 + m), s_start(start.begin() + r0, start.begin() + r0 + m);
        std::vector<int8_t> s_strand;
        if (has_strand) s_strand.assign(strand.begin() + r0, strand.begin() + r0 + m);
        std::vector<int64_t> s_off;
        if (ragged) s_off.assign(row_off.begin() + r0, row_off.begin() + r0 + m + 1);
        const unsigned tiles = (unsigned)((count + TB_TILE - 1) / TB_TILE);
        run_grid(TB_THREADS, tiles, [&] {
            if (has_strand)
                tb_bases_strand_kernel(table.data(), n_tracks, s_track.data(), s_start.data(), s_strand.data(), m, r0, width, ragged ? s_off.data() : nullptr, o0,
                                       count, do_mask, pad, out + o0, vec);
            else
                tb_bases_kernel(table.data(), n_tracks, s_track.data(), s_start.data(), m, r0, width, ragged ? s_off.data() : nullptr, o0, count, do_mask, pad,
                                out + o0, vec);
        });
    }
    if (g_misaligned_vector_store || (!vec && g_aligned_store_seen)) return 4;
    return finish(argv[2], raw.data() + lead, 2 * GUARD + (size_t)total);
}

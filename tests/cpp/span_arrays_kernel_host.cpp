// sa_arrays_kernel of bx-python_amd/csrc/span_arrays.hpp run on the host, its text compiled as it stands over kernel_host.hpp: a workgroup is SA_THREADS
// host threads that meet at a barrier where the kernel calls __syncthreads(), LDS is a static array, workgroups run one after
// another.  What this checks is everything in the kernel: which row an output element belongs to, the segments of a tile, the
// searches for a segment's run, the chunks, which staged item wins, every index and every store (build it with
// -fsanitize=address,undefined; the output sits between two guard bands in a buffer of exactly that size).
//
// usage: span_arrays_kernel_host IN OUT
//   IN:  int32 n_tracks, n, width, ragged, misalign, slab_tiles; int64 total; per track int32 items, ordered, then start[], end[]
//        (int32), value[] (float32); then track_of[n], start[n] (int32) and, when ragged, row_off[n + 1] (int64)
//        misalign: `out` starts this many elements past a 16-byte boundary (not 0: the kernel stores element by element)
//        slab_tiles: > 0 cuts the output into launches of that many tiles, each given only its own rows, cut by sa_rows_of as the
//        host form of bxmi_spans_arrays cuts them
//   OUT: uint32 [GUARD + total + GUARD]: the guard bands as they were filled (0xDEADBEEF) unless the kernel wrote there
#include "kernel_host.hpp"

static std::atomic<bool> g_aligned_store_seen{false}, g_misaligned_vector_store{false};
static void store_int4(int32_t *p, int a, int b, int c, int d)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) g_misaligned_vector_store = true;  // (the device would fault)
    g_aligned_store_seen = true;
    p[0] = a, p[1] = b, p[2] = c, p[3] = d;
}
#include "span_arrays.hpp"
using namespace bxmi;

constexpr size_t GUARD = 64;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<int64_t> total_in;
    if (!read_n(f, head, 6) || !read_n(f, total_in, 1)) return 2;
    const int n_tracks = head[0], n = head[1], width = head[2], ragged = head[3], misalign = head[4], slab_tiles = head[5];
    const int64_t total = total_in[0];
    std::vector<std::vector<int32_t>> st(n_tracks), en(n_tracks);
    std::vector<std::vector<float>> va(n_tracks);
    std::vector<SmTrack> table(n_tracks + 1);
    for (int t = 0; t < n_tracks; t++) {
        std::vector<int32_t> m;
        if (!read_n(f, m, 2) || !read_n(f, st[t], m[0]) || !read_n(f, en[t], m[0]) || !read_n(f, va[t], m[0])) return 2;
        table[t] = SmTrack{st[t].data(), en[t].data(), va[t].data(), m[0], m[1]};
    }
    table[n_tracks] = SmTrack{nullptr, nullptr, nullptr, 0, 1};
    std::vector<int32_t> track_of, start;
    std::vector<int64_t> row_off;
    if (!read_n(f, track_of, n) || !read_n(f, start, n) || (ragged && !read_n(f, row_off, (size_t)n + 1))) return 2;
    fclose(f);
    // [pad to the wanted alignment][GUARD][total][GUARD], the vector ending with the second guard band
    std::vector<uint32_t> raw(4 + misalign + 2 * GUARD + (size_t)total, 0xDEADBEEFu);
    size_t lead = 0;
    while ((reinterpret_cast<uintptr_t>(raw.data() + lead + GUARD) & 15) != 0) lead++;
    lead += misalign;
    raw.resize(lead + 2 * GUARD + (size_t)total);
    float *out = reinterpret_cast<float *>(raw.data() + lead + GUARD);
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (vec != (misalign == 0)) return 3;

    const int64_t slab = slab_tiles > 0 ? (int64_t)slab_tiles * SA_TILE : (total > 0 ? total : 1);
    for (int64_t o0 = 0; o0 < total; o0 += slab) {
        const int64_t count = total - o0 < slab ? total - o0 : slab;
        // (the library's own cutting: sa_rows_of of span_arrays.hpp)
        const SaRows rows = slab_tiles > 0 ? sa_rows_of(ragged ? row_off.data() : nullptr, n, width, o0, count) : SaRows{0, n};
        const int64_t r0 = rows.r0, m = rows.m;
        // (copies of exactly the slab's rows: an index outside them is an access outside an allocation)
        const std::vector<int32_t> s_track(track_of.begin() + r0, track_of.begin() + r0 + m), s_start(start.begin() + r0, start.begin() + r0 + m);
        std::vector<int64_t> s_off;
        if (ragged) s_off.assign(row_off.begin() + r0, row_off.begin() + r0 + m + 1);
        const unsigned tiles = (unsigned)((count + SA_TILE - 1) / SA_TILE);
        run_grid(SA_THREADS, tiles, [&] {
            sa_arrays_kernel(table.data(), n_tracks, s_track.data(), s_start.data(), m, r0, width, ragged ? s_off.data() : nullptr, o0, count, out + o0,
                             vec);
        });
    }
    if (g_misaligned_vector_store || (!vec && g_aligned_store_seen)) return 4;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const size_t words = 2 * GUARD + (size_t)total;
    if (fwrite(raw.data() + lead, sizeof(uint32_t), words, f) != words) return 2;
    fclose(f);
    puts("span arrays kernel host ok");
    return 0;
}

// The stranded kernels of bx-python_amd/csrc/pwm.hpp and pwm_hits.hpp run on the host, their text compiled as it stands over
// kernel_host.hpp: pw_scores_strand_kernel storing scores or folding best hits into keys, pw_hits_strand_kernel counting and placing
// hits.  What this checks is everything strand touches and everything behind it: pw_stage_columns -- the positions of a minus
// segment and of its halo at LOWER positions, the words a thread reads, the searches over the clipped range, the complement before
// the letter_col lookup, the byte-reversed 8-byte store at the mirrored place -- and then the unchanged window walk, keys and ranks
// on what was staged, every index and every store (build it with -fsanitize=address,undefined and -ffp-contract=off; the packed
// bytes are held in a buffer of exactly their whole words, every table AND THE STRAND ARRAY in one of exactly its size -- per slab
// exactly the slab's rows -- the outputs between two guard bands).
//
// usage: pwm_strand_kernel_host IN OUT
//   IN:  int32 mode (0 scores, 1 best, 2 hits), n_tracks, n, width, ragged, misalign, slab_tiles, do_mask, n_mats, n_cols, grid,
//        launch_tiles, plain; int64 total, cap; float32 threshold[n_mats]; int8 letter_col[10]; int32 mat_off[n_mats + 1];
//        float32 values[mat_off[n_mats]][n_cols]; per track int64 size, n_blocks, m_blocks, then packed[(size + 3) / 4] (uint8),
//        n_start[], n_size[], m_start[], m_size[] (int32); then track_of[n], start[n] (int32), strand[n] (int8) and, when ragged,
//        row_off[n + 1] (int64)
//        plain: 1 runs the UNSTRANDED kernels and does not pass the strand array on (for the comparison with a strand of zeros)
//        misalign, slab_tiles (mode 0), grid (modes 1, 2), launch_tiles, cap (mode 2): as pwm_kernel_host and pwm_hits_kernel_host
//   OUT: mode 0: float32 [GUARD + n_mats * total + GUARD]
//        mode 1: float32 [GUARD + n_mats * n + GUARD] best scores, then int32 [GUARD + n_mats * n + GUARD] best positions
//        mode 2: int64 mat_hits[n_mats + 1], int64 filled; then hit_row, hit_pos (int32), hit_score (float32), each
//        [GUARD + cap + GUARD]
#include "kernel_host.hpp"

#include "twobit_host.hpp"
static unsigned long long g_lane_keys[1024];
static unsigned long long host_wave_max64(unsigned long long key)
{
    g_lane_keys[threadIdx.x] = key;
    g_barrier.wait();
    const unsigned first = threadIdx.x & ~63u;
    unsigned long long top = 0;
    for (unsigned lane = first; lane < first + 64; lane++) top = g_lane_keys[lane] > top ? g_lane_keys[lane] : top;
    g_barrier.wait();
    return top;
}
#define PW_WAVE_MAX64(key) host_wave_max64(key)
static std::mutex g_atomic_lock;
static void host_atomic_max64(unsigned long long *at, unsigned long long key)
{
    std::lock_guard<std::mutex> hold(g_atomic_lock);
    if (key > *at) *at = key;
}
#define PW_ATOMIC_MAX64(at, key) host_atomic_max64(at, key)
static int g_lane_values[1024];
static int host_wave_prefix(int v)
{
    g_lane_values[threadIdx.x] = v;
    g_barrier.wait();
    int sum = 0;
    for (unsigned lane = threadIdx.x & ~63u; lane <= threadIdx.x; lane++) sum += g_lane_values[lane];
    g_barrier.wait();
    return sum;
}
#define PH_WAVE_PREFIX(v) host_wave_prefix(v)
#include "pwm_hits.hpp"
using namespace bxmi;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head, mat_off;
    std::vector<int64_t> wide;
    std::vector<int8_t> letter_col;
    std::vector<float> values, threshold;
    if (!read_n(f, head, 13) || !read_n(f, wide, 2)) return 2;
    const int mode = head[0], n_tracks = head[1], n = head[2], width = head[3], ragged = head[4], misalign = head[5], slab_tiles = head[6];
    const int do_mask = head[7], n_mats = head[8], n_cols = head[9], grid = head[10], launch_tiles = head[11], plain = head[12];
    const int64_t total = wide[0];
    if (n_mats < 1 || n_mats > PW_MATS_MAX) return 2;
    if (!read_n(f, threshold, n_mats) || !read_n(f, letter_col, PW_LETTERS) || !read_n(f, mat_off, (size_t)n_mats + 1) ||
        !read_n(f, values, (size_t)mat_off[n_mats] * n_cols))
        return 2;
    std::vector<Track> tracks(n_tracks);
    std::vector<TbTrack> table(n_tracks + 1);
    for (int t = 0; t < n_tracks; t++) {
        if (!read_track(f, tracks[t])) return 2;
        const Track &k = tracks[t];
        table[t] = TbTrack{k.packed.data(), k.n_start.data(), k.n_end.data(), k.m_start.data(), k.m_end.data(), nullptr, nullptr, nullptr, nullptr,
                           k.size, k.n_blocks, k.m_blocks};
    }
    table[n_tracks] = TbTrack{};
    std::vector<int32_t> track_of, start;
    std::vector<int8_t> strand;
    std::vector<int64_t> row_off;
    if (!read_n(f, track_of, n) || !read_n(f, start, n) || !read_n(f, strand, n) || (ragged && !read_n(f, row_off, (size_t)n + 1))) return 2;
    fclose(f);

    PwSet pw{values.data(), mat_off.data(), n_mats, n_cols, 0, 0ull};
    for (int m = 0; m < n_mats; m++) pw.max_width = mat_off[m + 1] - mat_off[m] > pw.max_width ? mat_off[m + 1] - mat_off[m] : pw.max_width;
    for (int k = 0; k < PW_LETTERS; k++) pw.letters |= (unsigned long long)(letter_col[k] + 1) << (5 * k);
    const int64_t *offsets = ragged ? row_off.data() : nullptr;

    if (mode == 1) {
        const size_t cells = (size_t)n_mats * n;
        std::vector<unsigned long long> keys(cells, 0ull);
        const int64_t tiles = (total + PW_TILE - 1) / PW_TILE;
        gridDim.x = (unsigned)(grid > 0 && grid < tiles ? grid : tiles);
        if (total > 0 && n > 0)
            run_grid(PW_THREADS, gridDim.x, [&] {
                if (plain)
                    pw_scores_kernel<true>(table.data(), n_tracks, track_of.data(), start.data(), n, 0, width, offsets, 0, total, do_mask, pw, nullptr, 0,
                                           keys.data(), n);
                else
                    pw_scores_strand_kernel<true>(table.data(), n_tracks, track_of.data(), start.data(), strand.data(), n, 0, width, offsets, 0, total,
                                                  do_mask, pw, nullptr, 0, keys.data(), n);
            });
        Banded score(cells, 0), pos(cells, 0);
        if (cells > 0)
            run_grid(PW_THREADS, (unsigned)((cells + PW_THREADS - 1) / PW_THREADS), [&] {
                pw_unpack_kernel(keys.data(), (int64_t)cells, reinterpret_cast<float *>(score.body()), reinterpret_cast<int32_t *>(pos.body()));
            });
        f = fopen(argv[2], "wb");
        if (!f || !score.write(f) || !pos.write(f)) return 2;
        fclose(f);
        puts("pwm strand kernel host ok");
        return 0;
    }

    if (mode == 2) {
        PhThresholds thr{};
        for (int m = 0; m < n_mats; m++) thr.t[m] = threshold[m];
        const int64_t tiles = n > 0 ? (total + PW_TILE - 1) / PW_TILE : 0, cells = tiles * n_mats;
        const int64_t per_launch = launch_tiles > 0 ? launch_tiles : PH_TILES_PER_LAUNCH, fill = grid > 0 ? grid : (tiles > 0 ? tiles : 1);
        std::vector<int32_t> counts((size_t)cells, -1);  // (a count the kernel does not store shows)
        std::vector<int64_t> bases((size_t)cells + 1, 0), mat_hits((size_t)n_mats + 1, 0);
        ph_each_launch(tiles, per_launch, fill, [&](int64_t first, int64_t count, unsigned blocks) {
            gridDim.x = blocks;
            run_grid(PW_THREADS, blocks, [&] {
                if (plain)
                    pw_hits_kernel<false>(table.data(), n_tracks, track_of.data(), start.data(), n, width, offsets, total, do_mask, pw, thr, first, count,
                                          tiles, counts.data(), nullptr, nullptr, nullptr, nullptr);
                else
                    pw_hits_strand_kernel<false>(table.data(), n_tracks, track_of.data(), start.data(), strand.data(), n, width, offsets, total, do_mask,
                                                 pw, thr, first, count, tiles, counts.data(), nullptr, nullptr, nullptr, nullptr);
            });
            return 0;
        });
        for (int64_t k = 0; k < cells; k++) {
            if (counts[k] < 0 || counts[k] > PW_TILE) return 3;
            bases[k + 1] = bases[k] + counts[k];
        }
        gridDim.x = 1;
        run_grid(64, 1, [&] { ph_heads_kernel(bases.data(), tiles, n_mats + 1, mat_hits.data()); });
        const int64_t hits = mat_hits[n_mats], cap = wide[1] < 0 ? hits : wide[1];
        if (hits != bases[cells]) return 3;
        Banded rows((size_t)cap), pos((size_t)cap), score((size_t)cap);
        const int64_t filled = hits <= cap && hits > 0;
        if (filled)
            ph_each_launch(tiles, per_launch, fill, [&](int64_t first, int64_t count, unsigned blocks) {
                gridDim.x = blocks;
                run_grid(PW_THREADS, blocks, [&] {
                    if (plain)
                        pw_hits_kernel<true>(table.data(), n_tracks, track_of.data(), start.data(), n, width, offsets, total, do_mask, pw, thr, first, count,
                                             tiles, counts.data(), bases.data(), reinterpret_cast<int32_t *>(rows.body()),
                                             reinterpret_cast<int32_t *>(pos.body()), reinterpret_cast<float *>(score.body()));
                    else
                        pw_hits_strand_kernel<true>(table.data(), n_tracks, track_of.data(), start.data(), strand.data(), n, width, offsets, total, do_mask,
                                                    pw, thr, first, count, tiles, counts.data(), bases.data(), reinterpret_cast<int32_t *>(rows.body()),
                                                    reinterpret_cast<int32_t *>(pos.body()), reinterpret_cast<float *>(score.body()));
                });
                return 0;
            });
        f = fopen(argv[2], "wb");
        if (!f || fwrite(mat_hits.data(), 8, mat_hits.size(), f) != mat_hits.size() || fwrite(&filled, 8, 1, f) != 1 || !rows.write(f) || !pos.write(f) ||
            !score.write(f))
            return 2;
        fclose(f);
        puts("pwm strand kernel host ok");
        return 0;
    }

    Banded out((size_t)n_mats * (size_t)total, misalign);
    float *planes = reinterpret_cast<float *>(out.body());
    if (((reinterpret_cast<uintptr_t>(planes) & 15) == 0) != (misalign == 0)) return 3;
    const int64_t slab = slab_tiles > 0 ? (int64_t)slab_tiles * PW_TILE : (total > 0 ? total : 1);
    for (int64_t o0 = 0; o0 < total && n > 0; o0 += slab) {
        const int64_t count = total - o0 < slab ? total - o0 : slab;
        gridDim.x = (unsigned)((count + PW_TILE - 1) / PW_TILE);
        if (slab_tiles <= 0) {
            run_grid(PW_THREADS, gridDim.x, [&] {
                if (plain)
                    pw_scores_kernel<false>(table.data(), n_tracks, track_of.data(), start.data(), n, 0, width, offsets, 0, total, do_mask, pw, planes, total,
                                            nullptr, 0);
                else
                    pw_scores_strand_kernel<false>(table.data(), n_tracks, track_of.data(), start.data(), strand.data(), n, 0, width, offsets, 0, total,
                                                   do_mask, pw, planes, total, nullptr, 0);
            });
            break;
        }
        const SaRows rows = sa_rows_of(offsets, n, width, o0, count);
        const int64_t r0 = rows.r0, m = rows.m;
        // (copies of exactly the slab's rows -- the strand among them -- and planes of exactly the slab's elements)
        const std::vector<int32_t> s_track(track_of.begin() + r0, track_of.begin() + r0 + m), s_start(start.begin() + r0, start.begin() + r0 + m);
        const std::vector<int8_t> s_strand(strand.begin() + r0, strand.begin() + r0 + m);
        std::vector<int64_t> s_off;
        if (ragged) s_off.assign(row_off.begin() + r0, row_off.begin() + r0 + m + 1);
        std::vector<float> part((size_t)n_mats * (size_t)count);
        run_grid(PW_THREADS, gridDim.x, [&] {
            if (plain)
                pw_scores_kernel<false>(table.data(), n_tracks, s_track.data(), s_start.data(), m, r0, width, ragged ? s_off.data() : nullptr, o0, count,
                                        do_mask, pw, part.data(), count, nullptr, 0);
            else
                pw_scores_strand_kernel<false>(table.data(), n_tracks, s_track.data(), s_start.data(), s_strand.data(), m, r0, width,
                                               ragged ? s_off.data() : nullptr, o0, count, do_mask, pw, part.data(), count, nullptr, 0);
        });
        for (int k = 0; k < n_mats; k++) memcpy(planes + (int64_t)k * total + o0, part.data() + (int64_t)k * count, (size_t)count * sizeof(float));
    }
    if (g_misaligned_vector_store) return 4;
    f = fopen(argv[2], "wb");
    if (!f || !out.write(f)) return 2;
    fclose(f);
    printf("vector stores %ld\n", g_vector_stores.load());
    puts("pwm strand kernel host ok");
    return 0;
}

// The kernels of bx-python_amd/csrc/twobit_build.hpp run on the host, their text compiled as it stands over kernel_host.hpp:
// bl_build_kernel<SRC, false> packing and counting, the scan of the counts in plain C++ here, bl_build_kernel<SRC, true> placing the
// block starts and ends, bl_sizes_kernel and a plain running sum.  What this checks is everything in the kernels: the loads (the
// input sits in a buffer of exactly its size, at a chosen misalignment), the classification, the run edges across threads, waves and
// tiles, the ranks, every index and every store (build it with -fsanitize=address,undefined; counts and bases are held in buffers of
// exactly their size, the packed words and the four block arrays between two guard bands).
//
// usage: build_kernel_host IN OUT
//   IN:  int32 n_cases; per case int32 src (0: ASCII bytes, 1: nib nibbles), int32 misalign (bytes the input lies past a 16-byte
//        boundary), int64 size, then the input: uint8 [size], or [(size + 1) / 2] of a nib
//   OUT: per case int64 n_blocks, m_blocks, first_other (all bits set: none); then uint32 [GUARD + words + GUARD] each, the guard bands
//        as they were filled (bits 0xEEEEEEEE): packed (whole checkpoint blocks), n_start, n_end, m_start, m_end; then int32
//        n_cum[n_blocks + 1], m_cum[m_blocks + 1]
#include "kernel_host.hpp"

#include "twobit_host.hpp"
// BL_WAVE_PREFIX for a workgroup of host threads: everyone leaves its value, meets at the barrier, sums its wave's lanes up to
// itself, meets again.  BL_ATOMIC_MIN64 under a lock.
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
#define BL_WAVE_PREFIX(v) host_wave_prefix(v)
static std::mutex g_min_lock;
static void host_atomic_min64(unsigned long long *at, unsigned long long key)
{
    std::lock_guard<std::mutex> hold(g_min_lock);
    if (key < *at) *at = key;
}
#define BL_ATOMIC_MIN64(at, key) host_atomic_min64(at, key)
#include "twobit_build.hpp"
using namespace bxmi;

constexpr int CKPT = 1024;  // TB_CKPT of twobit.hpp

template <int SRC>
static bool run_case(const uint8_t *src, int64_t size, int vec, FILE *out)
{
    const int64_t ckpts = (size + CKPT - 1) / CKPT, room_words = (ckpts > 0 ? ckpts : 1) * (CKPT / 16), tiles = (size + BL_TILE - 1) / BL_TILE;
    Banded packed((size_t)room_words);
    if (size == 0) memset(packed.body(), 0, (size_t)room_words * 4);  // (as the library does: the kernel is not launched)
    std::vector<int32_t> counts((size_t)tiles * BL_LISTS, -1);         // (a count the kernel does not store shows)
    std::vector<int64_t> bases((size_t)tiles * BL_LISTS + 1, 0);
    unsigned long long first_other = BL_NO_OTHER;
    if (tiles > 0)
        run_grid(BL_THREADS, (unsigned)tiles, [&] {
            bl_build_kernel<SRC, false>(src, size, vec, tiles, room_words, packed.body(), counts.data(), 1, &first_other, nullptr, nullptr, nullptr, nullptr,
                                        nullptr);
        });
    for (size_t k = 0; k < counts.size(); k++) {
        if (counts[k] < 0 || counts[k] > BL_TILE / 2) return false;
        bases[k + 1] = bases[k] + counts[k];
    }
    const int64_t n_blocks = bases[(size_t)tiles], m_blocks = bases[(size_t)(2 * tiles)] - n_blocks;
    if (bases[(size_t)(3 * tiles)] - bases[(size_t)(2 * tiles)] != n_blocks || bases[(size_t)(4 * tiles)] - bases[(size_t)(3 * tiles)] != m_blocks) return false;
    Banded n_start((size_t)n_blocks), n_end((size_t)n_blocks), m_start((size_t)m_blocks), m_end((size_t)m_blocks);
    if (n_blocks + m_blocks > 0)
        run_grid(BL_THREADS, (unsigned)tiles, [&] {
            bl_build_kernel<SRC, true>(src, size, vec, tiles, room_words, nullptr, counts.data(), 0, nullptr, bases.data(),
                                       reinterpret_cast<int32_t *>(n_start.body()), reinterpret_cast<int32_t *>(n_end.body()),
                                       reinterpret_cast<int32_t *>(m_start.body()), reinterpret_cast<int32_t *>(m_end.body()));
        });
    std::vector<int32_t> n_cum((size_t)n_blocks + 1, -1), m_cum((size_t)m_blocks + 1, -1);
    run_grid(BL_THREADS, (unsigned)((n_blocks + BL_THREADS) / BL_THREADS), [&] {
        bl_sizes_kernel(reinterpret_cast<int32_t *>(n_start.body()), reinterpret_cast<int32_t *>(n_end.body()), n_blocks, n_cum.data());
    });
    run_grid(BL_THREADS, (unsigned)((m_blocks + BL_THREADS) / BL_THREADS), [&] {
        bl_sizes_kernel(reinterpret_cast<int32_t *>(m_start.body()), reinterpret_cast<int32_t *>(m_end.body()), m_blocks, m_cum.data());
    });
    for (size_t i = 1; i < n_cum.size(); i++) n_cum[i] += n_cum[i - 1];
    for (size_t i = 1; i < m_cum.size(); i++) m_cum[i] += m_cum[i - 1];
    const int64_t head[3] = {n_blocks, m_blocks, (int64_t)first_other};
    return fwrite(head, 8, 3, out) == 3 && packed.write(out) && n_start.write(out) && n_end.write(out) && m_start.write(out) && m_end.write(out) &&
           fwrite(n_cum.data(), 4, n_cum.size(), out) == n_cum.size() && fwrite(m_cum.data(), 4, m_cum.size(), out) == m_cum.size();
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!f || !out) return 2;
    std::vector<int32_t> n_cases, head;
    std::vector<int64_t> wide;
    if (!read_n(f, n_cases, 1)) return 2;
    for (int k = 0; k < n_cases[0]; k++) {
        if (!read_n(f, head, 2) || !read_n(f, wide, 1)) return 2;
        const int src = head[0], misalign = head[1];
        const int64_t size = wide[0];
        const size_t bytes = (size_t)(src == BL_NIB ? (size + 1) / 2 : size);
        // the input in an allocation that ENDS with it (a read past it is a read past the allocation) and begins `misalign` bytes
        // before it: operator new[] aligns to 16 bytes
        std::vector<uint8_t> data;
        if (!read_n(f, data, bytes)) return 2;
        uint8_t *tight = new uint8_t[(size_t)misalign + bytes];
        uint8_t *at = tight + misalign;
        if (bytes) memcpy(at, data.data(), bytes);
        const int vec = (reinterpret_cast<uintptr_t>(at) & (src == BL_NIB ? 3 : 15)) == 0;
        const bool ok = src == BL_NIB ? run_case<BL_NIB>(at, size, vec, out) : run_case<BL_ASCII>(at, size, vec, out);
        delete[] tight;
        if (!ok) return 3;
    }
    fclose(f);
    fclose(out);
    printf("cases %d\n", n_cases[0]);
    puts("build kernel host ok");
    return 0;
}

// twobit_host.hpp -- what the host programs of the kernels over 2bit rows share (pwm_kernel_host, pwm_hits_kernel_host,
// kmer_kernel_host): what twobit.hpp uses that kernel_host.hpp lacks, a track as the IN files hold it, an output between guard bands.
// Include it after kernel_host.hpp and BEFORE the kernel headers.  (twobit_kernel_host keeps its own: its tracks hold the checkpoint
// tables and its stores are watched.)
#pragma once
#include <cstdlib>
#include <cstring>

struct int4 {
    int x, y, z, w;
};
static int4 load_int4(const int32_t *p)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) abort();  // (the device would fault)
    return int4{p[0], p[1], p[2], p[3]};
}
static std::atomic<bool> g_misaligned_vector_store{false};
static std::atomic<long> g_vector_stores{0};
static void store_int4(int32_t *p, int a, int b, int c, int d)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) g_misaligned_vector_store = true;
    g_vector_stores++;
    p[0] = a, p[1] = b, p[2] = c, p[3] = d;
}
static Dim gridDim;
static void host_wave_sum4(int v[4]) { (void)v; abort(); }  // (twobit.hpp's creation kernels, which these programs do not run)
#define TB_WAVE_SUM4(v) host_wave_sum4(v)

constexpr size_t GUARD = 64;
constexpr uint32_t GUARD_BITS = 0xEEEEEEEEu;

struct Track {
    int64_t size = 0, n_blocks = 0, m_blocks = 0;
    std::vector<uint32_t> packed;
    std::vector<int32_t> n_start, n_end, m_start, m_end;
};

static bool read_track(FILE *f, Track &t)
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
    t.n_end.resize(t.n_start.size());
    t.m_end.resize(t.m_start.size());
    for (size_t i = 0; i < t.n_start.size(); i++) t.n_end[i] = t.n_start[i] + n_size[i];
    for (size_t i = 0; i < t.m_start.size(); i++) t.m_end[i] = t.m_start[i] + m_size[i];
    return true;
}

// a vector of 32-bit words whose element `lead` is `misalign` words past a 16-byte boundary: [..][GUARD][cells][GUARD], ending there
struct Banded {
    std::vector<uint32_t> raw;
    size_t lead = 0, cells;
    explicit Banded(size_t cells_, int misalign = 0) : raw(8 + 2 * GUARD + cells_, GUARD_BITS), cells(cells_)
    {
        while ((reinterpret_cast<uintptr_t>(raw.data() + lead + GUARD) & 15) != 0) lead++;
        lead += misalign;
        raw.resize(lead + 2 * GUARD + cells);
    }
    uint32_t *body() { return raw.data() + lead + GUARD; }
    bool write(FILE *f) { return fwrite(raw.data() + lead, 4, 2 * GUARD + cells, f) == 2 * GUARD + cells; }
};

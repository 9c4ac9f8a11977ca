// zm_summary_kernel of bx-python_amd/csrc/zoom_summary.hpp run on the host, its text compiled as it stands (and summary.hpp's, for the
// search it shares) over kernel_host.hpp: a workgroup is 64 host threads that meet at a barrier where the kernel calls __syncthreads(), LDS is a static
// array, workgroups run one after another.  What this checks is everything in the kernel that is not the GPU's arithmetic: the run of
// leaves and of records a region loads, the front record of every bin, the chunks, which records a lane walks, the carried
// accumulators, every index (build it with -fsanitize=address,undefined).  Compile with -ffp-contract=off.
//
// usage: zoom_kernel_host IN OUT
//   IN:  int32 n_tracks, n, size; per track int32 records, leaves, then start[], end[] (int32), valid[] (uint32), min[], max[], sum[],
//        sumsq[] (float32), leaf_lo[], leaf_hi[] (int32), leaf_first[leaves + 1] (int64); then track_of[n], start[n], end[n] (int32)
//   OUT: five float64 planes [n, size]: valid, min, max, sum, sumsq
#include "kernel_host.hpp"
#include "summary.hpp"
#include "zoom_summary.hpp"
using namespace bxmi;

struct HostTrack {
    std::vector<int32_t> start, end, leaf_lo, leaf_hi;
    std::vector<uint32_t> valid;
    std::vector<float> mn, mx, sum, sumsq;
    std::vector<int64_t> leaf_first;
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    if (!read_n(f, head, 3)) return 2;
    const int n_tracks = head[0], n = head[1], size = head[2];
    std::vector<HostTrack> tracks(n_tracks);
    std::vector<ZmTrack> table(n_tracks + 1);
    for (int t = 0; t < n_tracks; t++) {
        std::vector<int32_t> m;
        HostTrack &h = tracks[t];
        if (!read_n(f, m, 2) || !read_n(f, h.start, m[0]) || !read_n(f, h.end, m[0]) || !read_n(f, h.valid, m[0]) || !read_n(f, h.mn, m[0]) ||
            !read_n(f, h.mx, m[0]) || !read_n(f, h.sum, m[0]) || !read_n(f, h.sumsq, m[0]) || !read_n(f, h.leaf_lo, m[1]) ||
            !read_n(f, h.leaf_hi, m[1]) || !read_n(f, h.leaf_first, (size_t)m[1] + 1))
            return 2;
        table[t] = ZmTrack{h.start.data(), h.end.data(), h.valid.data(), h.mn.data(), h.mx.data(), h.sum.data(), h.sumsq.data(),
                           h.leaf_lo.data(), h.leaf_hi.data(), h.leaf_first.data(), m[0], m[1]};
    }
    table[n_tracks] = ZmTrack{};
    std::vector<int32_t> track_of, start, end;
    if (!read_n(f, track_of, n) || !read_n(f, start, n) || !read_n(f, end, n)) return 2;
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f || !run_summary(zm_summary_kernel, table, track_of, start, end, size, f)) return 2;
    fclose(f);
    puts("zoom kernel host ok");
    return 0;
}

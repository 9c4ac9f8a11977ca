// sm_summary_kernel of bx-python_amd/csrc/summary.hpp run on the host, its text compiled as it stands over kernel_host.hpp: a workgroup is 64 host threads
// that meet at a barrier where the kernel calls __syncthreads(), LDS is a static array, workgroups run one after another.  What this
// checks is everything in the kernel that is not the GPU's arithmetic: the searches for a region's run, the chunks, which items a
// lane walks, the carried accumulators, every index (build it with -fsanitize=address,undefined).  Compile with -ffp-contract=off.
//
// usage: summary_kernel_host IN OUT
//   IN:  int32 n_tracks, n, size; per track int32 items, ordered, then start[], end[] (int32), value[] (float32);
//        then track_of[n], start[n], end[n] (int32)
//   OUT: five float64 planes [n, size]: valid, min, max, sum, sumsq
#include "kernel_host.hpp"
#include "summary.hpp"
using namespace bxmi;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    if (!read_n(f, head, 3)) return 2;
    const int n_tracks = head[0], n = head[1], size = head[2];
    std::vector<std::vector<int32_t>> st(n_tracks), en(n_tracks);
    std::vector<std::vector<float>> va(n_tracks);
    std::vector<SmTrack> table(n_tracks + 1);
    for (int t = 0; t < n_tracks; t++) {
        std::vector<int32_t> m;
        if (!read_n(f, m, 2) || !read_n(f, st[t], m[0]) || !read_n(f, en[t], m[0]) || !read_n(f, va[t], m[0])) return 2;
        table[t] = SmTrack{st[t].data(), en[t].data(), va[t].data(), m[0], m[1]};
    }
    table[n_tracks] = SmTrack{nullptr, nullptr, nullptr, 0, 1};
    std::vector<int32_t> track_of, start, end;
    if (!read_n(f, track_of, n) || !read_n(f, start, n) || !read_n(f, end, n)) return 2;
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f || !run_summary(sm_summary_kernel, table, track_of, start, end, size, f)) return 2;
    fclose(f);
    puts("summary kernel host ok");
    return 0;
}

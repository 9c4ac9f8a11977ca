// kernel_host.hpp -- a workgroup on the host, for the programs that compile a kernel header's text as it stands (summary_kernel_host,
// zoom_kernel_host, bed_summary_kernel_host, span_arrays_kernel_host): a workgroup is `threads` host threads that meet at a barrier
// where the kernel calls __syncthreads(), LDS is a static array, workgroups run one after another.  Include it BEFORE the kernel
// headers; build with -fsanitize=address,undefined so that every index is checked, and with -ffp-contract=off.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

struct Dim {
    unsigned x;
};
static thread_local Dim threadIdx;
static thread_local Dim blockIdx;

class Barrier {
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0;
    unsigned long generation = 0;

  public:
    int count = 0;  // the workgroup's threads: run_grid sets it while none is running
    void wait()
    {
        std::unique_lock<std::mutex> lock(m);
        const unsigned long g = generation;
        if (++waiting == count) {
            waiting = 0;
            generation++;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != g; });
        }
    }
};
static Barrier g_barrier;
static void __syncthreads() { g_barrier.wait(); }

// __ballot for a workgroup of up to 64 threads: everyone votes into the slot of this call, meets at the barrier and reads it.  Three
// slots in turn: the one cleared after call k's barrier was read for the last time before it and is voted into only after call k + 1's.
static std::atomic<unsigned long long> g_votes[3];
static thread_local unsigned long g_ballots = 0;
static unsigned long long host_ballot(bool p)
{
    const unsigned long k = g_ballots++;
    if (p) g_votes[k % 3].fetch_or(1ull << threadIdx.x);
    g_barrier.wait();
    const unsigned long long all = g_votes[k % 3].load();
    if (threadIdx.x == 0) g_votes[(k + 2) % 3].store(0);
    return all;
}
#define BD_BALLOT(p) host_ballot(p)

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
#define __shared__ static
#define BX_GLOBAL
template <typename T>
T *as_global(T *p)
{
    return p;
}

template <typename T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// body() in every thread of every workgroup of a grid, threadIdx.x and blockIdx.x set; the workgroups one after another
template <typename Body>
static void run_grid(int threads, unsigned blocks, Body body)
{
    g_barrier.count = threads;
    for (auto &v : g_votes) v.store(0);
    std::vector<std::thread> lanes;
    for (int lane = 0; lane < threads; lane++)
        lanes.emplace_back([&, lane] {
            threadIdx.x = lane;
            for (unsigned b = 0; b < blocks; b++) {
                blockIdx.x = b;
                body();
                g_barrier.wait();  // the next workgroup reuses the LDS
            }
        });
    for (auto &t : lanes) t.join();
}

// What the three summary kernels have in common: one workgroup of 64 per row, five float64 planes [n, size] (valid, min, max, sum,
// sumsq), which are appended to `f`.
template <typename Kernel, typename Entry>
static bool run_summary(Kernel kernel, const std::vector<Entry> &table, const std::vector<int32_t> &track_of, const std::vector<int32_t> &start,
                        const std::vector<int32_t> &end, int size, FILE *f)
{
    const size_t n = track_of.size();
    std::vector<double> out[5];
    for (auto &o : out) o.assign(n * size, -777.0);  // (a cell the kernel does not write shows)
    run_grid(64, (unsigned)n, [&] {
        kernel(table.data(), (int)table.size() - 1, track_of.data(), start.data(), end.data(), size, out[0].data(), out[1].data(), out[2].data(),
               out[3].data(), out[4].data());
    });
    for (auto &o : out)
        if (fwrite(o.data(), sizeof(double), o.size(), f) != o.size()) return false;
    return true;
}

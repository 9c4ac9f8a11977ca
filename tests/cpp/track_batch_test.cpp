// CPU check of the plain C++ half of bx-python_amd/csrc/track_batch.hpp (compiled by tests/test_host_logic.py with g++ under the
// address and undefined-behaviour sanitizers): the walk that fills a track table pack by pack -- which slots it writes, with
// what, in how many packs, and that it stops on an error -- and the argument checks of the track-batch entry points: their
// texts and their order.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "track_batch.hpp"

using namespace bxmi;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// the library's fail() (core.hip) keeps the text for bxmi_last_error and returns the code; so does this one
static std::string g_error;
int bxmi::fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

struct Two {  // the shape of a profile's entry: a pointer and a size
    const float *values;
    int64_t size;
    bool operator==(const Two &o) const { return values == o.values && size == o.size; }
};
struct Five {  // the shape of a summary's entry
    const int32_t *start, *end;
    const float *value;
    int64_t n, ordered;
    bool operator==(const Five &o) const { return start == o.start && end == o.end && value == o.value && n == o.n && ordered == o.ordered; }
};

static const float F[4] = {0, 0, 0, 0};
static const int32_t I[4] = {0, 0, 0, 0};
static Two two(int k) { return Two{F + (k & 3), 1000 + k}; }
static Five five(int k) { return Five{I + (k & 3), I + ((k + 1) & 3), F + (k & 3), 1000 + k, k & 1}; }

template <typename Entry, int P, typename Make>
static void walk(Make make, const Entry &spare, const Entry &poison)
{
    const int guard = 2 * P;
    for (int n_tracks : {0, 1, P - 1, P, P + 1, 2 * P + 1}) {
        std::vector<Entry> table((size_t)(n_tracks + 1 + guard), poison);
        int calls = 0, next = 0;
        const int rc = for_each_track_pack<Entry, P>(n_tracks, make, spare, [&](int base, int count, const TrackPack<Entry, P> &pack) {
            CHECK(base == next && count >= 1 && count <= P && base + count <= n_tracks + 1);
            for (int k = 0; k < count; k++) table[(size_t)(base + k)] = pack.t[k];
            next = base + count;
            calls++;
            return 0;
        });
        CHECK(rc == 0 && next == n_tracks + 1);
        CHECK(calls == n_tracks / P + 1);
        for (int k = 0; k < n_tracks; k++) CHECK(table[(size_t)k] == make(k));
        CHECK(table[(size_t)n_tracks] == spare);
        for (int k = n_tracks + 1; k < n_tracks + 1 + guard; k++) CHECK(table[(size_t)k] == poison);
        // a status from put ends the walk and is what the walk returns
        for (int fail_at = 0; fail_at < n_tracks / P + 1; fail_at++) {
            calls = 0;
            const int got = for_each_track_pack<Entry, P>(n_tracks, make, spare, [&](int, int, const TrackPack<Entry, P> &) { return calls++ == fail_at ? 7 : 0; });
            CHECK(got == 7 && calls == fail_at + 1);
        }
    }
}

static void checks()
{
    int a = 0, b = 0;
    int *good[3] = {&a, &b, &a}, *holes[3] = {&a, nullptr, nullptr};
    int **none = nullptr;
    const char *who = "bxmi_x";
    CHECK(track_batch_check(who, "width", 1, good, 3, 0) == BXMI_OK);
    CHECK(track_batch_check(who, "size", 2147483647, none, 0, 2147483647LL) == BXMI_OK);
    g_error.clear();
    // each refusal and its text; every case is also bad in everything checked LATER, so the text shows the order
    CHECK(track_batch_check(who, "width", 0, none, -1, -1) == BXMI_EINVAL && g_error == "bxmi_x: width = 0, must be at least 1");
    CHECK(track_batch_check(who, "size", -3, none, -1, -1) == BXMI_EINVAL && g_error == "bxmi_x: size = -3, must be at least 1");
    CHECK(track_batch_check(who, "size", 1, none, -1, -1) == BXMI_EINVAL && g_error == "bxmi_x: n = -1 outside [0, 2^31-1]");
    CHECK(track_batch_check(who, "size", 1, none, -1, 2147483648LL) == BXMI_EINVAL && g_error == "bxmi_x: n = 2147483648 outside [0, 2^31-1]");
    CHECK(track_batch_check(who, "size", 1, none, -2, 5) == BXMI_EINVAL && g_error == "bxmi_x: n_tracks = -2 is negative");
    CHECK(track_batch_check(who, "size", 1, none, 3, 5) == BXMI_EINVAL && g_error == "bxmi_x: NULL track list");
    CHECK(track_batch_check(who, "size", 1, holes, 3, 5) == BXMI_EINVAL && g_error == "bxmi_x: track 1 is a NULL handle");
    CHECK(track_batch_check(who, "size", 1, holes, 1, 5) == BXMI_OK);

    const int32_t rows[5] = {-1, 2, -2147483647 - 1, 3, 4};
    g_error.clear();
    CHECK(track_of_check(who, rows, 3, 3) == BXMI_OK && g_error.empty());  // negative: no track, legal
    CHECK(track_of_check(who, rows, 0, 0) == BXMI_OK && track_of_check(who, nullptr, 0, 0) == BXMI_OK);
    CHECK(track_of_check(who, rows, 5, 3) == BXMI_EINVAL && g_error == "bxmi_x: track_of[3] = 3, but there are 3 tracks");
    CHECK(track_of_check(who, rows, 5, 0) == BXMI_EINVAL && g_error == "bxmi_x: track_of[1] = 2, but there are 0 tracks");
}

int main()
{
    walk<Two, 16>(two, Two{F + 3, 0}, Two{nullptr, -77});
    walk<Five, 8>(five, Five{nullptr, nullptr, nullptr, 0, 1}, Five{I + 3, I + 3, F + 3, -77, -77});
    checks();
    std::printf("track batch ok\n");
    return 0;
}

// The host-only plan of the post-processing stream (ls_post_stream_plan, ls_post_stream_check; livelyspeaker_amd/csrc/ls_post_stream_plan.cpp)
// on its edges.  A stand-alone program: it links that unit alone, is built with the host sanitizers by tests/test_post_stream_host.py, and
// exits non-zero on a wrong answer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the entries of a series of N frames: [0, N) for TED, [0, N - 1) for BEAT
static int64_t entries(int dataset, int64_t N) { return dataset == 0 ? N : (N > 0 ? N - 1 : 0); }

// feed N frames in chunks of `chunk`, finish with the last chunk or with a push of its own: the ranges tile the entries once, in order
static void test_tiling(int dataset, int order, int64_t N, int64_t chunk, bool finish_alone) {
    int64_t n = 0, next = 0;
    while (n < N) {
        const int64_t k = chunk < N - n ? chunk : N - n;
        const bool last = n + k == N && !finish_alone;
        int64_t first = -7;
        int32_t count = -7;
        CHECK(ls_post_stream_plan(dataset, order, n, k, last, &first, &count) == LS_OK);
        CHECK(first == next && count >= 0);
        next = first + count;
        n += k;
        if (!last) CHECK(next == (dataset == 0 ? (n > 0 ? n - 1 : 0) : (n - order - 1 > 0 ? n - order - 1 : 0)));
    }
    if (finish_alone) {
        int64_t first = -7;
        int32_t count = -7;
        CHECK(ls_post_stream_plan(dataset, order, N, 0, 1, &first, &count) == LS_OK);
        CHECK(first == next);
        CHECK(count <= (dataset == 0 ? 1 : order));
        next = first + count;
    }
    CHECK(next == entries(dataset, N));
}

static void test_plan_refusals() {
    int64_t first = 0;
    int32_t count = 0;
    CHECK(ls_post_stream_plan(2, 1, 0, 1, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(-1, 1, 0, 1, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(1, 0, 0, 1, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(1, LS_POST_STREAM_MAX_ORDER + 1, 0, 1, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(0, 0, 0, 1, 0, &first, &count) == LS_OK);                  // TED has no order
    CHECK(ls_post_stream_plan(0, 1, -1, 1, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(0, 1, 0, -1, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(0, 1, 0, 0, 1, &first, &count) == LS_EINVAL);              // finishing a series without a frame
    CHECK(ls_post_stream_plan(0, 1, 0, 1, 0, nullptr, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(0, 1, 0, 1, 0, &first, nullptr) == LS_EINVAL);
    CHECK(ls_post_stream_plan(0, 1, INT64_MAX, 1, 0, &first, &count) == LS_EINVAL);      // the sum at its guard
    CHECK(ls_post_stream_plan(0, 1, 1, INT64_MAX, 0, &first, &count) == LS_EINVAL);
    CHECK(ls_post_stream_plan(0, 1, 0, (int64_t)1 << 40, 0, &first, &count) == LS_EINVAL);      // more entries than an int32 holds
    CHECK(ls_post_stream_plan(1, 8, ((int64_t)1 << 62) - 5, 5, 1, &first, &count) == LS_OK && count == 5 + 8);
}

static void test_check() {
    const std::vector<int64_t> n{0, 10, 3};
    std::vector<int32_t> k{4, 0, 256}, fin{0, 1, 0};
    std::vector<int64_t> first(3, -7);
    std::vector<int32_t> count(3, -7);
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, k.data(), fin.data(), 256, first.data(), count.data()) == LS_OK);
    CHECK((first == std::vector<int64_t>{0, 9, 2}) && (count == std::vector<int32_t>{3, 1, 256}));
    CHECK(ls_post_stream_check(1, 2, 3, n.data(), 256, k.data(), fin.data(), 256, first.data(), count.data()) == LS_OK);
    CHECK((first == std::vector<int64_t>{0, 7, 0}) && (count == std::vector<int32_t>{1, 2, 256}));
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, k.data(), nullptr, 256, nullptr, nullptr) == LS_OK);
    // the refusals, each ahead of the outputs
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, k.data(), fin.data(), 255, nullptr, nullptr) == LS_EINVAL);      // beat_capacity too small
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 257, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);      // a chunk over the cap
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 255, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);      // counts[s] > K
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, nullptr, fin.data(), 512, nullptr, nullptr) == LS_EINVAL);
    CHECK(ls_post_stream_check(0, 1, 3, nullptr, 256, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);
    CHECK(ls_post_stream_check(0, 1, 0, n.data(), 256, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);
    CHECK(ls_post_stream_check(1, 9, 3, n.data(), 256, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);      // order outside 1..8
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), -1, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);
    k[1] = -1;
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, k.data(), fin.data(), 512, nullptr, nullptr) == LS_EINVAL);      // a negative count
    k = {0, 0, 1};
    fin = {1, 0, 0};
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, k.data(), fin.data(), 512, nullptr, nullptr) == LS_ESTATE);      // finish on a slot with no frames
    k[0] = 1;                                                                                                          // ... one frame is enough
    CHECK(ls_post_stream_check(0, 1, 3, n.data(), 256, k.data(), fin.data(), 512, first.data(), count.data()) == LS_OK && count[0] == 1);
}

int main() {
    const int orders[] = {1, 2, 3, 4, 8};
    for (int64_t N = 1; N <= 40; ++N)
        for (int64_t chunk : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, N})
            for (int alone = 0; alone < 2; ++alone) {
                test_tiling(0, 1, N, chunk, alone != 0);
                for (int order : orders) test_tiling(1, order, N, chunk, alone != 0);
            }
    test_plan_refusals();
    test_check();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

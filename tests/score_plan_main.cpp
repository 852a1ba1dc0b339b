// The host-only plan of the score stream (ls_score_stream_plan, livelyspeaker_amd/csrc/ls_score_plan.cpp) on its edges.  A stand-alone
// program: it links that unit alone, is built with the host sanitizers by tests/test_score_stream_host.py, and exits non-zero on a wrong
// answer.
#include <cstdint>
#include <cstdio>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int64_t kMost = 2147483647LL - 2047;      // 2^31 - 2048

struct Range {
    int rc;
    int64_t first;
    int32_t count;
};

static Range plan(int32_t pad, int64_t before, int64_t fresh, int32_t finishing) {
    Range r{0, -7, -7};
    r.rc = ls_score_stream_plan(pad, before, fresh, finishing, &r.first, &r.count);
    return r;
}

// a series of L samples fed `step` at a time, then finished: the ranges tile [0, 1 + L / 512) in order, and no frame comes early
static void feed(int32_t pad, int64_t L, int64_t step) {
    int64_t n = 0, next = 0;
    while (n < L) {
        const int64_t k = step < L - n ? step : L - n;
        const Range r = plan(pad, n, k, 0);
        CHECK(r.rc == LS_OK && r.first == next && r.count >= 0);
        n += k;
        next += r.count;
        if (r.count) {
            const int64_t last = next - 1;
            CHECK(n >= 512 * last + 1024 && (pad == LS_ONSETS_PAD_CONSTANT || n >= 1025));
        }
        CHECK(n < 512 * next + 1024 || (pad == LS_ONSETS_PAD_REFLECT && n < 1025));      // and none is late
    }
    const Range r = plan(pad, L, 0, 1);
    if (pad == LS_ONSETS_PAD_REFLECT && L <= 1024) {
        CHECK(r.rc == LS_EINVAL);
        return;
    }
    CHECK(r.rc == LS_OK && r.first == next && r.first + r.count == 1 + L / 512);
}

static void test_tiling() {
    const int64_t lengths[] = {1, 511, 512, 1023, 1024, 1025, 1536, 2047, 2048, 36267, 2103486};
    const int64_t steps[] = {1, 511, 512, 513, 1024, 1025, 4096, 1 << 22};
    for (int32_t pad = 0; pad < 2; ++pad)
        for (int64_t L : lengths)
            for (int64_t step : steps)
                if (L / step < 5000) feed(pad, L, step);
    // the edges by name
    CHECK(plan(0, 0, 1023, 0).count == 0 && plan(0, 0, 1024, 0).count == 1 && plan(1, 0, 1024, 0).count == 0 && plan(1, 0, 1025, 0).count == 1);
    CHECK(plan(0, 1024, 511, 0).count == 0 && plan(0, 1024, 512, 0).count == 1 && plan(0, 1024, 512, 0).first == 1);
    CHECK(plan(0, 0, 1, 1).count == 1 && plan(0, 0, 512, 1).count == 2 && plan(0, 36267, 0, 1).first == 69 && plan(0, 36267, 0, 1).count == 2);
    // one call that feeds and finishes
    CHECK(plan(1, 1000, 25, 1).rc == LS_OK && plan(1, 1000, 25, 1).first == 0 && plan(1, 1000, 25, 1).count == 3);
}

static void test_refusals() {
    int64_t first = 0;
    int32_t count = 0;
    CHECK(ls_score_stream_plan(0, 0, 1024, 0, nullptr, &count) == LS_EINVAL);
    CHECK(ls_score_stream_plan(0, 0, 1024, 0, &first, nullptr) == LS_EINVAL);
    CHECK(plan(2, 0, 1024, 0).rc == LS_EINVAL && plan(-1, 0, 1024, 0).rc == LS_EINVAL);
    CHECK(plan(0, -1, 1024, 0).rc == LS_EINVAL && plan(0, 0, -1, 0).rc == LS_EINVAL);
    CHECK(plan(0, kMost, 0, 0).rc == LS_OK && plan(0, kMost, 1, 0).rc == LS_EINVAL && plan(0, 0, kMost + 1, 0).rc == LS_EINVAL);
    CHECK(plan(0, INT64_MAX, INT64_MAX, 0).rc == LS_EINVAL && plan(0, 1, INT64_MAX, 0).rc == LS_EINVAL);
    CHECK(plan(0, kMost, 0, 1).rc == LS_OK && plan(0, kMost, 0, 1).first + plan(0, kMost, 0, 1).count == 4194301);
    CHECK(plan(0, 0, 0, 1).rc == LS_EINVAL && plan(1, 0, 0, 1).rc == LS_EINVAL);        // finishing an empty series
    CHECK(plan(0, 0, 0, 0).rc == LS_OK && plan(0, 0, 0, 0).count == 0);                 // an empty push is no error
    CHECK(plan(1, 1024, 0, 1).rc == LS_EINVAL && plan(1, 1000, 24, 1).rc == LS_EINVAL && plan(1, 1025, 0, 1).rc == LS_OK);
    CHECK(plan(0, 1024, 0, 1).rc == LS_OK);
}

int main() {
    test_tiling();
    test_refusals();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

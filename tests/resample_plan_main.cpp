// The host-only half of the resampler (ls_resample_ratio, ls_resample_plan, ls_resample_taps,
// livelyspeaker_amd/csrc/ls_resample_plan.cpp) on its edges.  A stand-alone program: it links that unit alone, is built with the host
// sanitizers by tests/test_resample_host.py, and exits non-zero on a wrong answer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int64_t kMost = 1LL << 62;

struct Ratio {
    int rc;
    int64_t up, down, half, T, carry, n_taps;
};

static Ratio ratio(int32_t in_sr, int32_t out_sr, int32_t zeros) {
    Ratio r{0, -7, -7, -7, -7, -7, -7};
    r.rc = ls_resample_ratio(in_sr, out_sr, zeros, &r.up, &r.down, &r.half, &r.T, &r.carry, &r.n_taps);
    return r;
}

struct Range {
    int rc;
    int64_t first, count;
};

static Range plan(const Ratio& q, int64_t before, int64_t fresh, int32_t finishing) {
    Range r{0, -7, -7};
    r.rc = ls_resample_plan(q.up, q.down, q.half, before, fresh, finishing, &r.first, &r.count);
    return r;
}

static int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }
static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// a series of L samples fed `step` at a time (with an empty push after every one), then finished: the ranges tile [0, ceil(L up / down))
// in order; an emitted output has every sample it reads, and reads none further back than carry_len before the push
static void feed(const Ratio& q, int64_t L, int64_t step) {
    int64_t n = 0, next = 0;
    auto reads = [&](const Range& r, int64_t before, int64_t total, bool finishing) {
        if (!r.count) return;
        const int64_t m_lo = r.first, m_hi = r.first + r.count - 1;
        const int64_t k_lo = ceil_div(m_lo * q.down - q.half, q.up), k_hi = floor_div(m_hi * q.down + q.half, q.up);
        if (!finishing) CHECK(k_hi <= total - 1);                           // everything it reads is there
        CHECK(k_lo < 0 || k_lo >= before - q.carry);                       // the carry bound
        CHECK(k_lo < 0 || before - k_lo <= q.T - 1);        // and the sharper one the kernels' rows rely on
    };
    while (n < L) {
        const int64_t k = step < L - n ? step : L - n;
        const Range r = plan(q, n, k, 0);
        CHECK(r.rc == LS_OK && r.first == next && r.count >= 0);
        reads(r, n, n + k, false);
        n += k;
        next += r.count;
        CHECK(next <= ceil_div(n * q.up, q.down));
        CHECK(floor_div(next * q.down + q.half, q.up) >= n);               // none is late: output `next` still misses a sample
        const Range e = plan(q, n, 0, 0);
        CHECK(e.rc == LS_OK && e.first == next && e.count == 0);
    }
    const Range r = plan(q, L, 0, 1);                                       // a finish with no new sample
    if (L < 1) {
        CHECK(r.rc == LS_EINVAL);
        return;
    }
    CHECK(r.rc == LS_OK && r.first == next && r.first + r.count == ceil_div(L * q.up, q.down));
    reads(r, L, L, true);
}

static void test_tiling() {
    const int32_t rates[] = {48000, 44100, 22050, 8000, 11025, 16000, 96000, 12345};
    const int32_t zeros[] = {1, 4, 32};
    const int64_t lengths[] = {0, 1, 2, 3, 97, 700, 701, 2999, 6000};
    const int64_t steps[] = {1, 2, 7, 700, 701, 1500, 1 << 20};
    for (int32_t sr : rates)
        for (int32_t z : zeros) {
            const Ratio q = ratio(sr, 16000, z);
            CHECK(q.rc == LS_OK && q.n_taps == 2 * q.half + 1 && q.T == 2 * q.half / q.up + 1 && q.carry == ceil_div(2 * q.half + q.down, q.up) + 1);
            for (int64_t L : lengths)                                       // half is larger than the shorter series
                for (int64_t step : steps)
                    if (step == 1 ? L <= 701 : true) feed(q, L, step);
        }
    // the edges by name: 48 kHz, 32 zeros (up 1, down 3, half 96)
    const Ratio q = ratio(48000, 16000, 32);
    CHECK(q.up == 1 && q.down == 3 && q.half == 96 && q.T == 193 && q.carry == 196 && q.n_taps == 193);
    CHECK(plan(q, 0, 0, 0).rc == LS_OK && plan(q, 0, 0, 0).count == 0);     // an empty push is no error
    CHECK(plan(q, 0, 96, 0).count == 0 && plan(q, 0, 97, 0).count == 1 && plan(q, 0, 99, 0).count == 1 && plan(q, 0, 100, 0).count == 2);
    CHECK(plan(q, 0, 1, 1).count == 1 && plan(q, 0, 3, 1).count == 1 && plan(q, 0, 4, 1).count == 2);
    CHECK(plan(q, 3000, 0, 1).first == 968 && plan(q, 3000, 0, 1).count == 32);
    // a pass-through plans with half = 0: every sample at once
    const Ratio one{0, 1, 1, 0, 1, 0, 1};
    CHECK(plan(one, 0, 5, 0).count == 5 && plan(one, 5, 2, 0).first == 5 && plan(one, 7, 0, 1).count == 0);
}

static void test_large_counts() {
    const Ratio q{0, 1, 3, 96, 193, 196, 193};
    CHECK(plan(q, kMost, 0, 0).rc == LS_OK && plan(q, kMost, 0, 0).first == (kMost - 97) / 3 + 1);
    CHECK(plan(q, kMost - 5, 5, 1).rc == LS_OK && plan(q, kMost - 5, 5, 1).first + plan(q, kMost - 5, 5, 1).count == (kMost + 2) / 3);
    CHECK(plan(q, kMost, 1, 0).rc == LS_EINVAL && plan(q, kMost + 1, 0, 0).rc == LS_EINVAL && plan(q, 1, kMost, 0).rc == LS_EINVAL);
    CHECK(plan(q, INT64_MAX, INT64_MAX, 0).rc == LS_EINVAL && plan(q, 1, INT64_MAX, 0).rc == LS_EINVAL && plan(q, INT64_MAX, 0, 1).rc == LS_EINVAL);
    const Ratio u{0, 160, 441, 14112, 177, 180, 28225};                     // N up must stay at or below 2^62
    CHECK(plan(u, kMost / 160, 0, 0).rc == LS_OK && plan(u, kMost / 160 + 1, 0, 0).rc == LS_EINVAL && plan(u, kMost / 160, 1, 1).rc == LS_EINVAL);
    const Ratio big{0, kMost, kMost, kMost, 0, 0, 0};
    CHECK(plan(big, 1, 0, 0).rc == LS_OK && plan(big, 1, 0, 0).count == 0 && plan(big, 1, 0, 1).count == 1 && plan(big, 1, 1, 0).rc == LS_EINVAL);
    const Ratio over{0, kMost + 1, 1, 0, 0, 0, 0};
    CHECK(plan(over, 0, 0, 0).rc == LS_EINVAL);
}

static void test_refusals() {
    const Ratio q{0, 1, 3, 96, 193, 196, 193};
    int64_t a = 0, b = 0;
    CHECK(ls_resample_plan(1, 3, 96, 0, 5, 0, nullptr, &b) == LS_EINVAL && ls_resample_plan(1, 3, 96, 0, 5, 0, &a, nullptr) == LS_EINVAL);
    CHECK(ls_resample_plan(0, 3, 96, 0, 5, 0, &a, &b) == LS_EINVAL && ls_resample_plan(1, 0, 96, 0, 5, 0, &a, &b) == LS_EINVAL);
    CHECK(ls_resample_plan(1, 3, -1, 0, 5, 0, &a, &b) == LS_EINVAL);
    CHECK(plan(q, -1, 5, 0).rc == LS_EINVAL && plan(q, 5, -1, 0).rc == LS_EINVAL);
    CHECK(plan(q, 0, 0, 1).rc == LS_EINVAL && plan(q, 0, 1, 1).rc == LS_OK && plan(q, 1, 0, 1).rc == LS_OK);      // a finish needs a sample
    CHECK(ratio(0, 16000, 32).rc == LS_EINVAL && ratio(48000, 0, 32).rc == LS_EINVAL && ratio(48000, 16000, 0).rc == LS_EINVAL);
    CHECK(ratio(-1, 16000, 32).rc == LS_EINVAL);
    int64_t v[6];
    for (int hole = 0; hole < 6; ++hole) {
        int64_t* p[6] = {&v[0], &v[1], &v[2], &v[3], &v[4], &v[5]};
        p[hole] = nullptr;
        CHECK(ls_resample_ratio(48000, 16000, 32, p[0], p[1], p[2], p[3], p[4], p[5]) == LS_EINVAL);
    }
    CHECK(ratio(65535, 1, 32).rc == LS_OK && ratio(65535, 1, 32).n_taps == 2LL * 32 * 65535 + 1);
    CHECK(ratio(65536, 1, 32).rc == LS_EUNSUPPORTED && ratio(1, 65536, 32).rc == LS_EUNSUPPORTED);
    CHECK(ratio(2147483647, 2147483646, 2147483647).rc == LS_EUNSUPPORTED);
    double h64[9];
    float h32[9];
    CHECK(ls_resample_taps(1, 1, 4, 12.0, 0.95, nullptr, nullptr) == LS_EINVAL);
    CHECK(ls_resample_taps(0, 1, 4, 12.0, 0.95, h64, h32) == LS_EINVAL && ls_resample_taps(1, 0, 4, 12.0, 0.95, h64, h32) == LS_EINVAL);
    CHECK(ls_resample_taps(1, 1, 0, 12.0, 0.95, h64, h32) == LS_EINVAL && ls_resample_taps(1, 1, 4, -1.0, 0.95, h64, h32) == LS_EINVAL);
    CHECK(ls_resample_taps(1, 1, 4, 12.0, 0.0, h64, h32) == LS_EINVAL && ls_resample_taps(1, 1, 4, 12.0, 1.5, h64, h32) == LS_EINVAL);
    CHECK(ls_resample_taps(1, 1, 4, NAN, 0.95, h64, h32) == LS_EINVAL && ls_resample_taps(1, 1, 4, 12.0, NAN, h64, h32) == LS_EINVAL);
    CHECK(ls_resample_taps(1, 65536, 32, 12.0, 0.95, h64, h32) == LS_EUNSUPPORTED);
}

static void test_taps() {
    double h64[9];
    float h32[9];
    CHECK(ls_resample_taps(1, 1, 4, 12.0, 1.0, h64, h32) == LS_OK);         // rolloff 1, up == down: the identity but for rounding
    for (int i = 0; i < 9; ++i) CHECK(std::fabs(h64[i] - (i == 4 ? 1.0 : 0.0)) < 1e-15 && h32[i] == (float)h64[i]);
    const Ratio q = ratio(44100, 16000, 4);
    std::vector<double> a((size_t)q.n_taps);
    std::vector<float> f((size_t)q.n_taps);
    CHECK(ls_resample_taps(q.up, q.down, 4, 12.0, 0.95, a.data(), nullptr) == LS_OK && ls_resample_taps(q.up, q.down, 4, 12.0, 0.95, nullptr, f.data()) == LS_OK);
    double sum = 0.0;
    for (int64_t i = 0; i < q.n_taps; ++i) {
        CHECK(std::fabs(a[(size_t)i] - a[(size_t)(q.n_taps - 1 - i)]) <= 1e-15 && f[(size_t)i] == (float)a[(size_t)i]);      // symmetric
        sum += a[(size_t)i];
    }
    CHECK(std::fabs(sum / (double)q.up - 1.0) < 1e-3);                      // 4 zeros: a coarse filter, still unit gain at DC
    CHECK(a[0] == 0.0 || std::fabs(a[0]) < 1e-6);
}

int main() {
    test_tiling();
    test_large_counts();
    test_refusals();
    test_taps();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

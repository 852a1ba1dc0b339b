// The host-only plans of the chained-window engine (livelyspeaker_amd/csrc/ls_chain_plan.cpp) on their edges.  A stand-alone program:
// it links that unit alone, is built with the host sanitizers by tests/test_chain_plan_host.py, and exits non-zero on a wrong answer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int64_t S = LS_LONG_AUDIO_STRIDE;
static const int32_t AL = 36267;        // the TED model's audio_len; any value >= 1 would do

// ls_long_stream_plan at one call; -1, -1 when it refuses
struct Plan { int64_t first, n; };
static Plan stream(int64_t before, int64_t fresh, int closing, int32_t audio_len = AL) {
    Plan p{-7, -7};
    if (ls_long_stream_plan(before, fresh, audio_len, closing, &p.first, &p.n) != LS_OK) return {-1, -1};
    return p;
}

static void test_stream_plan() {
    // total samples -> windows complete / windows a closing call owes in all
    const int64_t k = 3;
    const struct { int64_t total, complete, closing; } rows[] = {
        {1, 0, 1}, {AL - 1, 0, 1}, {AL, 1, 1}, {AL + 1, 1, 2}, {AL + S * k - 1, k, k + 1}, {AL + S * k, k + 1, k + 1}, {AL + S * k + 1, k + 1, k + 2}};
    for (const auto& r : rows) {
        Plan p = stream(0, r.total, 0);
        CHECK(p.first == 0 && p.n == r.complete);
        p = stream(0, r.total, 1);
        CHECK(p.first == 0 && p.n == r.closing);
        p = stream(r.total, 0, 1);                      // everything fed before: the closing call runs the difference
        CHECK(p.first == r.complete && p.n == r.closing - r.complete);
        p = stream(r.total - 1, 1, 0);                  // the last sample alone
        CHECK(p.first + p.n == r.complete);
    }
    // the sum at its guard
    Plan p = stream(INT64_MAX - 5, 5, 0);
    const int64_t all = (INT64_MAX - AL) / S + 1;
    CHECK(p.first == (INT64_MAX - 5 - AL) / S + 1 && p.first + p.n == all);
    p = stream(INT64_MAX - 5, 5, 1);
    CHECK(p.first + p.n == all + ((INT64_MAX - AL) % S ? 1 : 0));
    p = stream(INT64_MAX - 5, 5, 1, 1);                 // audio_len 1: the rounding of the closing count must not pass INT64_MAX
    CHECK(p.first + p.n == (INT64_MAX - 2) / S + 2);
    CHECK(stream(INT64_MAX - 5, 6, 0).first == -1);
    CHECK(stream(INT64_MAX, 1, 1).first == -1);
    CHECK(stream(INT64_MAX, 0, 0).first == (INT64_MAX - AL) / S + 1);
    // refusals
    CHECK(stream(-1, 0, 0).first == -1 && stream(0, -1, 0).first == -1 && stream(0, 1, 0, 0).first == -1);
    CHECK(stream(0, 0, 1).first == -1);                 // a closed stream without a sample
    CHECK(stream(0, 0, 0).first == 0 && stream(0, 0, 0).n == 0);
    int64_t a = 0, b = 0;
    CHECK(ls_long_stream_plan(0, 1, AL, 0, nullptr, &b) == LS_EINVAL && ls_long_stream_plan(0, 1, AL, 0, &a, nullptr) == LS_EINVAL);
}

static void test_plan_drop() {
    const int64_t k = 2;
    const std::vector<int64_t> lens = {1, AL + S * k + 1, AL, AL + S * k, AL + 1, AL + S * k};      // windows 1, k + 2, 1, k + 1, 2, k + 1
    const int B = (int)lens.size();
    std::vector<int32_t> row(B, -1), wins(B, -1), active(8, -1);
    int32_t W = -1;
    CHECK(ls_long_plan_drop(B, AL, lens.data(), row.data(), wins.data(), active.data(), 8, &W) == LS_OK);
    CHECK(W == k + 2);
    const int32_t want_row[] = {1, 3, 5, 4, 0, 2}, want_wins[] = {4, 3, 3, 2, 1, 1}, want_active[] = {6, 4, 3, 1};     // longest first, ties in the caller's order
    for (int s = 0; s < B; ++s) CHECK(row[s] == want_row[s] && wins[s] == want_wins[s]);
    for (int w = 0; w < 4; ++w) CHECK(active[w] == want_active[w]);
    CHECK(active[4] == -1);
    // every output but the count is optional; a short `active` takes what fits
    W = -1;
    CHECK(ls_long_plan_drop(B, AL, lens.data(), nullptr, nullptr, nullptr, 0, &W) == LS_OK && W == 4);
    std::vector<int32_t> two(2, -1);
    CHECK(ls_long_plan_drop(B, AL, lens.data(), nullptr, nullptr, two.data(), 2, &W) == LS_OK && two[0] == 6 && two[1] == 4);
    CHECK(ls_long_plan_drop(B, AL, lens.data(), nullptr, nullptr, nullptr, 2, &W) == LS_EINVAL);
    CHECK(ls_long_plan_drop(B, AL, lens.data(), nullptr, nullptr, two.data(), -1, &W) == LS_EINVAL);
    CHECK(ls_long_plan_drop(B, AL, lens.data(), nullptr, nullptr, nullptr, 0, nullptr) == LS_EINVAL);
    CHECK(ls_long_plan_drop(B, AL, nullptr, nullptr, nullptr, nullptr, 0, &W) == LS_EINVAL);
    CHECK(ls_long_plan_drop(0, AL, lens.data(), nullptr, nullptr, nullptr, 0, &W) == LS_EINVAL);
    CHECK(ls_long_plan_drop(B, 0, lens.data(), nullptr, nullptr, nullptr, 0, &W) == LS_EINVAL);
    const int64_t zero[] = {AL, 0};
    CHECK(ls_long_plan_drop(2, AL, zero, nullptr, nullptr, nullptr, 0, &W) == LS_EINVAL);
    // the cap on a clip's windows: 2^20 strides beyond the first window pass, one more does not, nor does a length that would overflow
    const int64_t cap[] = {AL + S * (1 << 20) + S - 1, 5};
    std::vector<int32_t> big((size_t)(1 << 20) + 4, -1);
    CHECK(ls_long_plan_drop(2, AL, cap, nullptr, nullptr, big.data(), (int32_t)big.size(), &W) == LS_OK);
    CHECK(W == (1 << 20) + 2 && big[0] == 2 && big[1] == 1 && big[(size_t)W - 1] == 1 && big[(size_t)W] == -1);
    const int64_t past[] = {AL + S * ((1 << 20) + 1), 5}, huge[] = {INT64_MAX, 5};
    CHECK(ls_long_plan_drop(2, AL, past, nullptr, nullptr, nullptr, 0, &W) == LS_EINVAL);
    CHECK(ls_long_plan_drop(2, AL, huge, nullptr, nullptr, nullptr, 0, &W) == LS_EINVAL);
}

// the windows ls_long_edit_plan runs for one clip's [lo, hi) as a bit set; -1 when it refuses
static int edit(int32_t W, int32_t T, int32_t n_pre, int32_t lo, int32_t hi) {
    std::vector<int32_t> flags((size_t)(W > 0 ? W : 1), -1);
    int32_t n = -1;
    if (ls_long_edit_plan(1, W, T, n_pre, &lo, &hi, flags.data(), &n) != LS_OK) return -1;
    int bits = 0, count = 0;
    for (int w = 0; w < W; ++w) { CHECK(flags[w] == 0 || flags[w] == 1); bits |= flags[w] << w; count += flags[w]; }
    CHECK(count == n);
    return bits;
}

static void test_edit_plan() {
    const int32_t T = 34, P = 4, W = 3, Tt = T + (W - 1) * (T - P);       // 94 frames; window 0 owns [0, 34), 1 [34, 64), 2 [64, 94)
    CHECK(edit(W, T, P, 10, 10) == 0 && edit(W, T, P, 0, 0) == 0 && edit(W, T, P, Tt, Tt) == 0);      // lo == hi: nothing runs
    CHECK(edit(W, T, P, Tt - 1, Tt) == 4 && edit(W, T, P, 0, Tt) == 7 && edit(W, T, P, 0, 1) == 1);
    CHECK(edit(W, T, P, 30, 34) == 1);      // frames window 1 covers but window 0 owns
    CHECK(edit(W, T, P, 33, 35) == 3 && edit(W, T, P, 34, 35) == 2 && edit(W, T, P, 63, 65) == 6);
    CHECK(edit(W, T, P, 0, Tt + 1) == -1 && edit(W, T, P, 5, 4) == -1 && edit(W, T, P, -1, 4) == -1);
    CHECK(edit(1, T, P, 0, T) == 1 && edit(1, T, P, 0, T + 1) == -1);
    // n_pre == T - 1: a stride of one frame; window w > 0 owns the single frame T - 1 + w
    CHECK(edit(W, T, T - 1, 0, T) == 1 && edit(W, T, T - 1, T, T + 2) == 6 && edit(W, T, T - 1, T + 1, T + 2) == 4);
    CHECK(edit(W, T, T - 1, T, T + 3) == -1);
    CHECK(edit(W, T, T, 0, 1) == -1 && edit(W, T, 0, 0, 1) == -1 && edit(0, T, P, 0, 1) == -1);
    // two clips: a window runs when either range meets it; the flags are optional, the count is not
    const int32_t lo[] = {0, 70}, hi[] = {0, 71};
    int32_t n = -1, flags[3] = {-1, -1, -1};
    CHECK(ls_long_edit_plan(2, W, T, P, lo, hi, flags, &n) == LS_OK && n == 1 && flags[0] == 0 && flags[1] == 0 && flags[2] == 1);
    n = -1;
    CHECK(ls_long_edit_plan(2, W, T, P, lo, hi, nullptr, &n) == LS_OK && n == 1);
    CHECK(ls_long_edit_plan(2, W, T, P, lo, hi, flags, nullptr) == LS_EINVAL);
    CHECK(ls_long_edit_plan(2, W, T, P, nullptr, hi, flags, &n) == LS_EINVAL && ls_long_edit_plan(2, W, T, P, lo, nullptr, flags, &n) == LS_EINVAL);
    CHECK(ls_long_edit_plan(0, W, T, P, lo, hi, flags, &n) == LS_EINVAL);
}

// feed_copies is internal to the library (declared in csrc/ls_handle.h, which needs HIP); its five ints per copy are
// {first slot, slots, ring position, offset into the take, samples}
namespace ls { void feed_copies(int S, int R, const int* pos, const long long* from, const int* take, std::vector<int>& copies); }
using Ints = std::vector<int>;
static Ints feed(int R, const Ints& pos, const Ints& take, const std::vector<long long>& from = {}) {
    const std::vector<long long> zero(pos.size(), 0);
    Ints copies{-1, -1};
    ls::feed_copies((int)pos.size(), R, pos.data(), (from.empty() ? zero : from).data(), take.data(), copies);
    return copies;
}

static void test_feed_copies() {
    const int R = 68268;
    CHECK(feed(R, {5}, {100}) == (Ints{0, 1, 5, 0, 100}));                                      // S = 1
    CHECK(feed(R, {5}, {0}).empty() && feed(R, {5, 5, 9}, {0, 0, 0}).empty());                  // nothing to take: no copy, the output is cleared
    CHECK(feed(R, {7, 7, 7, 7}, {40, 40, 40, 40}) == (Ints{0, 4, 7, 0, 40}));                   // a stream: one run whatever its batch
    CHECK(feed(R, {7, 3, 3}, {40, 9, 9}) == (Ints{0, 1, 7, 0, 40, 1, 2, 3, 0, 9}));             // a run that ends at the last slot
    CHECK(feed(R, {3, 3, 3}, {9, 0, 9}) == (Ints{0, 1, 3, 0, 9, 2, 1, 3, 0, 9}));               // an idle slot splits what it stands between
    CHECK(feed(R, {3, 3}, {9, 8}) == (Ints{0, 1, 3, 0, 9, 1, 1, 3, 0, 8}));
    CHECK(feed(R, {3, 3}, {9, 9}, {0, 4}) == (Ints{0, 1, 3, 0, 9, 1, 1, 3, 0, 9}));             // alike in the ring, not in the chunk: two copies
    CHECK(feed(R, {R - 10, R - 10}, {10, 10}) == (Ints{0, 2, R - 10, 0, 10}));                  // a run that ends exactly at R does not wrap
    CHECK(feed(R, {R - 10, R - 10}, {11, 11}) == (Ints{0, 2, R - 10, 0, 10, 0, 2, 0, 10, 1}));  // one sample more does
    CHECK(feed(R, {R - 1}, {R}) == (Ints{0, 1, R - 1, 0, 1, 0, 1, 0, 1, R - 1}));               // a whole ring from its last position
    CHECK(feed(R, {0}, {R}) == (Ints{0, 1, 0, 0, R}));
}

// with arguments: R, then per case S, S ring positions, S takes -> one line of feed_copies' ints per case (tests/test_chain_plan_host.py)
static int print_feed_copies(int argc, char** argv) {
    const int R = std::atoi(argv[1]);
    for (int i = 2; i < argc;) {
        const int S = std::atoi(argv[i++]);
        if (S < 1 || i + 2 * S > argc) return 2;
        Ints pos, take;
        for (int s = 0; s < S; ++s) pos.push_back(std::atoi(argv[i + s]));
        for (int s = 0; s < S; ++s) take.push_back(std::atoi(argv[i + S + s]));
        i += 2 * S;
        for (int v : feed(R, pos, take)) std::printf("%d ", v);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return print_feed_copies(argc, argv);
    test_stream_plan();
    test_plan_drop();
    test_edit_plan();
    test_feed_copies();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

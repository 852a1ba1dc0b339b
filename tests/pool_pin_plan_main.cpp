// The host-only plan of a push of a session with pinned poses (ls_long_pool_pin_plan, livelyspeaker_amd/csrc/ls_chain_plan.cpp) on its
// edges.  A stand-alone program: it links that unit alone, is built with the host sanitizers by tests/test_long_pool_pins_host.py, and
// exits non-zero on a wrong answer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int32_t T = 34, NPRE = 4;
using V32 = std::vector<int32_t>;

struct Plan {
    int rc;
    V32 rows, counts, pinned, rounds;
    int32_t calls, entries;
};

// the two-call use of the entry: counts first, then the calls into arrays of exactly that size
static Plan plan(const std::vector<int64_t>& ran, const V32& wins, const std::vector<std::vector<int64_t>>* pins) {
    const int32_t n = (int32_t)ran.size();
    V32 first;
    std::vector<int64_t> frames;
    if (pins) {
        first.push_back(0);
        for (const auto& p : *pins) { frames.insert(frames.end(), p.begin(), p.end()); first.push_back((int32_t)frames.size()); }
    }
    const int32_t* pf = pins ? first.data() : nullptr;
    const int64_t* pn = frames.empty() ? nullptr : frames.data();
    Plan p{0, {}, {}, {}, {}, -7, -7};
    p.rc = ls_long_pool_pin_plan(n, T, NPRE, ran.data(), wins.data(), pf, pn, nullptr, 0, nullptr, nullptr, nullptr, 0, &p.calls, &p.entries);
    if (p.rc != LS_OK) return p;
    p.rows.assign((size_t)p.entries, -7); p.counts.assign((size_t)p.calls, -7); p.pinned.assign((size_t)p.calls, -7); p.rounds.assign((size_t)p.calls, -7);
    int32_t calls2 = -7, entries2 = -7;
    CHECK(ls_long_pool_pin_plan(n, T, NPRE, ran.data(), wins.data(), pf, pn, p.entries ? p.rows.data() : nullptr, p.entries, p.calls ? p.counts.data() : nullptr,
                                p.calls ? p.pinned.data() : nullptr, p.calls ? p.rounds.data() : nullptr, p.calls, &calls2, &entries2) == LS_OK);
    CHECK(calls2 == p.calls && entries2 == p.entries);
    return p;
}

using Pins = std::vector<std::vector<int64_t>>;
static Plan plan(const std::vector<int64_t>& ran, const V32& wins, const Pins& pins) { return plan(ran, wins, &pins); }

static void test_calls() {
    // slots 0 (window 1 next), 1 (window 0 next), 3 (windows 0 and 1 in this push); slot 2 runs nothing
    const std::vector<int64_t> ran{1, 0, 0, 0};
    const V32 wins{1, 1, 0, 2};
    // no pins at all, as null arrays and as an empty CSR: the calls are the rounds
    const std::vector<std::vector<int64_t>> none(4);
    for (const auto* pins : {(const std::vector<std::vector<int64_t>>*)nullptr, &none}) {
        Plan p = plan(ran, wins, pins);
        CHECK(p.rc == LS_OK && p.calls == 2 && p.entries == 4);
        CHECK((p.rows == V32{0, 1, 3, 3}) && (p.counts == V32{3, 1}) && (p.pinned == V32{0, 0}) && (p.rounds == V32{0, 1}));
    }
    // slot 0's window 1 owns 34 .. 63: frame 34 (its first owned) pins it, frame 33 (its prefix, owned by window 0) does not
    Plan p = plan(ran, wins, Pins{{34}, {}, {}, {}});
    CHECK(p.rc == LS_OK && p.calls == 3 && (p.rows == V32{1, 3, 0, 3}) && (p.counts == V32{2, 1, 1}) && (p.pinned == V32{0, 1, 0}) && (p.rounds == V32{0, 0, 1}));
    p = plan(ran, wins, Pins{{33}, {}, {}, {}});
    CHECK(p.rc == LS_OK && p.calls == 2 && (p.pinned == V32{0, 0}));
    p = plan(ran, wins, Pins{{63}, {}, {}, {}});
    CHECK(p.rc == LS_OK && p.calls == 3 && (p.pinned == V32{0, 1, 0}));
    p = plan(ran, wins, Pins{{64}, {}, {}, {}});        // owned by window 2, which does not run
    CHECK(p.rc == LS_OK && p.calls == 2);
    // frames 30 .. 33 belong to window 0: slot 3 is pinned in round 0 and plain in round 1; slot 1 beside it makes a round with only pinned rows
    p = plan(ran, wins, Pins{{40}, {0}, {}, {33, 30}});
    CHECK(p.rc == LS_OK && p.calls == 2 && (p.rows == V32{0, 1, 3, 3}) && (p.counts == V32{3, 1}) && (p.pinned == V32{1, 0}) && (p.rounds == V32{0, 1}));
    // a slot that runs no window is in no call, whatever it has pinned
    p = plan(ran, wins, Pins{{}, {}, {5}, {}});
    CHECK(p.rc == LS_OK && p.calls == 2 && (p.rows == V32{0, 1, 3, 3}));
    // nothing runs: no call, no entry
    p = plan({3, 0}, {0, 0}, Pins{{100}, {}});
    CHECK(p.rc == LS_OK && p.calls == 0 && p.entries == 0);
}

static void test_refusals() {
    const std::vector<int64_t> ran{1, 0};
    const V32 wins{1, 2};
    int32_t c = 0, e = 0, rows[3], counts[2], first[3] = {0, 1, 1};
    int64_t frames[1] = {40};
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, frames, rows, 3, counts, nullptr, nullptr, 2, &c, &e) == LS_EINVAL);     // three calls
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, frames, rows, 2, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);    // three rows
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, frames, rows, 3, nullptr, nullptr, nullptr, 0, &c, &e) == LS_OK && c == 3 && e == 3);
    CHECK(ls_long_pool_pin_plan(0, T, NPRE, ran.data(), wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, T, ran.data(), wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, 0, ran.data(), wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, nullptr, wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), nullptr, first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), nullptr, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);   // frames without a CSR
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);    // a CSR without frames
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, frames, nullptr, 1, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);     // a capacity without an array
    int32_t down[3] = {0, 1, 0}, late[3] = {1, 1, 1};
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), down, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), late, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    int64_t negative[1] = {-1};
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), wins.data(), first, negative, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    const std::vector<int64_t> bad_ran{-1, 0}, far{INT64_MAX / 30, 0};
    const V32 bad_wins{1, -2};
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, bad_ran.data(), wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, far.data(), wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);    // w S + T at its guard
    CHECK(ls_long_pool_pin_plan(2, T, NPRE, ran.data(), bad_wins.data(), first, frames, nullptr, 0, nullptr, nullptr, nullptr, 0, &c, &e) == LS_EINVAL);
}

int main() {
    test_calls();
    test_refusals();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

// The host-only plan of a session pool's push (ls_long_pool_plan, livelyspeaker_amd/csrc/ls_chain_plan.cpp) on its edges.  A stand-alone
// program: it links that unit alone, is built with the host sanitizers by tests/test_long_pool_host.py, and exits non-zero on a wrong answer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int64_t S = LS_LONG_AUDIO_STRIDE;
static const int32_t AL = 36267;        // the TED model's audio_len

struct Slots {
    std::vector<int64_t> fed, ran, fresh;
    std::vector<int32_t> closing, open;
};
struct Plan {
    int rc;
    std::vector<int32_t> wins, frames, flat;
    int32_t rounds, entries;
};

// the two-call use of the entry: counts first, then the rounds into an array of exactly that size
static Plan plan(const Slots& s) {
    const int32_t n = (int32_t)s.fed.size();
    Plan p{0, std::vector<int32_t>((size_t)n, -7), std::vector<int32_t>((size_t)n, -7), {}, -7, -7};
    p.rc = ls_long_pool_plan(n, AL, s.fed.data(), s.ran.data(), s.fresh.data(), s.closing.data(), s.open.data(), p.wins.data(), p.frames.data(), nullptr, 0,
                             &p.rounds, &p.entries);
    if (p.rc != LS_OK) return p;
    p.flat.assign((size_t)p.entries, -7);
    int32_t rounds2 = -7, entries2 = -7;
    std::vector<int32_t> wins2((size_t)n, -7);
    CHECK(ls_long_pool_plan(n, AL, s.fed.data(), s.ran.data(), s.fresh.data(), s.closing.data(), s.open.data(), wins2.data(), nullptr,
                            p.entries ? p.flat.data() : nullptr, p.entries, &rounds2, &entries2) == LS_OK);
    CHECK(rounds2 == p.rounds && entries2 == p.entries && wins2 == p.wins);
    return p;
}

static void test_rounds() {
    // slot 0 mid-stream with one more window, slot 1 one sample short, slot 2 free, slot 3 fresh with two windows in one chunk
    Slots s{{AL, AL - 1, 0, 0}, {1, 0, 0, 0}, {S, 0, 0, AL + S}, {0, 0, 0, 0}, {1, 1, 0, 1}};
    Plan p = plan(s);
    CHECK(p.rc == LS_OK && p.rounds == 2 && p.entries == 3);
    CHECK((p.wins == std::vector<int32_t>{1, 0, 0, 2}) && (p.frames == std::vector<int32_t>{30, 0, 0, 64}) && (p.flat == std::vector<int32_t>{0, 3, 3}));
    // every slot agrees with the stream's plan on that slot alone
    for (size_t i = 0; i < s.fed.size(); ++i) {
        int64_t first = -1, k = -1;
        CHECK(ls_long_stream_plan(s.fed[i], s.fresh[i], AL, s.closing[i], &first, &k) == LS_OK);
        CHECK(!s.open[i] || (first == s.ran[i] && k == p.wins[i]));
    }
    // closing: the padded window; exactly on a boundary nothing; the flag of a free slot is ignored
    s = Slots{{AL + 1, AL + S, 0}, {1, 2, 0}, {0, 0, 0}, {1, 1, 1}, {1, 1, 0}};
    p = plan(s);
    CHECK(p.rc == LS_OK && p.rounds == 1 && p.entries == 1 && (p.wins == std::vector<int32_t>{1, 0, 0}) && (p.frames == std::vector<int32_t>{30, 0, 0}));
    CHECK(p.flat == std::vector<int32_t>{0});
    // nothing to do: no round, no entry
    s = Slots{{5, 0}, {0, 0}, {0, 0}, {0, 0}, {1, 0}};
    p = plan(s);
    CHECK(p.rc == LS_OK && p.rounds == 0 && p.entries == 0 && p.flat.empty());
}

static void test_refusals() {
    const Slots good{{AL, 0}, {1, 0}, {S, 0}, {0, 0}, {1, 0}};
    CHECK(plan(good).rc == LS_OK);
    Slots s = good; s.fresh[1] = 1;                      // samples for a slot that is not open
    CHECK(plan(s).rc == LS_EINVAL);
    s = good; s.open[1] = 1; s.closing[1] = 1;           // closing a slot that was fed no sample at all
    CHECK(plan(s).rc == LS_EINVAL);
    s.fresh[1] = 1;                                      // ... one sample is enough: one padded window
    CHECK(plan(s).rc == LS_OK && plan(s).wins[1] == 1 && plan(s).frames[1] == 34);
    s = good; s.fresh[0] = -1;
    CHECK(plan(s).rc == LS_EINVAL);
    s = good; s.fed[0] = -1;
    CHECK(plan(s).rc == LS_EINVAL);
    s = good; s.ran[0] = -1;
    CHECK(plan(s).rc == LS_EINVAL);
    s = good; s.ran[0] = 0;                              // a window count that does not belong to the samples fed
    CHECK(plan(s).rc == LS_EINVAL);
    s = good; s.fed[0] = INT64_MAX; s.ran[0] = (INT64_MAX - AL) / S + 1; s.fresh[0] = 1;      // the sum at its guard
    CHECK(plan(s).rc == LS_EINVAL);
    // null arrays, a short round array
    int32_t w[2], r = 0, e = 0, flat[1];
    CHECK(ls_long_pool_plan(2, AL, nullptr, good.ran.data(), good.fresh.data(), good.closing.data(), good.open.data(), w, nullptr, nullptr, 0, &r, &e) == LS_EINVAL);
    CHECK(ls_long_pool_plan(2, AL, good.fed.data(), good.ran.data(), good.fresh.data(), good.closing.data(), good.open.data(), nullptr, nullptr, nullptr, 0, &r, &e) == LS_EINVAL);
    CHECK(ls_long_pool_plan(2, AL, good.fed.data(), good.ran.data(), good.fresh.data(), good.closing.data(), good.open.data(), w, nullptr, nullptr, 0, nullptr, &e) == LS_EINVAL);
    CHECK(ls_long_pool_plan(2, AL, good.fed.data(), good.ran.data(), good.fresh.data(), good.closing.data(), good.open.data(), w, nullptr, nullptr, 1, &r, &e) == LS_EINVAL);
    CHECK(ls_long_pool_plan(0, AL, good.fed.data(), good.ran.data(), good.fresh.data(), good.closing.data(), good.open.data(), w, nullptr, nullptr, 0, &r, &e) == LS_EINVAL);
    CHECK(ls_long_pool_plan(2, 0, good.fed.data(), good.ran.data(), good.fresh.data(), good.closing.data(), good.open.data(), w, nullptr, nullptr, 0, &r, &e) == LS_EINVAL);
    Slots two = good; two.fresh[0] = 2 * S;              // two windows: one entry of room is too little
    CHECK(ls_long_pool_plan(2, AL, two.fed.data(), two.ran.data(), two.fresh.data(), two.closing.data(), two.open.data(), w, nullptr, flat, 1, &r, &e) == LS_EINVAL);
}

int main() {
    test_rounds();
    test_refusals();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

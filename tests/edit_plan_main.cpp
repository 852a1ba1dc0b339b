// The plan of a compact timeline edit (ls_long_edit_plan_compact, livelyspeaker_amd/csrc/ls_chain_plan.cpp) on its edges.  A stand-alone
// program: it links that unit alone, is built with the host sanitizers by tests/test_long_edit_compact_host.py, and exits non-zero on
// a wrong answer.  T = 34, n_pre = 4, S = 30: window w owns [0, 34) for w = 0 and [30 w + 4, 30 w + 34) otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int32_t kT = 34, kPre = 4;

struct Plan {
    int rc;
    std::vector<int32_t> windows, counts, rows;
    int32_t n_run, n_pairs;
};

// the two-call use of the entry: the counts first, then the arrays at exactly that size (a guard word behind each stays as it was)
static Plan plan(int32_t W, const std::vector<int32_t>& lo, const std::vector<int32_t>& hi, const std::vector<unsigned char>* chan = nullptr,
                 int32_t n_chan = 0, const std::vector<int32_t>* frames = nullptr) {
    const int32_t B = (int32_t)lo.size();
    Plan p{0, {}, {}, {}, -7, -7};
    const unsigned char* ch = chan ? chan->data() : nullptr;
    const int32_t* fr = frames ? frames->data() : nullptr;
    p.rc = ls_long_edit_plan_compact(B, W, kT, kPre, lo.data(), hi.data(), ch, n_chan, fr, nullptr, nullptr, 0, nullptr, 0, &p.n_run, &p.n_pairs);
    if (p.rc != LS_OK) return p;
    p.windows.assign((size_t)p.n_run + 1, -99); p.counts.assign((size_t)p.n_run + 1, -99); p.rows.assign((size_t)p.n_pairs + 1, -99);
    int32_t again_w = -7, again_p = -7;
    CHECK(ls_long_edit_plan_compact(B, W, kT, kPre, lo.data(), hi.data(), ch, n_chan, fr, p.windows.data(), p.counts.data(), p.n_run, p.rows.data(),
                                    p.n_pairs, &again_w, &again_p) == LS_OK);
    CHECK(again_w == p.n_run && again_p == p.n_pairs);
    CHECK(p.windows.back() == -99 && p.counts.back() == -99 && p.rows.back() == -99);
    p.windows.pop_back(); p.counts.pop_back(); p.rows.pop_back();
    return p;
}

typedef std::vector<int32_t> V;

static void test_plans() {
    // the equal-length case of the GPU tests: A_0 = {0}, A_1 = {0, 3}, A_2 = {2, 3}; clip 1 is in no window
    Plan p = plan(3, {20, 0, 70, 40}, {50, 0, 80, 72});
    CHECK(p.rc == LS_OK && p.n_run == 3 && p.n_pairs == 5);
    CHECK(p.windows == (V{0, 1, 2}) && p.counts == (V{1, 2, 2}) && p.rows == (V{0, 0, 3, 2, 3}));
    // the ragged one: frames (94, 34, 94, 64) = W_b (3, 1, 3, 2); clip 3's range ends with its own frames
    const V frames{94, 34, 94, 64};
    p = plan(3, {20, 5, 70, 40}, {50, 30, 80, 64}, nullptr, 0, &frames);
    CHECK(p.rc == LS_OK && p.windows == (V{0, 1, 2}) && p.counts == (V{2, 2, 1}) && p.rows == (V{0, 1, 0, 3, 2}));
    // frames 30 .. 33 are window 0's alone; frame 34 is window 1's
    p = plan(3, {30}, {34});
    CHECK(p.rc == LS_OK && p.windows == (V{0}) && p.rows == (V{0}));
    p = plan(3, {34}, {35});
    CHECK(p.rc == LS_OK && p.windows == (V{1}) && p.rows == (V{0}));
    // a window nobody touches is skipped, and the rows of the next one start right behind
    p = plan(4, {10, 100}, {20, 110});
    CHECK(p.rc == LS_OK && p.windows == (V{0, 3}) && p.counts == (V{1, 1}) && p.rows == (V{0, 1}));
    // channels: a clip without a selected channel is in no window, one selected channel is enough
    const std::vector<unsigned char> chan{0, 0, 0, 0, 7, 0};
    p = plan(2, {0, 0}, {64, 64}, &chan, 3);
    CHECK(p.rc == LS_OK && p.windows == (V{0, 1}) && p.counts == (V{1, 1}) && p.rows == (V{1, 1}));
    // nothing to run is no error of the plan
    p = plan(3, {5, 94}, {5, 94});
    CHECK(p.rc == LS_OK && p.n_run == 0 && p.n_pairs == 0 && p.windows.empty() && p.rows.empty());
    // the whole timeline of every clip: the identity tables
    p = plan(3, {0, 0}, {94, 94});
    CHECK(p.rc == LS_OK && p.counts == (V{2, 2, 2}) && p.rows == (V{0, 1, 0, 1, 0, 1}));
    // the largest window count still adds up
    p = plan(1 << 20, {0}, {34 + 30 * ((1 << 20) - 1)});
    CHECK(p.rc == LS_OK && p.n_run == (1 << 20) && p.n_pairs == (1 << 20) && p.rows.back() == 0 && p.windows.back() == (1 << 20) - 1);
}

static void test_refusals() {
    CHECK(plan(3, {5}, {4}).rc == LS_EINVAL);                   // lo > hi
    CHECK(plan(3, {-1}, {4}).rc == LS_EINVAL);
    CHECK(plan(3, {0}, {95}).rc == LS_EINVAL);                  // beyond T + (W - 1) S = 94
    CHECK(plan(3, {0}, {94}).rc == LS_OK);
    const V short1{64}, odd{65}, tiny{4}, big{124}, full{94};
    CHECK(plan(3, {0}, {65}, nullptr, 0, &short1).rc == LS_EINVAL);      // beyond the clip's own frames
    CHECK(plan(3, {0}, {64}, nullptr, 0, &short1).rc == LS_OK);
    CHECK(plan(3, {0}, {10}, nullptr, 0, &odd).rc == LS_EINVAL);         // not 34 + 30 k
    CHECK(plan(3, {0}, {2}, nullptr, 0, &tiny).rc == LS_EINVAL);         // fewer than one window
    CHECK(plan(3, {0}, {10}, nullptr, 0, &big).rc == LS_EINVAL);         // more windows than the timeline holds
    CHECK(plan(3, {0}, {94}, nullptr, 0, &full).rc == LS_OK);
    const int32_t lo[2] = {0, 40}, hi[2] = {40, 60};
    int32_t w[2], c[2], r[3], nw = 0, np = 0;
    const unsigned char ch[2] = {1, 1};
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_OK && nw == 2 && np == 3);
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 1, r, 3, &nw, &np) == LS_EINVAL);     // two windows, room for one
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 2, &nw, &np) == LS_EINVAL);     // three rows, room for two
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, nullptr, c, 2, r, 3, &nw, &np) == LS_EINVAL);   // room without an array
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, nullptr, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, ch, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);          // channels without a count
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, nullptr, hi, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, nullptr, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 3, nullptr, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(2, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, nullptr) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(0, 2, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(2, 0, kT, kPre, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_compact(2, 2, 4, 4, lo, hi, nullptr, 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);          // T <= n_pre
}

int main() {
    test_plans();
    test_refusals();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

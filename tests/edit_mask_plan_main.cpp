// The plan of a timeline edit by element mask (ls_long_edit_plan_mask, livelyspeaker_amd/csrc/ls_chain_plan.cpp) on its edges: random
// masks against a restatement written here, the rectangle against ls_long_edit_plan_compact, the seam frames, empty masks, ragged
// frames and the capacity errors.  A stand-alone program: it links that unit alone, is built with the host sanitizers by
// tests/test_long_edit_mask_host.py, and exits non-zero on a wrong answer.  T = 34, n_pre = 4, S = 30: window w owns [0, 34) for
// w = 0 and [30 w + 4, 30 w + 34) otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int32_t kT = 34, kPre = 4, kS = 30;
typedef std::vector<int32_t> V;
typedef std::vector<unsigned char> M;

struct Plan {
    int rc;
    V windows, counts, rows;
    int32_t n_run, n_pairs;
};

// the two-call use of the entry: the counts first, then the arrays at exactly that size (a guard word behind each stays as it was)
static Plan plan(int32_t B, int32_t W, int32_t C, const M& mask, const V* frames = nullptr) {
    Plan p{0, {}, {}, {}, -7, -7};
    const int32_t* fr = frames ? frames->data() : nullptr;
    p.rc = ls_long_edit_plan_mask(B, W, kT, kPre, mask.data(), C, fr, nullptr, nullptr, 0, nullptr, 0, &p.n_run, &p.n_pairs);
    if (p.rc != LS_OK) return p;
    p.windows.assign((size_t)p.n_run + 1, -99); p.counts.assign((size_t)p.n_run + 1, -99); p.rows.assign((size_t)p.n_pairs + 1, -99);
    int32_t again_w = -7, again_p = -7;
    CHECK(ls_long_edit_plan_mask(B, W, kT, kPre, mask.data(), C, fr, p.windows.data(), p.counts.data(), p.n_run, p.rows.data(), p.n_pairs,
                                 &again_w, &again_p) == LS_OK);
    CHECK(again_w == p.n_run && again_p == p.n_pairs);
    CHECK(p.windows.back() == -99 && p.counts.back() == -99 && p.rows.back() == -99);
    p.windows.pop_back(); p.counts.pop_back(); p.rows.pop_back();
    return p;
}

static int32_t frames_of(int32_t W) { return kT + (W - 1) * kS; }

// one set byte of clip b, channel c, frame n
static M one(int32_t B, int32_t W, int32_t C, int32_t b, int32_t c, int32_t n) {
    M m((size_t)B * C * frames_of(W), 0);
    m[((size_t)b * C + c) * frames_of(W) + n] = 1;
    return m;
}

// the rule, restated: pair (b, w) iff some channel has a set byte on a frame n = w S + f with w == 0 or f >= n_pre
static Plan restated(int32_t B, int32_t W, int32_t C, const M& mask) {
    Plan p{0, {}, {}, {}, 0, 0};
    const int32_t N = frames_of(W);
    for (int32_t w = 0; w < W; ++w) {
        int32_t n_rows = 0;
        for (int32_t b = 0; b < B; ++b) {
            bool any = false;
            for (int32_t c = 0; c < C && !any; ++c)
                for (int32_t f = w ? kPre : 0; f < kT && !any; ++f) any = mask[((size_t)b * C + c) * N + w * kS + f] != 0;
            if (any) { p.rows.push_back(b); ++n_rows; }
        }
        if (n_rows) { p.windows.push_back(w); p.counts.push_back(n_rows); }
    }
    p.n_run = (int32_t)p.windows.size(); p.n_pairs = (int32_t)p.rows.size();
    return p;
}

static uint32_t rng_state = 20261021u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void test_random_masks() {
    for (int it = 0; it < 400; ++it) {
        const int32_t B = 1 + (int32_t)(rnd() % 5), W = 1 + (int32_t)(rnd() % 5), C = 1 + (int32_t)(rnd() % 4), N = frames_of(W);
        M m((size_t)B * C * N, 0);
        const int32_t n_set = (int32_t)(rnd() % 6);             // sparse: most pairs stay out of the plan
        for (int32_t k = 0; k < n_set; ++k) m[rnd() % m.size()] = (unsigned char)(1 + rnd() % 255);
        const Plan got = plan(B, W, C, m), want = restated(B, W, C, m);
        CHECK(got.rc == LS_OK && got.windows == want.windows && got.counts == want.counts && got.rows == want.rows);
        CHECK(got.n_run == want.n_run && got.n_pairs == want.n_pairs);
    }
}

static void test_rectangles_are_the_range_plan() {
    for (int it = 0; it < 200; ++it) {
        const int32_t B = 1 + (int32_t)(rnd() % 5), W = 1 + (int32_t)(rnd() % 5), C = 1 + (int32_t)(rnd() % 3), N = frames_of(W);
        V lo((size_t)B), hi((size_t)B), frames((size_t)B);
        M chan((size_t)B * C), m((size_t)B * C * N, 0);
        const bool ragged = rnd() % 2;
        for (int32_t b = 0; b < B; ++b) {
            frames[(size_t)b] = ragged ? frames_of(1 + (int32_t)(rnd() % W)) : N;
            lo[(size_t)b] = (int32_t)(rnd() % (frames[(size_t)b] + 1));
            hi[(size_t)b] = lo[(size_t)b] + (int32_t)(rnd() % 50);
            if (hi[(size_t)b] > frames[(size_t)b]) hi[(size_t)b] = frames[(size_t)b];
            for (int32_t c = 0; c < C; ++c) {
                chan[(size_t)b * C + c] = rnd() % 3 == 0;
                for (int32_t n = lo[(size_t)b]; n < hi[(size_t)b] && chan[(size_t)b * C + c]; ++n) m[((size_t)b * C + c) * N + n] = 1;
            }
        }
        const Plan got = plan(B, W, C, m, ragged ? &frames : nullptr);
        int32_t nw = -1, np = -1;
        CHECK(ls_long_edit_plan_compact(B, W, kT, kPre, lo.data(), hi.data(), chan.data(), C, ragged ? frames.data() : nullptr, nullptr, nullptr,
                                        0, nullptr, 0, &nw, &np) == LS_OK);
        V w((size_t)nw + 1), c((size_t)nw + 1), r((size_t)np + 1);
        CHECK(ls_long_edit_plan_compact(B, W, kT, kPre, lo.data(), hi.data(), chan.data(), C, ragged ? frames.data() : nullptr, w.data(), c.data(),
                                        nw, r.data(), np, &nw, &np) == LS_OK);
        w.pop_back(); c.pop_back(); r.pop_back();
        CHECK(got.rc == LS_OK && got.windows == w && got.counts == c && got.rows == r);
    }
}

static void test_seams_and_edges() {
    // frames 30 .. 33 are window 0's alone although window 1 covers them; frame 34 is window 1's first
    for (int32_t n = 30; n < 34; ++n) {
        const Plan p = plan(1, 3, 2, one(1, 3, 2, 0, 1, n));
        CHECK(p.rc == LS_OK && p.windows == (V{0}) && p.rows == (V{0}));
    }
    Plan p = plan(1, 3, 2, one(1, 3, 2, 0, 0, 34));
    CHECK(p.rc == LS_OK && p.windows == (V{1}) && p.counts == (V{1}));
    // frames w S .. w S + n_pre - 1 of every later window plan window w - 1, never w
    for (int32_t w = 1; w < 4; ++w)
        for (int32_t j = 0; j < kPre; ++j) {
            p = plan(2, 4, 1, one(2, 4, 1, 1, 0, w * kS + j));
            CHECK(p.rc == LS_OK && p.windows == (V{w - 1}) && p.rows == (V{1}));
        }
    // the first and the last frame of the timeline
    p = plan(2, 3, 3, one(2, 3, 3, 1, 2, 0));
    CHECK(p.rc == LS_OK && p.windows == (V{0}) && p.rows == (V{1}));
    p = plan(2, 3, 3, one(2, 3, 3, 0, 0, 93));
    CHECK(p.rc == LS_OK && p.windows == (V{2}) && p.rows == (V{0}));
    // an empty mask is no error of the plan
    p = plan(3, 3, 2, M((size_t)3 * 2 * 94, 0));
    CHECK(p.rc == LS_OK && p.n_run == 0 && p.n_pairs == 0 && p.windows.empty() && p.rows.empty());
    // a full mask: the identity tables
    p = plan(2, 3, 2, M((size_t)2 * 2 * 94, 1));
    CHECK(p.rc == LS_OK && p.counts == (V{2, 2, 2}) && p.rows == (V{0, 1, 0, 1, 0, 1}));
    // a window nobody touches is skipped
    M m = one(2, 4, 1, 0, 0, 10);
    m[(size_t)1 * 124 + 100] = 1;
    p = plan(2, 4, 1, m);
    CHECK(p.rc == LS_OK && p.windows == (V{0, 3}) && p.counts == (V{1, 1}) && p.rows == (V{0, 1}));
}

static void test_ragged_frames() {
    const V frames{94, 34, 64};
    // the last frame a clip holds is fine, the first one beyond it is an error -- not a silent no-op
    CHECK(plan(3, 3, 1, one(3, 3, 1, 1, 0, 33), &frames).rc == LS_OK);
    CHECK(plan(3, 3, 1, one(3, 3, 1, 1, 0, 34), &frames).rc == LS_EINVAL);
    CHECK(plan(3, 3, 1, one(3, 3, 1, 2, 0, 63), &frames).rc == LS_OK);
    CHECK(plan(3, 3, 1, one(3, 3, 1, 2, 0, 64), &frames).rc == LS_EINVAL);
    CHECK(plan(3, 3, 1, one(3, 3, 1, 2, 0, 93), &frames).rc == LS_EINVAL);
    CHECK(plan(3, 3, 1, one(3, 3, 1, 0, 0, 93), &frames).rc == LS_OK);
    Plan p = plan(3, 3, 1, one(3, 3, 1, 2, 0, 63), &frames);
    CHECK(p.windows == (V{1}) && p.rows == (V{2}));
    const M none((size_t)1 * 94, 0);
    for (int32_t bad : {65, 63, 33, 4, 0, -30, 124}) {          // not 34 + 30 k with k < W
        const V f{bad};
        CHECK(plan(1, 3, 1, none, &f).rc == LS_EINVAL);
    }
}

static void test_refusals() {
    M m = one(2, 2, 1, 0, 0, 10);
    m[10 + 30] = 1; m[(size_t)64 + 50] = 1;                     // clip 0: windows 0 and 1; clip 1: window 1
    int32_t w[2], c[2], r[3], nw = 0, np = 0;
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, 2, r, 3, &nw, &np) == LS_OK && nw == 2 && np == 3);
    CHECK(w[0] == 0 && w[1] == 1 && c[0] == 1 && c[1] == 2 && r[0] == 0 && r[1] == 0 && r[2] == 1);
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, 1, r, 3, &nw, &np) == LS_EINVAL);      // two windows, room for one
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, 2, r, 2, &nw, &np) == LS_EINVAL);      // three rows, room for two
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, nullptr, c, 2, r, 3, &nw, &np) == LS_EINVAL);    // room without an array
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, 2, nullptr, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, -1, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, nullptr, 1, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 0, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);          // no channel
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, 2, r, 3, nullptr, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(2, 2, kT, kPre, m.data(), 1, nullptr, w, c, 2, r, 3, &nw, nullptr) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(0, 2, kT, kPre, m.data(), 1, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(2, 0, kT, kPre, m.data(), 1, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);
    CHECK(ls_long_edit_plan_mask(2, 2, 4, 4, m.data(), 1, nullptr, w, c, 2, r, 3, &nw, &np) == LS_EINVAL);             // T <= n_pre
}

int main() {
    test_random_masks();
    test_rectangles_are_the_range_plan();
    test_seams_and_edges();
    test_ragged_frames();
    test_refusals();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

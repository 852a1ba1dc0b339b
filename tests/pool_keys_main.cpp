// The key table of a keyed session pool's push (ls_long_pool_keys, livelyspeaker_amd/csrc/ls_chain_plan.cpp) on its edges.  A stand-alone
// program: it links that unit alone, is built with the host sanitizers by tests/test_pool_keys_host.py, and exits non-zero on a wrong answer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const uint64_t kTop = (1ull << 48) - 1;       // the largest key

struct Table {
    int rc;
    std::vector<uint64_t> rows;
    int32_t entries;
};

// the two-call use of the entry: the count first, then the rows into an array of exactly that size
static Table table(const std::vector<uint64_t>& keys, const std::vector<int64_t>& ran, const std::vector<int32_t>& wins) {
    const int32_t n = (int32_t)keys.size();
    Table t{0, {}, -7};
    t.rc = ls_long_pool_keys(n, keys.data(), ran.data(), wins.data(), nullptr, 0, &t.entries);
    if (t.rc != LS_OK) return t;
    t.rows.assign((size_t)t.entries, 0xDEADull);
    int32_t again = -7;
    CHECK(ls_long_pool_keys(n, keys.data(), ran.data(), wins.data(), t.entries ? t.rows.data() : nullptr, t.entries, &again) == LS_OK);
    CHECK(again == t.entries);
    return t;
}

static uint64_t at(uint64_t key, uint64_t w) { return key + (w << 48); }

static void test_rows() {
    // slot 0 mid-clip with one more window, slot 1 idle (its key is not looked at), slot 3 fresh with two windows and a key above 2^32
    const uint64_t big = (1ull << 32) + 5;
    Table t = table({7, ~0ull, 0, big}, {3, 9, 0, 0}, {1, 0, 0, 2});
    CHECK(t.rc == LS_OK && t.entries == 3);
    CHECK((t.rows == std::vector<uint64_t>{at(7, 3), at(big, 0), at(big, 1)}));
    // the plan's row order: round 0 ascending, then round 1 ...
    t = table({1, 2, 3}, {0, 5, 0}, {2, 3, 1});
    CHECK(t.rc == LS_OK && t.entries == 6);
    CHECK((t.rows == std::vector<uint64_t>{at(1, 0), at(2, 5), at(3, 0), at(1, 1), at(2, 6), at(2, 7)}));
    // the largest key at the last window: every bit of the 64 set, no carry between the fields
    t = table({kTop}, {65535}, {1});
    CHECK(t.rc == LS_OK && t.entries == 1 && t.rows[0] == ~0ull);
    // a slot that joined again restarts at window 0 under its new key
    t = table({42}, {0}, {1});
    CHECK(t.rc == LS_OK && t.rows[0] == 42);
    // nothing to run
    t = table({1, 2}, {4, 4}, {0, 0});
    CHECK(t.rc == LS_OK && t.entries == 0 && t.rows.empty());
}

static void test_refusals() {
    CHECK(table({kTop + 1}, {0}, {1}).rc == LS_EINVAL);               // a key of 2^48
    CHECK(table({kTop + 1}, {0}, {0}).rc == LS_OK);                   // ... of a slot that runs nothing: not looked at
    CHECK(table({1}, {65536}, {1}).rc == LS_ESTATE);                  // window 2^16
    CHECK(table({1}, {65535}, {2}).rc == LS_ESTATE);                  // ... reached inside the call
    CHECK(table({1}, {65534}, {2}).rc == LS_OK);
    CHECK(table({1}, {INT64_MAX}, {1}).rc == LS_ESTATE);              // no overflow on the way to the answer
    CHECK(table({1}, {-1}, {1}).rc == LS_EINVAL);
    CHECK(table({1}, {0}, {-1}).rc == LS_EINVAL);
    const uint64_t k[2] = {1, 2};
    const int64_t ran[2] = {0, 0};
    const int32_t wins[2] = {2, 1};
    uint64_t rows[3];
    int32_t e = 0;
    CHECK(ls_long_pool_keys(2, nullptr, ran, wins, rows, 3, &e) == LS_EINVAL);
    CHECK(ls_long_pool_keys(2, k, nullptr, wins, rows, 3, &e) == LS_EINVAL);
    CHECK(ls_long_pool_keys(2, k, ran, nullptr, rows, 3, &e) == LS_EINVAL);
    CHECK(ls_long_pool_keys(2, k, ran, wins, rows, 3, nullptr) == LS_EINVAL);
    CHECK(ls_long_pool_keys(0, k, ran, wins, rows, 3, &e) == LS_EINVAL);
    CHECK(ls_long_pool_keys(2, k, ran, wins, nullptr, 3, &e) == LS_EINVAL);          // room without an array
    CHECK(ls_long_pool_keys(2, k, ran, wins, rows, 2, &e) == LS_EINVAL);             // three rows, room for two
    CHECK(ls_long_pool_keys(2, k, ran, wins, rows, 3, &e) == LS_OK && e == 3);
}

int main() {
    test_rows();
    test_refusals();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

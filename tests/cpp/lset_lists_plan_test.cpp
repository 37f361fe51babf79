// lset_lists_plan_test.cpp — the host side of a level set's lists probe
// (storage-engine_amd/csrc/lset_lists_plan.hpp): the radix pass count at its
// edges, the workspace layout (regions disjoint, aligned, summing to
// work_bytes) and lset_lists_ref, the plain statement of the transform, on
// hand-written cases and against the pass-by-pass route the kernels take.
// No HIP: a stand-alone host program (tests/test_lset_lists.py builds it with
// -fsanitize=address,undefined and runs it).
#include <stdio.h>

#include <random>
#include <vector>

#include "../../storage-engine_amd/csrc/lset_lists_plan.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static const uint32_t X = kLlNone;
typedef std::vector<uint64_t> S;
typedef std::vector<uint32_t> I;

static void test_passes() {
    CHECK(lset_lists_passes(0) == 1);
    CHECK(lset_lists_passes(1) == 1);
    CHECK(lset_lists_passes(2) == 1);
    CHECK(lset_lists_passes(256) == 1);
    CHECK(lset_lists_passes(257) == 2);
    CHECK(lset_lists_passes(65536) == 2);
    CHECK(lset_lists_passes(65537) == 3);
    CHECK(lset_lists_passes(1ull << 24) == 3);
    CHECK(lset_lists_passes((1ull << 24) + 1) == 4);
    CHECK(lset_lists_passes(0xFFFFFFFFull) == 4);
    // every ordinal below G fits the passes' digits
    for (uint64_t G : {1ull, 2ull, 255ull, 256ull, 257ull, 5000ull, 65536ull, 65537ull, 0xFFFFFFFFull})
        CHECK(lset_lists_passes(G) * kLlRadixBits >= 32 || ((G - 1) >> (lset_lists_passes(G) * kLlRadixBits)) == 0);
}

static void check_layout(uint64_t n, uint32_t R, uint64_t G) {
    const LsetListsPlan p = lset_lists_plan(n, R, G);
    CHECK(p.passes == lset_lists_passes(G));
    CHECK(p.tiles_per_row == (n + kLlTile - 1) / kLlTile && p.row_stride == p.tiles_per_row * kLlTile);
    CHECK(p.row_stride >= n && p.row_stride - n < kLlTile);
    CHECK(p.ntiles == R * p.tiles_per_row && p.pairs == R * n);
    uint64_t end = 0, sum = 0;
    for (int i = 0; i < LsetListsPlan::kRegions; i++) {
        CHECK(p.reg[i].off % kLlAlign == 0 && kLlAlign % 16 == 0);
        CHECK(p.reg[i].off >= end);  // in order, so disjoint
        end = p.reg[i].off + p.reg[i].bytes;
        sum += (p.reg[i].bytes + kLlAlign - 1) / kLlAlign * kLlAlign;
    }
    CHECK(end <= p.work_bytes && sum == p.work_bytes);
    CHECK(p.reg[LsetListsPlan::kMeta].bytes == (kLlDigits + 1) * 8);
    CHECK(p.reg[LsetListsPlan::kCounts].bytes == kLlDigits * p.ntiles * 8);
    CHECK(p.reg[LsetListsPlan::kAns].bytes == R * p.row_stride * 4);
    CHECK(p.reg[LsetListsPlan::kAns].bytes >= p.pairs * 4);  // it is the second key buffer too
    CHECK(p.reg[LsetListsPlan::kKeyA].bytes == p.pairs * 4);
    const uint64_t vals = p.passes > 1 ? p.pairs * 4 : 0;
    CHECK(p.reg[LsetListsPlan::kValA].bytes == vals && p.reg[LsetListsPlan::kValB].bytes == vals);
}

static void test_layout() {
    for (uint64_t n : {1ull, 63ull, 2047ull, 2048ull, 2049ull, 70001ull, 10000000ull, 0xFFFFFFFFull})
        for (uint32_t R : {1u, 3u, 8u})
            for (uint64_t G : {1ull, 256ull, 257ull, 65537ull}) check_layout(n, R, G);
    CHECK(lset_lists_plan(0, 3, 10).work_bytes == 0);
    CHECK(lset_lists_plan(10, 0, 0).work_bytes == 0);
    CHECK(lset_lists_plan(10, 3, 0).work_bytes == 0);
    CHECK(lset_lists_plan(0xFFFFFFFFull, 8, 1).ntiles <= 0xFFFFFFFFull);  // a grid dimension
}

static void both(const I& ord, uint32_t R, uint64_t n, uint64_t G, const S& es, const I& ei) {
    S s;
    I x;
    lset_lists_ref(ord.data(), R, n, n, G, &s, &x);
    CHECK(s == es);
    CHECK(x == ei);
    lset_lists_radix_ref(ord.data(), R, n, n, G, &s, &x);
    CHECK(s == es);
    CHECK(x == ei);
}

static void test_ref_by_hand() {
    // all NONE
    both({X, X, X, X}, 1, 4, 3, {0, 0, 0, 0}, {});
    both({X, X, X, X, X, X}, 2, 3, 2, {0, 0, 0}, {});
    // one table takes everything
    both({0, 0, 0, 0, 0}, 1, 5, 1, {0, 5}, {0, 1, 2, 3, 4});
    both({2, 2, 2}, 1, 3, 4, {0, 0, 0, 3, 3}, {0, 1, 2});
    // empty tables at both ends and in the middle (G = 6: tables 0, 3, 5 empty)
    both({4, 1, X, 2, 1, 4, 2}, 1, 7, 6, {0, 0, 2, 4, 4, 6, 6}, {1, 4, 3, 6, 0, 5});
    // an empty row between two non-empty rows: rows of 2, 0 and 2 tables
    // (ordinals 0-1 and 2-3), the middle row answers NONE everywhere
    both({1, 0, X, 1, X, X, X, X, 3, X, 2, 3}, 3, 4, 4, {0, 1, 3, 4, 6}, {1, 0, 3, 2, 0, 3});
    // one key listed by two rows; a padded row stride
    {
        const I ord = {0, X, 0, 77, 77, X, 1, 1, 77, 77};
        S s;
        I x;
        lset_lists_ref(ord.data(), 2, 3, 5, 2, &s, &x);
        CHECK((s == S{0, 2, 4}) && (x == I{0, 2, 1, 2}));
    }
    // n == 0, G == 0
    both({}, 3, 0, 5, {0, 0, 0, 0, 0, 0}, {});
    both({X, X}, 1, 2, 0, {0}, {});
}

static void test_ref_random() {
    std::mt19937_64 rng(7);
    for (uint64_t G : {1ull, 2ull, 255ull, 256ull, 257ull, 5000ull, 65536ull, 65537ull, 70000ull}) {
        const uint32_t R = 1 + (uint32_t)(rng() % 3);
        const uint64_t n = 3000;
        // row r owns the ordinals [G * r / R, G * (r + 1) / R)
        I ord(R * n);
        for (uint32_t r = 0; r < R; r++) {
            const uint64_t lo = G * r / R, hi = G * (r + 1) / R;
            for (uint64_t i = 0; i < n; i++)
                ord[r * n + i] = (hi == lo || rng() % 4 == 0) ? X : (uint32_t)(lo + rng() % (hi - lo));
        }
        S s, s2;
        I x, x2;
        lset_lists_ref(ord.data(), R, n, n, G, &s, &x);
        lset_lists_radix_ref(ord.data(), R, n, n, G, &s2, &x2);
        CHECK(s == s2 && x == x2);
        CHECK(s.size() == G + 1 && s[0] == 0 && s[G] == x.size());
        for (uint64_t g = 0; g < G; g++) {
            CHECK(s[g] <= s[g + 1]);
            for (uint64_t q = s[g]; q + 1 < s[g + 1]; q++) CHECK(x[q] < x[q + 1]);  // ascending
            uint32_t r = 0;
            while (g >= G * (r + 1) / R) r++;  // the row that owns g
            for (uint64_t q = s[g]; q < s[g + 1]; q++) CHECK(ord[r * n + x[q]] == g);
        }
        uint64_t hits = 0;
        for (uint32_t g : ord) hits += g != X;
        CHECK(hits == x.size());
    }
}

int main() {
    test_passes();
    test_layout();
    test_ref_by_hand();
    test_ref_random();
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

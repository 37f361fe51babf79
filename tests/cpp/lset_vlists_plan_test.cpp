// lset_vlists_plan_test.cpp — the host side of a level set's Version lists
// probe (storage-engine_amd/csrc/lset_vlists_plan.hpp): the mask row width at
// its edges, the workspace layout (regions aligned, disjoint, inside
// work_bytes, the rows' plan at the front) and lset_vlists_ref, the plain
// statement of the transform, against a brute-force scan per table.
// No HIP: a stand-alone host program (tests/test_lset_version_lists.py builds
// it plain and with -fsanitize=address,undefined and runs it).
#include <stdio.h>

#include <algorithm>
#include <random>
#include <utility>
#include <vector>

#include "../../storage-engine_amd/csrc/lset_vlists_plan.hpp"

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

static void test_row_bytes() {
    const std::pair<uint32_t, uint32_t> want[] = {{0, 1}, {1, 1}, {8, 1},  {9, 2}, {16, 2},
                                                  {17, 4}, {32, 4}, {33, 8}, {64, 8}};
    for (const auto& w : want) {
        CHECK(lset_vlists_row_bytes(w.first) == w.second);
        CHECK(w.first <= 8 * lset_vlists_row_bytes(w.first));                                   // covers T0
        CHECK(w.second == 1 || w.first > 4 * w.second);                                         // and is the narrowest
        CHECK(__builtin_popcountll(lset_vlists_live(w.first)) == (int)w.first);
        CHECK(w.first == 64 || (lset_vlists_live(w.first) >> w.first) == 0);
    }
}

static void check_layout(uint64_t n, uint32_t T0, uint32_t R, uint64_t G) {
    const LsetVlistsPlan p = lset_vlists_plan(n, T0, R, G);
    const LsetListsPlan rows = lset_lists_plan(n, R, G);
    CHECK(p.V == T0 + G && p.rb == lset_vlists_row_bytes(T0) && p.live == lset_vlists_live(T0));
    CHECK(p.rows.work_bytes == rows.work_bytes && p.rows.row_stride == rows.row_stride && p.rows.passes == rows.passes);
    CHECK(p.entries == (uint64_t)T0 * n + (R && G ? R * n : 0));
    if (T0 == 0) {  // the rows' plan alone
        CHECK(p.work_bytes == rows.work_bytes);
        return;
    }
    CHECK(p.work_bytes > 0);
    // the rows' regions keep their offsets; the three L0 regions follow them
    uint64_t end = 0;
    for (int i = 0; i < LsetListsPlan::kRegions; i++) {
        CHECK(p.rows.reg[i].off == rows.reg[i].off && p.rows.reg[i].bytes == rows.reg[i].bytes);
        end = std::max(end, rows.reg[i].off + rows.reg[i].bytes);
    }
    CHECK(end <= rows.work_bytes);
    end = rows.work_bytes;
    uint64_t sum = rows.work_bytes;
    for (int i = 0; i < LsetVlistsPlan::kRegions; i++) {
        CHECK(p.reg[i].off % kLlAlign == 0 && kLlAlign % 16 == 0);
        CHECK(p.reg[i].off >= end);  // in order, so disjoint
        end = p.reg[i].off + p.reg[i].bytes;
        sum += (p.reg[i].bytes + kLlAlign - 1) / kLlAlign * kLlAlign;
    }
    CHECK(end <= p.work_bytes && sum == p.work_bytes);
    CHECK(p.reg[LsetVlistsPlan::kMask].bytes == n * p.rb);
    CHECK(p.reg[LsetVlistsPlan::kTiles].bytes == fset_lists_tile_bytes(n, p.live));
    CHECK(p.reg[LsetVlistsPlan::kTiles].bytes >= (uint64_t)T0 * ((n + kListTile - 1) / kListTile) * 4);
    CHECK(p.reg[LsetVlistsPlan::kStarts].bytes == 65 * 8);
}

static void test_layout() {
    for (uint64_t n : {1ull, 63ull, 1023ull, 1024ull, 1025ull, 2047ull, 2048ull, 2049ull, 70001ull, 10000000ull,
                       0xFFFFFFFFull})
        for (uint32_t T0 : {0u, 1u, 8u, 9u, 16u, 17u, 32u, 33u, 64u})
            for (uint32_t R : {0u, 1u, 3u, 8u})
                for (uint64_t G : {0ull, 1ull, 256ull, 257ull, 65537ull}) {
                    if (R == 0 && G) continue;
                    check_layout(n, T0, R, G);
                }
    CHECK(lset_vlists_plan(0, 5, 3, 10).work_bytes == 0);
    CHECK(lset_vlists_plan(10, 0, 0, 0).work_bytes == 0);
    CHECK(lset_vlists_plan(10, 0, 3, 0).work_bytes == 0);
    CHECK(lset_vlists_plan(10, 3, 0, 0).work_bytes > 0 && lset_vlists_plan(10, 3, 0, 0).rows.work_bytes == 0);
    CHECK(lset_vlists_plan(10, 3, 2, 0).work_bytes == lset_vlists_plan(10, 3, 0, 0).work_bytes);
    CHECK(fset_lists_tile_bytes(1024, 0xFF) == 8 * 4 * 4 && fset_lists_tile_bytes(1025, 1) == 4 * 4);
    CHECK(fset_lists_tile_bytes(4097, ~0ull) == 64 * 8 * 4);
}

// Per Version ordinal, a scan over every key.
static void brute(const S& mask, uint32_t T0, const I& ord, uint32_t R, uint64_t n, uint64_t stride, uint64_t G, S* s,
                  I* x) {
    s->assign(T0 + G + 1, 0);
    x->clear();
    for (uint64_t v = 0; v < T0 + G; v++) {
        (*s)[v] = x->size();
        for (uint64_t i = 0; i < n; i++) {
            bool hit = false;
            if (v < T0)
                hit = (mask[i] >> v) & 1;
            else
                for (uint32_t r = 0; r < R; r++) hit = hit || ord[r * stride + i] == v - T0;
            if (hit) x->push_back((uint32_t)i);
        }
    }
    (*s)[T0 + G] = x->size();
}

static void test_ref_by_hand() {
    // T0 = 2, one row of 2 tables, 3 keys
    const S mask = {1, 3, 2};
    const I ord = {1, X, 0};
    S s;
    I x;
    lset_vlists_ref(mask.data(), 2, ord.data(), 1, 3, 3, 2, &s, &x);
    CHECK((s == S{0, 2, 4, 5, 6}) && (x == I{0, 1, 1, 2, 2, 0}));
}

static void test_ref_random() {
    std::mt19937_64 rng(11);
    const uint64_t ns[] = {0, 1, 1023, 1024, 1025, 2047, 2048, 2049};
    for (uint32_t T0 : {0u, 1u, 8u, 9u, 33u, 64u})
        for (uint64_t G : {0ull, 1ull, 7ull, 300ull})
            for (uint64_t n : ns) {
                const uint32_t R = G ? 1 + (uint32_t)(rng() % 3) : (uint32_t)(rng() % 2);
                const uint64_t stride = n + rng() % 5;
                S mask(n);
                for (auto& m : mask) {
                    m = rng() & rng();
                    if (T0 < 64) m &= (1ull << T0) - 1;
                }
                I ord(R * stride + 1, 77);
                for (uint32_t r = 0; r < R; r++) {
                    const uint64_t lo = G * r / R, hi = G * (r + 1) / R;  // row r owns the ordinals [lo, hi)
                    for (uint64_t i = 0; i < n; i++)
                        ord[r * stride + i] = (hi == lo || rng() % 3 == 0) ? X : (uint32_t)(lo + rng() % (hi - lo));
                }
                S s, s2;
                I x, x2;
                lset_vlists_ref(mask.data(), T0, ord.data(), R, n, stride, G, &s, &x);
                brute(mask, T0, ord, R, n, stride, G, &s2, &x2);
                CHECK(s == s2);
                CHECK(x == x2);
                CHECK(s.size() == T0 + G + 1 && s[0] == 0 && s[T0 + G] == x.size());
                uint64_t bits = 0;
                for (uint64_t m : mask) bits += __builtin_popcountll(m);
                CHECK(s[T0] == bits);  // the L0 entries
            }
}

int main() {
    test_row_bytes();
    test_layout();
    test_ref_by_hand();
    test_ref_random();
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

// lset_walk_plan_test.cpp — the host side of a level set's walk probe
// (storage-engine_amd/csrc/lset_walk_plan.hpp): the step-to-position and
// step-to-row mapping at its edges, the allowed-positions mask up to the
// 64-bit edge, the lists form's workspace against lset_lists_plan(n, 1, V),
// and lset_walk_ref, the plain statement of the per-key answer and the lists,
// against a brute-force walk over every step.
// No HIP: a stand-alone host program (tests/test_lset_walk.py builds it plain
// and with -fsanitize=address,undefined and runs it).
#include <stdio.h>

#include <random>
#include <vector>

#include "../../storage-engine_amd/csrc/lset_walk_plan.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static const uint32_t X = kWalkNone;
typedef std::vector<uint64_t> S;
typedef std::vector<uint32_t> I;

// Bit p set iff position p is consulted at some step w >= from: one step at a time.
static uint64_t allowed_by_steps(uint32_t T0, uint32_t from) {
    uint64_t m = 0;
    for (uint32_t w = from; w < T0; w++) m |= 1ull << lset_walk_l0_pos(T0, w);
    return m;
}

static void test_mapping() {
    static_assert(kWalkNone == 0xFFFFFFFFu, "LSMB_LSET_NONE");
    static_assert(lset_walk_allowed(64, 0) == ~0ull, "constexpr: the kernel calls the same functions");
    for (uint32_t T0 : {0u, 1u, 63u, 64u})
        for (uint32_t R : {0u, 1u, 3u, 8u}) {
            const uint32_t W = lset_walk_steps(T0, R);
            CHECK(W == T0 + R);
            // every step consults one thing, L0 newest first, then the rows in order
            for (uint32_t w = 0; w < W; w++) {
                if (w < T0) {
                    const uint32_t p = lset_walk_l0_pos(T0, w);
                    CHECK(p < T0 && p == T0 - 1 - w && lset_walk_l0_step(T0, p) == w);
                } else {
                    CHECK(lset_walk_first_row(T0, w) == w - T0 && lset_walk_row_step(T0, w - T0) == w);
                }
            }
            if (T0) CHECK(lset_walk_l0_pos(T0, 0) == T0 - 1 && lset_walk_l0_pos(T0, T0 - 1) == 0);
            // the resume points of the issue: 0, T0-1, T0, W-1, W, NONE (and their neighbours)
            std::vector<uint32_t> froms = {0, T0, W, W + 1, X, X - 1};
            if (T0) froms.push_back(T0 - 1);
            if (W) froms.push_back(W - 1);
            for (uint32_t f : froms) {
                const uint64_t a = lset_walk_allowed(T0, f);
                CHECK(a == allowed_by_steps(T0, f));
                CHECK(f < T0 ? __builtin_popcountll(a) == (int)(T0 - f) : a == 0);
                CHECK(T0 == 64 || (a >> T0) == 0);
                CHECK(lset_walk_first_row(T0, f) == (f > T0 ? f - T0 : 0));
            }
            // every resume point inside L0
            for (uint32_t f = 0; f < T0; f++) CHECK(lset_walk_allowed(T0, f) == allowed_by_steps(T0, f));
        }
    // the 64-bit edge: T0 - from == 64 is every bit, 63 all but the newest
    CHECK(lset_walk_allowed(64, 0) == ~0ull);
    CHECK(lset_walk_allowed(64, 1) == ~0ull >> 1);
    CHECK(lset_walk_allowed(64, 63) == 1);
    CHECK(lset_walk_allowed(64, 64) == 0);
    CHECK(lset_walk_allowed(63, 0) == ~0ull >> 1);
    CHECK(lset_walk_allowed(1, 0) == 1 && lset_walk_allowed(1, 1) == 0);
    CHECK(lset_walk_allowed(0, 0) == 0 && lset_walk_allowed(0, X) == 0 && lset_walk_allowed(64, X) == 0);
}

static void test_workspace() {
    for (uint64_t n : {0ull, 1ull, 2047ull, 2048ull, 2049ull, 70001ull, 10000000ull, 0xFFFFFFFFull})
        for (uint64_t V : {0ull, 1ull, 64ull, 256ull, 257ull, 65536ull, 65537ull, 0xFFFFFFFFull}) {
            const LsetListsPlan p = lset_walk_lists_plan(n, V), q = lset_lists_plan(n, 1, V);
            CHECK(p.work_bytes == q.work_bytes && p.R == 1 && p.G == V && p.n == n);
            CHECK(p.passes == q.passes && p.row_stride == q.row_stride && p.ntiles == q.ntiles && p.pairs == q.pairs);
            for (int i = 0; i < LsetListsPlan::kRegions; i++)
                CHECK(p.reg[i].off == q.reg[i].off && p.reg[i].bytes == q.reg[i].bytes);
            CHECK((p.work_bytes == 0) == (n == 0 || V == 0));
            if (p.work_bytes) {
                CHECK(p.pairs == n && p.row_stride >= n && p.row_stride % kLlTile == 0);  // at most one entry per key
                CHECK(p.reg[LsetListsPlan::kAns].bytes == p.row_stride * 4);              // the one answer row
                CHECK(p.reg[LsetListsPlan::kAns].off % 16 == 0);
            }
        }
}

// The walk one step at a time: what DB::get does with the filters' answers.
static void brute(const S& mask, uint32_t T0, const I& ord, uint32_t R, uint64_t n, uint64_t stride, const uint32_t* from,
                  I* step, I* ordv) {
    step->assign(n, X);
    ordv->assign(n, X);
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t w = from ? from[i] : 0; w < (uint64_t)T0 + R; w++) {
            uint32_t v = X;
            if (w < T0) {
                const uint32_t p = T0 - 1 - (uint32_t)w;
                if ((mask[i] >> p) & 1) v = p;
            } else if (ord[(w - T0) * stride + i] != X) {
                v = T0 + ord[(w - T0) * stride + i];
            }
            if (v == X) continue;
            (*step)[i] = (uint32_t)w;
            (*ordv)[i] = v;
            break;
        }
}

static void test_ref_by_hand() {
    // T0 = 2 (step 0 = position 1, step 1 = position 0), one row of 2 tables (step 2), 4 keys
    const S mask = {1, 3, 2, 0};
    const I ord = {1, X, 0, X};
    I step, ordv;
    lset_walk_ref(mask.data(), 2, ord.data(), 1, 4, 4, nullptr, &step, &ordv);
    CHECK((step == I{1, 0, 0, X}) && (ordv == I{0, 1, 1, X}));
    const I from = {2, 1, 1, 0};  // resumed: key 0 at the row, keys 1 and 2 past position 1
    lset_walk_ref(mask.data(), 2, ord.data(), 1, 4, 4, from.data(), &step, &ordv);
    CHECK((step == I{2, 1, 2, X}) && (ordv == I{3, 0, 2, X}));
    S s;
    I x;
    lset_walk_lists_ref(ordv, 4, &s, &x);
    CHECK((s == S{0, 1, 1, 2, 3}) && (x == I{1, 2, 0}));
    const I retired = {3, X, 2, 7};
    lset_walk_ref(mask.data(), 2, ord.data(), 1, 4, 4, retired.data(), &step, &ordv);
    CHECK((step == I{X, X, 2, X}) && (ordv == I{X, X, 2, X}));
}

static void test_ref_random() {
    std::mt19937_64 rng(12);
    for (uint32_t T0 : {0u, 1u, 2u, 7u, 63u, 64u})
        for (uint32_t R : {0u, 1u, 3u, 8u})
            for (uint64_t n : {0ull, 1ull, 65ull, 700ull})
                for (int sparse = 0; sparse < 2; sparse++) {
                    const uint32_t W = T0 + R;
                    const uint64_t stride = n + rng() % 5;
                    const uint64_t G = R ? 5 * R : 0;  // row r owns the rows' ordinals [5r, 5r + 5)
                    S mask(n);
                    for (auto& m : mask) {
                        m = sparse ? rng() & rng() & rng() & rng() : rng();
                        if (T0 < 64) m &= (1ull << T0) - 1;
                    }
                    I ord(R * stride + 1, 77);
                    for (uint32_t r = 0; r < R; r++)
                        for (uint64_t i = 0; i < n; i++)
                            ord[r * stride + i] = rng() % (sparse ? 4 : 2) ? X : (uint32_t)(5 * r + rng() % 5);
                    I from(n);
                    for (auto& f : from) f = rng() % 7 == 0 ? X : (uint32_t)(rng() % (W + 3));
                    for (const uint32_t* f : {(const uint32_t*)nullptr, (const uint32_t*)from.data()}) {
                        I step, ordv, step2, ordv2;
                        lset_walk_ref(mask.data(), T0, ord.data(), R, n, stride, f, &step, &ordv);
                        brute(mask, T0, ord, R, n, stride, f, &step2, &ordv2);
                        CHECK(step == step2);
                        CHECK(ordv == ordv2);
                        S s;
                        I x;
                        lset_walk_lists_ref(ordv, T0 + G, &s, &x);
                        CHECK(s.size() == T0 + G + 1 && s[0] == 0 && s[T0 + G] == x.size() && x.size() <= n);
                        uint64_t hits = 0;
                        for (uint64_t i = 0; i < n; i++) {
                            CHECK((step[i] == X) == (ordv[i] == X));
                            if (step[i] == X) continue;
                            hits++;
                            CHECK(step[i] >= (f ? f[i] : 0) && step[i] < W && ordv[i] < T0 + G);
                            CHECK(step[i] < T0 ? ordv[i] == T0 - 1 - step[i] : (ordv[i] - T0) / 5 == step[i] - T0);
                        }
                        CHECK(hits == x.size());
                        for (uint64_t v = 0; v < T0 + G; v++)
                            for (uint64_t e = s[v]; e < s[v + 1]; e++) {
                                CHECK(ordv[x[e]] == v);
                                CHECK(e == s[v] || x[e - 1] < x[e]);
                            }
                    }
                }
}

int main() {
    test_mapping();
    test_workspace();
    test_ref_by_hand();
    test_ref_random();
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

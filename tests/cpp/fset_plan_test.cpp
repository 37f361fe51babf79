// fset_plan_test.cpp — the host planning shared by filter sets and a level
// set's L0 part (storage-engine_amd/csrc/fset_plan.hpp) on a CPU: the region
// masks, the size classes and fset_plan_answer, the plain statement of what the
// kernels answer per key, against brute force over random overlapping ranges
// (every table's range compared byte-wise, every filter probed by a literal
// (h1 + i * h2) % num_bits loop of the test's own, src/bloom/mod.rs:82-94).
// A stand-alone program (tests/test_lset_version.py builds it with
// -fsanitize=address,undefined and runs it).
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../storage-engine_amd/csrc/fset_plan.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

struct Tab {
    std::string lo, hi;
    uint32_t num_bits, k;
    std::vector<uint64_t> words;
};

// The test's own filter arithmetic: wrapping sums and a plain `%`.
static void positions(const std::string& key, uint32_t nb, uint32_t k, std::vector<uint64_t>* out) {
    const H128 h = xxh3_128(u8(key), key.size());
    out->clear();
    for (uint32_t i = 0; i < k; i++) out->push_back((h.lo + (uint64_t)i * h.hi) % nb);
}
static void insert(Tab* t, const std::string& key) {
    std::vector<uint64_t> p;
    positions(key, t->num_bits, t->k, &p);
    for (uint64_t x : p) t->words[x >> 6] |= 1ull << (x & 63);
}
static bool may_contain(const Tab& t, const std::string& key) {
    std::vector<uint64_t> p;
    positions(key, t.num_bits, t.k, &p);
    for (uint64_t x : p)
        if (!((t.words[x >> 6] >> (x & 63)) & 1)) return false;
    return true;
}
static bool in_range(const Tab& t, const std::string& key) {
    return bytes_cmp(u8(t.lo), t.lo.size(), u8(key), key.size()) <= 0 &&
           bytes_cmp(u8(key), key.size(), u8(t.hi), t.hi.size()) <= 0;
}

// (num_bits, k): SST-sized (new(1000, 0.01)), tiny, too large for the LDS
// tables, k > 8, and a filter of no hash.
static const uint32_t kGeom[][2] = {{9586, 7}, {384, 7}, {383445, 7}, {767, 13}, {0, 0}};

static std::string rkey(std::mt19937_64& rng) {
    // a small alphabet and short lengths, so that bounds and keys collide,
    // nest and extend each other; some share a 16-byte prefix and go on
    static const char* pre16 = "shared-prefix-16";
    std::string s;
    const int kind = (int)(rng() % 8);
    if (kind == 0) s = pre16;
    const int len = (int)(rng() % (kind == 0 ? 9 : 5));
    for (int i = 0; i < len; i++) s.push_back("ab\0\xff"[rng() % 4]);
    return s;
}

static void one_set(uint32_t T0, bool mixed, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<Tab> tabs(T0);
    for (uint32_t d = 0; d < T0; d++) {
        Tab& t = tabs[d];
        std::string a = rkey(rng), b = rkey(rng);
        if (bytes_cmp(u8(a), a.size(), u8(b), b.size()) > 0) std::swap(a, b);
        t.lo = a;
        t.hi = b;
        if (d == 1) t.lo = tabs[0].lo, t.hi = tabs[0].hi;                       // identical ranges
        if (d == 2) t.lo = "", t.hi = std::string(24, '\xff');                   // spans everything, an empty-string bound
        if (d == 3) t.lo = tabs[0].hi, t.hi = tabs[0].hi + "b";                  // touches table 0 at one key
        if (d == 4) t.lo = "shared-prefix-16aa", t.hi = "shared-prefix-16ab\xff";  // long bounds sharing their first 16
        if (d == 5) t.lo = "shared-prefix-16", t.hi = "shared-prefix-16ab";      // nests table 4's lower part
        if (d == 6) t.lo = t.hi = "a";                                           // a one-key range
        const uint32_t* g = kGeom[mixed ? d % 5 : 0];
        t.num_bits = g[0];
        t.k = g[1];
        t.words.assign(((uint64_t)t.num_bits + 63) / 64 + 1, 0);
    }
    // members: keys inside the range, when it has room
    std::vector<std::string> q;
    for (uint32_t d = 0; d < T0; d++)
        for (int i = 0; i < 6; i++) {
            std::string m = i == 0 ? tabs[d].lo : i == 1 ? tabs[d].hi : tabs[d].lo + rkey(rng);
            if (tabs[d].k && in_range(tabs[d], m)) insert(&tabs[d], m);
            q.push_back(m);
        }
    std::vector<FsetPlanTable> pt;
    std::vector<const uint64_t*> words;
    for (const Tab& t : tabs) {
        pt.push_back(FsetPlanTable{u8(t.lo), t.lo.size(), u8(t.hi), t.hi.size(), t.num_bits, t.k});
        words.push_back(t.words.data());
    }
    FsetPlan pl;
    fset_plan(pt.data(), T0, &pl);
    // the points: sorted, distinct, at most two per table; blob and prefixes agree
    CHECK(pl.points.size() == pl.pts.size() && pl.pts.size() <= 2 * (size_t)T0);
    CHECK(pl.regmask.size() == 2 * pl.pts.size() + 1);
    for (size_t j = 0; j < pl.pts.size(); j++) {
        const auto& p = pl.pts[j];
        if (j) CHECK(bytes_cmp(pl.pts[j - 1].data(), pl.pts[j - 1].size(), p.data(), p.size()) < 0);
        const size_t at = (size_t)(uintptr_t)pl.points[j].p;
        CHECK(pl.points[j].len == p.size() && at + p.size() <= pl.blob.size());
        CHECK(p.empty() || memcmp(pl.blob.data() + at, p.data(), p.size()) == 0);
        const HostPfx16 px = host_prefix16(p.data(), p.size());
        CHECK(pl.points[j].w0 == px.w0 && pl.points[j].w1 == px.w1);
    }
    // the classes: every k > 0 table in exactly one class or walked; tables apart and within the LDS budget
    uint64_t seen = 0;
    CHECK(pl.cl.ncls <= kFsetMaxClasses && pl.cl.table_bytes <= kFsetTableBytes);
    for (uint32_t c = 0; c < pl.cl.ncls; c++) {
        const FsetClass& C = pl.cl.cls[c];
        CHECK(C.nmem >= 1 && C.nmem <= 8 * C.width && C.k > 0 && (C.off & 15) == 0);
        const uint64_t bytes = (((uint64_t)C.num_bits + 31) / 32) * 32 * C.width;
        CHECK(C.off + bytes <= pl.cl.table_bytes);
        if (c) {
            const FsetClass& P = pl.cl.cls[c - 1];
            CHECK(P.off + (((uint64_t)P.num_bits + 31) / 32) * 32 * P.width <= C.off);
        }
        uint64_t m = 0;
        for (uint32_t j = 0; j < C.nmem; j++) {
            CHECK(C.mem[j] < T0 && tabs[C.mem[j]].num_bits == C.num_bits && tabs[C.mem[j]].k == C.k);
            m |= 1ull << C.mem[j];
        }
        CHECK(m == C.mask && !(seen & m));
        seen |= m;
    }
    CHECK(!(seen & pl.cl.walk_mask));
    for (uint32_t d = 0; d < T0; d++) CHECK(((seen | pl.cl.walk_mask) >> d) & 1);
    if (T0 && !mixed) {  // one class; 64 members take 8-byte entries, 9 600 of them: past the 64 KiB of tables
        CHECK(pl.shared_nb == kGeom[0][0] && pl.shared_k == kGeom[0][1]);
        CHECK(T0 == 64 ? pl.cl.ncls == 0 && pl.cl.walk_mask == ~0ull : pl.cl.ncls == 1 && pl.cl.walk_mask == 0);
    }
    if (T0 > 5 && mixed) CHECK(pl.shared_nb == 0 && pl.cl.walk_mask != 0 && pl.cl.ncls >= 2);
    // keys: the members, every bound and its neighbours, random strings
    for (uint32_t d = 0; d < T0; d++)
        for (const std::string& b : {tabs[d].lo, tabs[d].hi}) {
            q.push_back(b);
            q.push_back(b + std::string(1, '\0'));
            q.push_back(b + "\xff");
            if (!b.empty()) q.push_back(b.substr(0, b.size() - 1));
            if (b.size() > 16) q.push_back(b.substr(0, 16));
        }
    for (int i = 0; i < 400; i++) q.push_back(rkey(rng));
    q.push_back("");
    q.push_back(std::string(40, '\xff'));
    uint64_t in_and_out = 0, multi = 0;
    for (const std::string& key : q) {
        uint64_t in = 0, ans = 0;
        for (uint32_t d = 0; d < T0; d++)
            if (in_range(tabs[d], key)) {
                in |= 1ull << d;
                if (may_contain(tabs[d], key)) ans |= 1ull << d;
            }
        const uint32_t reg = fset_plan_region(pl, u8(key), key.size());
        CHECK(reg < pl.regmask.size());
        if (reg >= pl.regmask.size()) continue;
        if (pl.regmask[reg] != in) {
            fprintf(stderr, "T0 %u seed %llu: region mask %llx, brute force %llx\n", T0, (unsigned long long)seed,
                    (unsigned long long)pl.regmask[reg], (unsigned long long)in);
            g_fail++;
        }
        const uint64_t got = fset_plan_answer(pl, pt.data(), words.data(), u8(key), key.size());
        if (got != ans) {
            fprintf(stderr, "T0 %u seed %llu: answer %llx, brute force %llx\n", T0, (unsigned long long)seed,
                    (unsigned long long)got, (unsigned long long)ans);
            g_fail++;
        }
        in_and_out += in != ans;
        multi += (ans & (ans - 1)) != 0;
    }
    if (T0 >= 8) CHECK(in_and_out > 0 && multi > 0);  // filters do mask in-range keys out; ranges do overlap
}

int main() {
    for (uint32_t T0 : {0u, 1u, 8u, 9u, 64u})
        for (int mixed = 0; mixed < 2; mixed++)
            for (uint64_t seed = 1; seed <= 6; seed++) one_set(T0, mixed != 0, 1000 * T0 + 10 * seed + mixed);
    // descriptors
    const RangedFilter r = fset_plan_desc((const uint32_t*)0x40, 9586, 7, 5);
    CHECK(r.f.words32 == (const uint32_t*)0x40 && r.f.num_bits == 9586 && r.f.k == 7 && r.f.out_bit == 5 && r.f.md.d == 9586);
    CHECK(fset_plan_desc(nullptr, 0, 0, 0).f.md.d == 1);  // a filter of no bits never divides by zero
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

// lset_order_test.cpp — the host side of a level set's rows
// (storage-engine_amd/csrc/lset_order.hpp): the order lsmb_lset_seal gives a
// row, every way it rejects one, and the plain search (prefix lower bound,
// tie-break, min check) against brute force over all tables.  No HIP: a
// stand-alone host program (tests/test_lset.py builds it with
// -fsanitize=address,undefined and runs it).
#include <stdio.h>

#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../storage-engine_amd/csrc/lset_order.hpp"

using namespace lsmb;
typedef std::pair<std::string, std::string> Range;  // [min_key, max_key]

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

static std::vector<LsetRange> ranges_of(const std::vector<Range>& t, const std::vector<uint32_t>& ids) {
    std::vector<LsetRange> r;
    for (size_t j = 0; j < t.size(); j++)
        r.push_back(LsetRange{u8(t[j].first), t[j].first.size(), u8(t[j].second), t[j].second.size(), ids[j]});
    return r;
}

// ok, or the two ids the rejection names
struct Verdict {
    bool ok;
    uint32_t a, b;
    bool inverted;
};
static Verdict order_of(const std::vector<Range>& t, std::vector<uint32_t>* order = nullptr) {
    std::vector<uint32_t> ids;
    for (size_t j = 0; j < t.size(); j++) ids.push_back(100 + (uint32_t)j);
    const std::vector<LsetRange> r = ranges_of(t, ids);
    std::vector<uint32_t> ord;
    LsetOrderError e;
    const bool ok = lset_order_row(r.data(), (uint32_t)r.size(), &ord, &e);
    if (order) *order = ord;
    return Verdict{ok, e.id_a, e.id_b, e.inverted};
}
static bool names(const Verdict& v, uint32_t x, uint32_t y) {
    return !v.ok && ((v.a == x && v.b == y) || (v.a == y && v.b == x));
}

static const std::string kP16 = "0123456789abcdef";  // a shared 16-byte prefix

static void test_rejections() {
    CHECK(order_of({}).ok);
    CHECK(order_of({{"a", "a"}}).ok);  // one-key table
    CHECK(order_of({{"", ""}, {std::string(1, '\0'), "b"}}).ok);  // the empty key below everything
    // equal neighbour bounds: max_t == min_{t+1}
    CHECK(names(order_of({{"a", "c"}, {"c", "e"}}), 100, 101));
    CHECK(names(order_of({{"c", "e"}, {"a", "c"}}), 100, 101));
    CHECK(order_of({{"a", "c"}, {"d", "e"}}).ok);
    // a range containing another
    CHECK(names(order_of({{"a", "z"}, {"c", "d"}}), 100, 101));
    CHECK(names(order_of({{"m", "n"}, {"c", "d"}, {"a", "z"}}), 102, 101));  // first bad pair in sorted order
    // partial overlap, equal minima
    CHECK(names(order_of({{"a", "m"}, {"k", "z"}}), 100, 101));
    CHECK(names(order_of({{"a", "b"}, {"a", "c"}}), 100, 101));
    // min > max
    {
        const Verdict v = order_of({{"a", "b"}, {"q", "p"}, {"x", "y"}});
        CHECK(!v.ok && v.inverted && v.a == 101 && v.b == 101);
    }
    // bounds that differ only past byte 16
    CHECK(order_of({{kP16 + "aaaa", kP16 + "bbbb"}, {kP16 + "bbbc", kP16 + "cccc"}}).ok);
    CHECK(names(order_of({{kP16 + "aaaa", kP16 + "bbbb"}, {kP16 + "bbbb", kP16 + "cccc"}}), 100, 101));
    CHECK(names(order_of({{kP16 + "aaaa", kP16 + "bbbd"}, {kP16 + "bbbc", kP16 + "cccc"}}), 100, 101));
    {
        const Verdict v = order_of({{kP16 + "b", kP16 + "a"}});
        CHECK(!v.ok && v.inverted && v.a == 100);
    }
    // a bound that is a proper prefix of the next: the prefix sorts first, so
    // max = "abc" below min = "abcd" (or "abc\0") is in order, the reverse is not
    CHECK(order_of({{"aa", "abc"}, {"abcd", "b"}}).ok);
    CHECK(order_of({{"aa", "abc"}, {std::string("abc\0", 4), "b"}}).ok);
    CHECK(names(order_of({{"aa", "abcd"}, {"abc", "b"}}), 100, 101));
    CHECK(names(order_of({{"aa", std::string("abc\0", 4)}, {"abc", "b"}}), 100, 101));
    CHECK(order_of({{kP16, kP16}, {kP16 + std::string(1, '\0'), kP16 + "x"}}).ok);
    CHECK(names(order_of({{kP16, kP16 + "x"}, {kP16, kP16}}), 100, 101));
}

// `count` distinct byte strings of one style, sorted:
//   0: shorter than 16 bytes (1..15), small alphabet with zero bytes
//   1: exactly 16 bytes
//   2: 17..40 bytes, the first 16 from a pool of few prefixes
//   3: all of these mixed
static std::vector<std::string> bounds_of(int style, size_t count, std::mt19937_64& rng) {
    std::vector<std::string> pool;
    for (int j = 0; j < 5; j++) {
        std::string p(16, 0);
        for (auto& c : p) c = (char)(rng() % 4 == 0 ? 0 : 'a' + rng() % 3);
        pool.push_back(p);
    }
    std::set<std::string> s;
    while (s.size() < count) {
        const int st = style == 3 ? (int)(rng() % 3) : style;
        std::string b;
        if (st == 0) {
            b.resize(1 + rng() % 15);
            for (auto& c : b) c = (char)(rng() % 5 == 0 ? 0 : (rng() % 7 == 0 ? 0xff : 'a' + rng() % 4));
        } else if (st == 1) {
            b.resize(16);
            for (auto& c : b) c = (char)(rng() % 6 == 0 ? 0 : 'a' + rng() % 3);
        } else {
            b = pool[rng() % pool.size()];
            const size_t tail = 1 + rng() % 24;
            for (size_t j = 0; j < tail; j++) b.push_back((char)(rng() % 5 == 0 ? 0 : 'a' + rng() % 3));
        }
        s.insert(b);
    }
    std::vector<std::string> v(s.begin(), s.end());
    // std::string's < is char_traits<char>::compare: unsigned bytes, a proper prefix first
    return v;
}

static uint32_t brute(const std::vector<Range>& t, const std::string& key) {
    uint32_t hit = kLsetNoTable;
    int hits = 0;
    for (size_t j = 0; j < t.size(); j++)
        if (bytes_cmp(u8(t[j].first), t[j].first.size(), u8(key), key.size()) <= 0 &&
            bytes_cmp(u8(key), key.size(), u8(t[j].second), t[j].second.size()) <= 0) {
            hit = (uint32_t)j;
            hits++;
        }
    CHECK(hits <= 1);
    return hit;
}

static void test_search(int style, size_t ntab, uint64_t seed) {
    std::mt19937_64 rng(seed);
    // 2 * ntab sorted distinct bounds, some tables of one key (min == max)
    const std::vector<std::string> b = bounds_of(style, 2 * ntab, rng);
    std::vector<Range> t;
    for (size_t j = 0; j < ntab; j++) t.push_back(rng() % 8 == 0 ? Range{b[2 * j], b[2 * j]} : Range{b[2 * j], b[2 * j + 1]});
    // added in shuffled order; ids = the position in sorted order
    std::vector<uint32_t> perm(ntab);
    for (size_t j = 0; j < ntab; j++) perm[j] = (uint32_t)j;
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<Range> shuffled;
    for (uint32_t j : perm) shuffled.push_back(t[j]);
    const std::vector<LsetRange> r = ranges_of(shuffled, perm);
    std::vector<uint32_t> order;
    LsetOrderError e;
    CHECK(lset_order_row(r.data(), (uint32_t)ntab, &order, &e));
    std::vector<LsetRange> sorted;
    std::vector<HostPfx16> pfx;
    for (size_t j = 0; j < ntab; j++) {
        sorted.push_back(r[order[j]]);
        CHECK(sorted.back().id == j);  // shuffled tables come out in min_key order
        pfx.push_back(host_prefix16(sorted.back().hi, sorted.back().hi_len));
        if (j) CHECK(!(pfx[j] < pfx[j - 1]));  // the searched array ascends
    }
    // queries: the bounds (every one, or about 800 spread over a long row) and
    // their neighbours in the order, the bounds' 16-byte prefixes, random
    // strings of the same style, the extremes
    std::vector<std::string> q = {"", std::string(1, '\0'), std::string(40, (char)0xff), std::string(16, '\0')};
    for (size_t at = 0; at < b.size(); at += b.size() > 800 ? b.size() / 800 : 1) {
        const std::string& s = b[at];
        q.push_back(s);
        q.push_back(s.substr(0, s.size() - 1));
        q.push_back(s + std::string(1, '\0'));
        q.push_back(s + "a");
        q.push_back(s.substr(0, 16));
        q.push_back(s.substr(0, 15));
        std::string up = s;
        up.back() = (char)(up.back() + 1);
        q.push_back(up);
    }
    const std::vector<std::string> rnd = bounds_of(style, 3000, rng);
    q.insert(q.end(), rnd.begin(), rnd.end());
    size_t found = 0;
    for (const auto& key : q) {
        const uint32_t got = lset_find(sorted.data(), pfx.data(), (uint32_t)ntab, u8(key), key.size());
        const uint32_t exp = brute(t, key);
        if (got != exp) {
            fprintf(stderr, "style %d, %zu tables: key of %zu bytes: got %u, expected %u\n", style, ntab, key.size(), got,
                    exp);
            g_fail++;
        }
        found += exp != kLsetNoTable;
    }
    CHECK(found > 0 && found < q.size());  // both answers occur
    CHECK(lset_find(nullptr, nullptr, 0, u8(q[1]), 1) == kLsetNoTable);  // an empty row
}

int main() {
    CHECK(bytes_cmp(u8("ab"), 2, u8("abc"), 3) < 0 && bytes_cmp(u8("b"), 1, u8("abc"), 3) > 0);
    CHECK(bytes_cmp(u8("\xff"), 1, u8("a"), 1) > 0 && bytes_cmp(nullptr, 0, nullptr, 0) == 0);
    {
        const HostPfx16 p = host_prefix16(u8("\x01\x02"), 2);
        CHECK(p.w0 == 0x0102000000000000ull && p.w1 == 0);
        const HostPfx16 l = host_prefix16(u8("0123456789abcdefXYZ"), 19);
        CHECK(l.w0 == 0x3031323334353637ull && l.w1 == 0x3839616263646566ull);
    }
    test_rejections();
    const size_t sizes[] = {1, 2, 63, 64, 65, 1000};
    uint64_t seed = 1;
    for (int style = 0; style < 4; style++)
        for (size_t n : sizes) test_search(style, n, seed++);
    printf("%s\n", g_fail ? "FAILED" : "all passed");
    return g_fail ? 1 : 0;
}

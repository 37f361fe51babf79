// lset_test.cpp — LevelSet of the C++ mirror (storage-engine_amd/cpp/lsm_bloom.hpp):
// probe() against the host's own may_contain (lsmb_may_contain, one key at a
// time) and memcmp-order range checks, over two rows of 3 and 70 tables.
// Usage: lset_test [--gpu]   (without --gpu: the argument checks only)
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../storage-engine_amd/cpp/lsm_bloom.hpp"

using lsm::bloom::BloomFilter;
using lsm::bloom::LevelSet;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static std::string key(const char* prefix, int i) {
    char k[32];
    snprintf(k, sizeof k, "%s%06d", prefix, i);
    return k;
}

// byte-string order, a proper prefix first (Rust's [u8] Ord)
static bool le(const std::string& a, const std::string& b) {
    const int c = memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
    return c < 0 || (c == 0 && a.size() <= b.size());
}

struct Table {
    uint32_t id;
    BloomFilter f;
    std::string lo, hi;
};

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        lsmb_lset* h = nullptr;
        uint32_t out[4];
        const uint8_t data[4] = {0};
        CHECK(lsmb_lset_open(nullptr, &h) == LSMB_EINVAL && h == nullptr);
        CHECK(lsmb_lset_rows(nullptr) == 0 && lsmb_lset_tables(nullptr, 0) == 0);
        CHECK(lsmb_lset_seal(nullptr) == LSMB_EINVAL);
        CHECK(lsmb_lset_probe(nullptr, data, nullptr, 1, 4, out) == LSMB_EINVAL);
        CHECK(lsmb_lset_probe_dev(nullptr, data, nullptr, 1, 4, out, nullptr) == LSMB_EINVAL);
        lsmb_lset_close(nullptr);
    }
    if (gpu) {
        // row 0: 3 tables of 300 keys; row 1: 70 tables of 30 keys; ids with gaps between tables
        std::vector<std::vector<Table>> rows(2);
        const int ntab[2] = {3, 70}, per[2] = {300, 30}, pitch[2] = {1000, 40};
        for (int r = 0; r < 2; r++)
            for (int t = 0; t < ntab[r]; t++) {
                BloomFilter f(per[r], 0.01);
                for (int i = 0; i < per[r]; i++) f.insert(key("key_", t * pitch[r] + i));
                rows[r].push_back(Table{(uint32_t)(500 * r + t + 1), std::move(f), key("key_", t * pitch[r]),
                                        key("key_", t * pitch[r] + per[r] - 1)});
            }
        LevelSet ls;
        for (int r = 1; r >= 0; r--)  // any order: last table first, half of them from the serialized block
            for (int t = ntab[r] - 1; t >= 0; t--) {
                const Table& T = rows[r][t];
                if (t % 2) ls.add(r, T.id, T.f.serialize(), T.lo, T.hi);
                else ls.add(r, T.id, T.f, T.lo, T.hi);
            }
        CHECK(ls.rows() == 2 && ls.tables(0) == 3 && ls.tables(1) == 70 && ls.tables(2) == 0);
        bool threw = false;
        try {
            ls.probe({"key_000000"});
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);  // not sealed yet
        ls.seal();
        std::vector<std::string> q;
        for (int i = 0; i < 3200; i++) q.push_back(key("key_", i));      // members and gaps of both rows
        for (int i = 0; i < 200; i++) q.push_back(key("kez_", i));       // past every range
        for (int i = 0; i < 70; i++) q.push_back(key("key_", 40 * i).substr(0, 9));  // proper prefixes of bounds
        q.push_back("");
        const std::vector<uint32_t> got = ls.probe(q);
        CHECK(got.size() == 2 * q.size());
        size_t hits = 0;
        for (int r = 0; r < 2 && got.size() == 2 * q.size(); r++)
            for (size_t i = 0; i < q.size(); i++) {
                uint32_t exp = LSMB_LSET_NONE;
                for (const Table& T : rows[r])
                    if (le(T.lo, q[i]) && le(q[i], T.hi) && T.f.may_contain(q[i])) exp = T.id;
                if (got[r * q.size() + i] != exp) {
                    fprintf(stderr, "row %d key %s: got %u, expected %u\n", r, q[i].c_str(), got[r * q.size() + i], exp);
                    g_fail++;
                }
                hits += exp != LSMB_LSET_NONE;
            }
        CHECK(hits >= 3 * 300 + 70 * 30 && hits < 2 * q.size());
        CHECK(ls.probe({}).empty());
        threw = false;
        try {
            ls.add(0, 99, rows[0][0].f, "x", "y");
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);  // sealed
        // overlapping tables do not seal
        LevelSet bad;
        bad.add(0, 1, rows[0][0].f, "a", "m");
        bad.add(0, 2, rows[0][1].f, "m", "z");
        threw = false;
        try {
            bad.seal();
        } catch (const std::invalid_argument& e) {
            threw = strstr(e.what(), "1") && strstr(e.what(), "2");
        }
        CHECK(threw);
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

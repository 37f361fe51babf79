// lset_census_test.cpp — LevelSet::version_geometry and LevelSet::census of
// the C++ mirror (storage-engine_amd/cpp/lsm_bloom.hpp): the fill of every
// table of a resident Version, against a count of the host's own filter words.
// Usage: lset_census_test [--gpu]   (without --gpu: the argument checks and the arithmetic only)
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <memory>
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

static std::string key(int i) {
    char k[32];
    snprintf(k, sizeof k, "key_%06d", i);
    return k;
}

struct Table {
    uint32_t id;
    BloomFilter f;
    std::string lo, hi;
};

// nkeys keys from `first` in a filter sized for `sized` of them.
static Table make(uint32_t id, int first, int nkeys, size_t sized) {
    BloomFilter f(sized, 0.01);
    for (int i = 0; i < nkeys; i++) f.insert(key(first + i));
    return Table{id, std::move(f), key(first), key(first + nkeys - 1)};
}

// The set bits below num_bits, bit by bit.
static uint64_t count(const BloomFilter& f) {
    uint64_t n = 0;
    for (uint32_t b = 0; b < f.num_bits(); b++) n += (f.words()[b / 64] >> (b % 64)) & 1;
    return n;
}

static void check_census(LevelSet& ls, const std::vector<const Table*>& in_order) {
    const LevelSet::Census c = ls.census();
    const LevelSet::VersionGeometry g = ls.version_geometry();
    CHECK(c.ids.size() == in_order.size() && c.set_bits.size() == in_order.size());
    CHECK(g.num_bits == c.num_bits && g.num_hashes == c.num_hashes);
    for (size_t v = 0; v < in_order.size() && c.ids.size() == in_order.size(); v++) {
        const Table& T = *in_order[v];
        const uint64_t exp = count(T.f);
        if (c.ids[v] != T.id || c.num_bits[v] != T.f.num_bits() || c.num_hashes[v] != T.f.num_hashes() ||
            c.set_bits[v] != exp) {
            fprintf(stderr, "table %zu: id %u bits %u k %u set %llu, expected id %u bits %u k %u set %llu\n", v, c.ids[v],
                    c.num_bits[v], c.num_hashes[v], (unsigned long long)c.set_bits[v], T.id, T.f.num_bits(),
                    T.f.num_hashes(), (unsigned long long)exp);
            g_fail++;
        }
        const double fpr = pow((double)exp / T.f.num_bits(), T.f.num_hashes());
        CHECK(fabs(c.fpr[v] - fpr) <= 1e-12 * fpr);
        CHECK(c.keys[v] > 0);
    }
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        uint32_t nb = 7, k = 7;
        uint64_t sb = 7;
        CHECK(lsmb_lset_version_geometry(nullptr, &nb, &k) == LSMB_EINVAL && nb == 7 && k == 7);
        CHECK(lsmb_lset_census(nullptr, &sb, nullptr) == LSMB_EINVAL && sb == 7);
        CHECK(lsmb_popcount_segs_dev(nullptr, nullptr, 0, nullptr, nullptr) == LSMB_EINVAL);
        CHECK(lsmb_fill_fpr(100, 0, 50) == 1.0 && lsmb_fill_fpr(0, 0, 0) == 1.0 && lsmb_fill_fpr(100, 7, 0) == 0.0);
        CHECK(lsmb_fill_fpr(100, 7, 100) == 1.0 && isnan(lsmb_fill_fpr(100, 7, 101)));
        CHECK(fabs(lsmb_fill_fpr(9586, 7, 4793) - pow(0.5, 7)) < 1e-15);
        CHECK(lsmb_fill_keys(100, 7, 0) == 0.0 && isinf(lsmb_fill_keys(100, 7, 100)) && lsmb_fill_keys(100, 7, 100) > 0);
        CHECK(isnan(lsmb_fill_keys(100, 0, 50)) && isnan(lsmb_fill_keys(100, 7, 101)));
        CHECK(fabs(lsmb_fill_keys(9586, 7, 4793) - 9586.0 / 7 * log(2.0)) < 1e-9);
        CHECK(lsmb_abi_version() == 6);
    }
    if (gpu) {
        // two L0 tables and a row of six: SST-sized ones at their design load, one holding 20 times
        // its estimate, one of 100 000 keys (several items), one with stray ones above num_bits
        std::vector<Table> l0, row;
        l0.push_back(make(900, 100, 1000, 1000));
        l0.push_back(make(901, 600, 20000, 1000));
        for (int t = 0; t < 4; t++) row.push_back(make(100 + t, 30000 * t, 1000 + t, 1000));
        row.push_back(make(104, 30000 * 4, 100000, 100000));
        row.push_back(make(105, 30000 * 8, 30, 30));
        CHECK(row[4].f.num_bits() > 8 * (64u << 10) && row[5].f.num_bits() % 64 != 0);
        const uint64_t before = count(row[5].f);
        row[5].f.words().back() |= ~0ull << (row[5].f.num_bits() % 64);  // deserialize lets these in (mod.rs:123-168)
        CHECK(count(row[5].f) == before);
        std::unique_ptr<LevelSet> ls(new LevelSet);
        bool threw = false;
        try {
            ls->census();
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);  // not sealed yet
        // the row in descending key order: the census answers in the sealed order
        for (size_t t = row.size(); t-- > 0;) {
            if (t % 2)
                ls->add(0, row[t].id, row[t].f, row[t].lo, row[t].hi);
            else
                ls->add(0, row[t].id, row[t].f.serialize(), row[t].lo, row[t].hi);
        }
        for (const Table& T : l0) ls->add(LSMB_LSET_ROW_L0, T.id, T.f, T.lo, T.hi);
        ls->seal();
        std::vector<const Table*> order;
        for (const Table& T : l0) order.push_back(&T);
        for (const Table& T : row) order.push_back(&T);
        const auto s0 = ls->stats();
        check_census(*ls, order);
        CHECK(ls->stats() == s0);
        const LevelSet::Census c = ls->census();
        CHECK(c.fpr[1] > 0.9 && c.fpr[0] < 0.05);           // the saturated table shows
        CHECK(c.keys[0] > 900 && c.keys[0] < 1100);         // 1000 distinct keys, estimated from the fill
        // a repacked child without table 101 and the saturated one
        std::unique_ptr<LevelSet> child = ls->derive_packed({101, 901}, LSMB_LSET_REPACK_ALL);
        child->seal();
        std::vector<const Table*> corder;
        for (const Table* T : order)
            if (T->id != 101 && T->id != 901) corder.push_back(T);
        check_census(*child, corder);
        ls.reset();
        check_census(*child, corder);
        // an empty set
        LevelSet none;
        none.seal();
        CHECK(none.census().ids.empty());
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

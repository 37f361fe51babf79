// lset_version_lists_test.cpp — version_order and probe_version_lists of the
// C++ mirror's LevelSet (storage-engine_amd/cpp/lsm_bloom.hpp): a whole
// Version's answer per table (src/db/mod.rs:238-267), against the mirror's own
// probe_version transposed on the host.
// Usage: lset_version_lists_test [--gpu]   (without --gpu: the argument checks only)
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

static Table make(uint32_t id, int first, int span, int step) {
    BloomFilter f(1000, 0.01);
    int last = first;
    for (int i = first; i < first + span; i += step) f.insert(key(last = i));
    return Table{id, std::move(f), key(first), key(last)};
}

// probe_version's answer transposed: the L0 lists by position, then the rows'
// lists by ordinal (ids unique here, so an id names its ordinal).
static void check_lists(LevelSet& ls, const std::vector<std::string>& q) {
    const LevelSet::VersionOrder o = ls.version_order();
    const LevelSet::VersionAnswer a = ls.probe_version(q);
    const LevelSet::Lists got = ls.probe_version_lists(q);
    const size_t T0 = ls.l0_tables(), V = ls.version_tables(), R = (size_t)ls.rows(), n = q.size();
    CHECK(V == T0 + ls.total_tables() && o.ids.size() == V && o.part_base.size() == R + 2);
    CHECK(o.part_base[0] == 0 && o.part_base[1] == T0 && o.part_base[R + 1] == V);
    std::vector<uint64_t> starts(V + 1, 0);
    std::vector<uint32_t> index;
    for (size_t v = 0; v < V; v++) {
        starts[v] = index.size();
        for (size_t i = 0; i < n; i++) {
            bool hit = false;
            if (v < T0)
                hit = (a.mask[i] >> v) & 1;
            else
                for (size_t r = 0; r < R; r++)
                    if (v >= o.part_base[1 + r] && v < o.part_base[2 + r]) hit = a.ids[r * n + i] == o.ids[v];
            if (hit) index.push_back((uint32_t)i);
        }
    }
    starts[V] = index.size();
    CHECK(got.starts == starts);
    CHECK(got.index == index);
    CHECK(!index.empty());
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        uint32_t ids[2] = {7, 7};
        uint64_t starts[2] = {7, 7};
        const uint8_t k[4] = {1, 2, 3, 4};
        CHECK(lsmb_abi_version() == 6);
        CHECK(lsmb_lset_version_tables(nullptr) == 0);
        CHECK(lsmb_lset_version_lists_work_bytes(nullptr, 1000) == 0);
        CHECK(lsmb_lset_version_order(nullptr, ids, starts) == LSMB_EINVAL);
        CHECK(lsmb_lset_version_order(nullptr, nullptr, nullptr) == LSMB_EINVAL);
        CHECK(lsmb_lset_probe_version_lists(nullptr, k, nullptr, 2, 2, starts, ids, 2) == LSMB_EINVAL);
        CHECK(lsmb_lset_probe_version_lists_dev(nullptr, k, nullptr, 2, 2, starts, ids, 2, ids, 1 << 20, nullptr) ==
              LSMB_EINVAL);
        CHECK(ids[0] == 7 && ids[1] == 7 && starts[0] == 7 && starts[1] == 7);
    }
    if (gpu) {
        // L0 = [a, b, c] overlapping, two rows of four and two disjoint tables
        const Table a = make(1, 0, 400, 3), b = make(2, 100, 400, 2), c = make(3, 0, 900, 7), d = make(4, 350, 100, 1);
        std::vector<Table> row;
        for (int t = 0; t < 4; t++) row.push_back(make(100 + t, 250 * t, 200, 2));
        const Table lo = make(200, 0, 450, 5), hi = make(201, 500, 450, 5);
        LevelSet parent;
        bool threw = false;
        try {
            parent.version_order();
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw && parent.version_tables() == 0);  // not sealed yet
        for (const Table* t : {&a, &b, &c}) parent.add(LSMB_LSET_ROW_L0, t->id, t->f, t->lo, t->hi);
        for (int t = 3; t >= 0; t--) parent.add(0, row[t].id, row[t].f, row[t].lo, row[t].hi);
        parent.add(1, hi.id, hi.f, hi.lo, hi.hi);
        parent.add(1, lo.id, lo.f, lo.lo, lo.hi);
        parent.seal();
        CHECK(parent.version_tables() == 9);
        const LevelSet::VersionOrder o = parent.version_order();
        CHECK(o.ids == (std::vector<uint32_t>{1, 2, 3, 100, 101, 102, 103, 200, 201}));
        CHECK(o.part_base == (std::vector<uint64_t>{0, 3, 7, 9}));
        std::vector<std::string> q;
        for (int i = 0; i < 1000; i++) q.push_back(key(i));
        q.push_back("");
        q.push_back("key_");
        q.push_back("zzz");
        check_lists(parent, q);
        // the Version edit: b and a row table go, d arrives in L0; positions after b shift down
        std::unique_ptr<LevelSet> child = parent.derive({b.id, row[1].id});
        child->add(LSMB_LSET_ROW_L0, d.id, d.f.serialize(), d.lo, d.hi);
        child->seal();
        CHECK(child->version_order().ids == (std::vector<uint32_t>{1, 3, 4, 100, 102, 103, 200, 201}));
        check_lists(*child, q);
        check_lists(parent, q);  // the parent is untouched
        // no L0 table: the rows' lists; no row: the L0 lists alone
        LevelSet rows_only;
        for (int t = 0; t < 4; t++) rows_only.add(0, row[t].id, row[t].f, row[t].lo, row[t].hi);
        rows_only.seal();
        const LevelSet::Lists r1 = rows_only.probe_version_lists(q), r2 = rows_only.probe_lists(q);
        CHECK(r1.starts == r2.starts && r1.index == r2.index && rows_only.version_tables() == 4);
        LevelSet l0_only;
        for (const Table* t : {&a, &b, &c}) l0_only.add(LSMB_LSET_ROW_L0, t->id, t->f, t->lo, t->hi);
        l0_only.seal();
        CHECK(l0_only.version_order().part_base == (std::vector<uint64_t>{0, 3}));
        check_lists(l0_only, q);
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

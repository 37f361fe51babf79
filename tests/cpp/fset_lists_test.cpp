// fset_lists_test.cpp — FilterSet::probe_lists of the C++ mirror
// (storage-engine_amd/cpp/lsm_bloom.hpp): the per-table key lists must be the
// transpose of FilterSet::probe's masks, taken in the same process.
// Usage: fset_lists_test [--gpu]   (without --gpu: the argument checks only)
#include <stdio.h>
#include <string.h>

#include <array>
#include <string>
#include <vector>

#include "../../storage-engine_amd/cpp/lsm_bloom.hpp"

using lsm::bloom::BloomFilter;
using lsm::bloom::BloomFilterBuilder;
using lsm::bloom::FilterSet;

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

// masks -> the lists they imply
static FilterSet::Lists lists_from_masks(const std::vector<uint64_t>& m) {
    FilterSet::Lists l;
    l.starts[0] = 0;
    for (int s = 0; s < 64; s++) {
        for (size_t i = 0; i < m.size(); i++)
            if (m[i] >> s & 1) l.index.push_back((uint32_t)i);
        l.starts[s + 1] = l.index.size();
    }
    return l;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        uint64_t starts[65];
        uint32_t index[4];
        const uint8_t data[4] = {0};
        CHECK(lsmb_fset_probe_lists(nullptr, data, nullptr, 1, 4, starts, index, 4) == LSMB_EINVAL);
        CHECK(lsmb_fset_probe_lists_dev(nullptr, data, nullptr, 1, 4, starts, index, 4, nullptr) == LSMB_EINVAL);
    }
    if (gpu) {
        FilterSet fs;
        // three tables with overlapping id ranges: [0, 1500), [1000, 2500), [2000, 3500)
        int slot[3];
        for (int t = 0; t < 3; t++) {
            BloomFilterBuilder b(1500, 0.01);
            for (int i = 0; i < 1500; i++) b.add_key(key("key_", t * 1000 + i));
            BloomFilter f = b.build();
            slot[t] = fs.add(f, key("key_", t * 1000), key("key_", t * 1000 + 1499));
        }
        CHECK(slot[0] == 0 && slot[1] == 1 && slot[2] == 2);
        std::vector<std::string> q;
        for (int i = 0; i < 3500; i++) q.push_back(key("key_", i));        // members (1000 of them of two tables)
        for (int i = 0; i < 200; i++) q.push_back(key("key_", 5000 + i));  // absent, past every range
        for (int i = 0; i < 200; i++) q.push_back(key("kez_", i));         // absent
        const std::vector<uint64_t> m = fs.probe(q);
        const FilterSet::Lists exp = lists_from_masks(m);
        const FilterSet::Lists got = fs.probe_lists(q);
        CHECK(exp.starts[64] >= 4500);  // every member listed by each of its tables
        CHECK(exp.starts[64] > q.size());  // more entries than keys: the mirror's second, exactly sized call
        CHECK(got.starts == exp.starts);
        CHECK(got.index == exp.index);
        for (int t = 0; t < 3; t++)  // the members of table t, in order, are in its list
            for (int i = 0; i < 1500; i++) CHECK(m[t * 1000 + i] >> t & 1);
        // no key, and no table
        const FilterSet::Lists none = fs.probe_lists({});
        CHECK(none.starts == (std::array<uint64_t, 65>{}) && none.index.empty());
        for (int t = 0; t < 3; t++) fs.remove(slot[t]);
        const FilterSet::Lists dead = fs.probe_lists(q);
        CHECK(dead.starts == (std::array<uint64_t, 65>{}) && dead.index.empty());
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

// lset_lists_test.cpp — LevelSet::probe_lists of the C++ mirror
// (storage-engine_amd/cpp/lsm_bloom.hpp) against the mirror's own probe(),
// mapped id -> ordinal through table_order() and grouped on the host, over
// three rows of 3, 0 and 70 tables.
// Usage: lset_lists_test [--gpu]   (without --gpu: the argument checks only)
#include <stdio.h>
#include <string.h>

#include <map>
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

template <class F>
static bool throws_invalid(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        uint64_t starts[4] = {7, 7, 7, 7}, base[4] = {7, 7, 7, 7};
        uint32_t index[4] = {9, 9, 9, 9}, ids[4] = {9, 9, 9, 9};
        const uint8_t data[4] = {0};
        CHECK(lsmb_lset_total_tables(nullptr) == 0);
        CHECK(lsmb_lset_lists_work_bytes(nullptr, 100) == 0);
        CHECK(lsmb_lset_table_order(nullptr, ids, base) == LSMB_EINVAL);
        CHECK(lsmb_lset_probe_lists(nullptr, data, nullptr, 1, 4, starts, index, 4) == LSMB_EINVAL);
        CHECK(lsmb_lset_probe_lists_dev(nullptr, data, nullptr, 1, 4, starts, index, 4, index, 16, nullptr) ==
              LSMB_EINVAL);
        CHECK(starts[0] == 7 && starts[3] == 7 && index[0] == 9 && ids[0] == 9 && base[0] == 7);
    }
    if (gpu) {
        const int ntab[3] = {3, 0, 70}, per[3] = {300, 0, 30}, pitch[3] = {1000, 0, 40};
        LevelSet ls;
        for (int r = 2; r >= 0; r--)  // any order: last table first, half of them from the serialized block
            for (int t = ntab[r] - 1; t >= 0; t--) {
                BloomFilter f(per[r], 0.01);
                for (int i = 0; i < per[r]; i++) f.insert(key("key_", t * pitch[r] + i));
                const std::string lo = key("key_", t * pitch[r]), hi = key("key_", t * pitch[r] + per[r] - 1);
                const uint32_t id = (uint32_t)(500 * r + t + 1);
                if (t % 2) ls.add(r, id, f.serialize(), lo, hi);
                else ls.add(r, id, f, lo, hi);
            }
        // before seal: nothing to list
        CHECK(ls.total_tables() == 0 && ls.lists_work_bytes(100) == 0);
        CHECK(throws_invalid([&] { ls.table_order(); }));
        CHECK(throws_invalid([&] { ls.probe_lists({"key_000000"}); }));
        CHECK(throws_invalid([&] {
            uint64_t s[80];
            ls.probe_lists_dev(s, nullptr, 1, 1, s, nullptr, 0, s, 1 << 20);
        }));
        ls.seal();
        CHECK(ls.total_tables() == 73 && ls.lists_work_bytes(100) > 0 && ls.lists_work_bytes(0) == 0);
        const LevelSet::TableOrder ord = ls.table_order();
        CHECK(ord.ids.size() == 73 && ord.row_base == (std::vector<uint64_t>{0, 3, 3, 73}));
        std::map<uint32_t, uint32_t> ordinal_of;  // ids are unique here
        for (size_t g = 0; g < ord.ids.size(); g++) ordinal_of[ord.ids[g]] = (uint32_t)g;
        for (int t = 0; t < 3; t++) CHECK(ord.ids[t] == (uint32_t)(t + 1));          // ascending min_key
        for (int t = 0; t < 70; t++) CHECK(ord.ids[3 + t] == (uint32_t)(1000 + t + 1));

        std::vector<std::string> q;
        for (int i = 0; i < 3200; i++) q.push_back(key("key_", i));  // members and gaps of both rows
        for (int i = 0; i < 200; i++) q.push_back(key("kez_", i));   // past every range
        q.push_back("");
        const std::vector<uint32_t> ids = ls.probe(q);
        const LevelSet::Lists got = ls.probe_lists(q);
        // the expectation: probe()'s answers grouped by ordinal, rows in order, keys ascending
        std::vector<std::vector<uint32_t>> exp(73);
        for (int r = 0; r < 3; r++)
            for (size_t i = 0; i < q.size(); i++) {
                const uint32_t id = ids[r * q.size() + i];
                if (id != LSMB_LSET_NONE) exp[ordinal_of.at(id)].push_back((uint32_t)i);
            }
        CHECK(got.starts.size() == 74 && got.starts[0] == 0);
        uint64_t at = 0;
        for (size_t g = 0; g < 73 && got.starts.size() == 74; g++) {
            CHECK(got.starts[g] == at);
            at += exp[g].size();
            if (got.starts[g + 1] != at || at > got.index.size()) {
                fprintf(stderr, "table %zu: list ends at %llu, expected %llu\n", g,
                        (unsigned long long)got.starts[g + 1], (unsigned long long)at);
                g_fail++;
                break;
            }
            for (size_t j = 0; j < exp[g].size(); j++)
                if (got.index[got.starts[g] + j] != exp[g][j]) {
                    fprintf(stderr, "table %zu entry %zu: got %u, expected %u\n", g, j,
                            got.index[got.starts[g] + j], exp[g][j]);
                    g_fail++;
                }
        }
        CHECK(got.index.size() == at && at >= 3 * 300 + 70 * 30);
        const LevelSet::Lists none = ls.probe_lists({});
        CHECK(none.index.empty() && none.starts == std::vector<uint64_t>(74, 0));
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

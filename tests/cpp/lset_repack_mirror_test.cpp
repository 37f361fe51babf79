// lset_repack_mirror_test.cpp — LevelSet::derive_packed of the C++ mirror
// (storage-engine_amd/cpp/lsm_bloom.hpp): a Version edit that repacks the
// parent's sparse chunks on the device, against the host's own may_contain
// (lsmb_may_contain) and memcmp-order range checks.
// Usage: lset_repack_mirror_test [--gpu]   (without --gpu: the argument checks only)
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
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

constexpr uint64_t CHUNK = 4u << 20;

static std::string key(int i) {
    char k[32];
    snprintf(k, sizeof k, "key_%06d", i);
    return k;
}

static bool le(const std::string& a, const std::string& b) {
    const int c = memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
    return c < 0 || (c == 0 && a.size() <= b.size());
}

struct Table {
    uint32_t id;
    BloomFilter f;
    std::string lo, hi;
};

static Table make(uint32_t id, int first) {
    BloomFilter f(30, 0.01);
    for (int i = 0; i < 30; i++) f.insert(key(first + i));
    return Table{id, std::move(f), key(first), key(first + 29)};
}

static void check_probe(LevelSet& ls, const std::vector<const Table*>& tabs, const std::vector<std::string>& q) {
    const std::vector<uint32_t> got = ls.probe(q);
    CHECK(got.size() == q.size());
    for (size_t i = 0; i < q.size() && got.size() == q.size(); i++) {
        uint32_t exp = LSMB_LSET_NONE;
        for (const Table* T : tabs)
            if (le(T->lo, q[i]) && le(q[i], T->hi) && T->f.may_contain(q[i])) exp = T->id;
        if (got[i] != exp) {
            fprintf(stderr, "key %s: got %u, expected %u\n", q[i].c_str(), got[i], exp);
            g_fail++;
        }
    }
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        lsmb_lset* h = (lsmb_lset*)0x10;
        uint64_t moved[2] = {7, 7};
        CHECK(lsmb_lset_derive_packed(nullptr, nullptr, 0, LSMB_LSET_REPACK_ALL, nullptr, moved, &h, nullptr) ==
                  LSMB_EINVAL &&
              h == nullptr && moved[0] == 7 && moved[1] == 7);
        CHECK(lsmb_lset_derive_packed(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr) == LSMB_EINVAL);
        CHECK(lsmb_copy_segs_dev(nullptr, nullptr, 0, nullptr) == LSMB_EINVAL);
    }
    if (gpu) {
        std::vector<Table> tabs;
        for (int t = 0; t < 20; t++) tabs.push_back(make(100 + t, 40 * t));
        std::vector<uint32_t> rows(20, 0), ids;
        std::vector<std::vector<uint8_t>> blocks;
        std::vector<LevelSet::TableRange> ranges;
        for (const Table& T : tabs) {
            ids.push_back(T.id);
            blocks.push_back(T.f.serialize());
            ranges.push_back({T.lo, T.hi});
        }
        std::unique_ptr<LevelSet> parent(new LevelSet);
        std::vector<int32_t> status;
        parent->add_many(rows, ids, blocks, ranges, nullptr, &status);
        bool threw = false;
        try {
            parent->derive_packed({}, LSMB_LSET_REPACK_ALL);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);  // not sealed yet
        parent->seal();
        threw = false;
        try {
            parent->derive_packed({}, LSMB_LSET_REPACK_ALL + 1);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        std::vector<std::string> q;
        for (int i = 0; i < 900; i++) q.push_back(key(i));
        uint64_t dropped = 0;
        std::array<uint64_t, 2> moved{0, 0};
        uint64_t slots = 0;
        for (const Table& T : tabs)
            if (T.id != 103 && T.id != 111) slots += (T.f.words().size() * 8 + 15) / 16 * 16;
        std::unique_ptr<LevelSet> child = parent->derive_packed({103, 111, 4242}, LSMB_LSET_REPACK_ALL, &dropped, &moved);
        CHECK(dropped == 2 && child->tables(0) == 18 && moved[0] == 18 && moved[1] == slots);
        // the plain derive next to it: the same tables, one chunk more once each has added
        std::unique_ptr<LevelSet> plain = parent->derive({103, 111, 4242});
        const Table extra = make(900, 40 * 3);  // into the gap table 103 left
        for (LevelSet* ls : {child.get(), plain.get()}) {
            ls->add(0, extra.id, extra.f.serialize(), extra.lo, extra.hi);
            ls->seal();
        }
        const auto s = child->stats(), sp = plain->stats();
        CHECK(s[0] == 19 && s[1] == 18 && s[2] == 8 * extra.f.words().size() && s[3] == 1);
        CHECK(s[4] == CHUNK && sp[4] == 2 * CHUNK && s[5] == sp[5] && s[1] == sp[1] && s[2] == sp[2]);
        parent.reset();  // the packed child holds none of the parent's chunks
        plain.reset();
        std::vector<const Table*> mine;
        for (const Table& T : tabs)
            if (T.id != 103 && T.id != 111) mine.push_back(&T);
        mine.push_back(&extra);
        check_probe(*child, mine, q);
        // min_ppm = 0 moves nothing
        std::unique_ptr<LevelSet> same = child->derive_packed({}, 0, &dropped, &moved);
        CHECK(dropped == 0 && moved[0] == 0 && moved[1] == 0 && same->stats()[4] == CHUNK);
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

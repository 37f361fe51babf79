// popcount_seg_test.cpp — the host side of the fill census
// (storage-engine_amd/csrc/popcount_seg.hpp) on a CPU: popcount_segs_ref,
// popcount_items and popcount_fold against a bit-by-bit loop, the items tiling
// every table exactly in pieces of at most kPopItemBytes, and the plan of a
// table of 2^32-1 bits.  Stand-alone; built plain and with
// -fsanitize=address,undefined by tests/test_lset_census.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../storage-engine_amd/csrc/popcount_seg.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Bits 0 .. nbits-1 of the bytes at p, one by one.
static uint64_t bit_by_bit(const uint8_t* p, uint64_t nbits) {
    uint64_t n = 0;
    for (uint64_t b = 0; b < nbits; b++) n += (p[b / 8] >> (b % 8)) & 1;
    return n;
}

static const uint64_t kBits[] = {0,     1,     63,    64,     65,     127,    128,    129,
                                 9586,  32767, 32768, 32769,  524287, 524288, 524289, 1310720};
constexpr size_t kNb = sizeof kBits / sizeof kBits[0];

// A heap block of exactly the table's words (the sanitizer sees a read past
// them), 16-byte aligned, random bytes: the bits at and above nbits of the last
// word mostly ones.
struct Words {
    uint8_t* p = nullptr;
    uint64_t bytes = 0;
    explicit Words(uint64_t nbits) : bytes(popcount_words(nbits) * 8) {
        if (bytes == 0) return;
        if (posix_memalign((void**)&p, 16, bytes) != 0) abort();
        for (uint64_t i = 0; i < bytes; i += 8) {
            const uint64_t r = rnd();
            memcpy(p + i, &r, 8);
        }
        if (nbits % 64) p[bytes - 1] |= 0x80;  // a stray one for certain (the last word has one free bit at least)
    }
    ~Words() { free(p); }
    Words(const Words&) = delete;
    Words& operator=(const Words&) = delete;
};

int main() {
    static_assert(kPopItemBytes == 64u << 10 && kPopItemBits == 524288, "the 64 KiB cut");
    static_assert(kPopSegIterBytes == 4096 && kPopSegLanes * kPopSegPerBlock == 256, "the kernel's geometry");
    // ---- the reference against the bit loop, segment by segment
    std::vector<Words*> tabs;
    for (size_t t = 0; t < kNb; t++) tabs.push_back(new Words(kBits[t]));
    std::vector<uint64_t> exp(kNb);
    for (size_t t = 0; t < kNb; t++) exp[t] = tabs[t]->p ? bit_by_bit(tabs[t]->p, kBits[t]) : 0;
    {
        std::vector<PopSeg> segs;
        for (size_t t = 0; t < kNb; t++) segs.push_back(PopSeg{tabs[t]->p, kBits[t]});
        std::vector<uint64_t> got(kNb, ~0ull);
        popcount_segs_ref(segs.data(), segs.size(), got.data());
        for (size_t t = 0; t < kNb; t++) CHECK(got[t] == exp[t]);
        CHECK(exp[0] == 0 && exp[1] <= 1 && exp[15] > 600000);
        popcount_segs_ref(segs.data(), 0, nullptr);  // nothing is touched
        // the stray ones do count once nbits covers them
        for (size_t t = 0; t < kNb; t++)
            if (kBits[t] % 64) {
                const PopSeg whole{tabs[t]->p, popcount_words(kBits[t]) * 64};
                uint64_t w = 0;
                popcount_segs_ref(&whole, 1, &w);
                CHECK(w > exp[t] && w == bit_by_bit(tabs[t]->p, whole.nbits));
            }
    }
    // ---- the items: a tiling of every table, at most 64 KiB each, whole words but a table's last
    {
        std::vector<const void*> words;
        std::vector<uint64_t> nbits;
        for (size_t t = 0; t < kNb; t++) {
            words.push_back(tabs[t]->p);
            nbits.push_back(kBits[t]);
        }
        std::vector<PopSeg> items;
        std::vector<uint32_t> table_of;
        popcount_items(words.data(), nbits.data(), kNb, &items, &table_of);
        CHECK(items.size() == table_of.size());
        size_t i = 0;
        for (size_t t = 0; t < kNb; t++) {
            uint64_t at = 0;  // bits of table t covered so far
            size_t n = 0;
            for (; i < items.size() && table_of[i] == t; i++, n++) {
                CHECK(items[i].words == tabs[t]->p + at / 8);
                CHECK(((uintptr_t)items[i].words & 15) == 0);
                CHECK(items[i].nbits > 0 && popcount_words(items[i].nbits) * 8 <= kPopItemBytes);
                at += items[i].nbits;
                if (at < kBits[t]) CHECK(items[i].nbits == kPopItemBits);  // not the last: whole words, the full cut
            }
            CHECK(at == kBits[t]);
            CHECK(n == (kBits[t] + kPopItemBits - 1) / kPopItemBits);
        }
        CHECK(i == items.size());
        CHECK(items.size() == 13 * 1 + 1 * 2 + 1 * 3);  // 0 bits: none; 524 289: two; 1 310 720: three
        // counted item by item and folded back: the tables' counts
        std::vector<uint64_t> counts(items.size()), got(kNb, ~0ull);
        popcount_segs_ref(items.data(), items.size(), counts.data());
        popcount_fold(counts.data(), table_of.data(), items.size(), kNb, got.data());
        for (size_t t = 0; t < kNb; t++) CHECK(got[t] == exp[t]);
        // a pad word of ones after a table is no part of any item: the fold of a copy with one is the same
        for (size_t t : {(size_t)3, (size_t)8, (size_t)14}) {
            std::vector<uint64_t> copy(popcount_words(kBits[t]) + 2, ~0ull);  // the words, then 16 bytes of ones
            memcpy(copy.data(), tabs[t]->p, tabs[t]->bytes);
            const void* w1 = copy.data();
            std::vector<PopSeg> it1;
            std::vector<uint32_t> of1;
            popcount_items(&w1, &kBits[t], 1, &it1, &of1);
            std::vector<uint64_t> c1(it1.size());
            popcount_segs_ref(it1.data(), it1.size(), c1.data());
            uint64_t g1 = ~0ull;
            popcount_fold(c1.data(), of1.data(), it1.size(), 1, &g1);
            CHECK(g1 == exp[t]);
        }
        // no table, and tables without bits
        popcount_items(nullptr, nullptr, 0, &items, &table_of);
        CHECK(items.empty() && table_of.empty());
        const void* none[2] = {nullptr, nullptr};
        const uint64_t zero[2] = {0, 0};
        uint64_t out2[2] = {7, 7};
        popcount_items(none, zero, 2, &items, &table_of);
        CHECK(items.empty());
        popcount_fold(nullptr, nullptr, 0, 2, out2);
        CHECK(out2[0] == 0 && out2[1] == 0);
    }
    // ---- 2^32-1 bits: planned only, nothing allocated
    {
        const void* base = (const void*)(uintptr_t)0x7F0000000000ull;
        const uint64_t nb = 0xFFFFFFFFull;
        std::vector<PopSeg> items;
        std::vector<uint32_t> table_of;
        popcount_items(&base, &nb, 1, &items, &table_of);
        CHECK(items.size() == 8192 && table_of.size() == 8192);
        uint64_t at = 0;
        for (size_t i = 0; i < items.size(); i++) {
            CHECK((uintptr_t)items[i].words == (uintptr_t)base + at / 8);
            CHECK(table_of[i] == 0);
            CHECK(items[i].nbits == (i + 1 < items.size() ? kPopItemBits : kPopItemBits - 1));
            at += items[i].nbits;
        }
        CHECK(at == nb);
        CHECK((uintptr_t)items.back().words + popcount_words(items.back().nbits) * 8 == (uintptr_t)base + (512ull << 20));
        std::vector<uint64_t> counts(items.size(), kPopItemBits);  // every item full: no overflow in the fold
        counts.back() = kPopItemBits - 1;
        uint64_t total = 0;
        popcount_fold(counts.data(), table_of.data(), items.size(), 1, &total);
        CHECK(total == nb);
    }
    for (Words* w : tabs) delete w;
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

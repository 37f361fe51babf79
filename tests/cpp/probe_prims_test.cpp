// probe_prims_test.cpp — the device steps every probe kernel shares
// (bloom_math.hpp), run on the host against literal restatements:
//   words_may_contain  against (h1 + i*h2 wrapping) % num_bits tested bit by bit
//                      for all k positions (src/bloom/mod.rs:82-94, 192-197);
//                      num_bits in {1, 63, 64, 65, 9 586, 2^20} x k in {0, 1, 7,
//                      8, 33}, 200 inserted keys, 2 000 other keys
//   table_and<7>, <0>  over the one-byte table sliced from 8 such filters: bit f
//                      of the result = words_may_contain of filter f
//   transpose8x8       output bit 8 i + f = input bit 8 f + i; an involution
// Seeded inputs, no GPU.  Host build of the device header; tests/test_capi_host.py
// builds it plain and with -fsanitize=address,undefined and runs it.
#include <stdio.h>

#include <random>
#include <vector>

#include "../../storage-engine_amd/csrc/bloom_math.hpp"

using namespace lsmb;

static long bad = 0, checked = 0;

static void expect(bool ok, const char* what, uint32_t nb, uint32_t k, uint64_t a, uint64_t b) {
    checked++;
    if (!ok && bad++ < 20)
        printf("FAIL %s num_bits=%u k=%u (%llu, %llu)\n", what, nb, k, (unsigned long long)a, (unsigned long long)b);
}

static uint64_t literal_pos(const H128& h, uint32_t i, uint32_t nb) { return (h.lo + (uint64_t)i * h.hi) % nb; }

static bool literal_contains(const std::vector<uint32_t>& w, uint32_t nb, uint32_t k, const H128& h) {
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t p = literal_pos(h, i, nb);
        if (!((w[p >> 5] >> (p & 31)) & 1u)) return false;
    }
    return true;
}

struct Filter {
    std::vector<uint32_t> w;  // LE u32 view of the u64 words
    std::vector<H128> members;
};

static Filter make_filter(uint32_t nb, uint32_t k, std::mt19937_64& rng, int nkeys) {
    Filter f;
    f.w.assign(2 * (((uint64_t)nb + 63) / 64), 0u);
    for (int t = 0; t < nkeys; t++) {
        const H128 h = xxh3_16(rng(), rng());
        f.members.push_back(h);
        for (uint32_t i = 0; i < k; i++) {
            const uint64_t p = literal_pos(h, i, nb);
            f.w[p >> 5] |= 1u << (p & 31);
        }
    }
    return f;
}

// table_and with walk W over `table` against words_may_contain of each filter
template <int K, class W>
static void check_table(const std::vector<uint8_t>& table, const typename W::Mod& md, const Mod32& md32,
                        const std::vector<Filter>& fl, uint32_t nb, uint32_t k, const H128& h, const char* what) {
    const uint8_t m = table_and<K>(table.data(), W(md, h.lo, h.hi), md, k, (uint8_t)0xFF);
    for (uint32_t f = 0; f < 8; f++)
        expect((bool)((m >> f) & 1) == words_may_contain(fl[f].w.data(), md32, k, h), what, nb, k, h.lo, f);
}

static void shape(uint32_t nb, uint32_t k, std::mt19937_64& rng) {
    const Mod32 md = Mod32::make(nb);
    std::vector<Filter> fl;
    for (int f = 0; f < 8; f++) fl.push_back(make_filter(nb, k, rng, 200));
    std::vector<H128> others;
    for (int t = 0; t < 2000; t++) others.push_back(xxh3_16(rng(), rng()));

    // words_may_contain: members all true, every other answer the literal one
    for (const H128& h : fl[0].members) expect(words_may_contain(fl[0].w.data(), md, k, h), "member", nb, k, h.lo, h.hi);
    for (const H128& h : others)
        expect(words_may_contain(fl[0].w.data(), md, k, h) == literal_contains(fl[0].w, nb, k, h), "other", nb, k, h.lo,
               h.hi);

    // the one-byte table of the 8 filters: entry p bit f = filter f's bit p, set
    // bit by bit; and the same bytes from the 8x8 transposes of the filters'
    // bytes, as the kernels build it
    const uint32_t nw32 = (uint32_t)fl[0].w.size();
    std::vector<uint8_t> table((size_t)nw32 * 32, 0);
    for (uint32_t p = 0; p < nw32 * 32; p++)
        for (uint32_t f = 0; f < 8; f++) table[p] |= (uint8_t)(((fl[f].w[p >> 5] >> (p & 31)) & 1u) << f);
    for (uint32_t it = 0; it < 4 * nw32; it++) {
        const uint32_t w = it >> 2, sh = 8 * (it & 3);
        uint64_t x = 0;
        for (uint32_t f = 0; f < 8; f++) x |= (uint64_t)((fl[f].w[w] >> sh) & 0xFFu) << (8 * f);
        x = transpose8x8(x);
        for (uint32_t i = 0; i < 8; i++) expect((uint8_t)(x >> (8 * i)) == table[8 * it + i], "table8", nb, k, it, i);
    }
    auto query = [&](const H128& h) {
        check_table<0, Walk32>(table, md, md, fl, nb, k, h, "table_and<0> Walk32");
        if (k == 7) check_table<7, Walk32>(table, md, md, fl, nb, k, h, "table_and<7> Walk32");
        if (Mod14::fits(nb)) {
            const Mod14 m14 = Mod14::make(nb);
            check_table<0, Walk14>(table, m14, md, fl, nb, k, h, "table_and<0> Walk14");
            if (k == 7) check_table<7, Walk14>(table, m14, md, fl, nb, k, h, "table_and<7> Walk14");
        }
    };
    for (const H128& h : others) query(h);
    for (const Filter& f : fl)
        for (const H128& h : f.members) query(h);
}

int main() {
    std::mt19937_64 rng(0x5EED0B00);
    for (uint32_t nb : {1u, 63u, 64u, 65u, 9586u, 1u << 20})
        for (uint32_t k : {0u, 1u, 7u, 8u, 33u}) shape(nb, k, rng);

    auto transpose_ok = [&](uint64_t x) {
        const uint64_t y = transpose8x8(x);
        bool ok = transpose8x8(y) == x;
        for (uint32_t i = 0; i < 8; i++)
            for (uint32_t f = 0; f < 8; f++) ok = ok && ((y >> (8 * i + f)) & 1) == ((x >> (8 * f + i)) & 1);
        expect(ok, "transpose8x8", 0, 0, x, y);
    };
    for (int b = 0; b < 64; b++) transpose_ok(1ull << b);
    for (int t = 0; t < 10000; t++) transpose_ok(rng());

    printf("probe_prims: %ld checked, %ld bad\n", checked, bad);
    return bad ? 1 : 0;
}

// build_batch_plan_test.cpp — the host side of the batched build
// (storage-engine_amd/csrc/build_batch_plan.hpp) on a CPU: the packed layout,
// the work list and build_batch_ref, the serial statement of what the kernels
// of build_batch.hip do, against a literal per-key insert loop
// (src/bloom/mod.rs:70-78, 192-197: (h1 + i * h2) % num_bits with a plain `%`).
// A stand-alone program (tests/test_build_batch.py builds it with
// -fsanitize=address,undefined and runs it).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../storage-engine_amd/csrc/build_batch_plan.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

struct Shape {
    uint64_t keys;
    uint32_t num_bits, k;
};

// The table shapes of one batch: every key count crossed with a rotating
// (num_bits, k), every num_bits at least once with k = 7, and two tables of
// two parts or more (one per class), their key counts taken from bb_parts.
static std::vector<Shape> shapes() {
    const uint64_t counts[] = {0, 1, 63, 64, 65, 1000};
    const uint32_t bits[] = {64, 65, 9586, 16383, 16384, 16385, kBbWaveMaxBits - 1, kBbWaveMaxBits, kBbWaveMaxBits + 1,
                             kBbMaxBits};
    const uint32_t ks[] = {0, 1, 7, 40};
    std::vector<Shape> s;
    size_t r = 0;
    for (uint32_t b : bits) s.push_back(Shape{counts[r++ % 6], b, 7});
    for (uint64_t c : counts)
        for (uint32_t k : ks) s.push_back(Shape{c, bits[r++ % 10], k});
    s.push_back(Shape{0, 0, 0});  // a filter of no bits: k = 0, no words, a slot all the same
    uint64_t kw = 1, kg = 1;
    while (bb_parts(kw, 9586) < 2) kw++;
    while (bb_parts(kg, kBbMaxBits) < 2) kg += 1024;
    s.push_back(Shape{kw, 9586, 7});
    s.push_back(Shape{2 * kw + 5, 64, 1});
    s.push_back(Shape{kg, kBbMaxBits, 7});
    return s;
}

// Key i of a run: 16 bytes, or 1 .. 300 bytes (every XXH3 length class).
static void make_keys(uint64_t n, bool var, std::vector<uint8_t>* data, std::vector<uint64_t>* offs) {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    offs->assign(1, 0);
    data->clear();
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t len = var ? 1 + (i * 7) % 300 : 16;
        for (uint64_t b = 0; b < len; b++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            data->push_back((uint8_t)(x >> 56));
        }
        offs->push_back(data->size());
    }
    data->resize(data->size() + 16);  // (xxh3 reads whole 8-byte words inside the key only; slack for the checker)
}

static void literal_insert(uint64_t* words, uint32_t num_bits, uint32_t k, const uint8_t* key, uint64_t len) {
    const H128 h = xxh3_128(key, len);
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t p = (h.lo + (uint64_t)i * h.hi) % (uint64_t)num_bits;
        words[p >> 6] |= 1ull << (p & 63);
    }
}

static void check_plan(const std::vector<Shape>& sh, const std::vector<uint64_t>& seg, const BbPlan& pl) {
    const uint64_t ntab = sh.size();
    CHECK(pl.word_off.size() == ntab + 1 && pl.word_off[0] == 0);
    // slots: 16-byte aligned, disjoint, each at least the filter's words
    for (uint64_t t = 0; t < ntab; t++) {
        const uint64_t nw = ((uint64_t)sh[t].num_bits + 63) / 64, slot = pl.word_off[t + 1] - pl.word_off[t];
        CHECK(pl.word_off[t] % 2 == 0 && pl.word_off[t + 1] > pl.word_off[t]);
        CHECK(slot == bb_slot_words(sh[t].num_bits) && slot >= std::max<uint64_t>(nw, 1) && slot <= nw + 2 && slot % 2 == 0);
    }
    // LDS: every item within its region, every workgroup within the CU's 160 KiB
    CHECK(pl.wave_region32 % 4 == 0 && pl.wave_region32 <= kBbWaveMaxBits / 32);
    CHECK((uint64_t)pl.wave_region32 * 4 * kBbWavesPerGroup <= kBbLdsBytes);
    CHECK(pl.group_region32 % 4 == 0 && (uint64_t)pl.group_region32 * 4 <= kBbLdsBytes);
    // the items of every table partition its keys exactly once
    std::vector<std::vector<BbItem>> of(ntab);
    for (int cls = 0; cls < 2; cls++)
        for (const BbItem& it : cls ? pl.group : pl.wave) {
            CHECK(it.table < ntab);
            if (it.table >= ntab) continue;
            const Shape& s = sh[it.table];
            CHECK((cls == 0) == bb_is_wave(s.num_bits));
            CHECK(it.nw32 <= (cls ? pl.group_region32 : pl.wave_region32) && it.nw32 % 4 == 0);
            CHECK(it.dst == pl.word_off[it.table] && it.dst + it.nw32 / 2 == pl.word_off[it.table + 1]);
            CHECK(it.k == s.k && it.md.d == (s.num_bits ? s.num_bits : 1));
            CHECK(it.key_hi - it.key_lo <= (cls ? kBbGroupKeys : kBbWaveKeys));
            of[it.table].push_back(it);
        }
    size_t nzero = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        std::vector<BbItem>& v = of[t];
        CHECK(v.size() == bb_parts(sh[t].keys, sh[t].num_bits) && !v.empty());
        uint64_t at = seg[t];
        for (const BbItem& it : v) {  // (the plan emits a table's parts in key order)
            CHECK(it.parts == v.size() && it.key_lo == at && it.key_hi >= it.key_lo);
            at = it.key_hi;
        }
        CHECK(at == seg[t + 1]);
        if (v.size() > 1) nzero++;
    }
    CHECK(pl.zero.size() == nzero && nzero >= 2);
    for (const BbItem& z : pl.zero) CHECK(z.parts > 1 && z.dst == pl.word_off[z.table]);
}

static void run(bool var) {
    const std::vector<Shape> sh = shapes();
    const uint64_t ntab = sh.size(), before = 5, after = 3;
    std::vector<uint64_t> seg(ntab + 1);
    std::vector<uint32_t> nb(ntab), kk(ntab);
    seg[0] = before;  // keys no table claims on both sides of the run
    for (uint64_t t = 0; t < ntab; t++) {
        seg[t + 1] = seg[t] + sh[t].keys;
        nb[t] = sh[t].num_bits;
        kk[t] = sh[t].k;
    }
    const uint64_t n = seg[ntab] + after;
    std::vector<uint8_t> data;
    std::vector<uint64_t> offs;
    make_keys(n, var, &data, &offs);
    const BbPlan pl = bb_plan(ntab, seg.data(), nb.data(), kk.data());
    check_plan(sh, seg, pl);

    const uint64_t total = pl.word_off[ntab], guard = 8;
    std::vector<uint64_t> words(total + guard, ~0ull);  // dirty, then a guard
    build_batch_ref(pl, data.data(), var ? offs.data() : nullptr, 16, words.data());
    for (uint64_t gq = 0; gq < guard; gq++) CHECK(words[total + gq] == ~0ull);
    for (uint64_t t = 0; t < ntab; t++) {
        const uint64_t nw = ((uint64_t)nb[t] + 63) / 64;
        std::vector<uint64_t> exp(nw, 0);
        for (uint64_t i = seg[t]; i < seg[t + 1]; i++)
            literal_insert(exp.data(), nb[t], kk[t], data.data() + offs[i], offs[i + 1] - offs[i]);
        const bool same = nw == 0 || memcmp(exp.data(), words.data() + pl.word_off[t], nw * 8) == 0;
        if (!same) fprintf(stderr, "table %llu (%llu keys, %u bits, k %u, var %d) differs\n", (unsigned long long)t,
                           (unsigned long long)sh[t].keys, nb[t], kk[t], (int)var);
        CHECK(same);
        for (uint64_t q = pl.word_off[t] + nw; q < pl.word_off[t + 1]; q++) CHECK(words[q] == 0);  // pad words
        // tail bits past num_bits stay clear
        if (nw && nb[t] % 64) CHECK((words[pl.word_off[t] + nw - 1] >> (nb[t] % 64)) == 0);
    }
}

int main() {
    // the layout by hand
    {
        const uint32_t nb[5] = {0, 1, 64, 65, 9586};
        uint64_t off[6];
        bb_layout(5, nb, off);
        const uint64_t exp[6] = {0, 2, 4, 6, 8, 158};
        CHECK(memcmp(off, exp, sizeof exp) == 0);
    }
    // parts: at least one, non-decreasing in the key count, one for an SSTable-sized table
    for (uint32_t b : {64u, 9586u, kBbWaveMaxBits, kBbWaveMaxBits + 1, kBbMaxBits}) {
        uint32_t last = 1;
        for (uint64_t keys = 0; keys < 300000; keys += 997) {
            const uint32_t p = bb_parts(keys, b);
            CHECK(p >= last);
            last = p;
        }
        CHECK(bb_parts(0, b) == 1 && bb_parts(1000, b) == 1 && bb_parts(~0ull, b) == kBbMaxParts);
    }
    run(false);
    run(true);
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

// sst_blocks_test.cpp — the data-block key source of the batched build
// (storage-engine_amd/csrc/sst_blocks.hpp) on a CPU: the block format
// (src/sstable/block/builder.rs:40-76), the plan over runs of blocks and
// build_batch_sst_ref, the serial statement of what the kernels of
// build_batch_sst.hip do, against a literal per-key insert loop over the keys a
// straightforward parser of its own extracts; and the check of a caller's
// claimed blocks with their span (sst_check_claim, sst_claim_span), rule by
// rule, over arrays of exactly their length.  Every block under test lives in
// a heap allocation of exactly its length, so one byte read past a block aborts
// the program.  A stand-alone program (tests/test_build_batch_sst.py builds it
// with -fsanitize=address,undefined and runs it).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../storage-engine_amd/csrc/sst_blocks.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

typedef std::vector<uint8_t> Bytes;
typedef std::pair<std::string, std::string> Entry;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}
static std::string rnd_str(size_t len) {
    std::string s(len, 0);
    for (char& c : s) c = (char)rnd();
    return s;
}

static void put16(Bytes* b, size_t v) {
    b->push_back((uint8_t)(v & 0xFF));
    b->push_back((uint8_t)((v >> 8) & 0xFF));
}

// BlockBuilder::add for every entry, then build (block/builder.rs:50-75).
static Bytes encode_block(const std::vector<Entry>& es) {
    Bytes b;
    std::vector<size_t> offs;
    for (const Entry& e : es) {
        offs.push_back(b.size());
        put16(&b, e.first.size());
        put16(&b, e.second.size());
        b.insert(b.end(), e.first.begin(), e.first.end());
        b.insert(b.end(), e.second.begin(), e.second.end());
    }
    for (size_t o : offs) put16(&b, o);
    put16(&b, offs.size());
    return b;
}

// The format read the plain way, with bounds-checked indexing: false = malformed.
static bool parse_plain(const Bytes& b, std::vector<std::string>* keys) {
    keys->clear();
    const size_t len = b.size();
    if (len < 2) return false;
    const size_t n = b.at(len - 2) | (size_t)b.at(len - 1) << 8;
    if (2 + 2 * n > len) return false;
    const size_t data_end = len - 2 - 2 * n;
    for (size_t i = 0; i < n; i++) {
        const size_t off = b.at(data_end + 2 * i) | (size_t)b.at(data_end + 2 * i + 1) << 8;
        if (off + 4 > data_end) return false;
        const size_t klen = b.at(off) | (size_t)b.at(off + 1) << 8, vlen = b.at(off + 2) | (size_t)b.at(off + 3) << 8;
        if (off + 4 + klen + vlen > data_end) return false;
        keys->push_back(std::string(b.begin() + off + 4, b.begin() + off + 4 + klen));
    }
    return true;
}

static void literal_insert(uint64_t* words, uint32_t num_bits, uint32_t k, const std::string& key) {
    const H128 h = xxh3_128((const uint8_t*)key.data(), key.size());
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t p = (h.lo + (uint64_t)i * h.hi) % (uint64_t)num_bits;
        words[p >> 6] |= 1ull << (p & 63);
    }
}

// A copy of the block in an allocation of exactly its length.
static std::unique_ptr<uint8_t[]> exact(const Bytes& b) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[b.size()]);
    if (!b.empty()) memcpy(p.get(), b.data(), b.size());
    return p;
}

// One block through the header's functions alone (sst_block_ref) in its exact
// allocation, against the plain parser: the verdict, the count and the bits.
static void check_block(const Bytes& b, const char* what) {
    const uint32_t nb = 9586, k = 7;
    const Mod32 md = Mod32::make(nb);
    std::vector<std::string> keys;
    const bool good = parse_plain(b, &keys);
    const std::unique_ptr<uint8_t[]> p = exact(b);
    std::vector<uint32_t> img((nb + 31) / 32, 0);
    const uint32_t got = sst_block_ref(p.get(), (uint32_t)b.size(), md, k, [&](uint32_t w, uint32_t m) { img.at(w) |= m; });
    if (!good) {
        if (got != kSstBadBlock) fprintf(stderr, "%s: a malformed block of %zu bytes was accepted\n", what, b.size());
        CHECK(got == kSstBadBlock);
        return;
    }
    if (got != keys.size()) fprintf(stderr, "%s: %u entries reported, %zu expected\n", what, got, keys.size());
    CHECK(got == keys.size());
    std::vector<uint64_t> exp((nb + 63) / 64, 0);
    for (const std::string& key : keys) literal_insert(exp.data(), nb, k, key);
    for (size_t q = 0; q < exp.size(); q++) {
        const uint64_t v = (uint64_t)img[2 * q] | (2 * q + 1 < img.size() ? (uint64_t)img[2 * q + 1] << 32 : 0);
        CHECK(v == exp[q]);
    }
    // the head and every entry, one by one
    const SstHead hd = sst_block_head(p.get(), (uint32_t)b.size());
    CHECK(hd.ok && hd.n == keys.size());
    for (uint32_t i = 0; i < hd.n; i++) {
        const SstKey e = sst_block_entry(p.get(), hd.data_end, hd.n, i);
        CHECK(e.ok && e.len == keys[i].size() && memcmp(p.get() + e.at, keys[i].data(), e.len) == 0);
    }
    CHECK(!sst_block_entry(p.get(), hd.data_end, hd.n, hd.n).ok);
}

static std::vector<Entry> entries(size_t n, size_t first, size_t vlen) {
    std::vector<Entry> es;
    for (size_t i = 0; i < n; i++) {
        char k[32];
        snprintf(k, sizeof k, "user%08zu", first + i);
        es.push_back(Entry(k, rnd_str(vlen)));
    }
    return es;
}

// The malformed blocks of the issue's list, each checked to be malformed by the plain parser.
static std::vector<std::pair<const char*, Bytes>> malformed() {
    std::vector<std::pair<const char*, Bytes>> out;
    const Bytes good = encode_block(entries(5, 0, 9));  // 5 entries of 4 + 12 + 9 bytes: data_end = 125
    const size_t data_end = good.size() - 2 - 10;
    auto patched = [&](size_t at, size_t v) {
        Bytes b = good;
        b[at] = (uint8_t)(v & 0xFF);
        b[at + 1] = (uint8_t)(v >> 8);
        return b;
    };
    out.push_back({"len 0", Bytes()});
    out.push_back({"len 1", Bytes(1, 0)});
    out.push_back({"n past len", patched(good.size() - 2, 70)});            // 2 + 140 > len
    out.push_back({"n = 65535", patched(good.size() - 2, 65535)});
    out.push_back({"off == data_end", patched(data_end + 4, data_end)});
    out.push_back({"off > data_end", patched(data_end + 4, data_end + 7)});
    out.push_back({"off past len", patched(data_end + 4, 65535)});
    out.push_back({"off + 4 > data_end", patched(data_end + 2, data_end - 2)});
    out.push_back({"klen overruns", patched(25 * 4, 13)});                   // the last entry: one byte too many
    out.push_back({"klen = 65535", patched(25 * 2, 65535)});
    out.push_back({"vlen overruns", patched(25 * 4 + 2, 9 + 1)});
    out.push_back({"vlen = 65535", patched(25 * 1 + 2, 65535)});
    out.push_back({"all 0xFF", Bytes(100, 0xFF)});
    out.push_back({"all 0xFF, 2 bytes", Bytes(2, 0xFF)});
    out.push_back({"all 0xFF, 200 000 bytes", Bytes(200000, 0xFF)});        // n = 65 535 fits; every offset is 65 535
    std::vector<std::string> keys;
    for (const auto& m : out) {
        const bool is_good = parse_plain(m.second, &keys);
        if (is_good) fprintf(stderr, "generator '%s' is well-formed\n", m.first);
        CHECK(!is_good);
    }
    return out;
}

struct Table {
    std::vector<Bytes> blocks;
    uint32_t num_bits, k;
};

// Tables -> one buffer with the blocks at odd offsets (junk between them), or
// every block in its own exact allocation addressed from the lowest one.
struct Batch {
    std::vector<std::unique_ptr<uint8_t[]>> own;
    Bytes flat;
    const uint8_t* base = nullptr;
    std::vector<uint64_t> blk_off, bseg;
    std::vector<uint32_t> blk_len, nb, kk;
};

static Batch make_batch(const std::vector<Table>& tabs, bool exact_allocs) {
    Batch bt;
    // two blocks no table claims in front, one behind
    std::vector<Bytes> all = {encode_block(entries(3, 900, 5)), Bytes(7, 0xFF)};
    bt.bseg.push_back(all.size());
    for (const Table& t : tabs) {
        all.insert(all.end(), t.blocks.begin(), t.blocks.end());
        bt.bseg.push_back(all.size());
        bt.nb.push_back(t.num_bits);
        bt.kk.push_back(t.k);
    }
    all.push_back(Bytes(3, 0xFF));
    if (exact_allocs) {
        for (const Bytes& b : all) bt.own.push_back(exact(b));
        bt.base = bt.own[0].get();
        for (const auto& p : bt.own) bt.base = std::min<const uint8_t*>(bt.base, p.get());
        for (size_t i = 0; i < all.size(); i++) {
            bt.blk_off.push_back((uint64_t)(bt.own[i].get() - bt.base));
            bt.blk_len.push_back((uint32_t)all[i].size());
        }
    } else {
        for (const Bytes& b : all) {
            bt.flat.push_back(0xEE);
            if (bt.flat.size() % 2 == 0) bt.flat.push_back(0xEE);  // every block starts at an odd offset
            bt.blk_off.push_back(bt.flat.size());
            bt.blk_len.push_back((uint32_t)b.size());
            bt.flat.insert(bt.flat.end(), b.begin(), b.end());
        }
        bt.own.push_back(exact(bt.flat));
        bt.base = bt.own[0].get();
    }
    return bt;
}

static void check_plan(const std::vector<Table>& tabs, const Batch& bt, const BbPlan& pl) {
    const uint64_t ntab = tabs.size();
    CHECK(pl.word_off.size() == ntab + 1 && pl.word_off[0] == 0);
    CHECK(pl.wave_region32 % 4 == 0 && pl.wave_region32 <= kBbWaveMaxBits / 32);
    CHECK((uint64_t)pl.wave_region32 * 4 * kBbWavesPerGroup <= kBbLdsBytes);
    CHECK(pl.group_region32 % 4 == 0 && (uint64_t)pl.group_region32 * 4 <= kBbLdsBytes);
    std::vector<std::vector<BbItem>> of(ntab);
    for (int cls = 0; cls < 2; cls++)
        for (const BbItem& it : cls ? pl.group : pl.wave) {
            CHECK(it.table < ntab);
            if (it.table >= ntab) continue;
            const Table& t = tabs[it.table];
            CHECK((cls == 0) == bb_is_wave(t.num_bits));
            CHECK(it.nw32 <= (cls ? pl.group_region32 : pl.wave_region32) && it.nw32 % 4 == 0);
            CHECK(it.dst == pl.word_off[it.table] && it.dst + it.nw32 / 2 == pl.word_off[it.table + 1]);
            CHECK(it.k == t.k && it.md.d == (t.num_bits ? t.num_bits : 1));
            of[it.table].push_back(it);
        }
    size_t nzero = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        uint64_t bytes = 0;
        for (const Bytes& b : tabs[t].blocks) bytes += b.size();
        std::vector<BbItem>& v = of[t];
        CHECK(v.size() == sst_parts(tabs[t].blocks.size(), bytes, tabs[t].num_bits) && !v.empty());
        uint64_t at = bt.bseg[t];  // (the plan emits a table's parts in block order)
        for (const BbItem& it : v) {
            CHECK(it.parts == v.size() && it.key_lo == at && it.key_hi >= it.key_lo);
            at = it.key_hi;
        }
        CHECK(at == bt.bseg[t + 1]);  // every block of the table exactly once
        if (v.size() > 1) nzero++;
    }
    CHECK(pl.zero.size() == nzero);
    for (const BbItem& z : pl.zero) CHECK(z.parts > 1 && z.dst == pl.word_off[z.table]);
}

static void run(const std::vector<Table>& tabs, bool exact_allocs, size_t want_split) {
    const Batch bt = make_batch(tabs, exact_allocs);
    const uint64_t ntab = tabs.size(), nblk = bt.blk_off.size();
    const BbPlan pl = sst_plan(bt.blk_len.data(), ntab, bt.bseg.data(), bt.nb.data(), bt.kk.data());
    check_plan(tabs, bt, pl);
    CHECK(pl.zero.size() >= want_split);
    const uint64_t total = pl.word_off[ntab], guard = 8;
    std::vector<uint64_t> words(total + guard, ~0ull);  // dirty, then a guard
    std::vector<uint32_t> ent(nblk, 0xABABABABu);
    build_batch_sst_ref(pl, bt.base, bt.blk_off.data(), bt.blk_len.data(), words.data(), ent.data());
    for (uint64_t g = 0; g < guard; g++) CHECK(words[total + g] == ~0ull);
    for (uint64_t b = 0; b < nblk; b++)
        if (b < bt.bseg[0] || b >= bt.bseg[ntab]) CHECK(ent[b] == 0xABABABABu);  // unclaimed: left as it was
    std::vector<std::string> keys;
    for (uint64_t t = 0; t < ntab; t++) {
        const uint32_t nb = bt.nb[t];
        const uint64_t nw = ((uint64_t)nb + 63) / 64;
        std::vector<uint64_t> exp(nw, 0);
        for (size_t j = 0; j < tabs[t].blocks.size(); j++) {
            const bool good = parse_plain(tabs[t].blocks[j], &keys);
            CHECK(good);  // (the tables here hold well-formed blocks only)
            CHECK(ent[bt.bseg[t] + j] == keys.size());
            for (const std::string& key : keys) literal_insert(exp.data(), nb, tabs[t].k, key);
        }
        const bool same = nw == 0 || memcmp(exp.data(), words.data() + pl.word_off[t], nw * 8) == 0;
        if (!same) fprintf(stderr, "table %llu (%zu blocks, %u bits, k %u) differs\n", (unsigned long long)t,
                           tabs[t].blocks.size(), nb, tabs[t].k);
        CHECK(same);
        for (uint64_t q = pl.word_off[t] + nw; q < pl.word_off[t + 1]; q++) CHECK(words[q] == 0);  // pad words
        if (nw && nb % 64) CHECK((words[pl.word_off[t] + nw - 1] >> (nb % 64)) == 0);
    }
}

// entries cut into blocks by BlockBuilder::add's rule (block/builder.rs:41-47)
static std::vector<Bytes> split(const std::vector<Entry>& es, size_t block_size) {
    std::vector<Bytes> out;
    std::vector<Entry> cur;
    size_t data = 0;
    for (const Entry& e : es) {
        const size_t sz = 4 + e.first.size() + e.second.size();
        if (!cur.empty() && data + cur.size() * 2 + 2 + sz > block_size) {
            out.push_back(encode_block(cur));
            cur.clear();
            data = 0;
        }
        cur.push_back(e);
        data += sz;
    }
    if (!cur.empty()) out.push_back(encode_block(cur));
    return out;
}

// ---- the caller's claim: sst_check_claim and sst_claim_span ---------------------------------
// A claim whose three arrays live in heap allocations of exactly their length:
// a read past blk_off[nblk - 1], blk_len[nblk - 1] or seg[ngroups] aborts the
// program.  `bytes` is never dereferenced by the check, so any non-null
// pointer stands for the buffer.
struct Claim {
    std::unique_ptr<uint64_t[]> off, seg;
    std::unique_ptr<uint32_t[]> len;
    SstClaim cl;
};
static const uint8_t g_some_byte = 0;
static Claim claim(uint64_t nbytes, const std::vector<uint64_t>& off, const std::vector<uint32_t>& len,
                   const std::vector<uint64_t>& seg) {
    Claim c;
    c.off.reset(new uint64_t[off.size()]);
    c.len.reset(new uint32_t[len.size()]);
    c.seg.reset(new uint64_t[seg.size()]);
    std::copy(off.begin(), off.end(), c.off.get());
    std::copy(len.begin(), len.end(), c.len.get());
    std::copy(seg.begin(), seg.end(), c.seg.get());
    c.cl = SstClaim{&g_some_byte, nbytes, off.size(), c.off.get(), c.len.get(), seg.size() - 1, c.seg.get()};
    return c;
}
static SstClaimFault check(const SstClaim& cl) {
    return sst_check_claim(cl, [](uint64_t) { return 0; });
}

static void check_claims() {
    const uint64_t top = ~0ull;
    // three blocks of a 100-byte buffer, two groups: accepted, the hook seen once per group in order
    {
        Claim c = claim(100, {0, 10, 50}, {10, 40, 50}, {0, 1, 3});
        std::vector<uint64_t> seen;
        const SstClaimFault f = sst_check_claim(c.cl, [&](uint64_t g) {
            seen.push_back(g);
            return 0;
        });
        CHECK(f.rule == kClaimOk && seen == std::vector<uint64_t>({0, 1}));
        const SstSpan sp = sst_claim_span(c.cl);
        CHECK(sp.lo == 0 && sp.hi == 100);
    }
    // each null array; blk_off and blk_len may be null when there is no block at all
    {
        Claim c = claim(100, {0, 10}, {10, 40}, {0, 1, 2});
        SstClaim cl = c.cl;
        cl.seg = nullptr;
        CHECK(check(cl).rule == kClaimNullSeg);
        cl = c.cl;
        cl.blk_off = nullptr;
        CHECK(check(cl).rule == kClaimNullBlocks);
        cl = c.cl;
        cl.blk_len = nullptr;
        CHECK(check(cl).rule == kClaimNullBlocks);
        Claim e = claim(100, {}, {}, {0, 0});
        e.cl.blk_off = nullptr;
        e.cl.blk_len = nullptr;
        e.cl.bytes = nullptr;
        CHECK(check(e.cl).rule == kClaimOk);
        const SstSpan sp = sst_claim_span(e.cl);  // no claimed block
        CHECK(sp.lo == 0 && sp.hi == 0);
    }
    // seg descends at group 1 of 3; the blocks are not looked at (block 0 leaves the buffer)
    {
        Claim c = claim(100, {90, 0, 0}, {20, 1, 1}, {0, 2, 1, 3});
        const SstClaimFault f = check(c.cl);
        CHECK(f.rule == kClaimSegDescends && f.group == 1);
    }
    // seg[ngroups] past nblk
    {
        Claim c = claim(100, {0, 10}, {10, 10}, {0, 1, 3});
        const SstClaimFault f = check(c.cl);
        CHECK(f.rule == kClaimSegPast && f.seg_end == 3);
    }
    // 2^31 groups over a valid 2-entry seg: refused before seg[2] would be read
    {
        Claim c = claim(100, {0}, {10}, {0, 1});
        c.cl.ngroups = 1ull << 31;
        CHECK(check(c.cl).rule == kClaimGroups);
        c.cl.ngroups = top;
        CHECK(check(c.cl).rule == kClaimGroups);
    }
    // a block that starts past the buffer; one that starts inside it and ends past it, the sum wrapping or not
    {
        Claim c = claim(100, {0, 101, 0}, {10, 0, 10}, {0, 1, 3});
        SstClaimFault f = check(c.cl);
        CHECK(f.rule == kClaimBlockLeaves && f.group == 1 && f.block == 1 && f.off == 101 && f.len == 0);
        c = claim(100, {0, 100}, {10, 1}, {0, 2});
        f = check(c.cl);
        CHECK(f.rule == kClaimBlockLeaves && f.group == 0 && f.block == 1 && f.off == 100 && f.len == 1);
        c = claim(100, {top}, {1}, {0, 1});
        f = check(c.cl);
        CHECK(f.rule == kClaimBlockLeaves && f.block == 0 && f.off == top);
        c = claim(top, {top}, {1}, {0, 1});  // off <= nbytes, off + len wraps to 0
        f = check(c.cl);
        CHECK(f.rule == kClaimBlockLeaves && f.off == top && f.len == 1);
        c = claim(100, {100, 99}, {0, 1}, {0, 2});  // the last byte and the empty block behind it are inside
        CHECK(check(c.cl).rule == kClaimOk);
    }
    // a non-empty block with null bytes; empty blocks need no bytes
    {
        Claim c = claim(100, {0, 5}, {0, 1}, {0, 2});
        c.cl.bytes = nullptr;
        const SstClaimFault f = check(c.cl);
        CHECK(f.rule == kClaimNullBytes && f.block == 1);
        c = claim(100, {0, 5}, {0, 0}, {0, 2});
        c.cl.bytes = nullptr;
        CHECK(check(c.cl).rule == kClaimOk);
    }
    // the hook's refusal of group 1 comes before group 1's bad block and after group 0's good one
    {
        Claim c = claim(100, {0, 200}, {10, 1}, {0, 1, 2});
        SstClaimFault f = sst_check_claim(c.cl, [](uint64_t g) { return g == 1 ? -7 : 0; });
        CHECK(f.rule == kClaimGroupHook && f.group == 1 && f.hook_rc == -7);
        f = check(c.cl);
        CHECK(f.rule == kClaimBlockLeaves && f.group == 1 && f.block == 1);
    }
    // a strict sub-run claimed: the faults of blocks 0 and 4 are no one's business
    {
        Claim c = claim(100, {500, 10, 20, 30, top}, {9, 10, 10, 10, 9}, {1, 2, 4});
        CHECK(check(c.cl).rule == kClaimOk);
        const SstSpan sp = sst_claim_span(c.cl);
        CHECK(sp.lo == 10 && sp.hi == 40);
    }
    // accepted: empty blocks at both ends of the claim; they do not widen the span
    {
        Claim c = claim(100, {0, 40, 60, 100}, {0, 5, 7, 0}, {0, 1, 4});
        CHECK(check(c.cl).rule == kClaimOk);
        const SstSpan sp = sst_claim_span(c.cl);
        CHECK(sp.lo == 40 && sp.hi == 67);
    }
    // the span of only empty blocks, of one block, and of blocks out of address order
    {
        Claim c = claim(100, {30, 70}, {0, 0}, {0, 2});
        SstSpan sp = sst_claim_span(c.cl);
        CHECK(sp.lo == 0 && sp.hi == 0);
        c = claim(100, {33}, {11}, {0, 1});
        sp = sst_claim_span(c.cl);
        CHECK(sp.lo == 33 && sp.hi == 44);
        c = claim(100, {80, 3, 41}, {20, 5, 1}, {0, 1, 3});
        CHECK(check(c.cl).rule == kClaimOk);
        sp = sst_claim_span(c.cl);
        CHECK(sp.lo == 3 && sp.hi == 100);
    }
}

int main() {
    check_claims();
    // ---- single blocks, well-formed: the counts, the odd keys and values, the long block
    for (size_t n : {0, 1, 63, 64, 65, 200}) check_block(encode_block(entries(n, 0, 3)), "n entries");
    check_block(encode_block({Entry("", "v"), Entry(rnd_str(300), "value"), Entry("k", "")}),
                "empty key, 300-byte key, tombstone");
    check_block(encode_block({Entry("", "")}), "one empty entry");
    check_block(encode_block(entries(40, 0, 0)), "tombstones only");
    {
        const Bytes big = encode_block({Entry(rnd_str(300), rnd_str(65535))});
        CHECK(big.size() > 65535);
        check_block(big, "a single entry past 65 535 bytes");
    }
    {
        // offsets that descend and entries that overlap are still well-formed
        Bytes b = encode_block(entries(4, 0, 2));
        const size_t de = b.size() - 2 - 8;
        std::swap(b[de], b[de + 6]);
        std::swap(b[de + 1], b[de + 7]);
        b[de + 2] = b[de + 4];
        b[de + 3] = b[de + 5];
        std::vector<std::string> keys;
        CHECK(parse_plain(b, &keys) && keys.size() == 4 && keys[1] == keys[2]);
        check_block(b, "descending and repeated offsets");
    }
    // ---- malformed blocks: reported, never read out of bounds
    const auto bad = malformed();
    for (const auto& m : bad) check_block(m.second, m.first);
    size_t n_good = 0, n_bad = 0;
    for (int r = 0; r < 4000; r++) {
        Bytes b(rnd() % 601);
        for (uint8_t& c : b) c = (uint8_t)rnd();
        if (r % 2 && b.size() >= 2) {  // a plausible count, so that the entries are reached
            const size_t n = rnd() % 6;
            b[b.size() - 2] = (uint8_t)n;
            b[b.size() - 1] = 0;
            for (size_t i = 0; i < n && 2 + 2 * n <= b.size(); i++)  // and offsets that often land inside
                if (rnd() % 4) {
                    b[b.size() - 2 - 2 * n + 2 * i] = (uint8_t)(rnd() % (b.size() / 2 + 1));
                    b[b.size() - 2 - 2 * n + 2 * i + 1] = 0;
                }
        }
        std::vector<std::string> keys;
        (parse_plain(b, &keys) ? n_good : n_bad)++;
        check_block(b, "random bytes");
    }
    CHECK(n_good >= 100 && n_bad >= 1000);  // the random strings reach both verdicts

    // ---- sst_parts: at least one, non-decreasing in bytes, never more than the blocks
    for (uint32_t nbits : {64u, 9586u, kBbWaveMaxBits, kBbWaveMaxBits + 1, kBbMaxBits}) {
        uint32_t last = 1;
        for (uint64_t bytes = 0; bytes < (64u << 20); bytes += 99991) {
            const uint32_t p = sst_parts(1u << 20, bytes, nbits);
            CHECK(p >= last);
            last = p;
        }
        CHECK(sst_parts(0, 0, nbits) == 1 && sst_parts(29, 29 * 4096, nbits) == 1 && sst_parts(3, ~0ull, nbits) == 3);
        CHECK(sst_parts(~0ull, ~0ull, nbits) == kBbMaxParts);
    }

    // ---- whole batches through build_batch_sst_ref
    {
        std::vector<Table> tabs;
        tabs.push_back(Table{{}, 9586, 7});                                   // no blocks
        tabs.push_back(Table{{encode_block({})}, 9586, 7});                   // one empty block
        for (size_t n : {1, 63, 64, 65, 200}) tabs.push_back(Table{{encode_block(entries(n, 1000 * n, 3))}, 9586, 7});
        tabs.push_back(Table{split(entries(1000, 5000, 100), 4096), 9586, 7});
        tabs.push_back(Table{{encode_block({Entry("", "v"), Entry(rnd_str(300), ""), Entry("k", "")}),
                              encode_block({Entry(rnd_str(300), rnd_str(65535))})}, 65537, 7});
        tabs.push_back(Table{split(entries(300, 7000, 20), 512), 64, 1});
        tabs.push_back(Table{split(entries(300, 8000, 20), 512), 65536, 40});
        tabs.push_back(Table{split(entries(50, 9000, 20), 512), 1310720, 0});
        tabs.push_back(Table{{encode_block(entries(2, 0, 1))}, 0, 0});        // a filter of no bits
        tabs.push_back(Table{{encode_block(std::vector<Entry>(90, Entry("same key", "v")))}, 9586, 7});
        run(tabs, true, 0);   // every block in an allocation of exactly its length
        run(tabs, false, 0);  // every block at an odd offset of one buffer
    }
    {
        // one table of two parts or more per class, the block count by search
        std::vector<Table> tabs;
        for (uint32_t nbits : {9586u, kBbMaxBits}) {
            const std::vector<Bytes> blocks = split(entries(45000, 0, 100), 4096);
            uint64_t bytes = 0;
            size_t n = 0;
            while (n < blocks.size() && sst_parts(n, bytes, nbits) < 2) bytes += blocks[n++].size();
            CHECK(sst_parts(n, bytes, nbits) >= 2);
            tabs.push_back(Table{std::vector<Bytes>(blocks.begin(), blocks.begin() + n), nbits, 7});
        }
        run(tabs, false, 2);
    }
    printf("%s\n", g_fail ? "FAIL" : "all passed");
    return g_fail ? 1 : 0;
}

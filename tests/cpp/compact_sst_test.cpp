// compact_sst_test.cpp — the compaction's output filter through the C++ mirror
// (storage-engine_amd/cpp/lsm_bloom.hpp): Context::compact_sst_bloom.  Three
// sources' blocks are encoded the way BlockBuilder does
// (src/sstable/block/builder.rs:40-76); the returned bloom block is compared
// with the mirror's own per-key inserts of the keys a std::map merge keeps
// (src/iterator/merge.rs:98-121, src/compaction/scheduler.rs:152-158), and a
// malformed block must surface as Corruption.
// Usage: compact_sst_test [--gpu]   (without --gpu: the argument checks only)
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../storage-engine_amd/cpp/lsm_bloom.hpp"

using lsm::bloom::BloomFilter;
using lsm::bloom::Context;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

typedef std::pair<std::string, std::string> Entry;

static void put16(std::vector<uint8_t>* b, size_t v) {
    b->push_back((uint8_t)(v & 0xFF));
    b->push_back((uint8_t)((v >> 8) & 0xFF));
}

// [klen u16][vlen u16][key][value] ... [off u16 ...][n u16]
static std::vector<uint8_t> encode_block(const std::vector<Entry>& es) {
    std::vector<uint8_t> b;
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

static std::string key(int i) {
    char k[32];
    snprintf(k, sizeof k, "key_%06d", i);
    return k;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        const uint32_t len[2] = {2, 2};
        const uint64_t off[2] = {0, 2}, sseg[3] = {0, 1, 2};
        uint64_t blen = 7, count = 9;
        uint32_t nb = 9, kk = 9;
        uint8_t bytes[4] = {0, 0, 0, 0}, out[8] = {0};
        CHECK(lsmb_compact_sst_work_bytes(0, nullptr) == 0 && lsmb_compact_sst_work_bytes(2, len) == 2 * 56);
        CHECK(lsmb_compact_sst_mark_dev(nullptr, bytes, 4, 2, off, len, 2, sseg, 0, out, 1 << 20, nullptr, out, nullptr) ==
              LSMB_EINVAL);
        CHECK(lsmb_compact_sst_gather_dev(nullptr, bytes, 4, 2, off, len, 2, sseg, out, out, 8, out, 1, nullptr) == LSMB_EINVAL);
        CHECK(lsmb_compact_sst_bloom(nullptr, bytes, 4, 2, off, len, 2, sseg, 0, 1000, 0.01, out, sizeof out, &blen, &count, &nb,
                                     &kk) == LSMB_EINVAL);
        CHECK(blen == 7 && count == 9 && nb == 9 && kk == 9 && out[0] == 0);
    }
    if (gpu) {
        // three sources of 300 keys each, overlapping by half, in blocks of at most 40; every seventh value empty
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> blk_off, sseg;
        std::vector<uint32_t> blk_len;
        std::map<std::string, std::pair<int, bool>> newest;  // key -> (source, live)
        auto add_block = [&](const std::vector<uint8_t>& b) {
            bytes.push_back(0xEE);  // blocks at arbitrary byte offsets
            blk_off.push_back(bytes.size());
            blk_len.push_back((uint32_t)b.size());
            bytes.insert(bytes.end(), b.begin(), b.end());
        };
        add_block(encode_block({Entry("unclaimed", "x")}));
        for (int s = 0; s < 3; s++) {
            sseg.push_back(blk_off.size());
            for (int i = 0; i < 300; i += 40) {
                std::vector<Entry> es;
                for (int j = i; j < std::min(i + 40, 300); j++) {
                    const std::string k = key(150 * s + j);
                    const bool live = (j + s) % 7 != 0;
                    es.push_back(Entry(k, live ? std::string(1 + j % 50, 'v') : std::string()));
                    newest.insert({k, {s, live}});
                }
                add_block(encode_block(es));
            }
        }
        sseg.push_back(blk_off.size());
        add_block(std::vector<uint8_t>(5, 0xFF));  // malformed, and no source's

        Context ctx(0);
        for (int drop = 0; drop < 2; drop++)
            for (uint64_t expected : {(uint64_t)1000, (uint64_t)0}) {
                const Context::CompactedFilter got = ctx.compact_sst_bloom(bytes, blk_off, blk_len, sseg, drop != 0, expected);
                std::vector<std::string> keep;
                for (const auto& kv : newest)
                    if (!drop || kv.second.second) keep.push_back(kv.first);
                CHECK(got.entry_count == keep.size() && keep.size() < 900);
                uint32_t nb = 0, kk = 0;
                lsm::bloom::check(lsmb_params(expected ? expected : keep.size(), 0.01, &nb, &kk));
                CHECK(got.num_bits == nb && got.num_hashes == kk && got.bloom.size() == lsmb_serialized_size(nb));
                // the survivors' bits and nothing else: equal to the mirror's own per-key inserts
                BloomFilter have = BloomFilter::deserialize(got.bloom);
                BloomFilter own = BloomFilter::deserialize(got.bloom);
                std::fill(own.words().begin(), own.words().end(), 0);
                for (const std::string& k : keep) own.insert(k);
                CHECK(own.words() == have.words());
            }
        // the malformed block claimed by a fourth source: Corruption, naming it
        sseg.push_back(blk_off.size());
        bool threw = false;
        try {
            ctx.compact_sst_bloom(bytes, blk_off, blk_len, sseg, false, 1000);
        } catch (const lsm::bloom::Corruption& e) {
            threw = strstr(e.what(), "source 3") != nullptr;
        }
        CHECK(threw);
        // a block that leaves the buffer is refused before anything runs
        blk_len.back() += 1;
        threw = false;
        try {
            ctx.compact_sst_bloom(bytes, blk_off, blk_len, sseg, false, 1000);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

// build_batch_test.cpp — the batched build through the C++ mirror
// (storage-engine_amd/cpp/lsm_bloom.hpp): Context::build_batch_blocks and
// LevelSet::add_built.  A few tables are built from one key run; every member
// key is checked with the mirror's own may_contain on the returned blocks and
// with the probe of a level set that took the device-built words directly.
// Usage: build_batch_test [--gpu]   (without --gpu: the argument checks only)
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../storage-engine_amd/cpp/lsm_bloom.hpp"

using lsm::bloom::BloomFilter;
using lsm::bloom::Context;
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

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    {
        const uint32_t nb[2] = {64, 9586}, kk[2] = {1, 7};
        const uint64_t seg[3] = {0, 0, 0};
        uint64_t off[3] = {7, 7, 7};
        uint8_t blk[8] = {0};
        CHECK(lsmb_build_batch_max_bits() == 1310720u);
        CHECK(lsmb_build_batch_layout(2, nb, nullptr) == LSMB_EINVAL);
        CHECK(lsmb_build_batch_layout(2, nullptr, off) == LSMB_EINVAL && off[0] == 7);
        CHECK(lsmb_build_batch_layout(2, nb, off) == LSMB_OK && off[0] == 0 && off[1] == 2 && off[2] == 2 + 150);
        CHECK(lsmb_build_batch_parts(0, 9586) == 1 && lsmb_build_batch_parts(1000, 9586) == 1);
        off[0] = off[1] = off[2] = 7;
        CHECK(lsmb_build_batch_dev(nullptr, nullptr, nullptr, 16, 0, 2, seg, nb, kk, blk, 1 << 20, nullptr) == LSMB_EINVAL);
        CHECK(lsmb_build_batch_blocks(nullptr, nullptr, nullptr, 16, 0, 2, seg, nb, kk, blk, sizeof blk, off) == LSMB_EINVAL);
        CHECK(off[0] == 7 && off[2] == 7 && blk[0] == 0);
        CHECK(lsmb_lset_add_batch_dev(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) == LSMB_EINVAL);
    }
    if (gpu) {
        // five tables of 0, 1, 70, 200 and 1 000 keys, with unclaimed keys before and after
        const int counts[5] = {0, 1, 70, 200, 1000};
        std::vector<std::string> keys;
        std::vector<uint64_t> seg;
        std::vector<uint32_t> nb, kk, rows, ids;
        std::vector<LevelSet::TableRange> ranges;
        for (int i = 0; i < 5; i++) keys.push_back(key(900000 + i));
        int next = 0;
        for (int t = 0; t < 5; t++) {
            seg.push_back(keys.size());
            uint32_t b = 0, h = 0;
            lsm::bloom::check(lsmb_params(counts[t] ? counts[t] : 1, 0.01, &b, &h));
            nb.push_back(b);
            kk.push_back(h);
            rows.push_back(t & 1);
            ids.push_back(100 + t);
            // (an empty table still owns a range, disjoint from the others)
            ranges.push_back({key(next), key(next + (counts[t] ? counts[t] - 1 : 0))});
            for (int i = 0; i < counts[t]; i++) keys.push_back(key(next + i));
            next += counts[t] + 10;
        }
        seg.push_back(keys.size());
        for (int i = 0; i < 3; i++) keys.push_back(key(910000 + i));

        Context ctx(0);
        const std::vector<std::vector<uint8_t>> blocks = ctx.build_batch_blocks(keys, seg, nb, kk);
        CHECK(blocks.size() == 5);
        std::vector<BloomFilter> filt;
        for (size_t t = 0; t < blocks.size(); t++) {
            CHECK(blocks[t].size() == lsmb_serialized_size(nb[t]));
            filt.push_back(BloomFilter::deserialize(blocks[t]));
            CHECK(filt.back().num_bits() == nb[t] && filt.back().num_hashes() == kk[t]);
            for (uint64_t i = seg[t]; i < seg[t + 1]; i++) CHECK(filt.back().may_contain(keys[i]));
            // and nothing but the members' bits: equal to the mirror's own per-key inserts
            BloomFilter own = BloomFilter::deserialize(blocks[t]);
            std::fill(own.words().begin(), own.words().end(), 0);
            for (uint64_t i = seg[t]; i < seg[t + 1]; i++) own.insert(keys[i]);
            CHECK(own.words() == filt.back().words());
        }

        // the same run on the device, the built words straight into a level set
        std::string data;
        std::vector<uint64_t> offs(keys.size() + 1, 0), woff(6, 0);
        for (size_t i = 0; i < keys.size(); i++) {
            data += keys[i];
            offs[i + 1] = data.size();
        }
        lsm::bloom::check(lsmb_build_batch_layout(5, nb.data(), woff.data()));
        void *d_data = nullptr, *d_offs = nullptr, *d_words = nullptr;
        CHECK(hipMalloc(&d_data, data.size() + 16) == hipSuccess);
        CHECK(hipMalloc(&d_offs, offs.size() * 8) == hipSuccess);
        CHECK(hipMalloc(&d_words, woff[5] * 8) == hipSuccess);
        CHECK(hipMemcpy(d_data, data.data(), data.size(), hipMemcpyHostToDevice) == hipSuccess);
        CHECK(hipMemcpy(d_offs, offs.data(), offs.size() * 8, hipMemcpyHostToDevice) == hipSuccess);
        lsm::bloom::check(lsmb_build_batch_dev(ctx.get(), d_data, d_offs, 0, keys.size(), 5, seg.data(), nb.data(),
                                               kk.data(), d_words, woff[5], nullptr));
        LevelSet ls(ctx);
        ls.add_built(rows, ids, d_words, nb, kk, ranges);
        const auto st = ls.stats();
        CHECK(st[0] == 5 && st[2] == 0 && st[3] == 0);
        std::vector<uint64_t> got(woff[5]);
        CHECK(hipMemcpy(got.data(), d_words, woff[5] * 8, hipMemcpyDeviceToHost) == hipSuccess);
        for (size_t t = 0; t < 5; t++)
            CHECK(memcmp(got.data() + woff[t], filt[t].words().data(), filt[t].words().size() * 8) == 0);
        (void)hipFree(d_words);  // add_built has returned: the source buffer is free to go
        ls.seal();
        const std::vector<uint32_t> ans = ls.probe(keys);
        CHECK(ans.size() == 2 * keys.size());
        for (size_t t = 0; t < 5 && ans.size() == 2 * keys.size(); t++)
            for (uint64_t i = seg[t]; i < seg[t + 1]; i++) {
                CHECK(ans[rows[t] * keys.size() + i] == ids[t]);
                CHECK(ans[(1 - rows[t]) * keys.size() + i] == LSMB_LSET_NONE);
            }
        for (size_t i = 0; i < keys.size(); i++)
            if (i < seg[0] || i >= seg[5]) CHECK(ans[i] == LSMB_LSET_NONE && ans[keys.size() + i] == LSMB_LSET_NONE);
        (void)hipFree(d_data);
        (void)hipFree(d_offs);
    }
    printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}

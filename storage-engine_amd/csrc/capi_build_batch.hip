// capi_build_batch.hip — the C ABI of the batched build (lsmb_build_batch_*,
// include/lsmbloom.h).  Host-side plumbing only; the plan is in
// build_batch_plan.hpp, the kernels in build_batch.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "build_batch_plan.hpp"
#include "ctx.hpp"

using namespace lsmb;

extern "C" {

// ---------------------------------------------------------------- batched build
// Many tables' filters from one key run (build_batch_plan.hpp, build_batch.hip):
// SSTableBuilder::new + add per key + finish (src/sstable/builder.rs:74,93,
// 177-182) for every output table of a bulk load or of compactions finishing
// together (src/compaction/scheduler.rs:147-177), one launch per geometry class.
namespace {

// Measurement switch (the geometry A/B of tools/mb_build_batch.py), read at every
// call: LSMB_BB_WAVE_MAX_BITS below the wave class's limit sends smaller
// filters to the group class too.  The filter bits never depend on it.
uint32_t bb_wave_max_bits() {
    const char* s = getenv("LSMB_BB_WAVE_MAX_BITS");
    return s ? (uint32_t)std::min<uint64_t>(strtoull(s, nullptr, 10), kBbWaveMaxBits) : kBbWaveMaxBits;
}

// The same for the group class's workgroup: LSMB_BB_GROUP_LANES = 64 .. 1024.
uint32_t bb_group_lanes() {
    const char* s = getenv("LSMB_BB_GROUP_LANES");
    const uint64_t v = s ? strtoull(s, nullptr, 10) : kBbGroupLanes;
    return v >= kBbWaveLanes && v <= kBbGroupLanes && v % kBbWaveLanes == 0 ? (uint32_t)v : kBbGroupLanes;
}

// What every batched build checks before anything is written.
int bb_check(uint64_t n, uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes) {
    if (!seg || !num_bits || !num_hashes) return fail(LSMB_EINVAL, "batched build: null seg, num_bits or num_hashes");
    if (ntab >= (1ull << 31)) return fail(LSMB_EINVAL, "batched build: more than 2^31-1 tables");
    uint64_t items = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        if (seg[t + 1] < seg[t])
            return fail(LSMB_EINVAL, "batched build: seg descends at table %llu", (unsigned long long)t);
        if (check_filter(num_bits[t], num_hashes[t]) != LSMB_OK) {
            const std::string msg = last_error();
            return fail(LSMB_EINVAL, "batched build: table %llu: %s", (unsigned long long)t, msg.c_str());
        }
        if (num_bits[t] > kBbMaxBits)
            return fail(LSMB_EINVAL,
                        "batched build: table %llu has %u bits, above lsmb_build_batch_max_bits() = %u "
                        "(build it with lsmb_build_fixed_dev_new / lsmb_build_var_dev_new)",
                        (unsigned long long)t, num_bits[t], kBbMaxBits);
        items += bb_parts(seg[t + 1] - seg[t], num_bits[t], bb_wave_max_bits());
    }
    if (seg[ntab] > n)
        return fail(LSMB_EINVAL, "batched build: seg[ntab] = %llu is past the run's %llu keys",
                    (unsigned long long)seg[ntab], (unsigned long long)n);
    if (items >= (1ull << 31)) return fail(LSMB_EINVAL, "batched build: more than 2^31-1 work items");
    return LSMB_OK;
}

// The plan's items through a staging slot to the device and the launches, all
// on st; nothing is synchronised but the slot's own reuse (see lsmb_ctx).
int bb_enqueue(lsmb_ctx* c, const KeyBatch& kb, const BbPlan& pl, uint64_t* d_words, hipStream_t st) {
    const size_t nz = pl.zero.size(), nw = pl.wave.size(), ng = pl.group.size();
    const size_t bytes = (nz + nw + ng) * sizeof(BbItem);
    const int s = c->bb_slot;
    c->bb_slot ^= 1;
    if (!c->bb_done[s])
        HIP_TRY(hipEventCreateWithFlags(&c->bb_done[s], hipEventDisableTiming));
    else if (c->bb_stream[s])
        HIP_TRY(hipEventSynchronize(c->bb_done[s]));  // the copy out of this slot, two batches ago
    if (int rc = pinned_ensure(c->pinned_retired, &c->bb_pin[s], &c->bb_pin_cap[s], bytes, "batched build")) return rc;
    HIP_TRY(c->bb_items[s].ensure(bytes));
    BbItem* h = (BbItem*)c->bb_pin[s];
    if (nz) memcpy(h, pl.zero.data(), nz * sizeof(BbItem));
    if (nw) memcpy(h + nz, pl.wave.data(), nw * sizeof(BbItem));
    if (ng) memcpy(h + nz + nw, pl.group.data(), ng * sizeof(BbItem));
    if (c->bb_stream[s] && c->bb_stream[s] != st) HIP_TRY(hipStreamWaitEvent(st, c->bb_done[s], 0));
    HIP_TRY(hipMemcpyAsync(c->bb_items[s].p, h, bytes, hipMemcpyHostToDevice, st));
    const hipError_t e = launch_build_batch(kb, (const BbItem*)c->bb_items[s].p, (uint32_t)nz, (uint32_t)nw,
                                            (uint32_t)ng, pl.wave_region32, pl.group_region32, bb_group_lanes(), d_words,
                                            st, c->bb_done[s]);
    c->bb_stream[s] = st;
    if (e != hipSuccess) {
        (void)hipEventRecord(c->bb_done[s], st);  // (a failed launch may not have completed the event)
        return hip_fail(e, "launch_build_batch");
    }
    return LSMB_OK;
}

}  // namespace

uint32_t lsmb_build_batch_max_bits(void) { return kBbMaxBits; }

int lsmb_build_batch_layout(uint64_t ntab, const uint32_t* num_bits, uint64_t* word_off) {
    if (!word_off || (ntab && !num_bits)) return fail(LSMB_EINVAL, "batched build layout: null argument");
    bb_layout(ntab, num_bits, word_off);
    return LSMB_OK;
}

int lsmb_build_batch_parts(uint64_t keys, uint32_t num_bits) {
    return (int)bb_parts(keys, num_bits, bb_wave_max_bits());
}

int lsmb_build_batch_dev(lsmb_ctx* c, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                         uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes,
                         void* d_words, uint64_t words_cap, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (ntab == 0) return LSMB_OK;
    if (int rc = bb_check(n, ntab, seg, num_bits, num_hashes)) return rc;
    if (!d_words) return fail(LSMB_EINVAL, "batched build: null d_words");
    if (reinterpret_cast<uintptr_t>(d_words) & 15) return fail(LSMB_EINVAL, "batched build: d_words is not 16-byte aligned");
    // fixed-length keys of length 0 are all the empty key: nothing is read for them
    if (seg[ntab] > seg[0] && (d_offsets || key_len) && !d_data) return fail(LSMB_EINVAL, "batched build: null keys");
    const BbPlan pl = bb_plan(ntab, seg, num_bits, num_hashes, bb_wave_max_bits());
    if (words_cap < pl.word_off[ntab])
        return fail(LSMB_EINVAL, "batched build: words_cap %llu < the layout's %llu words", (unsigned long long)words_cap,
                    (unsigned long long)pl.word_off[ntab]);
    DevGuard g(c->dev);
    const KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    return bb_enqueue(c, kb, pl, (uint64_t*)d_words, pick_stream(c, stream));
}

int lsmb_build_batch_blocks(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                            uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes,
                            uint8_t* blocks, uint64_t blocks_cap, uint64_t* block_off) {
    if (!c) return fail(LSMB_EINVAL, "null ctx: the batched build runs on the GPU whatever the key count");
    if (!block_off) return fail(LSMB_EINVAL, "batched build: null block_off");
    if (ntab == 0) {
        block_off[0] = 0;
        return LSMB_OK;
    }
    if (int rc = bb_check(n, ntab, seg, num_bits, num_hashes)) return rc;
    if (n && host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "batched build: null keys");
    if (n && offsets) {
        if (int rc = check_offsets(offsets, n)) return rc;
    }
    block_off[0] = 0;
    for (uint64_t t = 0; t < ntab; t++) block_off[t + 1] = block_off[t] + 12 + 8 * nwords64(num_bits[t]);
    if (!blocks || blocks_cap < block_off[ntab])
        return fail(LSMB_EINVAL, "batched build: blocks buffer %llu B < the %llu B of the batch's blocks",
                    (unsigned long long)(blocks ? blocks_cap : 0), (unsigned long long)block_off[ntab]);
    DevGuard g(c->dev);
    const BbPlan pl = bb_plan(ntab, seg, num_bits, num_hashes, bb_wave_max_bits());
    const uint64_t wbytes = pl.word_off[ntab] * 8;
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    HIP_TRY(c->bb_words.ensure(wbytes));
    if (int rc = pinned_ensure(c->pinned_retired, &c->bb_host, &c->bb_host_cap, wbytes, "batched build")) return rc;
    if (int rc = bb_enqueue(c, kb, pl, (uint64_t*)c->bb_words.p, c->st)) return rc;
    HIP_TRY(hipMemcpyAsync(c->bb_host, c->bb_words.p, wbytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    for (uint64_t t = 0; t < ntab; t++) {
        uint8_t* b = blocks + block_off[t];
        write_header(b, num_bits[t], num_hashes[t]);
        const uint64_t nw = nwords64(num_bits[t]);
        if (nw) memcpy(b + 12, c->bb_host + pl.word_off[t] * 8, nw * 8);
    }
    return LSMB_OK;
}

}  // extern "C"

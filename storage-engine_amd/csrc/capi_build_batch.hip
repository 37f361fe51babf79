// capi_build_batch.hip — the C ABI of the batched build (lsmb_build_batch_*,
// include/lsmbloom.h).  Host-side plumbing only; the plan is in
// build_batch_plan.hpp, the kernels in build_batch.hip; from data blocks
// (lsmb_build_batch_sst_*), in sst_blocks.hpp and build_batch_sst.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "build_batch_plan.hpp"
#include "ctx.hpp"

using namespace lsmb;

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

// What every batched build asks of table t's filter; `hint` ends the message.
int bb_check_table(const char* who, uint64_t t, uint32_t num_bits, uint32_t k, const char* hint) {
    if (check_filter(num_bits, k) != LSMB_OK) {
        const std::string msg = last_error();
        return fail(LSMB_EINVAL, "%s: table %llu: %s", who, (unsigned long long)t, msg.c_str());
    }
    if (num_bits > kBbMaxBits)
        return fail(LSMB_EINVAL, "%s: table %llu has %u bits, above lsmb_build_batch_max_bits() = %u%s", who,
                    (unsigned long long)t, num_bits, kBbMaxBits, hint);
    return LSMB_OK;
}

// What every batched build checks before anything is written.
int bb_check(uint64_t n, uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes) {
    if (!seg || !num_bits || !num_hashes) return fail(LSMB_EINVAL, "batched build: null seg, num_bits or num_hashes");
    if (ntab >= (1ull << 31)) return fail(LSMB_EINVAL, "batched build: more than 2^31-1 tables");
    uint64_t items = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        if (seg[t + 1] < seg[t])
            return fail(LSMB_EINVAL, "batched build: seg descends at table %llu", (unsigned long long)t);
        if (int rc = bb_check_table("batched build", t, num_bits[t], num_hashes[t],
                                    " (build it with lsmb_build_fixed_dev_new / lsmb_build_var_dev_new)"))
            return rc;
        items += bb_parts(seg[t + 1] - seg[t], num_bits[t], bb_wave_max_bits());
    }
    if (seg[ntab] > n)
        return fail(LSMB_EINVAL, "batched build: seg[ntab] = %llu is past the run's %llu keys",
                    (unsigned long long)seg[ntab], (unsigned long long)n);
    if (items >= (1ull << 31)) return fail(LSMB_EINVAL, "batched build: more than 2^31-1 work items");
    return LSMB_OK;
}

// The items through a staging slot to the device and the launches, all on st
// (slot_enqueue, ctx.hpp).  The three lists are parts of whole 64-byte items, so
// the device sees one array, zero items first, at the first part's address.
static_assert(sizeof(BbItem) % kSlotAlign == 0, "the item lists are staged back to back");

int bb_enqueue(lsmb_ctx* c, const KeyBatch& kb, const BbPlan& pl, uint64_t* d_words, hipStream_t st) {
    SlotPart p[] = {slot_part(pl.zero), slot_part(pl.wave), slot_part(pl.group)};
    return slot_enqueue(c, p, 3, st, "batched build", "launch_build_batch", [&](hipEvent_t done) {
        return launch_build_batch(kb, (const BbItem*)p[0].d, (uint32_t)pl.zero.size(), (uint32_t)pl.wave.size(),
                                  (uint32_t)pl.group.size(), pl.wave_region32, pl.group_region32, bb_group_lanes(),
                                  d_words, st, done);
    });
}

// ---- from data blocks (sst_blocks.hpp, build_batch_sst.hip) -----------------------
// Measurement switches of tools/mb_build_batch_sst.py, read at every call: the
// block bytes one item walks, per class (LSMB_SST_WAVE_BYTES, LSMB_SST_GROUP_BYTES),
// beside the batched build's own.  The filter bits never depend on them.
SstBounds bbs_bounds() {
    SstBounds bd;
    if (const char* s = getenv("LSMB_SST_WAVE_BYTES")) bd.wave_bytes = strtoull(s, nullptr, 10);
    if (const char* s = getenv("LSMB_SST_GROUP_BYTES")) bd.group_bytes = strtoull(s, nullptr, 10);
    bd.wave_max_bits = bb_wave_max_bits();
    return bd;
}

// What lsmb_build_batch_sst_* check before anything is written or any byte is read:
// sst_check_claim's rules (sst_blocks.hpp), table t's own in front of t's blocks.
int bbs_check(const SstClaim& cl, const uint32_t* num_bits, const uint32_t* num_hashes) {
    if (!cl.seg || !num_bits || !num_hashes)
        return fail(LSMB_EINVAL, "batched build from blocks: null bseg, num_bits or num_hashes");
    const char* who = "batched build from blocks";
    const SstClaimFault f =
        sst_check_claim(cl, [&](uint64_t t) { return bb_check_table(who, t, num_bits[t], num_hashes[t], ""); });
    // (a table has at most one part per block: fewer than 2^31 work items)
    return claim_fail(f, cl, who, "bseg", "ntab", "table", true);
}

// The claimed blocks [bseg[0], bseg[ntab]) renumbered from 0: their descriptors
// (offsets less `origin`) and the plan over them.
struct BbsWork {
    std::vector<SstBlk> blks;
    BbPlan pl;
};
BbsWork bbs_work(const uint64_t* blk_off, const uint32_t* blk_len, uint64_t ntab, const uint64_t* bseg,
                 const uint32_t* num_bits, const uint32_t* num_hashes, uint64_t origin) {
    BbsWork w;
    const uint64_t b0 = bseg[0], nb = bseg[ntab] - b0;
    w.blks.resize(nb);
    for (uint64_t b = 0; b < nb; b++) w.blks[b] = SstBlk{blk_off[b0 + b] - origin, blk_len[b0 + b], 0};
    std::vector<uint64_t> seg(ntab + 1);
    for (uint64_t t = 0; t <= ntab; t++) seg[t] = bseg[t] - b0;
    w.pl = sst_plan(nb ? blk_len + b0 : nullptr, ntab, seg.data(), num_bits, num_hashes, bbs_bounds());
    return w;
}

// d_blk_entries: of the claimed blocks, renumbered like the descriptors.
int bbs_enqueue(lsmb_ctx* c, const uint8_t* d_bytes, const BbsWork& w, uint64_t* d_words, uint32_t* d_blk_entries,
                hipStream_t st) {
    const BbPlan& pl = w.pl;
    SlotPart p[] = {slot_part(pl.zero), slot_part(pl.wave), slot_part(pl.group), slot_part(w.blks)};
    return slot_enqueue(c, p, 4, st, "batched build", "launch_build_batch_sst", [&](hipEvent_t done) {
        return launch_build_batch_sst(d_bytes, (const SstBlk*)p[3].d, (const BbItem*)p[0].d, (uint32_t)pl.zero.size(),
                                      (uint32_t)pl.wave.size(), (uint32_t)pl.group.size(), pl.wave_region32,
                                      pl.group_region32, bb_group_lanes(), d_words, d_blk_entries, st, done);
    });
}

static_assert(LSMB_SST_BAD_BLOCK == kSstBadBlock, "the header's value is the kernels'");

}  // namespace

extern "C" {

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

// ---------------------------------------------------------------- from data blocks
int lsmb_build_batch_sst_parts(uint64_t blocks, uint64_t bytes, uint32_t num_bits) {
    return (int)sst_parts(blocks, bytes, num_bits, bbs_bounds());
}

int lsmb_build_batch_sst_dev(lsmb_ctx* c, const void* d_bytes, uint64_t nbytes, uint64_t nblk, const uint64_t* blk_off,
                             const uint32_t* blk_len, uint64_t ntab, const uint64_t* bseg, const uint32_t* num_bits,
                             const uint32_t* num_hashes, void* d_words, uint64_t words_cap, void* d_blk_entries,
                             void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (ntab == 0) return LSMB_OK;
    if (int rc = bbs_check(SstClaim{d_bytes, nbytes, nblk, blk_off, blk_len, ntab, bseg}, num_bits, num_hashes)) return rc;
    if (!d_words) return fail(LSMB_EINVAL, "batched build from blocks: null d_words");
    if (reinterpret_cast<uintptr_t>(d_words) & 15)
        return fail(LSMB_EINVAL, "batched build from blocks: d_words is not 16-byte aligned");
    const BbsWork w = bbs_work(blk_off, blk_len, ntab, bseg, num_bits, num_hashes, 0);
    if (words_cap < w.pl.word_off[ntab])
        return fail(LSMB_EINVAL, "batched build from blocks: words_cap %llu < the layout's %llu words",
                    (unsigned long long)words_cap, (unsigned long long)w.pl.word_off[ntab]);
    DevGuard g(c->dev);
    uint32_t* ent = d_blk_entries ? (uint32_t*)d_blk_entries + bseg[0] : nullptr;
    return bbs_enqueue(c, (const uint8_t*)d_bytes, w, (uint64_t*)d_words, ent, pick_stream(c, stream));
}

int lsmb_build_batch_sst_blocks(lsmb_ctx* c, const uint8_t* bytes, uint64_t nbytes, uint64_t nblk,
                                const uint64_t* blk_off, const uint32_t* blk_len, uint64_t ntab, const uint64_t* bseg,
                                const uint32_t* num_bits, const uint32_t* num_hashes, uint8_t* blooms,
                                uint64_t blooms_cap, uint64_t* bloom_off, uint64_t* entries, int32_t* status) {
    if (!c) return fail(LSMB_EINVAL, "null ctx: the batched build runs on the GPU whatever the block count");
    if (!bloom_off) return fail(LSMB_EINVAL, "batched build from blocks: null bloom_off");
    if (ntab == 0) {
        bloom_off[0] = 0;
        return LSMB_OK;
    }
    const SstClaim cl{bytes, nbytes, nblk, blk_off, blk_len, ntab, bseg};
    if (int rc = bbs_check(cl, num_bits, num_hashes)) return rc;
    bloom_off[0] = 0;
    for (uint64_t t = 0; t < ntab; t++) bloom_off[t + 1] = bloom_off[t] + 12 + 8 * nwords64(num_bits[t]);
    if (!blooms || blooms_cap < bloom_off[ntab])
        return fail(LSMB_EINVAL, "batched build from blocks: blooms buffer %llu B < the %llu B of the batch's blocks",
                    (unsigned long long)(blooms ? blooms_cap : 0), (unsigned long long)bloom_off[ntab]);
    DevGuard g(c->dev);
    // the bytes the claimed blocks span cross once, the blocks renumbered and rebased onto them
    const uint64_t b0 = bseg[0], nb = bseg[ntab] - b0;
    const SstSpan sp = sst_claim_span(cl);
    const BbsWork w = bbs_work(blk_off, blk_len, ntab, bseg, num_bits, num_hashes, sp.lo);
    const uint64_t wbytes = w.pl.word_off[ntab] * 8, obytes = wbytes + nb * 4;  // the words, then the blocks' counts
    if (int rc = stage_claim_span(c, bytes, sp)) return rc;
    HIP_TRY(c->bb_words.ensure(obytes));
    if (int rc = pinned_ensure(c->pinned_retired, &c->bb_host, &c->bb_host_cap, obytes, "batched build")) return rc;
    if (int rc = bbs_enqueue(c, (const uint8_t*)c->keys.p, w, (uint64_t*)c->bb_words.p,
                             (uint32_t*)((uint8_t*)c->bb_words.p + wbytes), c->st))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->bb_host, c->bb_words.p, obytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    const uint32_t* got = (const uint32_t*)(c->bb_host + wbytes);
    int first = LSMB_OK;
    for (uint64_t t = 0; t < ntab; t++) {
        uint8_t* out = blooms + bloom_off[t];
        write_header(out, num_bits[t], num_hashes[t]);
        const uint64_t nw = nwords64(num_bits[t]);
        if (nw) memcpy(out + 12, c->bb_host + w.pl.word_off[t] * 8, nw * 8);
        uint64_t sum = 0;
        int st_t = LSMB_OK;
        for (uint64_t b = bseg[t]; b < bseg[t + 1]; b++) {
            if (got[b - b0] != LSMB_SST_BAD_BLOCK) {
                sum += got[b - b0];
                continue;
            }
            if (st_t == LSMB_OK && first == LSMB_OK)
                first = fail(LSMB_ECORRUPT, "batched build from blocks: table %llu: block %llu is malformed",
                             (unsigned long long)t, (unsigned long long)b);
            st_t = LSMB_ECORRUPT;
        }
        if (entries) entries[t] = sum;
        if (status) status[t] = st_t;
    }
    return first;
}

}  // extern "C"

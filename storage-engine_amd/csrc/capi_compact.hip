// capi_compact.hip — the C ABI of the compaction survivors (lsmb_compact_sst_*,
// include/lsmbloom.h).  Host-side plumbing only; the contract, the plan and the
// work buffer's layout are in sst_compact.hpp, the kernels in compact_sst.hip.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "sst_compact.hpp"

using namespace lsmb;

namespace {

// Before anything is written or any byte is read: sst_check_claim's rules (sst_blocks.hpp).
int cs_check(const SstClaim& cl) {
    return claim_fail(sst_check_claim(cl, [](uint64_t) { return 0; }), cl, "compaction", "sseg", "nsrc", "source", false);
}

int cs_check_work(const CsPlan& pl, const void* d_work, uint64_t work_bytes) {
    if (!d_work) return fail(LSMB_EINVAL, "compaction: null d_work");
    if (reinterpret_cast<uintptr_t>(d_work) % kCsWorkAlign)
        return fail(LSMB_EINVAL, "compaction: d_work is not %llu-byte aligned", (unsigned long long)kCsWorkAlign);
    if (work_bytes < pl.lay.bytes)
        return fail(LSMB_EINVAL, "compaction: work_bytes %llu < the %llu bytes these blocks need (lsmb_compact_sst_work_bytes)",
                    (unsigned long long)work_bytes, (unsigned long long)pl.lay.bytes);
    return LSMB_OK;
}

// Measurement switch of tools/mb_compact_sst.py, read at every call: LSMB_CS_STAGES
// = 1 stops a mark behind its index pass, 2 behind the flags (no scans, no
// totals), so that the passes can be timed by difference.  Anything else: the
// whole mark.
int cs_stages() {
    const char* s = getenv("LSMB_CS_STAGES");
    const int v = s ? atoi(s) : 3;
    return v == 1 || v == 2 ? v : 3;
}

// Both calls stage the block descriptors, then the source bounds (slot_enqueue, ctx.hpp).
int cs_mark(lsmb_ctx* c, const uint8_t* d_bytes, const CsPlan& pl, int drop_tombstones, void* d_work,
            uint32_t* d_blk_entries, void* d_totals, hipStream_t st) {
    SlotPart p[] = {slot_part(pl.blks), slot_part(pl.seg)};
    return slot_enqueue(c, p, 2, st, "compaction", "launch_compact_sst_mark", [&](hipEvent_t done) {
        return launch_compact_sst_mark(d_bytes, (const CsBlk*)p[0].d, (const uint32_t*)p[1].d, (uint32_t)pl.blks.size(),
                                       pl.lay, drop_tombstones, (uint8_t*)d_work, d_blk_entries, (uint64_t*)d_totals, st,
                                       done, cs_stages());
    });
}

int cs_gather(lsmb_ctx* c, const uint8_t* d_bytes, const CsPlan& pl, const void* d_work, void* d_key_data,
              uint64_t data_cap, void* d_key_offsets, uint64_t offs_cap, hipStream_t st) {
    SlotPart p[] = {slot_part(pl.blks), slot_part(pl.seg)};
    return slot_enqueue(c, p, 2, st, "compaction", "launch_compact_sst_gather", [&](hipEvent_t done) {
        return launch_compact_sst_gather(d_bytes, (const CsBlk*)p[0].d, (uint32_t)pl.blks.size(), pl.lay,
                                         (const uint8_t*)d_work, (uint8_t*)d_key_data, data_cap,
                                         (uint64_t*)d_key_offsets, offs_cap, st, done);
    });
}

}  // namespace

extern "C" {

uint64_t lsmb_compact_sst_work_bytes(uint64_t nblk, const uint32_t* blk_len) {
    if (nblk && !blk_len) return 0;
    return cs_work_bytes(nblk, blk_len);
}

int lsmb_compact_sst_mark_dev(lsmb_ctx* c, const void* d_bytes, uint64_t nbytes, uint64_t nblk, const uint64_t* blk_off,
                              const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg, int drop_tombstones,
                              void* d_work, uint64_t work_bytes, void* d_blk_entries, void* d_totals, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (!d_totals) return fail(LSMB_EINVAL, "compaction: null d_totals");
    if (int rc = cs_check(SstClaim{d_bytes, nbytes, nblk, blk_off, blk_len, nsrc, sseg})) return rc;
    const CsPlan pl = cs_plan(blk_off, blk_len, nsrc, sseg, 0);
    if (int rc = cs_check_work(pl, d_work, work_bytes)) return rc;
    DevGuard g(c->dev);
    uint32_t* ent = d_blk_entries ? (uint32_t*)d_blk_entries + sseg[0] : nullptr;
    return cs_mark(c, (const uint8_t*)d_bytes, pl, drop_tombstones, d_work, ent, d_totals, pick_stream(c, stream));
}

int lsmb_compact_sst_gather_dev(lsmb_ctx* c, const void* d_bytes, uint64_t nbytes, uint64_t nblk, const uint64_t* blk_off,
                                const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg, const void* d_work,
                                void* d_key_data, uint64_t data_cap, void* d_key_offsets, uint64_t offs_cap,
                                void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (int rc = cs_check(SstClaim{d_bytes, nbytes, nblk, blk_off, blk_len, nsrc, sseg})) return rc;
    const CsPlan pl = cs_plan(blk_off, blk_len, nsrc, sseg, 0);
    if (int rc = cs_check_work(pl, d_work, pl.lay.bytes)) return rc;  // (its size was the mark's to check)
    if ((data_cap && !d_key_data) || (offs_cap && !d_key_offsets))
        return fail(LSMB_EINVAL, "compaction: null d_key_data or d_key_offsets with a capacity");
    if (reinterpret_cast<uintptr_t>(d_key_offsets) & 7) return fail(LSMB_EINVAL, "compaction: d_key_offsets is not 8-byte aligned");
    DevGuard g(c->dev);
    return cs_gather(c, (const uint8_t*)d_bytes, pl, d_work, d_key_data, data_cap, d_key_offsets, offs_cap,
                     pick_stream(c, stream));
}

int lsmb_compact_sst_bloom(lsmb_ctx* c, const uint8_t* bytes, uint64_t nbytes, uint64_t nblk, const uint64_t* blk_off,
                           const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg, int drop_tombstones,
                           uint64_t expected_items, double fpr, uint8_t* bloom, uint64_t bloom_cap, uint64_t* bloom_len,
                           uint64_t* entry_count, uint32_t* num_bits, uint32_t* num_hashes) {
    if (!c) return fail(LSMB_EINVAL, "null ctx: the compaction's survivors are resolved on the GPU whatever the block count");
    if (!bloom_len) return fail(LSMB_EINVAL, "compaction: null bloom_len");
    uint32_t nb = 0, k = 0;
    if (int rc = lsmb_params(expected_items ? expected_items : 1, fpr, &nb, &k)) return rc;
    const SstClaim cl{bytes, nbytes, nblk, blk_off, blk_len, nsrc, sseg};
    if (int rc = cs_check(cl)) return rc;
    DevGuard g(c->dev);
    // the bytes the claimed blocks span cross once, the blocks rebased onto them
    const uint64_t b0 = sseg[0], B = sseg[nsrc] - b0;
    const SstSpan sp = sst_claim_span(cl);
    const CsPlan pl = cs_plan(blk_off, blk_len, nsrc, sseg, sp.lo);
    // the work buffer, then the totals, then the blocks' counts
    const uint64_t tot_at = (pl.lay.bytes + 15) & ~15ull, ent_at = tot_at + 32, wbytes = ent_at + B * 4;
    if (int rc = stage_claim_span(c, bytes, sp)) return rc;
    HIP_TRY(c->bb_words.ensure(wbytes));
    uint8_t* dw = (uint8_t*)c->bb_words.p;
    if (int rc = cs_mark(c, (const uint8_t*)c->keys.p, pl, drop_tombstones, dw, (uint32_t*)(dw + ent_at), dw + tot_at, c->st))
        return rc;
    uint64_t tot[4];
    HIP_TRY(hipMemcpyAsync(tot, dw + tot_at, sizeof tot, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    if (tot[3]) {
        std::vector<uint32_t> ent(B);
        HIP_TRY(hipMemcpyAsync(ent.data(), dw + ent_at, B * 4, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        const uint64_t i = std::find(ent.begin(), ent.end(), LSMB_SST_BAD_BLOCK) - ent.begin();
        const uint64_t s = std::upper_bound(pl.seg.begin(), pl.seg.end(), (uint32_t)i) - pl.seg.begin() - 1;
        return fail(LSMB_ECORRUPT, "compaction: source %llu: block %llu is malformed or empty (%llu such blocks)",
                    (unsigned long long)s, (unsigned long long)(b0 + i), (unsigned long long)tot[3]);
    }
    const uint64_t surv = tot[0];
    if (!expected_items)
        if (int rc = lsmb_params(std::max<uint64_t>(surv, 1), fpr, &nb, &k)) return rc;
    const uint64_t nw = nwords64(nb);
    *bloom_len = 12 + 8 * nw;
    if (entry_count) *entry_count = surv;
    if (num_bits) *num_bits = nb;
    if (num_hashes) *num_hashes = k;
    if (!bloom || bloom_cap < *bloom_len)
        return fail(LSMB_EINVAL, "compaction: bloom buffer %llu B < the %llu B of the filter's block",
                    (unsigned long long)(bloom ? bloom_cap : 0), (unsigned long long)*bloom_len);
    HIP_TRY(c->out.ensure(tot[1] + 16));
    HIP_TRY(c->offs.ensure((surv + 1) * 8));
    HIP_TRY(c->words.ensure(nw * 8 + 16));
    if (int rc = cs_gather(c, (const uint8_t*)c->keys.p, pl, dw, c->out.p, tot[1], c->offs.p, surv + 1, c->st)) return rc;
    if (int rc = lsmb_build_var_dev_new(c, c->out.p, c->offs.p, surv, nb, k, c->words.p, c->st)) return rc;
    write_header(bloom, nb, k);
    if (nw) HIP_TRY(hipMemcpyAsync(bloom + 12, c->words.p, nw * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

}  // extern "C"

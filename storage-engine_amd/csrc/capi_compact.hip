// capi_compact.hip — the C ABI of the compaction survivors (lsmb_compact_sst_*,
// include/lsmbloom.h).  Host-side plumbing only; the contract, the plan and the
// work buffer's layout are in sst_compact.hpp, the kernels in compact_sst.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "sst_compact.hpp"

using namespace lsmb;

namespace {

// What every lsmb_compact_sst_* call checks of the blocks and the sources before
// anything is written or any of the bytes is read; `bytes` is only compared
// with NULL.
int cs_check(const void* bytes, uint64_t nbytes, uint64_t nblk, const uint64_t* blk_off, const uint32_t* blk_len,
             uint64_t nsrc, const uint64_t* sseg) {
    if (!sseg) return fail(LSMB_EINVAL, "compaction: null sseg");
    if (nblk && (!blk_off || !blk_len)) return fail(LSMB_EINVAL, "compaction: null blk_off or blk_len");
    if (nsrc >= (1ull << 31)) return fail(LSMB_EINVAL, "compaction: more than 2^31-1 sources");
    for (uint64_t s = 0; s < nsrc; s++)
        if (sseg[s + 1] < sseg[s]) return fail(LSMB_EINVAL, "compaction: sseg descends at source %llu", (unsigned long long)s);
    if (sseg[nsrc] > nblk)
        return fail(LSMB_EINVAL, "compaction: sseg[nsrc] = %llu is past the %llu blocks", (unsigned long long)sseg[nsrc],
                    (unsigned long long)nblk);
    if (sseg[nsrc] - sseg[0] >= (1ull << 31)) return fail(LSMB_EINVAL, "compaction: more than 2^31-1 blocks");
    // the device never sees a block that leaves the buffer
    for (uint64_t b = sseg[0]; b < sseg[nsrc]; b++) {
        if (blk_off[b] > nbytes || blk_len[b] > nbytes - blk_off[b])
            return fail(LSMB_EINVAL, "compaction: block %llu (%llu + %u) leaves the %llu bytes", (unsigned long long)b,
                        (unsigned long long)blk_off[b], blk_len[b], (unsigned long long)nbytes);
        if (blk_len[b] && !bytes) return fail(LSMB_EINVAL, "compaction: null bytes");
    }
    return LSMB_OK;
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

// The plan's block descriptors and source bounds through one of the batched
// build's two staging slots to the device and the launches, all on st, under
// that slot's protocol (lsmb_ctx, bb_enqueue_with of capi_build_batch.hip):
// nothing is synchronised but the slot's own reuse.
// launch(d_blks, d_seg, done) -> hipError_t enqueues the kernels.
template <class Launch>
int cs_enqueue(lsmb_ctx* c, const CsPlan& pl, hipStream_t st, const char* what, Launch&& launch) {
    const size_t bbytes = pl.blks.size() * sizeof(CsBlk), sbytes = pl.seg.size() * sizeof(uint32_t);
    const size_t bytes = bbytes + sbytes;  // (CsBlk is 24 B: the bounds behind them stay 4-byte aligned)
    const int s = c->bb_slot;
    c->bb_slot ^= 1;
    if (!c->bb_done[s])
        HIP_TRY(hipEventCreateWithFlags(&c->bb_done[s], hipEventDisableTiming));
    else if (c->bb_stream[s])
        HIP_TRY(hipEventSynchronize(c->bb_done[s]));  // the copy out of this slot, two calls ago
    if (int rc = pinned_ensure(c->pinned_retired, &c->bb_pin[s], &c->bb_pin_cap[s], bytes, "compaction")) return rc;
    HIP_TRY(c->bb_items[s].ensure(bytes));
    if (bbytes) memcpy(c->bb_pin[s], pl.blks.data(), bbytes);
    memcpy(c->bb_pin[s] + bbytes, pl.seg.data(), sbytes);
    if (c->bb_stream[s] && c->bb_stream[s] != st) HIP_TRY(hipStreamWaitEvent(st, c->bb_done[s], 0));
    HIP_TRY(hipMemcpyAsync(c->bb_items[s].p, c->bb_pin[s], bytes, hipMemcpyHostToDevice, st));
    const uint8_t* d = (const uint8_t*)c->bb_items[s].p;
    const hipError_t e = launch((const CsBlk*)d, (const uint32_t*)(d + bbytes), c->bb_done[s]);
    c->bb_stream[s] = st;
    if (e != hipSuccess) {
        (void)hipEventRecord(c->bb_done[s], st);  // (a failed launch may not have completed the event)
        return hip_fail(e, what);
    }
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

int cs_mark(lsmb_ctx* c, const uint8_t* d_bytes, const CsPlan& pl, int drop_tombstones, void* d_work,
            uint32_t* d_blk_entries, void* d_totals, hipStream_t st) {
    return cs_enqueue(c, pl, st, "launch_compact_sst_mark", [&](const CsBlk* d_blks, const uint32_t* d_seg, hipEvent_t done) {
        return launch_compact_sst_mark(d_bytes, d_blks, d_seg, (uint32_t)pl.blks.size(), pl.lay, drop_tombstones,
                                       (uint8_t*)d_work, d_blk_entries, (uint64_t*)d_totals, st, done, cs_stages());
    });
}

int cs_gather(lsmb_ctx* c, const uint8_t* d_bytes, const CsPlan& pl, const void* d_work, void* d_key_data,
              uint64_t data_cap, void* d_key_offsets, uint64_t offs_cap, hipStream_t st) {
    return cs_enqueue(c, pl, st, "launch_compact_sst_gather", [&](const CsBlk* d_blks, const uint32_t*, hipEvent_t done) {
        return launch_compact_sst_gather(d_bytes, d_blks, (uint32_t)pl.blks.size(), pl.lay, (const uint8_t*)d_work,
                                         (uint8_t*)d_key_data, data_cap, (uint64_t*)d_key_offsets, offs_cap, st, done);
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
    if (int rc = cs_check(d_bytes, nbytes, nblk, blk_off, blk_len, nsrc, sseg)) return rc;
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
    if (int rc = cs_check(d_bytes, nbytes, nblk, blk_off, blk_len, nsrc, sseg)) return rc;
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
    if (int rc = cs_check(bytes, nbytes, nblk, blk_off, blk_len, nsrc, sseg)) return rc;
    DevGuard g(c->dev);
    // the bytes the claimed blocks span cross once, the blocks rebased onto them
    const uint64_t b0 = sseg[0], B = sseg[nsrc] - b0;
    uint64_t lo = nbytes, hi = 0;
    for (uint64_t b = b0; b < b0 + B; b++)
        if (blk_len[b]) {
            lo = std::min(lo, blk_off[b]);
            hi = std::max(hi, blk_off[b] + blk_len[b]);
        }
    if (hi < lo) lo = hi = 0;
    const CsPlan pl = cs_plan(blk_off, blk_len, nsrc, sseg, lo);
    // the work buffer, then the totals, then the blocks' counts
    const uint64_t tot_at = (pl.lay.bytes + 15) & ~15ull, ent_at = tot_at + 32, wbytes = ent_at + B * 4;
    HIP_TRY(c->keys.ensure(hi - lo + 16));
    if (hi > lo) HIP_TRY(hipMemcpyAsync(c->keys.p, bytes + lo, hi - lo, hipMemcpyHostToDevice, c->st));
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

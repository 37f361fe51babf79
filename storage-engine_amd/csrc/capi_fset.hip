// capi_fset.hip — the C ABI of the filter set (lsmb_fset_*, include/lsmbloom.h).
// Host-side plumbing only; the kernels are in bloom_probe.hip and fset_lists.hip.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "fset_plan.hpp"

using namespace lsmb;

extern "C" {

// ---------------------------------------------------------------- filter sets
// A device-resident set of up to 64 SSTable filters with their key ranges:
// the multi-get pre-check of DB::get (src/db/mod.rs:243-267 -> SSTable::get,
// src/sstable/reader.rs:192-199), without re-opening and re-deserializing
// every table per lookup (mod.rs:245,259).
struct lsmb_fset {
    lsmb_ctx* c = nullptr;
    struct Slot {
        bool live = false;
        DevBuf words;
        uint32_t num_bits = 0, k = 0;
        std::vector<uint8_t> lo, hi;
    };
    Slot slot[64];
    DevBuf ranges;  // the distinct boundary keys' bytes
    DevBuf points;  // FsetPoint[npts] then regmask[2 * npts + 1]
    DevBuf desc;    // RangedFilter[ndesc]
    FsetRanges rg{};
    FsetClasses cl{};
    uint32_t ndesc = 0;
    uint32_t shared_nb = 0, shared_k = 0;  // (num_bits, k) of every live slot, or 0 when they differ
    bool dirty = true;
    // Uploads go through the set's own non-blocking stream; before a buffer a
    // probe may still read is rewritten, the host waits for the events
    // recorded after this set's probes (one per stream used) — never for the
    // whole device, so another context's builds keep running.
    hipStream_t ust = nullptr;
    std::vector<std::pair<hipStream_t, hipEvent_t>> probe_ev;
    // Lists probes (lsmb_fset_probe_lists*): the mask rows and the per-tile
    // counts are the set's own scratch, shared by every lists probe whatever
    // its stream.  lists_ev (one of probe_ev's events) is completed by the
    // last lists probe's last kernel on lists_stream; a lists probe on
    // another stream waits for it first.
    DevBuf lrows, ltiles;
    DevBuf lstarts, lindex;  // device outputs of the host-memory entry point
    hipStream_t lists_stream = nullptr;
    hipEvent_t lists_ev = nullptr;
};

namespace {

int fset_wait_probes(lsmb_fset* fs) {
    for (auto& pe : fs->probe_ev) HIP_TRY(hipEventSynchronize(pe.second));
    return LSMB_OK;
}

// After a probe on stream st: remember it so later rewrites wait for it.  At
// most kFsetProbeStreams streams are tracked (a caller probing on pooled or
// per-request streams would otherwise grow the list, and every add would wait
// on all of it): a new stream past that takes the least recently used entry,
// whose probe the host waits for first.
constexpr size_t kFsetProbeStreams = 4;

// The event that will mark the completion of the next probe on stream st
// (the set's buffers are rewritten only after every probe that reads them
// is done): one per stream, at most kFsetProbeStreams of them, the least
// recently used evicted after a wait.  The probe's own dispatch completes it
// (launch_done), so repeated probes put no marker packets in the stream.
int fset_probe_event(lsmb_fset* fs, hipStream_t st, hipEvent_t* out) {
    for (size_t i = 0; i < fs->probe_ev.size(); i++)
        if (fs->probe_ev[i].first == st) {
            *out = fs->probe_ev[i].second;
            std::rotate(fs->probe_ev.begin() + i, fs->probe_ev.begin() + i + 1, fs->probe_ev.end());  // most recent last
            return LSMB_OK;
        }
    hipEvent_t ev;
    if (fs->probe_ev.size() < kFsetProbeStreams) {
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    } else {
        ev = fs->probe_ev.front().second;
        HIP_TRY(hipEventSynchronize(ev));
        fs->probe_ev.erase(fs->probe_ev.begin());
    }
    fs->probe_ev.push_back({st, ev});
    *out = ev;
    return LSMB_OK;
}

// Rebuilds the device descriptors after an add/remove (rare; probes re-use
// them): the descriptors, and the sorted boundary points of the live tables'
// key ranges with one in-range mask per region (FsetRanges, kernels.hpp), as
// fset_plan.hpp lays them out.
int fset_refresh(lsmb_fset* fs) {
    if (!fs->dirty) return LSMB_OK;
    std::vector<const lsmb_fset::Slot*> live;
    std::vector<uint32_t> slot_of;
    for (uint32_t s = 0; s < 64; s++)
        if (fs->slot[s].live) {
            live.push_back(&fs->slot[s]);
            slot_of.push_back(s);
        }
    std::vector<FsetPlanTable> tabs;
    for (const auto* S : live)
        tabs.push_back(FsetPlanTable{S->lo.data(), S->lo.size(), S->hi.data(), S->hi.size(), S->num_bits, S->k});
    FsetPlan pl;  // the points, the region masks and the size classes (fset_plan.hpp)
    fset_plan(tabs.data(), (uint32_t)tabs.size(), &pl);
    const uint32_t m = (uint32_t)pl.points.size();
    if (int rc = fset_wait_probes(fs)) return rc;  // no probe may still read the old descriptors
    // grow geometrically from 4 KiB (an outgrown buffer is retired, not freed:
    // DevBuf)
    size_t want = 4096;
    while (want < pl.blob.size()) want *= 2;
    HIP_TRY(fs->ranges.ensure(want));
    if (!pl.blob.empty())
        HIP_TRY(hipMemcpyAsync(fs->ranges.p, pl.blob.data(), pl.blob.size(), hipMemcpyHostToDevice, fs->ust));
    const uint8_t* rb = (const uint8_t*)fs->ranges.p;
    std::vector<uint8_t> pbuf(sizeof(FsetPoint) * kFsetMaxPoints + 8 * (2 * kFsetMaxPoints + 1));
    FsetPoint* fp = (FsetPoint*)pbuf.data();
    for (uint32_t j = 0; j < m; j++) {
        fp[j] = pl.points[j];
        fp[j].p = rb + (uintptr_t)pl.points[j].p;
    }
    memcpy(pbuf.data() + sizeof(FsetPoint) * m, pl.regmask.data(), 8 * pl.regmask.size());
    HIP_TRY(fs->points.ensure(pbuf.size()));
    HIP_TRY(hipMemcpyAsync(fs->points.p, pbuf.data(), sizeof(FsetPoint) * m + 8 * pl.regmask.size(),
                           hipMemcpyHostToDevice, fs->ust));
    fs->rg.pts = (const FsetPoint*)fs->points.p;
    fs->rg.regmask = (const uint64_t*)((const uint8_t*)fs->points.p + sizeof(FsetPoint) * m);
    fs->rg.npts = m;
    std::vector<RangedFilter> d;
    for (uint32_t j = 0; j < live.size(); j++)
        d.push_back(fset_plan_desc((const uint32_t*)live[j]->words.p, live[j]->num_bits, live[j]->k, slot_of[j]));
    HIP_TRY(fs->desc.ensure(sizeof(RangedFilter) * 64));
    if (!d.empty())
        HIP_TRY(hipMemcpyAsync(fs->desc.p, d.data(), sizeof(RangedFilter) * d.size(), hipMemcpyHostToDevice, fs->ust));
    fs->cl = pl.cl;
    HIP_TRY(hipStreamSynchronize(fs->ust));  // pl, pbuf and d are host temporaries
    fs->ndesc = (uint32_t)d.size();
    fs->shared_nb = pl.shared_nb;
    fs->shared_k = pl.shared_k;
    fs->dirty = false;
    return LSMB_OK;
}

// expect_crc (optional): CRC-32 of the whole serialized block (`hdr` = its
// 12-B header), checked against the device copy before the slot goes live.
int fset_add_common(lsmb_fset* fs, const uint8_t* words_le, uint32_t num_bits, uint32_t k, const uint8_t* min_key,
                    uint64_t min_len, const uint8_t* max_key, uint64_t max_len, const uint8_t* hdr = nullptr,
                    const uint32_t* expect_crc = nullptr) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if ((min_len && !min_key) || (max_len && !max_key)) return fail(LSMB_EINVAL, "null key range");
    if (min_len > UINT32_MAX || max_len > UINT32_MAX) return fail(LSMB_EINVAL, "range key too long");
    int s = 0;
    while (s < 64 && fs->slot[s].live) s++;
    if (s == 64) return fail(LSMB_EINVAL, "filter set full (64 filters)");
    DevGuard g(fs->c->dev);
    auto& S = fs->slot[s];
    const uint64_t nw = nwords64(num_bits);
    if (int rc = fset_wait_probes(fs)) return rc;  // the slot's old buffer may still be read by a probe
    HIP_TRY(S.words.ensure(std::max<uint64_t>(nw, 2) * 8));
    if (nw) {
        HIP_TRY(hipMemcpyAsync(S.words.p, words_le, nw * 8, hipMemcpyHostToDevice, fs->ust));
        HIP_TRY(hipStreamSynchronize(fs->ust));
    }
    if (expect_crc) {  // the copy now in HBM, not the host bytes, is what probes will read
        uint32_t got = 0;
        if (int rc = crc32_dev(fs->c, (const uint8_t*)S.words.p, nw * 8, crc32_host(hdr, 12, 0), fs->ust, &got))
            return rc;
        if (got != *expect_crc)
            return fail(LSMB_ECORRUPT, "bloom block CRC-32 mismatch: expected %08x, device copy %08x", *expect_crc, got);
    }
    S.num_bits = num_bits;
    S.k = k;
    S.lo.assign(min_key, min_key + min_len);
    S.hi.assign(max_key, max_key + max_len);
    S.live = true;
    fs->dirty = true;
    return s;
}

}  // namespace

int lsmb_fset_open(lsmb_ctx* c, lsmb_fset** out) {
    if (!c || !out) return fail(LSMB_EINVAL, "null argument");
    *out = nullptr;
    DevGuard g(c->dev);
    lsmb_fset* fs = new lsmb_fset;
    fs->c = c;
    if (hipStreamCreateWithFlags(&fs->ust, hipStreamNonBlocking) != hipSuccess) {
        delete fs;
        return fail(LSMB_EHIP, "filter set: stream creation failed");
    }
    *out = fs;
    return LSMB_OK;
}

void lsmb_fset_close(lsmb_fset* fs) {
    if (!fs) return;
    {
        DevGuard g(fs->c->dev);
        fset_wait_probes(fs);
        for (auto& pe : fs->probe_ev) hipEventDestroy(pe.second);
        if (fs->ust) hipStreamSynchronize(fs->ust), hipStreamDestroy(fs->ust);
        for (auto& S : fs->slot) S.words.release();
        fs->ranges.release();
        fs->points.release();
        fs->desc.release();
        fs->lrows.release();
        fs->ltiles.release();
        fs->lstarts.release();
        fs->lindex.release();
    }
    delete fs;
}

int lsmb_fset_add(lsmb_fset* fs, const uint8_t* block, uint64_t len, const uint8_t* min_key, uint64_t min_len,
                  const uint8_t* max_key, uint64_t max_len) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    uint32_t k, nb, nw;
    if (int rc = lsmb_deserialize_header(block, len, &k, &nb, &nw)) return rc;
    return fset_add_common(fs, block + 12, nb, k, min_key, min_len, max_key, max_len);
}

int lsmb_fset_add_crc(lsmb_fset* fs, const uint8_t* block, uint64_t len, uint32_t crc, const uint8_t* min_key,
                      uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    uint32_t k, nb, nw;
    if (int rc = lsmb_deserialize_header(block, len, &k, &nb, &nw)) return rc;
    return fset_add_common(fs, block + 12, nb, k, min_key, min_len, max_key, max_len, block, &crc);
}

int lsmb_fset_add_words(lsmb_fset* fs, const uint64_t* words, uint32_t num_bits, uint32_t num_hashes,
                        const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    if (!words && nwords64(num_bits)) return fail(LSMB_EINVAL, "null words");
    return fset_add_common(fs, (const uint8_t*)words, num_bits, num_hashes, min_key, min_len, max_key, max_len);
}

int lsmb_fset_remove(lsmb_fset* fs, int slot) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    if (slot < 0 || slot >= 64 || !fs->slot[slot].live) return fail(LSMB_EINVAL, "no filter in slot %d", slot);
    fs->slot[slot].live = false;  // the buffer is re-used by a later add
    fs->dirty = true;
    return LSMB_OK;
}

uint64_t lsmb_fset_live_mask(const lsmb_fset* fs) {
    uint64_t m = 0;
    if (fs)
        for (int s = 0; s < 64; s++)
            if (fs->slot[s].live) m |= 1ull << s;
    return m;
}

int lsmb_fset_probe_dev_rows(lsmb_fset* fs, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                             void* d_out, uint32_t row_bytes, void* stream) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    if (row_bytes != 1 && row_bytes != 2 && row_bytes != 4 && row_bytes != 8)
        return fail(LSMB_EINVAL, "row_bytes must be 1, 2, 4 or 8");
    const uint64_t live = lsmb_fset_live_mask(fs);
    if (row_bytes < 8 && (live >> (8 * row_bytes)) != 0)
        return fail(LSMB_EINVAL, "a live slot does not fit %u-byte rows", row_bytes);
    if (n == 0) return LSMB_OK;
    if (!d_out || !d_data) return fail(LSMB_EINVAL, "null keys or output");
    DevGuard g(fs->c->dev);
    if (int rc = fset_refresh(fs)) return rc;
    const hipStream_t st = pick_stream(fs->c, stream);
    if (fs->ndesc == 0) {
        HIP_TRY(hipMemsetAsync(d_out, 0, n * row_bytes, st));
        return LSMB_OK;
    }
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    hipEvent_t ev;
    if (int rc = fset_probe_event(fs, st, &ev)) return rc;
    HIP_TRY(launch_fset_probe(kb, (const RangedFilter*)fs->desc.p, fs->ndesc, fs->rg, fs->cl, fs->shared_nb, fs->shared_k,
                              (uint8_t*)d_out, row_bytes, fs->c->num_cus, st, ev));
    return LSMB_OK;
}

int lsmb_fset_probe_dev(lsmb_fset* fs, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                        void* d_out, void* stream) {
    return lsmb_fset_probe_dev_rows(fs, d_data, d_offsets, key_len, n, d_out, 8, stream);
}

int lsmb_fset_probe(lsmb_fset* fs, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                    uint64_t* out_mask) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    if (n == 0) return LSMB_OK;
    if (!out_mask || host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "null keys or output");
    lsmb_ctx* c = fs->c;
    DevGuard g(c->dev);
    if (int rc = fset_refresh(fs)) return rc;
    HIP_TRY(c->out.ensure(n * 8));
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    if (fs->ndesc == 0) {
        memset(out_mask, 0, n * 8);
        return LSMB_OK;
    }
    hipEvent_t ev;
    if (int rc = fset_probe_event(fs, c->st, &ev)) return rc;
    HIP_TRY(launch_fset_probe(kb, (const RangedFilter*)fs->desc.p, fs->ndesc, fs->rg, fs->cl, fs->shared_nb, fs->shared_k,
                              (uint8_t*)c->out.p, 8, c->num_cus, c->st, ev));
    HIP_TRY(hipMemcpyAsync(out_mask, c->out.p, n * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

// The lists probe on `st` over device keys: the mask probe into the set's row
// scratch (the narrowest rows that hold every live slot), then the three
// compaction kernels (fset_lists.hip).  kb.n >= 1.
static int fset_lists_dev(lsmb_fset* fs, const KeyBatch& kb, uint64_t* d_starts, uint32_t* d_index, uint64_t cap,
                          hipStream_t st) {
    if (int rc = fset_refresh(fs)) return rc;
    if (fs->ndesc == 0) {
        HIP_TRY(hipMemsetAsync(d_starts, 0, 65 * 8, st));
        return LSMB_OK;
    }
    const uint64_t live = lsmb_fset_live_mask(fs);
    const uint32_t rb = (live >> 8) == 0 ? 1 : (live >> 16) == 0 ? 2 : (live >> 32) == 0 ? 4 : 8;
    hipEvent_t ev;
    if (int rc = fset_probe_event(fs, st, &ev)) return rc;
    // the scratch is the previous lists probe's too: in order on its stream,
    // after its last kernel on any other
    if (fs->lists_ev && fs->lists_stream != st) HIP_TRY(hipStreamWaitEvent(st, fs->lists_ev, 0));
    HIP_TRY(fs->lrows.ensure(kb.n * rb));
    HIP_TRY(fs->ltiles.ensure(fset_lists_tile_bytes(kb.n, live)));
    fs->lists_stream = st;
    fs->lists_ev = ev;
    hipError_t e = launch_fset_probe(kb, (const RangedFilter*)fs->desc.p, fs->ndesc, fs->rg, fs->cl, fs->shared_nb,
                                     fs->shared_k, (uint8_t*)fs->lrows.p, rb, fs->c->num_cus, st);
    if (e == hipSuccess)
        e = launch_fset_lists((const uint8_t*)fs->lrows.p, rb, kb.n, live, (uint32_t*)fs->ltiles.p, d_starts, d_index,
                              cap, st, ev);  // (its last dispatch completes the guard event)
    if (e != hipSuccess) {
        (void)hipEventRecord(ev, st);  // whatever was launched still reads the set's buffers
        return hip_fail(e, "filter set lists probe");
    }
    return LSMB_OK;
}

int lsmb_fset_probe_lists_dev(lsmb_fset* fs, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                              void* d_starts, void* d_index, uint64_t cap, void* stream) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    if (n > UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-1 keys (the lists hold 32-bit indices)");
    if (!d_starts || (cap && !d_index)) return fail(LSMB_EINVAL, "null output");
    if (n && !d_data) return fail(LSMB_EINVAL, "null keys");
    DevGuard g(fs->c->dev);
    const hipStream_t st = pick_stream(fs->c, stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_starts, 0, 65 * 8, st));
        return LSMB_OK;
    }
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    return fset_lists_dev(fs, kb, (uint64_t*)d_starts, (uint32_t*)d_index, cap, st);
}

int lsmb_fset_probe_lists(lsmb_fset* fs, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                          uint64_t* starts, uint32_t* index, uint64_t cap) {
    if (!fs) return fail(LSMB_EINVAL, "null filter set");
    if (n > UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-1 keys (the lists hold 32-bit indices)");
    if (!starts || (cap && !index)) return fail(LSMB_EINVAL, "null output");
    if (n && host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "null keys");
    memset(starts, 0, 65 * 8);
    if (n == 0 || lsmb_fset_live_mask(fs) == 0) return LSMB_OK;
    lsmb_ctx* c = fs->c;
    DevGuard g(c->dev);
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    // no list is longer than the live slots' n entries each
    const uint64_t dcap = std::min<uint64_t>(cap, n * 64);
    HIP_TRY(fs->lstarts.ensure(65 * 8));
    HIP_TRY(fs->lindex.ensure(std::max<uint64_t>(dcap, 1) * 4));
    if (int rc = fset_lists_dev(fs, kb, (uint64_t*)fs->lstarts.p, (uint32_t*)fs->lindex.p, dcap, c->st)) return rc;
    return lists_to_host(starts, (const uint64_t*)fs->lstarts.p, 64, index, (const uint32_t*)fs->lindex.p, dcap, c->st);
}

}  // extern "C"

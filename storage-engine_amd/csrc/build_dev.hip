// build_dev.hip — orchestration of the device build on one context: strategy
// choice, the shared workspace (sized by build_plan.hip's workspace_bytes and
// bounded by LSMB_WORKSPACE_MB through key chunks), and the host-memory builds
// that stage keys through the context's slots.  Declared in ctx.hpp.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "ctx.hpp"
#include "keysrc.hpp"

namespace lsmb {

namespace {
uint64_t workspace_limit_bytes() {
    const char* s = getenv("LSMB_WORKSPACE_MB");
    uint64_t mb = s ? strtoull(s, nullptr, 10) : 8192;
    if (mb < 16) mb = 16;
    return mb << 20;
}

// Grows the context's workspace buffers to `need` and hands them out.  The
// overflow words and marks are all-zero between builds: each is zeroed right
// after it is (re)allocated, before the next allocation can fail, so a grown
// buffer never stays unzeroed.
int take_workspace(lsmb_ctx* c, const WorkspaceBytes& need, hipStream_t st, PartitionWorkspace* ws) {
    const size_t ob = c->ws_ovf.bytes, db = c->ws_dirty.bytes;
    HIP_TRY(c->ws_regions.ensure(need.regions));
    HIP_TRY(c->ws_counts.ensure(need.counts));
    HIP_TRY(c->ws_ovf.ensure(need.ovf));
    if (c->ws_ovf.bytes != ob) HIP_TRY(hipMemsetAsync(c->ws_ovf.p, 0, c->ws_ovf.bytes, st));
    HIP_TRY(c->ws_dirty.ensure(need.dirty));
    if (c->ws_dirty.bytes != db) HIP_TRY(hipMemsetAsync(c->ws_dirty.p, 0, c->ws_dirty.bytes, st));
    HIP_TRY(c->ws_ovl.ensure(need.ovl));
    HIP_TRY(c->ws_ovn.ensure(need.ovn));
    HIP_TRY(c->ws_hashes.ensure(need.hashes));
    // (a buffer the build does not need is not handed out: its pointer stays null)
    auto hand = [](DevBuf& b, uint64_t want, auto*& p, uint64_t& have) {
        if (!want) return;
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(b.p);
        have = b.bytes;
    };
    hand(c->ws_regions, need.regions, ws->regions, ws->have.regions);
    hand(c->ws_counts, need.counts, ws->counts, ws->have.counts);
    hand(c->ws_ovf, need.ovf, ws->ovf, ws->have.ovf);
    hand(c->ws_dirty, need.dirty, ws->dirty, ws->have.dirty);
    hand(c->ws_ovl, need.ovl, ws->ovl, ws->have.ovl);
    hand(c->ws_ovn, need.ovn, ws->ovn, ws->have.ovn);
    hand(c->ws_hashes, need.hashes, ws->hashes, ws->have.hashes);
    ws->err = (uint32_t*)c->err.p;
    return LSMB_OK;
}

int build_dev_ws(lsmb_ctx* c, const KeyBatch& kb_all, uint32_t num_bits, uint32_t k, uint32_t* dw, hipStream_t st,
                 BuildStrategy s, int sweep, bool fresh, hipEvent_t done = nullptr) {
    BuildTimers* tm = c->timing ? &c->tm : nullptr;
    const bool aligned16 = ks::is_fixed16(kb_all);
    PartitionWorkspace ws;
    if (s != BuildStrategy::Partition) {  // one launch: Lds and Atomic builds take no workspace
        WorkspaceBytes need =
            workspace_bytes(s, PartitionPlan{}, plan_tiled(num_bits, kb_all.n, c->num_cus), num_bits, k, kb_all.n, aligned16, fresh);
        if (getenv("LSMB_TILED_NO_PREHASH")) need.hashes = 0;  // measurement switch
        if (int rc = take_workspace(c, need, st, &ws)) return rc;
        HIP_TRY(launch_build(kb_all, num_bits, k, dw, s, ws, c->num_cus, st, tm, sweep, fresh, done));
        return LSMB_OK;
    }
    uint64_t chunk = partition_chunk_keys(num_bits, k, workspace_limit_bytes(), c->num_cus);
    if (chunk == 0) return fail(LSMB_ENOMEM, "partition workspace limit too small");
    chunk = std::min(chunk, kb_all.n);
    // sized by the first (largest, and only fresh) chunk; every chunk is planned for its own size
    const PartitionPlan pl = plan_partition(num_bits, k, chunk, c->num_cus);
    const WorkspaceBytes need = workspace_bytes(s, pl, TiledPlan{}, num_bits, k, chunk, aligned16, fresh);
    if (int rc = take_workspace(c, need, st, &ws)) return rc;
    for (uint64_t first = 0; first < kb_all.n; first += chunk) {
        KeyBatch kb = kb_all;
        kb.n = std::min(chunk, kb_all.n - first);
        if (kb.offsets)
            kb.offsets += first;  // VarLen offsets are absolute into data
        else
            kb.data += first * kb.key_len;
        // fresh: the first chunk writes every word of the range, the rest accumulate
        HIP_TRY(launch_build(kb, num_bits, k, dw, s, ws, c->num_cus, st, tm, sweep, fresh && first == 0,
                             done));  // (each chunk's last kernel re-arms `done`)
    }
    return LSMB_OK;
}
}  // namespace

// Device build of one batch, chunked so the partition workspace stays bounded.
int build_dev(lsmb_ctx* c, const KeyBatch& kb_all, uint32_t num_bits, uint32_t k, uint32_t* dw,
              hipStream_t st, int sweep, bool fresh) {
    BuildStrategy s = pick_build_strategy(num_bits, k, kb_all.n);
    // LSMB_FORCE_STRATEGY=atomic: measurement override;
    // the filter is the same either way.
    if (const char* f = getenv("LSMB_FORCE_STRATEGY"))
        if ((s == BuildStrategy::Partition || s == BuildStrategy::Tiled) && !strcmp(f, "atomic")) s = BuildStrategy::Atomic;
    c->tm.valid = false;
    if (s == BuildStrategy::None) {  // fresh: new() with no inserts, all-zero words
        if (fresh && num_bits) HIP_TRY(hipMemsetAsync(dw, 0, nwords64(num_bits) * 8, st));
        return LSMB_OK;
    }
    if (s != BuildStrategy::Tiled && s != BuildStrategy::Partition)
        return build_dev_ws(c, kb_all, num_bits, k, dw, st, s, sweep, fresh);
    // Tiled and partition builds use the context's shared workspace: a build
    // issued on a different stream than the last one waits for it (two
    // streams' builds would otherwise overwrite each other's regions).  On the
    // same stream, stream order already serialises them: no wait packet (a
    // barrier packet between consecutive builds costs the stream ~10 us).
    // ws_done is completed by the build's last kernel itself (launch_done): a
    // separate event record would put a marker packet, ~6 us, between
    // back-to-back builds.
    if (c->ws_stream && c->ws_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->ws_done, 0));
    const int rc = build_dev_ws(c, kb_all, num_bits, k, dw, st, s, sweep, fresh, c->ws_done);
    if (rc != LSMB_OK) HIP_TRY(hipEventRecord(c->ws_done, st));  // (a failed build may have launched nothing)
    c->ws_stream = st;
    return rc;
}

static uint64_t h2d_chunk_bytes() {
    const char* s = getenv("LSMB_H2D_CHUNK_MB");
    uint64_t mb = s ? strtoull(s, nullptr, 10) : 128;
    if (mb < 1) mb = 1;
    return mb << 20;
}

// Build from keys in host memory (the flush / compaction path: keys come from a
// memtable or merge iterator, src/db/mod.rs:379-383).  The keys go up in chunks
// of <= h2d_chunk_bytes() through two device staging slots: chunk i+1's H2D on
// the copy stream overlaps chunk i's kernels on the build stream, so the build
// hides under the PCIe transfer.  words_in == NULL starts from a zeroed filter
// (BloomFilter::new), else from those words (OR-accumulate); the finished words
// are copied to words_out (host, any alignment: lsmb_build_block points it at
// the serialized block body).  Synchronous.
// Small host builds (an SST flush of a few thousand keys): one pinned staging
// buffer, plain memcpys into and out of it and true async DMA on the build
// stream — pageable copies would each stage synchronously — and no copy
// stream.  Latency, not bandwidth, is what these calls pay.
constexpr uint64_t kSmallHostBuild = 1ull << 20;  // bytes of keys + offsets + words

static int host_build_small(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                     uint32_t num_bits, uint32_t k, const uint64_t* words_in, uint8_t* words_out) {
    const uint64_t nw = nwords64(num_bits);
    const uint64_t base = offsets ? offsets[0] : 0;
    const uint64_t kbytes = offsets ? offsets[n] - base : n * (uint64_t)key_len;
    const uint64_t obytes = offsets ? (n + 1) * 8 : 0;
    const uint64_t kpad = (kbytes + 15) & ~15ull, opad = (obytes + 15) & ~15ull;
    const uint64_t need = kpad + opad + nw * 8 + 64;
    if (c->pin_small_cap < need) {
        c->pinned_retired.retire(c->pin_small);  // a D2H of an earlier call may not have left it
        c->pin_small = nullptr;
        c->pin_small_cap = 0;
        const uint64_t cap = std::max<uint64_t>(need, kSmallHostBuild + 64);
        if (hipHostMalloc((void**)&c->pin_small, cap, 0) != hipSuccess)
            return fail(LSMB_ENOMEM, "pinned staging (%llu B)", (unsigned long long)cap);
        c->pin_small_cap = cap;
    }
    uint8_t* pk = c->pin_small;
    uint64_t* po = (uint64_t*)(c->pin_small + kpad);
    uint64_t* pw = (uint64_t*)(c->pin_small + kpad + opad);
    HIP_TRY(c->words.ensure(nw * 8));
    HIP_TRY(c->kslot[0].ensure(kpad + 16));
    uint32_t* dw = (uint32_t*)c->words.p;
    // the previous small build's D2H out of this buffer has completed (synchronous calls)
    if (kbytes) memcpy(pk, data + base, kbytes);
    if (kbytes) HIP_TRY(hipMemcpyAsync(c->kslot[0].p, pk, kbytes, hipMemcpyHostToDevice, c->st));
    if (offsets) {
        for (uint64_t j = 0; j <= n; j++) po[j] = offsets[j] - base;
        HIP_TRY(c->oslot[0].ensure(obytes));
        HIP_TRY(hipMemcpyAsync(c->oslot[0].p, po, obytes, hipMemcpyHostToDevice, c->st));
    }
    if (words_in) {
        memcpy(pw, words_in, nw * 8);
        HIP_TRY(hipMemcpyAsync(dw, pw, nw * 8, hipMemcpyHostToDevice, c->st));
    } else {
        HIP_TRY(hipMemsetAsync(dw, 0, nw * 8, c->st));
    }
    KeyBatch kb{(const uint8_t*)c->kslot[0].p, offsets ? (const uint64_t*)c->oslot[0].p : nullptr, key_len,
                (!offsets && key_len == 0) ? 1 : n};
    if (int rc = build_dev(c, kb, num_bits, k, dw, c->st)) return rc;
    HIP_TRY(hipMemcpyAsync(pw, dw, nw * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    memcpy(words_out, pw, nw * 8);
    return LSMB_OK;
}

int host_build_dev(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                   uint32_t num_bits, uint32_t k, uint32_t* dw) {
    if (!offsets && key_len == 0) {
        // every key is the empty key: one insert covers them all
        HIP_TRY(c->kslot[0].ensure(16));
        KeyBatch kb{(const uint8_t*)c->kslot[0].p, nullptr, 0, 1};
        if (int rc = build_dev(c, kb, num_bits, k, dw, c->st)) return rc;
        n = 0;
    }
    const uint64_t budget = h2d_chunk_bytes();
    const uint64_t max_keys = 32ull << 20;  // per chunk (bounds the offsets slot)
    uint64_t f = 0;
    for (int i = 0; f < n; i++) {
        const int s = i & 1;
        uint64_t e;
        if (offsets) {  // largest e with offsets[e] - offsets[f] <= budget, at least one key
            const uint64_t* hi = std::upper_bound(offsets + f + 1, offsets + n + 1, offsets[f] + budget);
            e = std::max<uint64_t>(f + 1, (uint64_t)(hi - offsets) - 1);
            e = std::min(e, f + max_keys);
        } else {
            e = std::min(n, f + std::max<uint64_t>(1, budget / key_len));
        }
        const uint64_t m = e - f;
        const uint64_t base = offsets ? offsets[f] : f * key_len;
        const uint64_t bytes = offsets ? offsets[e] - offsets[f] : m * key_len;
        // slot s was last read by chunk i-2's kernels
        if (i >= 2) HIP_TRY(hipEventSynchronize(c->ev_built[s]));
        HIP_TRY(c->kslot[s].ensure(std::max<uint64_t>(bytes, std::min(budget, n * (uint64_t)(key_len ? key_len : 1))) + 16));
        if (bytes) HIP_TRY(hipMemcpyAsync(c->kslot[s].p, data + base, bytes, hipMemcpyHostToDevice, c->cst));
        if (offsets) {
            if (c->offs_pin_cap[s] < m + 1) {
                c->pinned_retired.retire(c->offs_pin[s]);
                c->offs_pin[s] = nullptr;
                c->offs_pin_cap[s] = 0;
                const uint64_t cap = std::max<uint64_t>(m + 1, std::min<uint64_t>(n, max_keys) + 1);
                if (hipHostMalloc((void**)&c->offs_pin[s], cap * 8, 0) != hipSuccess)
                    return fail(LSMB_ENOMEM, "pinned offsets staging (%llu B)", (unsigned long long)(cap * 8));
                c->offs_pin_cap[s] = cap;
            }
            uint64_t* o = c->offs_pin[s];
            for (uint64_t j = 0; j <= m; j++) o[j] = offsets[f + j] - base;
            HIP_TRY(c->oslot[s].ensure(c->offs_pin_cap[s] * 8));
            HIP_TRY(hipMemcpyAsync(c->oslot[s].p, o, (m + 1) * 8, hipMemcpyHostToDevice, c->cst));
        }
        HIP_TRY(hipEventRecord(c->ev_copy[s], c->cst));
        HIP_TRY(hipStreamWaitEvent(c->st, c->ev_copy[s], 0));
        KeyBatch kb{(const uint8_t*)c->kslot[s].p, offsets ? (const uint64_t*)c->oslot[s].p : nullptr, key_len, m};
        if (int rc = build_dev(c, kb, num_bits, k, dw, c->st)) return rc;
        HIP_TRY(hipEventRecord(c->ev_built[s], c->st));
        f = e;
    }
    return LSMB_OK;
}

// crc (optional): CRC-32 of the words appended to *crc (the CRC of the bytes
// before them), computed on the device copy for device builds.
int host_build(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
               uint32_t num_bits, uint32_t k, const uint64_t* words_in, uint8_t* words_out, uint32_t* crc) {
    const uint64_t nw = nwords64(num_bits);
    {
        const uint64_t kb = offsets ? offsets[n] - offsets[0] : n * (uint64_t)key_len;
        if (kb + (offsets ? (n + 1) * 8 : 0) + nw * 8 <= kSmallHostBuild) {
            const int rc = host_build_small(c, data, offsets, key_len, n, num_bits, k, words_in, words_out);
            if (!rc && crc) *crc = crc32_host(words_out, nw * 8, *crc);
            return rc;
        }
    }
    HIP_TRY(c->words.ensure(nw * 8));
    uint32_t* dw = (uint32_t*)c->words.p;
    if (words_in)
        HIP_TRY(hipMemcpyAsync(dw, words_in, nw * 8, hipMemcpyHostToDevice, c->st));
    else
        HIP_TRY(hipMemsetAsync(dw, 0, nw * 8, c->st));
    if (int rc = host_build_dev(c, data, offsets, key_len, n, num_bits, k, dw)) return rc;
    HIP_TRY(hipMemcpyAsync(words_out, dw, nw * 8, hipMemcpyDeviceToHost, c->st));
    if (crc) {
        if (int rc = crc32_dev(c, (const uint8_t*)dw, nw * 8, *crc, c->st, crc)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

}  // namespace lsmb

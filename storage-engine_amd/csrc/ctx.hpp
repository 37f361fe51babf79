// ctx.hpp — the per-GPU context behind lsmb_ctx and the host plumbing shared by
// capi.hip and capi_*.hip (the C ABI, one file per handle), build_dev.hip (build
// orchestration), stream.hip and multi.hip (one process, several GPUs).  Helpers
// that cross those files are declared here and defined once, in capi.hip: the
// error returns, the argument checks, the staging of host keys
// (stage_host_keys), the copy-back of a lists probe (lists_to_host), the builds
// and the CRCs.
// Internal.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/lsmbloom.h"
#include "growbuf.hpp"
#include "kernels.hpp"
#include "sst_blocks.hpp"

namespace lsmb {

// A grow-only device buffer: GrowBuf's policy (growbuf.hpp) over hipMalloc.
// Outgrown buffers are retired, not freed, and freed by release() at teardown
// (lsmb_close and the handles' close functions, after their streams are
// synchronised); out of memory, the retired and then the live buffer are freed
// before the last try.
struct HipAlloc {
    hipError_t last = hipSuccess;
    void* alloc(size_t n) {
        void* q = nullptr;
        last = hipMalloc(&q, n);
        if (last != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return q;
    }
    void free(void* q) { (void)hipFree(q); }  // teardown / out-of-memory only
};
struct DevBuf : GrowBuf<HipAlloc> {
    hipError_t ensure(size_t want) {
        if (GrowBuf<HipAlloc>::ensure(want)) return hipSuccess;
        return al.last != hipSuccess ? al.last : hipErrorOutOfMemory;
    }
};

// Pinned host staging with the same policy (hipHostFree waits for the device
// too): outgrown blocks are retired and freed at teardown.
struct PinnedPool {
    std::vector<void*> retired;
    void retire(void* p) {
        if (p) retired.push_back(p);
    }
    void release() {
        for (void* r : retired) (void)hipHostFree(r);  // teardown
        retired.clear();
    }
};

struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev) {
        hipGetDevice(&prev);
        if (prev != dev) hipSetDevice(dev);
    }
    ~DevGuard() {
        int cur = -1;
        hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) hipSetDevice(prev);
    }
};

// Thread-local error message (lsmb_last_error) and the error returns.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char* what);
const std::string& last_error();
void set_last_error(const std::string& s);

#define HIP_TRY(expr)                                           \
    do {                                                        \
        hipError_t e_ = (expr);                                 \
        if (e_ != hipSuccess) return ::lsmb::hip_fail(e_, #expr); \
    } while (0)

// A grow-only pinned block (*p, *cap) over a PinnedPool: growth of at least
// 1.5x, the outgrown block retired to the pool (freed at its owner's teardown),
// never freed here.  `who` words the LSMB_ENOMEM message.
inline int pinned_ensure(PinnedPool& pool, uint8_t** p, uint64_t* cap, uint64_t need, const char* who) {
    if (need <= *cap) return LSMB_OK;
    const uint64_t want = std::max<uint64_t>(need, *cap + *cap / 2);
    void* q = nullptr;
    if (hipHostMalloc(&q, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LSMB_ENOMEM, "%s: %llu bytes of pinned staging", who, (unsigned long long)want);
    }
    pool.retire(*p);
    *p = (uint8_t*)q;
    *cap = want;
    return LSMB_OK;
}

// The two staging slots of slot_enqueue (below).
struct StagingSlots {
    uint8_t* pin[2] = {};
    uint64_t pin_cap[2] = {};
    DevBuf dev[2];
    hipEvent_t done[2] = {};     // completed by the last launch of the slot's last call
    hipStream_t stream[2] = {};  // stream of the slot's last call (nullptr: none yet)
    int next = 0;                // alternates by call, whatever the route
    void release() {
        for (int s = 0; s < 2; s++) {
            dev[s].release();
            if (pin[s]) (void)hipHostFree(pin[s]);  // teardown
            if (done[s]) (void)hipEventDestroy(done[s]);
        }
    }
};

inline uint64_t nwords64(uint32_t num_bits) { return ((uint64_t)num_bits + 63) / 64; }

// The 12-byte header of BloomFilter::serialize (src/bloom/mod.rs:102-115).
void write_header(uint8_t* out, uint32_t num_bits, uint32_t k);

// offsets[0..n] must be non-decreasing (key i = data[offsets[i] .. offsets[i+1]).
int check_offsets(const uint64_t* offsets, uint64_t n);

// Reference arguments that would panic (% by zero in get_position, mod.rs:195).
int check_filter(uint32_t num_bits, uint32_t k);

// Builds of at most this many keys run the library's host loop (the
// reference's own per-key insert, src/bloom/mod.rs:70-78) instead of a device
// round trip; see lsmb_host_max_keys().
uint64_t host_max_keys();
void set_host_max_keys(uint64_t n);
constexpr uint64_t kDefaultHostMaxKeys = 2048;  // SST-sized flush latency

}  // namespace lsmb

// Calls on different streams.  Every device entry point takes the caller's
// stream, and three groups of device buffers below are shared by all calls on
// the context.  Each group has one event that the last user's final kernel
// completes itself (launch_done: no marker packet), and the stream of that
// user; a call on the same stream relies on stream order alone:
//  - build workspace (ws_*): ws_done / ws_stream.  A tiled or partition build
//    on another stream than the last one's waits for ws_done on its stream
//    before anything of it runs (build_dev, build_dev.hip).  Builds are
//    thereby serialised in call order; Lds and Atomic builds take no
//    workspace and are not ordered.
//  - probe descriptors (filt_desc, desc_pinned): desc_done / desc_stream.  A
//    generic probe with new descriptors waits for desc_done on the host
//    before it refills the staging and uploads; one with the uploaded
//    descriptors on another stream waits for it on that stream
//    (probe_common, capi.hip).  Generic probes are thereby one chain in call
//    order; bit-sliced probes read no descriptors and are not ordered.
//  - staged work lists (slots.dev[s], slots.pin[s]): slots.done[s] /
//    slots.stream[s], per slot, the two slots alternating by call and shared
//    by the batched builds and the compaction calls.  The rules are stated
//    once, at slot_enqueue (below; capi.hip).
// The host-side state itself is not locked: calls on one context come from
// one thread at a time.
struct lsmb_ctx {
    int dev = 0;
    int num_cus = 256;
    hipStream_t st = nullptr;
    lsmb::BuildTimers tm;
    lsmb::DevBuf ws_regions, ws_counts;  // partition / tiled workspace
    lsmb::DevBuf crc_parts;              // CRC-32 workgroup partials (crc32.hip)
    lsmb::DevBuf ws_hashes;              // k_hash records (var-len / odd-length keys)
    lsmb::DevBuf err;                    // LSMB_STATS builds: pass A's overflow counters
    lsmb::DevBuf ws_ovf, ws_dirty;       // partition: overflow words + unit marks (all-zero between builds)
    lsmb::DevBuf ws_ovl, ws_ovn;         // fresh partition builds: overflow position lists + lengths
    // The workspace above is shared by every build on this context, whatever
    // stream it is issued on: ws_done marks the last build that used it, and a
    // build on another stream waits for it first (build_dev).
    hipEvent_t ws_done = nullptr;
    hipStream_t ws_stream = nullptr;     // stream of the last workspace user (nullptr: none yet)
    lsmb::DevBuf keys, offs, words, out; // staging for the host-memory entry points
    lsmb::DevBuf filt_words;             // probe: device copies of host filters
    lsmb::DevBuf filt_desc;              // probe: ProbeFilter array
    std::vector<lsmb::ProbeFilter> hfilt;
    std::vector<lsmb::ProbeFilter> desc_uploaded;  // what filt_desc currently holds
    lsmb::ProbeFilter* desc_pinned = nullptr;      // pinned staging for descriptor uploads
    hipEvent_t desc_done = nullptr;                // last kernel that read filt_desc
    hipStream_t desc_stream = nullptr;             // stream of the last generic probe (nullptr: none yet)
    std::vector<uint64_t> offs_tmp;
    bool timing = true;                  // per-build HIP events (lsmb_set_timing)
    // host-memory builds: two staging slots, H2D on `cst` overlapping the
    // kernels of the previous chunk on `st` (host_build_dev)
    hipStream_t cst = nullptr;
    hipEvent_t ev_copy[2] = {nullptr, nullptr}, ev_built[2] = {nullptr, nullptr};
    lsmb::DevBuf kslot[2], oslot[2];
    uint64_t* offs_pin[2] = {nullptr, nullptr};  // pinned rebased offsets per slot
    uint64_t offs_pin_cap[2] = {0, 0};
    uint8_t* pin_small = nullptr;  // pinned staging of small host builds (host_build_small)
    uint64_t pin_small_cap = 0;
    lsmb::PinnedPool pinned_retired;  // outgrown pinned staging, freed by lsmb_close
    lsmb::StagingSlots slots;  // work lists of lsmb_build_batch_* and lsmb_compact_sst_* (slot_enqueue)
    // lsmb_build_batch_blocks: the packed words on the device and, pinned, back on the host
    lsmb::DevBuf bb_words;
    uint8_t* bb_host = nullptr;
    uint64_t bb_host_cap = 0;
};

namespace lsmb {

// `stream` of an entry point, NULL = the context's own build stream.
hipStream_t pick_stream(lsmb_ctx* c, void* stream);

// Copies a host key batch into the context's staging buffers (ctx stream).
int stage_host_keys(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                    KeyBatch* kb);
// A host key batch of n >= 1 keys that has bytes to read and no pointer to them.
inline bool host_keys_null(const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n) {
    return !data && (offsets ? offsets[n] > offsets[0] : key_len > 0);
}

// The staging-slot protocol.  slot_enqueue takes the next slot, waits on the
// host for the slot's event (its last call, two calls ago), lays the host parts
// into the pinned block, each on a 16-byte boundary (parts of whole 16 bytes lie
// back to back), makes st wait for the event if the slot's last call was on
// another stream, uploads the block on st and sets each part's device address.
// launch(done) -> hipError_t then enqueues the kernels on st, the last of them
// completing `done` itself; st becomes the slot's stream, and a failed launch
// has the event recorded by hand and fails with `what`.  `who`: of LSMB_ENOMEM.
constexpr size_t kSlotAlign = 16;
struct SlotPart {
    const void* p;
    size_t bytes;
    const uint8_t* d;  // out: where the part lies on the device
};
template <class T>
SlotPart slot_part(const std::vector<T>& v) { return SlotPart{v.data(), v.size() * sizeof(T), nullptr}; }
int slot_enqueue(lsmb_ctx* c, SlotPart* parts, int nparts, hipStream_t st, const char* who, const char* what,
                 const std::function<hipError_t(hipEvent_t done)>& launch);

// A block claim that sst_check_claim refused as the call's error, in the route's
// words ("compaction", "sseg", "nsrc", "source"; in_block: "table T: " before
// "block B"); a claim's span from host memory into c->keys, on c->st.
int claim_fail(const SstClaimFault& f, const SstClaim& cl, const char* who, const char* seg, const char* count,
               const char* group, bool in_block);
int stage_claim_span(lsmb_ctx* c, const uint8_t* bytes, SstSpan sp);

// The copy-back of every host lists probe (lsmb_fset_probe_lists,
// lsmb_lset_probe_lists, lsmb_lset_probe_version_lists), in two steps on st:
// the last + 1 starts and a wait, then the min(starts[last], dcap) index
// entries the device wrote and a wait.
int lists_to_host(uint64_t* starts, const uint64_t* d_starts, uint64_t last, uint32_t* index, const uint32_t* d_index,
                  uint64_t dcap, hipStream_t st);

// Device build of one batch on `st` into d_words (OR-accumulate; fresh =
// BloomFilter::new + inserts: d_words is output-only), chunked so the
// partition workspace stays bounded.  Asynchronous.
int build_dev(lsmb_ctx* c, const KeyBatch& kb, uint32_t num_bits, uint32_t k, uint32_t* d_words, hipStream_t st,
              int sweep = -1, bool fresh = false);

// Keys in host memory -> OR-accumulated into the device words dw (already
// zeroed or loaded by the caller) on c->st: chunked H2D through the two
// staging slots, overlapped with the build.  Returns once everything is
// enqueued; the caller synchronises c->st.
int host_build_dev(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                   uint32_t num_bits, uint32_t k, uint32_t* dw);

// Synchronous build from keys in host memory: words_in == NULL starts from a
// zeroed filter, else from those words; the finished words go to words_out
// (host, any alignment).  crc (optional): CRC-32 of the words appended to *crc.
int host_build(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
               uint32_t num_bits, uint32_t k, const uint64_t* words_in, uint8_t* words_out, uint32_t* crc = nullptr);

// Host build (the library's native per-key loop) into words (OR-accumulate).
void host_insert_batch(const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                       uint32_t num_bits, uint32_t k, uint64_t* words);

// LSMB_STATS builds only: prints and clears pass A's overflow counters
// (ring overflow, full regions).  Requires the builds to have completed.
void report_stats(lsmb_ctx* c);
// CRC-32 (crc32fast::hash / zlib crc32) of device bytes appended to `crc`
// (crc32.hip); synchronises `st`.
int crc32_dev(lsmb_ctx* c, const uint8_t* d, uint64_t len, uint32_t crc, hipStream_t st, uint32_t* out);
// CRC-32 of every device segment (pointer, length) of d_segs into d_out, both
// in device memory: one launch of k_crc32_seg on st, nothing synchronised.
struct CrcSeg;
int crc32_seg_dev(const CrcSeg* d_segs, uint64_t nseg, uint32_t* d_out, hipStream_t st);
// Every item (source, destination, length) of d_segs, in device memory, moved
// device to device: one launch of k_copy_segs (lset_repack.hip) on st, nothing
// synchronised.
struct CopySeg;
int copy_segs_dev(const CopySeg* d_segs, uint64_t nseg, hipStream_t st);
// The set bits of every segment (words, bits) of d_segs into d_out, both in
// device memory: one launch of k_popcount_segs (lset_census.hip) on st,
// nothing synchronised.
struct PopSeg;
int popcount_segs_dev(const PopSeg* d_segs, uint64_t nseg, uint64_t* d_out, hipStream_t st);
uint32_t crc32_host(const uint8_t* p, uint64_t len, uint32_t crc);
uint32_t crc32_combine_host(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

}  // namespace lsmb

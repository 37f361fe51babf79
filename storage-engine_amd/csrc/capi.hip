// capi.hip — the C ABI (include/lsmbloom.h) over the HIP kernels.
//
// Host-side plumbing only: argument validation with the reference's error
// behaviour, the per-GPU context (stream, events, grow-only device arenas),
// the format functions of src/bloom/mod.rs, the single builds and the probe,
// and the helpers the other C ABI files share (ctx.hpp).  The handles have a
// file each: capi_fset.hip (filter sets), capi_build_batch.hip (batched
// builds), capi_lset.hip (level sets).  The builds themselves are orchestrated
// in build_dev.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "ctx.hpp"

using namespace lsmb;

namespace lsmb {

namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(LSMB_EHIP, "%s: %s", what, hipGetErrorString(e));
}

const std::string& last_error() { return g_err; }
void set_last_error(const std::string& s) { g_err = s; }

int check_filter(uint32_t num_bits, uint32_t k) {
    if (num_bits == 0 && k > 0)
        return fail(LSMB_EINVAL, "num_bits == 0 with num_hashes > 0 (reference panics: %% by zero)");
    return LSMB_OK;
}

namespace {
std::atomic<uint64_t> g_host_max_keys{~0ull};  // ~0: not yet read from the environment

uint32_t rd32le(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
}  // namespace

// The 12-byte header of BloomFilter::serialize (src/bloom/mod.rs:102-115):
// num_hashes, num_bits, num_u64s as little-endian u32.
void write_header(uint8_t* out, uint32_t num_bits, uint32_t k) {
    const uint32_t hdr[3] = {k, num_bits, (uint32_t)nwords64(num_bits)};
    for (int j = 0; j < 3; j++)
        for (int b = 0; b < 4; b++) out[4 * j + b] = (uint8_t)(hdr[j] >> (8 * b));
}

void set_host_max_keys(uint64_t n) { g_host_max_keys.store(n == ~0ull ? n - 1 : n, std::memory_order_relaxed); }

uint64_t host_max_keys() {
    uint64_t v = g_host_max_keys.load(std::memory_order_relaxed);
    if (v == ~0ull) {
        const char* s = getenv("LSMB_HOST_MAX_KEYS");
        v = s ? strtoull(s, nullptr, 10) : kDefaultHostMaxKeys;
        g_host_max_keys.store(v, std::memory_order_relaxed);
    }
    return v;
}

hipStream_t pick_stream(lsmb_ctx* c, void* stream) {
    return stream ? reinterpret_cast<hipStream_t>(stream) : c->st;
}

// LSMB_STATS builds only (diagnostics, never the product): pass A counts the
// positions that went past a ring or a full region to exact global atomics.
void report_stats(lsmb_ctx* c) {
#ifdef LSMB_STATS
    uint32_t st[16];
    if (hipMemcpyAsync(st, c->err.p, 64, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
        hipStreamSynchronize(c->st) != hipSuccess)
        return;
    fprintf(stderr, "[lsmb stats] ring_overflow=%u region_full=%u\n", st[9], st[7]);
    (void)hipMemsetAsync(c->err.p, 0, 64, c->st);
#else
    (void)c;
#endif
}

// Host single-key walks (the same arithmetic the kernels run).
template <class W, class F>
void walk_key(const uint8_t* key, uint64_t len, uint32_t num_bits, uint32_t k, F&& f) {
    const typename W::Mod md = W::Mod::make(num_bits);
    const H128 h = xxh3_128(key, len);
    W w(md, h.lo, h.hi);
    for (uint32_t i = 0; i < k; i++) {
        if (!f(w.pos())) return;
        w.next(md);
    }
}

template <class F>
void for_positions(const uint8_t* key, uint64_t len, uint32_t num_bits, uint32_t k, F&& f) {
    if (Mod14::fits(num_bits))
        walk_key<Walk14>(key, len, num_bits, k, f);
    else if (fits_walk32(num_bits))
        walk_key<Walk32>(key, len, num_bits, k, f);
    else
        walk_key<Walk64>(key, len, num_bits, k, f);
}

// offsets[0..n] must be non-decreasing (key i = data[offsets[i] .. offsets[i+1]).
int check_offsets(const uint64_t* offsets, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i])
            return fail(LSMB_EINVAL, "offsets not non-decreasing at %llu", (unsigned long long)i);
    return LSMB_OK;
}

// Copies a host key batch into the context's staging buffers (ctx stream).
int stage_host_keys(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                    KeyBatch* kb) {
    uint64_t kbytes;
    if (offsets) {
        for (uint64_t i = 0; i < n; i++)
            if (offsets[i + 1] < offsets[i]) return fail(LSMB_EINVAL, "offsets not non-decreasing");
        kbytes = offsets[n] - offsets[0];
        c->offs_tmp.resize(n + 1);
        for (uint64_t i = 0; i <= n; i++) c->offs_tmp[i] = offsets[i] - offsets[0];
        HIP_TRY(c->offs.ensure((n + 1) * 8));
        HIP_TRY(hipMemcpyAsync(c->offs.p, c->offs_tmp.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->st));
        HIP_TRY(c->keys.ensure(kbytes + 16));
        if (kbytes) HIP_TRY(hipMemcpyAsync(c->keys.p, data + offsets[0], kbytes, hipMemcpyHostToDevice, c->st));
    } else {
        kbytes = (uint64_t)key_len * n;
        HIP_TRY(c->keys.ensure(kbytes + 16));
        if (kbytes) HIP_TRY(hipMemcpyAsync(c->keys.p, data, kbytes, hipMemcpyHostToDevice, c->st));
    }
    *kb = KeyBatch{(const uint8_t*)c->keys.p, offsets ? (const uint64_t*)c->offs.p : nullptr, key_len, n};
    return LSMB_OK;
}

int slot_enqueue(lsmb_ctx* c, SlotPart* parts, int nparts, hipStream_t st, const char* who, const char* what,
                 const std::function<hipError_t(hipEvent_t done)>& launch) {
    StagingSlots& sl = c->slots;
    const auto up = [](size_t v) { return (v + kSlotAlign - 1) & ~(kSlotAlign - 1); };
    size_t bytes = 0, at = 0;
    for (int i = 0; i < nparts; i++) bytes = up(bytes) + parts[i].bytes;
    const int s = sl.next;
    sl.next ^= 1;
    if (!sl.done[s])
        HIP_TRY(hipEventCreateWithFlags(&sl.done[s], hipEventDisableTiming));
    else if (sl.stream[s])
        HIP_TRY(hipEventSynchronize(sl.done[s]));  // the copy out of this slot, two calls ago
    if (int rc = pinned_ensure(c->pinned_retired, &sl.pin[s], &sl.pin_cap[s], bytes, who)) return rc;
    HIP_TRY(sl.dev[s].ensure(bytes));
    for (int i = 0; i < nparts; i++) {
        at = up(at);
        if (parts[i].bytes) memcpy(sl.pin[s] + at, parts[i].p, parts[i].bytes);
        parts[i].d = (const uint8_t*)sl.dev[s].p + at;
        at += parts[i].bytes;
    }
    if (sl.stream[s] && sl.stream[s] != st) HIP_TRY(hipStreamWaitEvent(st, sl.done[s], 0));
    HIP_TRY(hipMemcpyAsync(sl.dev[s].p, sl.pin[s], bytes, hipMemcpyHostToDevice, st));
    const hipError_t e = launch(sl.done[s]);
    sl.stream[s] = st;
    if (e == hipSuccess) return LSMB_OK;
    (void)hipEventRecord(sl.done[s], st);  // (a failed launch may not have completed the event)
    return hip_fail(e, what);
}

int claim_fail(const SstClaimFault& f, const SstClaim& cl, const char* who, const char* seg, const char* count,
               const char* group, bool in_block) {
    typedef unsigned long long ull;
    const std::string of = in_block ? std::string(group) + " " + std::to_string(f.group) + ": " : std::string();
    switch (f.rule) {
        case kClaimOk: return LSMB_OK;
        case kClaimGroupHook: return f.hook_rc;  // (the hook worded it)
        case kClaimNullSeg: return fail(LSMB_EINVAL, "%s: null %s", who, seg);
        case kClaimNullBlocks: return fail(LSMB_EINVAL, "%s: null blk_off or blk_len", who);
        case kClaimGroups: return fail(LSMB_EINVAL, "%s: more than 2^31-1 %ss", who, group);
        case kClaimSegDescends: return fail(LSMB_EINVAL, "%s: %s descends at %s %llu", who, seg, group, (ull)f.group);
        case kClaimSegPast:
            return fail(LSMB_EINVAL, "%s: %s[%s] = %llu is past the %llu blocks", who, seg, count, (ull)f.seg_end, (ull)cl.nblk);
        case kClaimBlocks: return fail(LSMB_EINVAL, "%s: more than 2^31-1 blocks", who);
        case kClaimBlockLeaves:
            return fail(LSMB_EINVAL, "%s: %sblock %llu (%llu + %u) leaves the %llu bytes", who, of.c_str(), (ull)f.block,
                        (ull)f.off, f.len, (ull)cl.nbytes);
        case kClaimNullBytes: break;
    }
    return fail(LSMB_EINVAL, "%s: null bytes", who);
}

int stage_claim_span(lsmb_ctx* c, const uint8_t* bytes, SstSpan sp) {
    HIP_TRY(c->keys.ensure(sp.hi - sp.lo + 16));
    if (sp.hi > sp.lo) HIP_TRY(hipMemcpyAsync(c->keys.p, bytes + sp.lo, sp.hi - sp.lo, hipMemcpyHostToDevice, c->st));
    return LSMB_OK;
}

int lists_to_host(uint64_t* starts, const uint64_t* d_starts, uint64_t last, uint32_t* index, const uint32_t* d_index,
                  uint64_t dcap, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(starts, d_starts, (last + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t got = std::min<uint64_t>(starts[last], dcap);
    if (got) {
        HIP_TRY(hipMemcpyAsync(index, d_index, got * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return LSMB_OK;
}

// The library's own host build: BloomFilter::insert per key
// (src/bloom/mod.rs:70-78) with the same xxh3 / exact-modulo code the kernels
// run, compiled for the host.  Used below host_max_keys(), where a device round
// trip (H2D, launch, D2H, sync: ~40 us) costs more than the whole loop.
template <class W>
static void host_insert_batch_w(const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                                uint32_t num_bits, uint32_t k, uint64_t* words) {
    const Mod32 md = Mod32::make(num_bits);
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* key = offsets ? data + offsets[i] : data + i * (uint64_t)key_len;
        const uint64_t len = offsets ? offsets[i + 1] - offsets[i] : key_len;
        const H128 h = xxh3_128(key, len);
        W w(md, h.lo, h.hi);
        for (uint32_t j = 0; j < k; j++) {
            const uint32_t p = w.pos();
            words[p >> 6] |= 1ull << (p & 63);
            w.next(md);
        }
    }
}

void host_insert_batch(const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                       uint32_t num_bits, uint32_t k, uint64_t* words) {
    if (k == 0 || n == 0) return;
    if (fits_walk32(num_bits))
        host_insert_batch_w<Walk32>(data, offsets, key_len, n, num_bits, k, words);
    else
        host_insert_batch_w<Walk64>(data, offsets, key_len, n, num_bits, k, words);
}

bool bloom_params(uint64_t n, double fpr, uint32_t* num_bits, uint32_t* num_hashes) {
    if (n == 0 || !(fpr > 0.0 && fpr < 1.0)) return false;
    auto sat = [](double x) -> uint32_t {  // Rust `f64 as u32` saturates
        if (!(x == x) || x <= 0.0) return 0;
        if (x >= 4294967295.0) return 4294967295u;
        return (uint32_t)x;
    };
    const double bpk = -1.44 * log2(fpr);                      // mod.rs:46
    uint32_t nb = sat(ceil((double)n * bpk));                   // mod.rs:49
    if (nb < 64) nb = 64;                                       // mod.rs:52
    uint32_t k = sat(ceil(bpk * log(2.0)));                     // mod.rs:55
    if (k < 1) k = 1;                                           // mod.rs:56
    *num_bits = nb;
    *num_hashes = k;
    return true;
}

}  // namespace lsmb

extern "C" {

int lsmb_abi_version(void) { return LSMB_ABI_VERSION; }
const char* lsmb_last_error(void) { return last_error().c_str(); }

int lsmb_params(uint64_t n, double fpr, uint32_t* num_bits, uint32_t* num_hashes) {
    if (!num_bits || !num_hashes) return fail(LSMB_EINVAL, "null output pointer");
    if (n == 0) return fail(LSMB_EINVAL, "expected_items must be > 0");
    if (!bloom_params(n, fpr, num_bits, num_hashes)) return fail(LSMB_EINVAL, "FPR must be in (0, 1)");
    return LSMB_OK;
}

// What a filter's fill says (BloomFilter::new sizes for fill 1/2 at expected_items, mod.rs:38-68;
// SSTableBuilder hands it an estimate, src/sstable/builder.rs:74).
double lsmb_fill_fpr(uint32_t num_bits, uint32_t num_hashes, uint64_t set_bits) {
    if (set_bits > num_bits) return NAN;
    if (num_hashes == 0) return 1.0;  // may_contain's loop is empty: always true (mod.rs:82-94)
    return pow((double)set_bits / (double)num_bits, (double)num_hashes);
}

double lsmb_fill_keys(uint32_t num_bits, uint32_t num_hashes, uint64_t set_bits) {
    if (set_bits > num_bits || num_hashes == 0) return NAN;
    const double m = (double)num_bits;
    return -(m / (double)num_hashes) * log(1.0 - (double)set_bits / m) + 0.0;  // + 0.0: an empty filter holds 0, not -0
}

uint64_t lsmb_num_words(uint32_t num_bits) { return nwords64(num_bits); }
uint64_t lsmb_serialized_size(uint32_t num_bits) { return 12 + 8 * nwords64(num_bits); }

int lsmb_serialize(const uint64_t* words, uint32_t num_bits, uint32_t k, uint8_t* out, uint64_t out_len) {
    const uint64_t nw = nwords64(num_bits);
    if (out_len < 12 + 8 * nw) return fail(LSMB_EINVAL, "serialize: output buffer too small");
    if (nw && !words) return fail(LSMB_EINVAL, "serialize: null words");
    write_header(out, num_bits, k);
    // words are little-endian u64 on this (x86-64) host: a straight copy.
    if (nw) memcpy(out + 12, words, 8 * nw);
    return LSMB_OK;
}

int lsmb_deserialize_header(const uint8_t* data, uint64_t len, uint32_t* k, uint32_t* num_bits,
                            uint32_t* num_u64s) {
    if (len < 12 || !data) return fail(LSMB_ECORRUPT, "bloom filter too short for header");
    const uint32_t nh = rd32le(data), nb = rd32le(data + 4), nw = rd32le(data + 8);
    const uint64_t expect = nwords64(nb);
    if ((uint64_t)nw != expect)
        return fail(LSMB_ECORRUPT, "bloom filter num_u64s mismatch: got %u, expected %llu", nw,
                    (unsigned long long)expect);
    const uint64_t want = 12 + 8 * (uint64_t)nw;
    if (len != want)
        return fail(LSMB_ECORRUPT, "bloom filter data length mismatch: got %llu, expected %llu",
                    (unsigned long long)len, (unsigned long long)want);
    if (k) *k = nh;
    if (num_bits) *num_bits = nb;
    if (num_u64s) *num_u64s = nw;
    return LSMB_OK;
}

int lsmb_deserialize(const uint8_t* data, uint64_t len, uint64_t* words, uint64_t cap) {
    uint32_t k, nb, nw;
    int rc = lsmb_deserialize_header(data, len, &k, &nb, &nw);
    if (rc) return rc;
    if (cap < nw) return fail(LSMB_EINVAL, "deserialize: words buffer too small");
    if (nw) memcpy(words, data + 12, 8 * (uint64_t)nw);
    return LSMB_OK;
}

int lsmb_positions(const uint8_t* key, uint64_t len, uint32_t num_bits, uint32_t k, uint32_t* out) {
    if (int rc = check_filter(num_bits, k)) return rc;
    uint32_t i = 0;
    if (k) for_positions(key, len, num_bits, k, [&](uint32_t p) { out[i++] = p; return true; });
    return LSMB_OK;
}

int lsmb_insert(uint64_t* words, uint32_t num_bits, uint32_t k, const uint8_t* key, uint64_t len) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if (k)
        for_positions(key, len, num_bits, k, [&](uint32_t p) {
            words[p >> 6] |= 1ull << (p & 63);
            return true;
        });
    return LSMB_OK;
}

int lsmb_may_contain(const uint64_t* words, uint32_t num_bits, uint32_t k, const uint8_t* key,
                     uint64_t len) {
    if (int rc = check_filter(num_bits, k)) return rc;
    bool all = true;  // k == 0: the reference's k-loop is empty -> true
    if (k)
        for_positions(key, len, num_bits, k, [&](uint32_t p) {
            all = (words[p >> 6] >> (p & 63)) & 1;
            return all;  // early exit on the first clear bit (mod.rs:88-90)
        });
    return all ? 1 : 0;
}

int lsmb_open(lsmb_ctx** out, int device) {
    if (!out) return fail(LSMB_EINVAL, "null ctx pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(LSMB_ENODEV, "no HIP device visible (this engine runs its batched path on MI355X only)");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= n) return fail(LSMB_ENODEV, "device %d out of range (%d visible)", device, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(LSMB_ENODEV, "hipGetDeviceProperties(%d) failed", device);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(LSMB_ENODEV, "device %d is %s; kernels are built for gfx950 only", device, prop.gcnArchName);
    lsmb_ctx* c = new lsmb_ctx;
    c->dev = device;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    DevGuard g(device);
    // The context's stream is a BLOCKING stream: it is ordered with the legacy
    // null stream, which is what torch's default stream is.  The device entry
    // points map stream == NULL to this stream, so a caller that allocates or
    // zeroes buffers on the null stream and then builds with stream == NULL
    // gets the two in order (tests/test_gpu_parity.py relies on it).  Two
    // contexts' blocking streams do not wait for each other; the library
    // itself issues nothing on the null stream after lsmb_open (the filter
    // set uploads on a non-blocking stream of its own).
    if (hipStreamCreateWithFlags(&c->st, hipStreamDefault) != hipSuccess ||
        hipEventCreateWithFlags(&c->desc_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ws_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->tm.t0) != hipSuccess || hipEventCreate(&c->tm.t1) != hipSuccess ||
        hipEventCreate(&c->tm.t2) != hipSuccess ||
        hipStreamCreateWithFlags(&c->cst, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_copy[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_copy[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_built[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_built[1], hipEventDisableTiming) != hipSuccess) {
        delete c;
        return fail(LSMB_ENODEV, "stream/event creation failed on device %d", device);
    }
    if (c->err.ensure(64) != hipSuccess || hipMemsetAsync(c->err.p, 0, 64, c->st) != hipSuccess ||
        hipStreamSynchronize(c->st) != hipSuccess) {
        lsmb_close(c);
        return fail(LSMB_ENOMEM, "counter allocation failed on device %d", device);
    }
    *out = c;
    return LSMB_OK;
}

void lsmb_close(lsmb_ctx* c) {
    if (!c) return;
    {
        DevGuard g(c->dev);
        hipStreamSynchronize(c->st);
        if (c->cst) hipStreamSynchronize(c->cst);
        for (DevBuf* b : {&c->ws_regions, &c->ws_counts, &c->ws_hashes, &c->ws_ovf, &c->ws_dirty, &c->ws_ovl, &c->ws_ovn, &c->crc_parts, &c->err, &c->keys, &c->offs, &c->words, &c->out,
                          &c->filt_words, &c->filt_desc, &c->kslot[0], &c->kslot[1], &c->oslot[0], &c->oslot[1]})
            b->release();
        for (int s = 0; s < 2; s++) {
            if (c->offs_pin[s]) hipHostFree(c->offs_pin[s]);  // teardown
            if (c->ev_copy[s]) hipEventDestroy(c->ev_copy[s]);
            if (c->ev_built[s]) hipEventDestroy(c->ev_built[s]);
        }
        if (c->cst) hipStreamDestroy(c->cst);
        if (c->pin_small) hipHostFree(c->pin_small);  // teardown
        c->slots.release();
        c->bb_words.release();
        if (c->bb_host) hipHostFree(c->bb_host);  // teardown
        c->pinned_retired.release();
        hipEventDestroy(c->tm.t0);
        hipEventDestroy(c->tm.t1);
        hipEventDestroy(c->tm.t2);
        hipEventDestroy(c->desc_done);
        if (c->ws_done) hipEventDestroy(c->ws_done);
        if (c->desc_pinned) hipHostFree(c->desc_pinned);  // teardown
        hipStreamDestroy(c->st);
    }
    delete c;
}

int lsmb_sync(lsmb_ctx* c) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    DevGuard g(c->dev);
    HIP_TRY(hipStreamSynchronize(c->st));
    report_stats(c);
    return LSMB_OK;
}

// The device build entry points: null ctx, then the filter arguments, then
// null pointers (fresh builds write d_words even with no keys), then the sweep
// range (sweep builds; NULL: every sweep); then the build on the caller's
// stream.  kb.n is set here: fixed-length keys of length 0 are all the empty
// key, one insert covers them.
static int build_dev_checked(lsmb_ctx* c, KeyBatch kb, bool var, uint64_t n, uint32_t num_bits, uint32_t k,
                             void* d_words, void* stream, bool fresh, const int* sweep = nullptr) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (int rc = check_filter(num_bits, k)) return rc;
    const void* d_keys = var ? (const void*)kb.offsets : (const void*)kb.data;
    if (fresh ? (!d_words || (n && !d_keys)) : (n && (!d_keys || !d_words))) return fail(LSMB_EINVAL, "null device pointer");
    if (sweep) {
        const int ns = lsmb_build_sweeps(num_bits, k, n);
        if (*sweep < 0 || *sweep >= ns) return fail(LSMB_EINVAL, "sweep %d out of range [0, %d)", *sweep, ns);
    }
    kb.n = var || kb.key_len ? n : (n ? 1 : 0);
    DevGuard g(c->dev);
    return build_dev(c, kb, num_bits, k, (uint32_t*)d_words, pick_stream(c, stream), sweep ? *sweep : -1, fresh);
}

int lsmb_build_fixed_dev(lsmb_ctx* c, const void* d_keys, uint32_t key_len, uint64_t n,
                         uint32_t num_bits, uint32_t k, void* d_words, void* stream) {
    return build_dev_checked(c, KeyBatch{(const uint8_t*)d_keys, nullptr, key_len, 0}, /*var=*/false, n, num_bits, k, d_words, stream,
                             /*fresh=*/false);
}

int lsmb_build_var_dev(lsmb_ctx* c, const void* d_data, const void* d_offsets, uint64_t n,
                       uint32_t num_bits, uint32_t k, void* d_words, void* stream) {
    return build_dev_checked(c, KeyBatch{(const uint8_t*)d_data, (const uint64_t*)d_offsets, 0, 0}, /*var=*/true, n, num_bits, k,
                             d_words, stream, /*fresh=*/false);
}

// BloomFilterBuilder::{new, add_key, build} (src/bloom/builder.rs:14-28): BloomFilter::new
// (src/bloom/mod.rs:38-67, all-zero words) + insert of every key.  The words
// are output-only: the partition build writes each of them once in pass B
// without reading it, so no zeroing pass and no read of the old words.
int lsmb_build_fixed_dev_new(lsmb_ctx* c, const void* d_keys, uint32_t key_len, uint64_t n, uint32_t num_bits,
                             uint32_t k, void* d_words, void* stream) {
    return build_dev_checked(c, KeyBatch{(const uint8_t*)d_keys, nullptr, key_len, 0}, /*var=*/false, n, num_bits, k, d_words, stream,
                             /*fresh=*/true);
}

int lsmb_build_var_dev_new(lsmb_ctx* c, const void* d_data, const void* d_offsets, uint64_t n, uint32_t num_bits,
                           uint32_t k, void* d_words, void* stream) {
    return build_dev_checked(c, KeyBatch{(const uint8_t*)d_data, (const uint64_t*)d_offsets, 0, 0}, /*var=*/true, n, num_bits, k,
                             d_words, stream, /*fresh=*/true);
}

// Builds of n <= host_max_keys() keys run the library's host loop (no device
// round trip, ctx may be NULL); bigger ones need a device context.
static int need_ctx(lsmb_ctx* c, uint64_t n) {
    if (!c)
        return fail(LSMB_EINVAL, "null ctx: builds of more than %llu keys run on the GPU (lsmb_host_max_keys)",
                    (unsigned long long)host_max_keys());
    (void)n;
    return LSMB_OK;
}

// (the sweep layout is a function of (num_bits, k): no device needed)
int lsmb_build_sweeps(uint32_t num_bits, uint32_t k, uint64_t n) {
    if (pick_build_strategy(num_bits, k, n) != BuildStrategy::Partition) return 1;
    return (int)partition_layout(num_bits, k).sweeps;
}

int lsmb_sweep_words(uint32_t num_bits, uint32_t k, uint64_t n, int sweep, uint64_t* word_lo, uint64_t* word_hi) {
    if (!word_lo || !word_hi) return fail(LSMB_EINVAL, "null output pointer");
    const int ns = lsmb_build_sweeps(num_bits, k, n);
    if (sweep < 0 || sweep >= ns) return fail(LSMB_EINVAL, "sweep %d out of range [0, %d)", sweep, ns);
    const uint64_t nw = nwords64(num_bits);
    if (ns == 1) {
        *word_lo = 0;
        *word_hi = nw;
        return LSMB_OK;
    }
    const PartitionPlan pl = partition_layout(num_bits, k);
    const uint64_t w_per_slice = (1ull << pl.slice_log2) / 64;
    *word_lo = std::min<uint64_t>(nw, (uint64_t)sweep * pl.bins_per_sweep * w_per_slice);
    *word_hi = std::min<uint64_t>(nw, ((uint64_t)sweep + 1) * pl.bins_per_sweep * w_per_slice);
    return LSMB_OK;
}

int lsmb_build_fixed_dev_sweep(lsmb_ctx* c, const void* d_keys, uint32_t key_len, uint64_t n, uint32_t num_bits,
                               uint32_t k, void* d_words, int sweep, void* stream) {
    return build_dev_checked(c, KeyBatch{(const uint8_t*)d_keys, nullptr, key_len, 0}, /*var=*/false, n, num_bits, k, d_words, stream,
                             /*fresh=*/false, &sweep);
}

int lsmb_build_fixed_dev_sweep_new(lsmb_ctx* c, const void* d_keys, uint32_t key_len, uint64_t n, uint32_t num_bits,
                                   uint32_t k, void* d_words, int sweep, void* stream) {
    return build_dev_checked(c, KeyBatch{(const uint8_t*)d_keys, nullptr, key_len, 0}, /*var=*/false, n, num_bits, k, d_words, stream,
                             /*fresh=*/true, &sweep);
}

int lsmb_build_fixed(lsmb_ctx* c, const uint8_t* keys, uint32_t key_len, uint64_t n, uint32_t num_bits,
                     uint32_t k, uint64_t* words) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if (n == 0 || k == 0) return LSMB_OK;
    if (!keys && key_len) return fail(LSMB_EINVAL, "null keys");
    if (!words) return fail(LSMB_EINVAL, "null words");
    if (n <= host_max_keys()) {
        host_insert_batch(keys, nullptr, key_len, key_len ? n : 1, num_bits, k, words);
        return LSMB_OK;
    }
    if (int rc = need_ctx(c, n)) return rc;
    DevGuard g(c->dev);
    return host_build(c, keys, nullptr, key_len, n, num_bits, k, words, (uint8_t*)words);
}

int lsmb_build_var(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint64_t n,
                   uint32_t num_bits, uint32_t k, uint64_t* words) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if (n == 0 || k == 0) return LSMB_OK;
    if (!offsets || !words) return fail(LSMB_EINVAL, "null pointer");
    if (int rc = check_offsets(offsets, n)) return rc;
    if (n <= host_max_keys()) {
        host_insert_batch(data, offsets, 0, n, num_bits, k, words);
        return LSMB_OK;
    }
    if (int rc = need_ctx(c, n)) return rc;
    DevGuard g(c->dev);
    return host_build(c, data, offsets, 0, n, num_bits, k, words, (uint8_t*)words);
}

static int build_block(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                       uint32_t num_bits, uint32_t k, uint8_t* block, uint64_t block_len, uint32_t* crc) {
    if (int rc = check_filter(num_bits, k)) return rc;
    const uint64_t nw = nwords64(num_bits);
    const uint64_t size = 12 + 8 * nw;
    if (!block) return fail(LSMB_EINVAL, "null block");
    if (block_len < size)
        return fail(LSMB_EINVAL, "block buffer %llu B < serialized size %llu B", (unsigned long long)block_len,
                    (unsigned long long)size);
    if (n && !offsets && !data && key_len) return fail(LSMB_EINVAL, "null keys");
    if (n && offsets) {
        if (int rc = check_offsets(offsets, n)) return rc;
    }
    write_header(block, num_bits, k);
    if (n == 0 || k == 0) {  // new() + no inserts: all-zero words
        memset(block + 12, 0, nw * 8);
        if (crc) *crc = crc32_host(block, size, 0);
        return LSMB_OK;
    }
    if (n <= host_max_keys()) {
        // the block body is not 8-byte aligned (12-B header): build into an
        // aligned word array, then copy
        std::vector<uint64_t> w(nw, 0);
        host_insert_batch(data, offsets, key_len, (!offsets && key_len == 0) ? 1 : n, num_bits, k, w.data());
        memcpy(block + 12, w.data(), nw * 8);
        if (crc) *crc = crc32_host(block, size, 0);
        return LSMB_OK;
    }
    if (int rc = need_ctx(c, n)) return rc;
    DevGuard g(c->dev);
    if (crc) *crc = crc32_host(block, 12, 0);  // the header; the words' CRC is appended on the device
    return host_build(c, data, offsets, key_len, n, num_bits, k, nullptr, block + 12, crc);
}

int lsmb_build_block(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                     uint32_t num_bits, uint32_t k, uint8_t* block, uint64_t block_len) {
    return build_block(c, data, offsets, key_len, n, num_bits, k, block, block_len, nullptr);
}

int lsmb_build_block_crc(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                         uint32_t num_bits, uint32_t k, uint8_t* block, uint64_t block_len, uint32_t* crc) {
    if (!crc) return fail(LSMB_EINVAL, "null crc");
    return build_block(c, data, offsets, key_len, n, num_bits, k, block, block_len, crc);
}



uint64_t lsmb_host_max_keys(void) { return host_max_keys(); }

void lsmb_set_host_max_keys(uint64_t n) { set_host_max_keys(n); }

static int probe_common(lsmb_ctx* c, const uint32_t* const* wptrs, const uint32_t* filt_bits,
                        const uint32_t* filt_k, uint32_t nfilt, const KeyBatch& kb, uint8_t* d_out,
                        hipStream_t st) {
    if (nfilt == 0 || nfilt > 64) return fail(LSMB_EINVAL, "nfilt must be in [1, 64]");
    c->hfilt.resize(nfilt);
    for (uint32_t f = 0; f < nfilt; f++) {
        if (int rc = check_filter(filt_bits[f], filt_k[f])) return rc;
        ProbeFilter& p = c->hfilt[f];
        memset(&p, 0, sizeof p);
        p.words32 = wptrs[f];
        p.md = Mod32::make(filt_bits[f] ? filt_bits[f] : 1);
        p.num_bits = filt_bits[f];
        p.k = filt_k[f];
        p.out_bit = f;
        p.group = f;
    }
    if (kb.n == 0) return LSMB_OK;  // (no launch: nothing would complete the guard event below)
    // The bit-sliced kernels (filters sharing one size, the store's SST
    // filters) take the filters in their kernel arguments: nothing to upload
    // and no event to record, so back-to-back probes are back-to-back kernels.
    if (!probe_reads_descriptors(c->hfilt.data(), nfilt)) {
        HIP_TRY(launch_probe(kb, c->hfilt.data(), nfilt, nullptr, d_out, c->num_cus, st));
        return LSMB_OK;
    }
    // Descriptors go to the device only when they change (a probe loop over the
    // same level filters re-uses them).  filt_desc is shared by every generic
    // probe on this context, whatever its stream, so the generic probes are
    // kept in one chain: desc_done is completed by the last one's kernel
    // (launch_done), and the next one starts after it.
    //  - New descriptors: the host waits for desc_done before it refills the
    //    pinned staging and queues the upload.  The chain makes that enough:
    //    once the last kernel is done, so is every earlier one, on any stream.
    //  - Same descriptors on another stream than the last probe's: that stream
    //    waits for desc_done, or its kernel could run before the upload still
    //    queued on the other stream and read what filt_desc held before.
    //  - Same descriptors on the same stream: stream order already holds, so
    //    no wait packet and no host sync sits between repeat probes; they stay
    //    back-to-back kernels.
    HIP_TRY(c->filt_desc.ensure(sizeof(ProbeFilter) * 64));
    const bool same = c->desc_uploaded.size() == nfilt &&
                      memcmp(c->desc_uploaded.data(), c->hfilt.data(), sizeof(ProbeFilter) * nfilt) == 0;
    if (!same) {
        if (!c->desc_pinned) HIP_TRY(hipHostMalloc((void**)&c->desc_pinned, sizeof(ProbeFilter) * 64, 0));
        HIP_TRY(hipEventSynchronize(c->desc_done));
        memcpy(c->desc_pinned, c->hfilt.data(), sizeof(ProbeFilter) * nfilt);
        HIP_TRY(hipMemcpyAsync(c->filt_desc.p, c->desc_pinned, sizeof(ProbeFilter) * nfilt,
                               hipMemcpyHostToDevice, st));
        c->desc_uploaded = c->hfilt;
    } else if (c->desc_stream != st) {
        HIP_TRY(hipStreamWaitEvent(st, c->desc_done, 0));
    }
    c->desc_stream = st;
    const hipError_t e = launch_probe(kb, c->hfilt.data(), nfilt, (ProbeFilter*)c->filt_desc.p, d_out, c->num_cus, st,
                                      c->desc_done);  // (the dispatch completes the guard event)
    if (e != hipSuccess) {
        (void)hipEventRecord(c->desc_done, st);  // (a failed launch may not have completed it; an upload may be queued)
        return hip_fail(e, "launch_probe");
    }
    return LSMB_OK;
}

int lsmb_probe_dev(lsmb_ctx* c, const void* const* d_filt_words, const uint32_t* filt_bits,
                   const uint32_t* filt_k, uint32_t nfilt, const void* d_data, const void* d_offsets,
                   uint32_t key_len, uint64_t n, void* d_out, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (!d_filt_words || !filt_bits || !filt_k) return fail(LSMB_EINVAL, "null filter arrays");
    if (n && !d_out) return fail(LSMB_EINVAL, "null output");
    DevGuard g(c->dev);
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    return probe_common(c, (const uint32_t* const*)d_filt_words, filt_bits, filt_k, nfilt, kb,
                        (uint8_t*)d_out, pick_stream(c, stream));
}

int lsmb_probe(lsmb_ctx* c, const uint64_t* const* filt_words, const uint32_t* filt_bits,
               const uint32_t* filt_k, uint32_t nfilt, const uint8_t* data, const uint64_t* offsets,
               uint32_t key_len, uint64_t n, uint8_t* out) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (!filt_words || !filt_bits || !filt_k) return fail(LSMB_EINVAL, "null filter arrays");
    if (nfilt == 0 || nfilt > 64) return fail(LSMB_EINVAL, "nfilt must be in [1, 64]");
    if (n == 0) return LSMB_OK;
    if (!out) return fail(LSMB_EINVAL, "null output");
    DevGuard g(c->dev);
    // filters -> one device arena
    uint64_t tot = 0;
    std::vector<uint64_t> at(nfilt);
    for (uint32_t f = 0; f < nfilt; f++) {
        at[f] = tot;
        tot += (nwords64(filt_bits[f]) + 1) & ~1ull;  // keep 16-B alignment
    }
    HIP_TRY(c->filt_words.ensure(std::max<uint64_t>(tot, 2) * 8));
    std::vector<const uint32_t*> dptr(nfilt);
    for (uint32_t f = 0; f < nfilt; f++) {
        uint64_t* d = (uint64_t*)c->filt_words.p + at[f];
        if (nwords64(filt_bits[f]))
            HIP_TRY(hipMemcpyAsync(d, filt_words[f], nwords64(filt_bits[f]) * 8, hipMemcpyHostToDevice, c->st));
        dptr[f] = (const uint32_t*)d;
    }
    const uint32_t stride = (nfilt + 7) / 8;
    HIP_TRY(c->out.ensure(n * stride));
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    if (int rc = probe_common(c, dptr.data(), filt_bits, filt_k, nfilt, kb, (uint8_t*)c->out.p, c->st)) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->out.p, n * stride, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

int lsmb_or_reduce_dev(lsmb_ctx* c, void* dst, const void* src, uint64_t nwords, uint32_t nsrc,
                       uint64_t stride_words, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (nwords == 0 || nsrc == 0) return LSMB_OK;
    DevGuard g(c->dev);
    HIP_TRY(launch_or_reduce((uint32_t*)dst, (const uint32_t*)src, 2 * nwords, nsrc, 2 * stride_words,
                             pick_stream(c, stream)));
    return LSMB_OK;
}

int lsmb_gen_splitmix_dev(lsmb_ctx* c, uint64_t seed, uint64_t first, uint64_t n, uint32_t mod, uint32_t add,
                          void* d_out, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (n && !d_out) return fail(LSMB_EINVAL, "null device pointer");
    if (((uintptr_t)d_out) & 7) return fail(LSMB_EINVAL, "d_out must be 8-byte aligned");
    DevGuard g(c->dev);
    HIP_TRY(launch_gen_splitmix(seed, first, n, mod, add, (uint64_t*)d_out, pick_stream(c, stream)));
    return LSMB_OK;
}

int lsmb_gen_key16_dev(lsmb_ctx* c, uint64_t seed, uint64_t first, uint64_t n, void* d_keys, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    if (n == 0) return LSMB_OK;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15) return fail(LSMB_EINVAL, "d_keys must be 16-byte aligned");
    DevGuard g(c->dev);
    HIP_TRY(launch_gen_key16(seed, first, n, (uint8_t*)d_keys, pick_stream(c, stream)));
    return LSMB_OK;
}

const char* lsmb_build_strategy(uint32_t num_bits, uint32_t k, uint64_t n) {
    return strategy_name(pick_build_strategy(num_bits, k, n));
}

int lsmb_set_timing(lsmb_ctx* c, int enable) {
    if (!c) return fail(LSMB_EINVAL, "null ctx");
    c->timing = enable != 0;
    return LSMB_OK;
}

int lsmb_last_build_ms(lsmb_ctx* c, float* out3) {
    if (!c || !out3) return fail(LSMB_EINVAL, "null argument");
    if (!c->tm.valid) return fail(LSMB_EINVAL, "no timed build on this context");
    DevGuard g(c->dev);
    // the build may run on a caller's stream: wait for its end marker, not c->st
    HIP_TRY(hipEventSynchronize(c->tm.t2));
    HIP_TRY(hipEventElapsedTime(&out3[0], c->tm.t0, c->tm.t2));
    HIP_TRY(hipEventElapsedTime(&out3[1], c->tm.t0, c->tm.t1));
    HIP_TRY(hipEventElapsedTime(&out3[2], c->tm.t1, c->tm.t2));
    return LSMB_OK;
}

}  // extern "C"

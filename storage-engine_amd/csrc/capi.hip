// capi.hip — the C ABI (include/lsmbloom.h) over the HIP kernels.
//
// Host-side plumbing only: argument validation with the reference's error
// behaviour, the per-GPU context (stream, events, grow-only device arenas),
// the format functions of src/bloom/mod.rs, the probe and the filter set.
// The builds themselves are orchestrated in build_dev.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "build_batch_plan.hpp"
#include "crc_seg.hpp"
#include "ctx.hpp"
#include "lset_lists_plan.hpp"
#include "lset_order.hpp"

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

// The 12-byte header of BloomFilter::serialize (src/bloom/mod.rs:102-115):
// num_hashes, num_bits, num_u64s as little-endian u32.
void write_header(uint8_t* out, uint32_t num_bits, uint32_t k) {
    const uint32_t hdr[3] = {k, num_bits, (uint32_t)nwords64(num_bits)};
    for (int j = 0; j < 3; j++)
        for (int b = 0; b < 4; b++) out[4 * j + b] = (uint8_t)(hdr[j] >> (8 * b));
}
}  // namespace

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
        for (int s = 0; s < 2; s++) {
            c->bb_items[s].release();
            if (c->bb_pin[s]) hipHostFree(c->bb_pin[s]);  // teardown
            if (c->bb_done[s]) hipEventDestroy(c->bb_done[s]);
        }
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

// Copies a host key batch into the context's staging buffers (ctx stream).
static int stage_host_keys(lsmb_ctx* c, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
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
    // same level filters re-uses them); the upload waits for the last kernel
    // that read the previous set, so no host sync sits between repeat probes.
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
    }
    HIP_TRY(launch_probe(kb, c->hfilt.data(), nfilt, (ProbeFilter*)c->filt_desc.p, d_out, c->num_cus, st,
                         c->desc_done));  // (the dispatch completes the guard event)
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
// key ranges with one in-range mask per region (FsetRanges, kernels.hpp).
int fset_refresh(lsmb_fset* fs) {
    if (!fs->dirty) return LSMB_OK;
    std::vector<const lsmb_fset::Slot*> live;
    std::vector<uint32_t> slot_of;
    for (uint32_t s = 0; s < 64; s++)
        if (fs->slot[s].live) {
            live.push_back(&fs->slot[s]);
            slot_of.push_back(s);
        }
    // distinct bounds, sorted as Rust's [u8] Ord (std::vector<uint8_t> < is
    // the same unsigned lexicographic order, a proper prefix first)
    std::vector<std::vector<uint8_t>> pts;
    for (const auto* S : live) {
        pts.push_back(S->lo);
        pts.push_back(S->hi);
    }
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    const uint32_t m = (uint32_t)pts.size();
    // region masks over descriptor indices: region 2r = (P[r-1], P[r]),
    // region 2r+1 = {P[r]}
    std::vector<uint64_t> regmask(2 * m + 1, 0);
    for (uint32_t d = 0; d < live.size(); d++) {
        const auto* S = live[d];
        if (S->hi < S->lo) continue;  // an empty range holds no key
        const uint32_t a = (uint32_t)(std::lower_bound(pts.begin(), pts.end(), S->lo) - pts.begin());
        const uint32_t b = (uint32_t)(std::lower_bound(pts.begin(), pts.end(), S->hi) - pts.begin());
        for (uint32_t reg = 2 * a + 1; reg <= 2 * b + 1; reg++) regmask[reg] |= 1ull << d;
    }
    std::vector<uint8_t> blob;
    std::vector<uint64_t> at;
    for (const auto& p : pts) {
        at.push_back(blob.size());
        blob.insert(blob.end(), p.begin(), p.end());
    }
    if (int rc = fset_wait_probes(fs)) return rc;  // no probe may still read the old descriptors
    // grow geometrically from 4 KiB (an outgrown buffer is retired, not freed:
    // DevBuf)
    size_t want = 4096;
    while (want < blob.size()) want *= 2;
    HIP_TRY(fs->ranges.ensure(want));
    if (!blob.empty()) HIP_TRY(hipMemcpyAsync(fs->ranges.p, blob.data(), blob.size(), hipMemcpyHostToDevice, fs->ust));
    const uint8_t* rb = (const uint8_t*)fs->ranges.p;
    std::vector<uint8_t> pbuf(sizeof(FsetPoint) * kFsetMaxPoints + 8 * (2 * kFsetMaxPoints + 1));
    FsetPoint* fp = (FsetPoint*)pbuf.data();
    for (uint32_t j = 0; j < m; j++) {
        const auto& p = pts[j];
        uint8_t pad[16] = {0};
        memcpy(pad, p.data(), std::min<size_t>(16, p.size()));
        uint64_t w0 = 0, w1 = 0;
        for (int b = 0; b < 8; b++) {
            w0 = (w0 << 8) | pad[b];
            w1 = (w1 << 8) | pad[8 + b];
        }
        fp[j].w0 = w0;
        fp[j].w1 = w1;
        fp[j].p = rb + at[j];
        fp[j].len = (uint32_t)p.size();
        fp[j].pad = 0;
    }
    memcpy(pbuf.data() + sizeof(FsetPoint) * m, regmask.data(), 8 * regmask.size());
    HIP_TRY(fs->points.ensure(pbuf.size()));
    HIP_TRY(hipMemcpyAsync(fs->points.p, pbuf.data(), sizeof(FsetPoint) * m + 8 * regmask.size(), hipMemcpyHostToDevice,
                           fs->ust));
    fs->rg.pts = (const FsetPoint*)fs->points.p;
    fs->rg.regmask = (const uint64_t*)((const uint8_t*)fs->points.p + sizeof(FsetPoint) * m);
    fs->rg.npts = m;
    std::vector<RangedFilter> d;
    for (uint32_t j = 0; j < live.size(); j++) {
        const auto* S = live[j];
        RangedFilter r;
        memset(&r, 0, sizeof r);
        r.f.words32 = (const uint32_t*)S->words.p;
        r.f.md = Mod32::make(S->num_bits ? S->num_bits : 1);
        r.f.num_bits = S->num_bits;
        r.f.k = S->k;
        r.f.out_bit = slot_of[j];
        r.f.group = slot_of[j];
        d.push_back(r);
    }
    HIP_TRY(fs->desc.ensure(sizeof(RangedFilter) * 64));
    if (!d.empty())
        HIP_TRY(hipMemcpyAsync(fs->desc.p, d.data(), sizeof(RangedFilter) * d.size(), hipMemcpyHostToDevice, fs->ust));
    // size classes: descriptors grouped by (num_bits, k); the classes with the
    // smallest tables go to LDS first (most filters per byte), the rest and
    // k = 0 filters are walked from L2
    std::vector<FsetClass> cls;
    {
        std::vector<std::pair<uint64_t, uint32_t>> keyd;  // (num_bits << 32 | k, descriptor)
        for (uint32_t j = 0; j < d.size(); j++)
            if (d[j].f.k) keyd.push_back({((uint64_t)d[j].f.num_bits << 32) | d[j].f.k, j});
        std::sort(keyd.begin(), keyd.end());
        std::vector<FsetClass> all;
        for (size_t a = 0; a < keyd.size();) {
            size_t b = a;
            while (b < keyd.size() && keyd[b].first == keyd[a].first) b++;
            FsetClass c;
            memset(&c, 0, sizeof c);
            c.num_bits = (uint32_t)(keyd[a].first >> 32);
            c.k = (uint32_t)keyd[a].first;
            c.md = Mod32::make(c.num_bits);
            c.md14 = Mod14::make(Mod14::fits(c.num_bits) ? c.num_bits : 1);
            c.nmem = (uint32_t)(b - a);
            c.width = c.nmem <= 8 ? 1 : c.nmem <= 16 ? 2 : c.nmem <= 32 ? 4 : 8;
            for (size_t j = a; j < b; j++) {
                c.mem[j - a] = (uint8_t)keyd[j].second;
                c.mask |= 1ull << keyd[j].second;
            }
            all.push_back(c);
            a = b;
        }
        auto tbytes = [](const FsetClass& c) { return (((uint64_t)c.num_bits + 31) / 32) * 32 * c.width; };
        std::stable_sort(all.begin(), all.end(),
                         [&](const FsetClass& x, const FsetClass& y) { return tbytes(x) < tbytes(y); });
        uint64_t off = 0, in_lds = 0;
        for (auto& c : all) {
            const uint64_t tb = (tbytes(c) + 15) & ~15ull;
            if (cls.size() < kFsetMaxClasses && off + tb <= kFsetTableBytes) {
                c.off = (uint32_t)off;
                off += tb;
                in_lds |= c.mask;
                cls.push_back(c);
            }
        }
        uint64_t all_desc = d.size() == 64 ? ~0ull : (1ull << d.size()) - 1;
        fs->cl.ncls = (uint32_t)cls.size();
        fs->cl.table_bytes = (uint32_t)off;
        fs->cl.walk_mask = all_desc & ~in_lds;
    }
    for (size_t i = 0; i < cls.size(); i++) fs->cl.cls[i] = cls[i];
    HIP_TRY(hipStreamSynchronize(fs->ust));  // blob, pbuf and d are host temporaries
    fs->ndesc = (uint32_t)d.size();
    fs->shared_nb = d.empty() ? 0 : d[0].f.num_bits;
    fs->shared_k = d.empty() ? 0 : d[0].f.k;
    for (const auto& r : d)
        if (r.f.num_bits != fs->shared_nb || r.f.k != fs->shared_k) fs->shared_nb = fs->shared_k = 0;
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
    if (!out_mask || (!data && (offsets ? offsets[n] > offsets[0] : key_len > 0)))
        return fail(LSMB_EINVAL, "null keys or output");
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
    if (n && !data && (offsets ? offsets[n] > offsets[0] : key_len > 0)) return fail(LSMB_EINVAL, "null keys");
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
    HIP_TRY(hipMemcpyAsync(starts, fs->lstarts.p, 65 * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    const uint64_t got = std::min<uint64_t>(starts[64], dcap);
    if (got) {
        HIP_TRY(hipMemcpyAsync(index, fs->lindex.p, got * 4, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    return LSMB_OK;
}

// ---------------------------------------------------------------- batched build
// Many tables' filters from one key run (build_batch_plan.hpp, build_batch.hip):
// SSTableBuilder::new + add per key + finish (src/sstable/builder.rs:74,93,
// 177-182) for every output table of a bulk load or of compactions finishing
// together (src/compaction/scheduler.rs:147-177), one launch per geometry class.
namespace {

// A grow-only pinned block: the outgrown one is retired until lsmb_close.
int bb_pinned_ensure(lsmb_ctx* c, uint8_t** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return LSMB_OK;
    const uint64_t want = std::max<uint64_t>(need, *cap + *cap / 2);
    void* q = nullptr;
    if (hipHostMalloc(&q, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LSMB_ENOMEM, "batched build: %llu bytes of pinned staging", (unsigned long long)want);
    }
    c->pinned_retired.retire(*p);
    *p = (uint8_t*)q;
    *cap = want;
    return LSMB_OK;
}

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
    if (int rc = bb_pinned_ensure(c, &c->bb_pin[s], &c->bb_pin_cap[s], bytes)) return rc;
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
    if (n && !offsets && !data && key_len) return fail(LSMB_EINVAL, "batched build: null keys");
    if (n && offsets && offsets[n] > offsets[0] && !data) return fail(LSMB_EINVAL, "batched build: null keys");
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
    if (int rc = bb_pinned_ensure(c, &c->bb_host, &c->bb_host_cap, wbytes)) return rc;
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

// ---------------------------------------------------------------- level sets
// An immutable, device-resident snapshot of the store's non-overlapping
// levels (one per Version, src/db/mod.rs:255-267): rows of tables with
// pairwise disjoint key ranges, any number per row.  Tables are added in any
// order, each filter copied into a device arena as it arrives; seal sorts the
// rows, checks them (lset_order.hpp) and uploads the descriptors.  A sealed
// set is only read, so its probes need no scratch and no ordering.
//
// A Version edit (src/compaction/scheduler.rs:163-177) derives the next set
// from a sealed one: the child holds the surviving tables with their device
// words where they are, so the arena chunks are reference-counted (the counts
// are shared_ptr's, atomic: a parent may be probed while a child is derived)
// and a chunk goes when the last set holding one of its tables is closed.  A
// set bump-allocates only in chunks it allocated itself (own_tail), never in
// the tail of an inherited one: two children of one parent would collide
// there, and a sealed set's memory stays read-only for probes in flight.
namespace lsmb {
struct LsetChunk {
    int dev = 0;
    DevBuf buf;
    ~LsetChunk() {  // the last set holding the chunk closes (or a failed batch gives its chunks back)
        DevGuard g(dev);
        buf.release();
    }
};
}  // namespace lsmb

struct lsmb_lset {
    lsmb_ctx* c = nullptr;
    struct Table {
        uint32_t id = 0, num_bits = 0, k = 0;
        uint32_t chunk = 0;               // index into chunks
        const uint32_t* words = nullptr;  // in the arena
        std::vector<uint8_t> lo, hi;
    };
    std::vector<Table> row[kLsetMaxRows];
    uint32_t nrows = 0;  // 1 + highest row added
    bool sealed = false;
    // filter words: bump-allocated from chunks that are never reallocated;
    // a derived set's inherited chunks come first
    std::vector<std::shared_ptr<LsetChunk>> chunks;
    size_t chunk_used = 0;
    bool own_tail = false;  // chunks.back() is this set's own: the bump pointer may advance in it
    // lsmb_lset_stats: tables taken over by derive, filter bytes and copy calls of this set's uploads
    uint64_t inherited = 0, up_bytes = 0, up_copies = 0;
    // lsmb_lset_add_batch: pinned staging (words in the arena's layout, CRC
    // segments and results) and the device side of the CRC check
    uint8_t* pin = nullptr;
    size_t pin_cap = 0;
    PinnedPool pin_retired;
    DevBuf segs;
    DevBuf bounds, desc, pfx;  // seal: the bound keys' bytes, LsetTable[], prefix pairs
    LsetRows rows{};
    // seal: the table id of every ordinal (row by row, each in its sealed
    // order) and the first ordinal of every row, base[nrows] = all tables
    std::vector<uint32_t> ids;
    uint64_t base[kLsetMaxRows + 1] = {0};
    hipStream_t ust = nullptr;  // uploads
};

namespace {

constexpr size_t kLsetChunkBytes = 4u << 20;

// 16-B-aligned device memory for one filter's words (a filter larger than a
// chunk gets a chunk of its own).
inline size_t lset_slot_bytes(uint64_t nw) { return (std::max<size_t>(nw * 8, 8) + 15) & ~(size_t)15; }

int lset_arena_alloc(lsmb_lset* ls, size_t bytes, void** out, uint32_t* chunk) {
    bytes = lset_slot_bytes(bytes / 8);
    if (!ls->own_tail || ls->chunk_used + bytes > ls->chunks.back()->buf.bytes) {
        if (ls->chunks.size() >= UINT32_MAX) return fail(LSMB_EINVAL, "level set arena is full");
        auto ch = std::make_shared<LsetChunk>();
        ch->dev = ls->c->dev;
        HIP_TRY(ch->buf.ensure(std::max(bytes, kLsetChunkBytes)));
        ls->chunks.push_back(std::move(ch));
        ls->chunk_used = 0;
        ls->own_tail = true;
    }
    *out = (uint8_t*)ls->chunks.back()->buf.p + ls->chunk_used;
    *chunk = (uint32_t)(ls->chunks.size() - 1);
    ls->chunk_used += bytes;
    return LSMB_OK;
}

int lset_add_common(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint8_t* words_le, uint32_t num_bits,
                    uint32_t k, const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if ((min_len && !min_key) || (max_len && !max_key)) return fail(LSMB_EINVAL, "null key range");
    if (min_len > UINT32_MAX || max_len > UINT32_MAX) return fail(LSMB_EINVAL, "range key too long");
    if (ls->row[row].size() >= UINT32_MAX) return fail(LSMB_EINVAL, "level set row %u is full", row);
    DevGuard g(ls->c->dev);
    const uint64_t nw = nwords64(num_bits);
    void* dw = nullptr;
    uint32_t chunk = 0;
    if (int rc = lset_arena_alloc(ls, nw * 8, &dw, &chunk)) return rc;
    if (nw) {
        HIP_TRY(hipMemcpyAsync(dw, words_le, nw * 8, hipMemcpyHostToDevice, ls->ust));
        HIP_TRY(hipStreamSynchronize(ls->ust));  // the caller's block is free to go
        ls->up_bytes += nw * 8;
        ls->up_copies++;
    }
    lsmb_lset::Table t;
    t.id = table_id;
    t.num_bits = num_bits;
    t.k = k;
    t.chunk = chunk;
    t.words = (const uint32_t*)dw;
    t.lo.assign(min_key, min_key + min_len);
    t.hi.assign(max_key, max_key + max_len);
    ls->row[row].push_back(std::move(t));
    ls->nrows = std::max(ls->nrows, row + 1);
    return LSMB_OK;
}

int lset_add_check(const lsmb_lset* ls, uint32_t row, uint32_t table_id) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return fail(LSMB_EINVAL, "level set is sealed: a new Version takes a new set");
    if (row >= kLsetMaxRows) return fail(LSMB_EINVAL, "row %u: a level set has %u rows", row, kLsetMaxRows);
    if (table_id == LSMB_LSET_NONE) return fail(LSMB_EINVAL, "table id 0xFFFFFFFF is the probe's 'no table' answer");
    return LSMB_OK;
}

int lset_probe_check(const lsmb_lset* ls) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (!ls->sealed) return fail(LSMB_EINVAL, "level set not sealed");
    return LSMB_OK;
}

}  // namespace

int lsmb_lset_open(lsmb_ctx* c, lsmb_lset** out) {
    if (!c || !out) return fail(LSMB_EINVAL, "null argument");
    *out = nullptr;
    DevGuard g(c->dev);
    lsmb_lset* ls = new lsmb_lset;
    ls->c = c;
    if (hipStreamCreateWithFlags(&ls->ust, hipStreamNonBlocking) != hipSuccess) {
        delete ls;
        return fail(LSMB_EHIP, "level set: stream creation failed");
    }
    *out = ls;
    return LSMB_OK;
}

void lsmb_lset_close(lsmb_lset* ls) {
    if (!ls) return;
    {
        DevGuard g(ls->c->dev);
        if (ls->ust) hipStreamSynchronize(ls->ust), hipStreamDestroy(ls->ust);
        ls->chunks.clear();  // each chunk goes with the last set holding it
        ls->segs.release();
        if (ls->pin) (void)hipHostFree(ls->pin);  // teardown
        ls->pin_retired.release();
        ls->bounds.release();
        ls->desc.release();
        ls->pfx.release();
    }
    delete ls;
}

int lsmb_lset_add(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint8_t* block, uint64_t len,
                  const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if (int rc = lset_add_check(ls, row, table_id)) return rc;
    uint32_t k, nb, nw;
    if (int rc = lsmb_deserialize_header(block, len, &k, &nb, &nw)) return rc;
    return lset_add_common(ls, row, table_id, block + 12, nb, k, min_key, min_len, max_key, max_len);
}

int lsmb_lset_add_words(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint64_t* words, uint32_t num_bits,
                        uint32_t num_hashes, const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key,
                        uint64_t max_len) {
    if (int rc = lset_add_check(ls, row, table_id)) return rc;
    if (!words && nwords64(num_bits)) return fail(LSMB_EINVAL, "null words");
    return lset_add_common(ls, row, table_id, (const uint8_t*)words, num_bits, num_hashes, min_key, min_len, max_key,
                           max_len);
}

int lsmb_lset_derive(const lsmb_lset* parent, const uint32_t* drop_ids, uint64_t ndrop, uint64_t* dropped,
                     lsmb_lset** out) {
    if (out) *out = nullptr;
    if (!parent || !out) return fail(LSMB_EINVAL, "null argument");
    if (!parent->sealed) return fail(LSMB_EINVAL, "derive from an unsealed level set");
    if (ndrop && !drop_ids) return fail(LSMB_EINVAL, "null drop_ids");
    std::vector<uint32_t> drop(drop_ids, drop_ids + ndrop);
    std::sort(drop.begin(), drop.end());
    lsmb_lset* ls = nullptr;
    if (int rc = lsmb_lset_open(parent->c, &ls)) return rc;
    // the surviving tables, each in its row, and only the chunks that hold one
    std::vector<uint32_t> remap(parent->chunks.size(), UINT32_MAX);
    uint64_t nd = 0;
    for (uint32_t r = 0; r < parent->nrows; r++)
        for (const auto& T : parent->row[r]) {
            if (std::binary_search(drop.begin(), drop.end(), T.id)) {
                nd++;
                continue;
            }
            if (remap[T.chunk] == UINT32_MAX) {
                remap[T.chunk] = (uint32_t)ls->chunks.size();
                ls->chunks.push_back(parent->chunks[T.chunk]);
            }
            ls->row[r].push_back(T);
            ls->row[r].back().chunk = remap[T.chunk];
            ls->inherited++;
        }
    ls->nrows = parent->nrows;
    if (dropped) *dropped = nd;
    *out = ls;
    return LSMB_OK;
}

namespace {

// One table of a batch after its host-side checks.
struct LsetBatchItem {
    uint32_t nb = 0, k = 0;
    uint64_t nw = 0;
    uint8_t* dw = nullptr;   // its slot in the arena
    uint32_t chunk = 0;
    size_t stage = 0;        // its words in the pinned staging
};

// A run of slots in one chunk: one host-to-device copy.
struct LsetBatchSpan {
    uint32_t chunk;
    uint8_t* lo;
    size_t bytes, stage;
};

int lset_batch_check_one(const lsmb_lset* ls, uint64_t ntab, uint32_t row, uint32_t id, const uint8_t* blocks,
                         const uint64_t* boff, const uint8_t* keys, const uint64_t* koff, LsetBatchItem* it) {
    if (int rc = lset_add_check(ls, row, id)) return rc;
    if (boff[1] < boff[0]) return fail(LSMB_EINVAL, "block offsets descend");
    uint32_t nw32 = 0;
    if (int rc = lsmb_deserialize_header(blocks ? blocks + boff[0] : nullptr, boff[1] - boff[0], &it->k, &it->nb, &nw32))
        return rc;
    it->nw = nw32;
    if (int rc = check_filter(it->nb, it->k)) return rc;
    if (koff[1] < koff[0] || koff[2] < koff[1]) return fail(LSMB_EINVAL, "key offsets descend");
    if (koff[2] > koff[0] && !keys) return fail(LSMB_EINVAL, "null key range");
    if (koff[1] - koff[0] > UINT32_MAX || koff[2] - koff[1] > UINT32_MAX) return fail(LSMB_EINVAL, "range key too long");
    if (ls->row[row].size() + ntab >= UINT32_MAX) return fail(LSMB_EINVAL, "level set row %u is full", row);
    return LSMB_OK;
}

int lset_pin_ensure(lsmb_lset* ls, size_t need) {
    if (need <= ls->pin_cap) return LSMB_OK;
    const size_t cap = std::max(need, ls->pin_cap + ls->pin_cap / 2);
    void* q = nullptr;
    if (hipHostMalloc(&q, cap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LSMB_ENOMEM, "level set: %llu bytes of pinned staging", (unsigned long long)cap);
    }
    ls->pin_retired.retire(ls->pin);  // freed at close
    ls->pin = (uint8_t*)q;
    ls->pin_cap = cap;
    return LSMB_OK;
}

// Slots, staging, copies and the CRC check of a batch whose headers passed.
// On any error the caller rolls the arena back.
int lset_batch_upload(lsmb_lset* ls, uint64_t ntab, const uint32_t* ids, const uint8_t* blocks, const uint64_t* boff,
                      const uint32_t* crcs, int32_t* status, std::vector<LsetBatchItem>& items, uint64_t* up_bytes,
                      uint64_t* up_copies) {
    // slots in the arena, 16-B aligned, and the runs they form per chunk
    std::vector<LsetBatchSpan> spans;
    size_t stage = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        LsetBatchItem& it = items[t];
        void* dw = nullptr;
        if (int rc = lset_arena_alloc(ls, it.nw * 8, &dw, &it.chunk)) return rc;
        it.dw = (uint8_t*)dw;
        const size_t slot = lset_slot_bytes(it.nw);
        if (spans.empty() || spans.back().chunk != it.chunk) spans.push_back(LsetBatchSpan{it.chunk, it.dw, 0, stage});
        it.stage = stage;
        spans.back().bytes += slot;
        stage += slot;
    }
    // the CRC segments (up to 128 KiB each: one wave per segment) and their results after the words
    std::vector<uint64_t> seg_of;
    if (crcs)
        for (uint64_t t = 0; t < ntab; t++)
            if (items[t].nw * 8 <= kCrcSegWaveMax) seg_of.push_back(t);
    const size_t nseg = seg_of.size();
    const size_t seg_at = stage, out_at = seg_at + nseg * sizeof(CrcSeg);
    if (int rc = lset_pin_ensure(ls, out_at + nseg * 4 + 16)) return rc;
    for (uint64_t t = 0; t < ntab; t++) {
        const LsetBatchItem& it = items[t];
        const size_t slot = lset_slot_bytes(it.nw);
        if (it.nw) memcpy(ls->pin + it.stage, blocks + boff[t] + 12, it.nw * 8);
        memset(ls->pin + it.stage + it.nw * 8, 0, slot - it.nw * 8);
    }
    for (const auto& sp : spans) {  // one copy per chunk touched
        HIP_TRY(hipMemcpyAsync(sp.lo, ls->pin + sp.stage, sp.bytes, hipMemcpyHostToDevice, ls->ust));
        (*up_copies)++;
    }
    for (uint64_t t = 0; t < ntab; t++) *up_bytes += items[t].nw * 8;
    if (nseg) {
        CrcSeg* hs = (CrcSeg*)(ls->pin + seg_at);
        for (size_t s = 0; s < nseg; s++) hs[s] = CrcSeg{items[seg_of[s]].dw, items[seg_of[s]].nw * 8};
        HIP_TRY(ls->segs.ensure(nseg * (sizeof(CrcSeg) + 4)));
        uint8_t* ds = (uint8_t*)ls->segs.p;
        uint32_t* dout = (uint32_t*)(ds + nseg * sizeof(CrcSeg));
        HIP_TRY(hipMemcpyAsync(ds, hs, nseg * sizeof(CrcSeg), hipMemcpyHostToDevice, ls->ust));
        if (int rc = crc32_seg_dev((const CrcSeg*)ds, nseg, dout, ls->ust)) return rc;
        HIP_TRY(hipMemcpyAsync(ls->pin + out_at, dout, nseg * 4, hipMemcpyDeviceToHost, ls->ust));
    }
    HIP_TRY(hipStreamSynchronize(ls->ust));  // the batch's one wait: the caller's blocks are free to go
    if (!crcs) return LSMB_OK;
    // the copies now in HBM, not the host bytes, are what probes will read
    std::vector<uint32_t> words_crc(ntab, 0);
    const uint32_t* hout = (const uint32_t*)(ls->pin + out_at);
    for (size_t s = 0; s < nseg; s++) words_crc[seg_of[s]] = hout[s];
    for (uint64_t t = 0; t < ntab; t++)
        if (items[t].nw * 8 > kCrcSegWaveMax)
            if (int rc = crc32_dev(ls->c, items[t].dw, items[t].nw * 8, 0, ls->ust, &words_crc[t])) return rc;
    int first = LSMB_OK;
    uint64_t f_len = 0;
    uint32_t f = 1u << 31;  // x^(8·f_len): the tables of a store mostly share one size
    for (uint64_t t = 0; t < ntab; t++) {
        if (items[t].nw * 8 != f_len) f = x8nmodp(f_len = items[t].nw * 8);
        const uint32_t got = multmodp(f, crc32_host(blocks + boff[t], 12, 0)) ^ words_crc[t];  // header ‖ words
        if (got == crcs[t]) continue;
        if (status) status[t] = LSMB_ECORRUPT;
        if (first == LSMB_OK)
            first = fail(LSMB_ECORRUPT,
                         "table %llu of the batch (id %u): bloom block CRC-32 mismatch: expected %08x, device copy %08x",
                         (unsigned long long)t, ids[t], crcs[t], got);
    }
    return first;
}

}  // namespace

int lsmb_lset_add_batch(lsmb_lset* ls, uint64_t ntab, const uint32_t* rows, const uint32_t* table_ids,
                        const uint8_t* blocks, const uint64_t* block_off, const uint32_t* crcs, const uint8_t* keys,
                        const uint64_t* key_off, int32_t* status) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return fail(LSMB_EINVAL, "level set is sealed: a new Version takes a new set");
    if (ntab == 0) return LSMB_OK;
    if (!rows || !table_ids || !block_off || !key_off) return fail(LSMB_EINVAL, "null argument");
    if (ntab >= UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-2 tables in one batch");
    // every header on the host first: nothing is allocated or uploaded for a batch that fails here
    std::vector<LsetBatchItem> items(ntab);
    int first_rc = LSMB_OK;
    uint64_t first_t = 0;
    std::string first_msg;
    for (uint64_t t = 0; t < ntab; t++) {
        const int rc = lset_batch_check_one(ls, ntab, rows[t], table_ids[t], blocks, block_off + t, keys,
                                            key_off + 2 * t, &items[t]);
        if (status) status[t] = rc;
        if (rc && first_rc == LSMB_OK) {
            first_rc = rc;
            first_t = t;
            first_msg = last_error();
        }
    }
    if (first_rc)
        return fail(first_rc, "table %llu of the batch (id %u): %s", (unsigned long long)first_t, table_ids[first_t],
                    first_msg.c_str());
    DevGuard g(ls->c->dev);
    const size_t chunks0 = ls->chunks.size(), used0 = ls->chunk_used;
    const bool own0 = ls->own_tail;
    uint64_t up_bytes = 0, up_copies = 0;
    if (int rc = lset_batch_upload(ls, ntab, table_ids, blocks, block_off, crcs, status, items, &up_bytes, &up_copies)) {
        // all or nothing: the bump pointer back, this call's chunks gone, no table appended
        const std::string msg = last_error();
        (void)hipStreamSynchronize(ls->ust);
        ls->chunks.resize(chunks0);
        ls->chunk_used = used0;
        ls->own_tail = own0;
        set_last_error(msg);
        return rc;
    }
    for (uint64_t t = 0; t < ntab; t++) {
        const LsetBatchItem& it = items[t];
        lsmb_lset::Table T;
        T.id = table_ids[t];
        T.num_bits = it.nb;
        T.k = it.k;
        T.chunk = it.chunk;
        T.words = (const uint32_t*)it.dw;
        const uint64_t* ko = key_off + 2 * t;
        if (ko[1] > ko[0]) T.lo.assign(keys + ko[0], keys + ko[1]);
        if (ko[2] > ko[1]) T.hi.assign(keys + ko[1], keys + ko[2]);
        ls->row[rows[t]].push_back(std::move(T));
        ls->nrows = std::max(ls->nrows, rows[t] + 1);
    }
    ls->up_bytes += up_bytes;
    ls->up_copies += up_copies;
    return LSMB_OK;
}

// Filters a batched build left on the set's device (lsmb_build_batch_dev: the
// outputs of src/compaction/scheduler.rs:147-177 pushed into the next Version
// without a trip through the host): the slots of the packed buffer are the
// arena's slots, so each run of tables landing in one chunk is one
// device-to-device copy.
int lsmb_lset_add_batch_dev(lsmb_lset* ls, uint64_t ntab, const uint32_t* rows, const uint32_t* table_ids,
                            const void* d_words, const uint64_t* word_off, const uint32_t* num_bits,
                            const uint32_t* num_hashes, const uint8_t* keys, const uint64_t* key_off, void* stream) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return fail(LSMB_EINVAL, "level set is sealed: a new Version takes a new set");
    if (ntab == 0) return LSMB_OK;
    if (!rows || !table_ids || !d_words || !word_off || !num_bits || !num_hashes || !key_off)
        return fail(LSMB_EINVAL, "null argument");
    if (ntab >= UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-2 tables in one batch");
    if (reinterpret_cast<uintptr_t>(d_words) & 15) return fail(LSMB_EINVAL, "d_words is not 16-byte aligned");
    // every table on the host first: nothing is allocated or copied for a batch that fails here
    uint64_t at = 0;  // the layout's word_off[t]
    auto off_check = [&](uint64_t t) {
        if (word_off[t] == at) return LSMB_OK;
        return fail(LSMB_EINVAL, "word_off[%llu] = %llu, lsmb_build_batch_layout gives %llu", (unsigned long long)t,
                    (unsigned long long)word_off[t], (unsigned long long)at);
    };
    for (uint64_t t = 0; t < ntab; t++) {
        const uint64_t* ko = key_off + 2 * t;
        int rc = off_check(t);
        if (!rc) rc = lset_add_check(ls, rows[t], table_ids[t]);
        if (!rc) rc = check_filter(num_bits[t], num_hashes[t]);
        if (!rc && (ko[1] < ko[0] || ko[2] < ko[1])) rc = fail(LSMB_EINVAL, "key offsets descend");
        if (!rc && ko[2] > ko[0] && !keys) rc = fail(LSMB_EINVAL, "null key range");
        if (!rc && (ko[1] - ko[0] > UINT32_MAX || ko[2] - ko[1] > UINT32_MAX)) rc = fail(LSMB_EINVAL, "range key too long");
        if (!rc && ls->row[rows[t]].size() + ntab >= UINT32_MAX) rc = fail(LSMB_EINVAL, "level set row %u is full", rows[t]);
        if (rc) {
            const std::string msg = last_error();
            return fail(rc, "table %llu of the batch (id %u): %s", (unsigned long long)t, table_ids[t], msg.c_str());
        }
        at += bb_slot_words(num_bits[t]);
    }
    if (int rc = off_check(ntab)) return rc;
    DevGuard g(ls->c->dev);
    hipStream_t st = pick_stream(ls->c, stream);
    const size_t chunks0 = ls->chunks.size(), used0 = ls->chunk_used;
    const bool own0 = ls->own_tail;
    struct Span {  // a run of slots in one chunk: one device-to-device copy
        uint32_t chunk;
        uint8_t* lo;
        size_t bytes, src;
    };
    std::vector<Span> spans;
    std::vector<LsetBatchItem> items(ntab);
    auto place = [&]() -> int {
        for (uint64_t t = 0; t < ntab; t++) {
            LsetBatchItem& it = items[t];
            it.nw = nwords64(num_bits[t]);
            void* dw = nullptr;
            if (int rc = lset_arena_alloc(ls, it.nw * 8, &dw, &it.chunk)) return rc;
            it.dw = (uint8_t*)dw;
            if (spans.empty() || spans.back().chunk != it.chunk)
                spans.push_back(Span{it.chunk, it.dw, 0, (size_t)word_off[t] * 8});
            spans.back().bytes += lset_slot_bytes(it.nw);
        }
        for (const Span& sp : spans)
            HIP_TRY(hipMemcpyAsync(sp.lo, (const uint8_t*)d_words + sp.src, sp.bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // the batch's one wait: the source buffer is free to go
        return LSMB_OK;
    };
    if (int rc = place()) {
        // all or nothing: the bump pointer back, this call's chunks gone, no table appended
        const std::string msg = last_error();
        (void)hipStreamSynchronize(st);
        ls->chunks.resize(chunks0);
        ls->chunk_used = used0;
        ls->own_tail = own0;
        set_last_error(msg);
        return rc;
    }
    for (uint64_t t = 0; t < ntab; t++) {
        lsmb_lset::Table T;
        T.id = table_ids[t];
        T.num_bits = num_bits[t];
        T.k = num_hashes[t];
        T.chunk = items[t].chunk;
        T.words = (const uint32_t*)items[t].dw;
        const uint64_t* ko = key_off + 2 * t;
        if (ko[1] > ko[0]) T.lo.assign(keys + ko[0], keys + ko[1]);
        if (ko[2] > ko[1]) T.hi.assign(keys + ko[1], keys + ko[2]);
        ls->row[rows[t]].push_back(std::move(T));
        ls->nrows = std::max(ls->nrows, rows[t] + 1);
    }
    return LSMB_OK;
}

int lsmb_lset_stats(const lsmb_lset* ls, uint64_t out[6]) {
    if (!ls || !out) return fail(LSMB_EINVAL, "null argument");
    uint64_t ntab = 0, fbytes = 0, cbytes = 0;
    for (uint32_t r = 0; r < ls->nrows; r++) {
        ntab += ls->row[r].size();
        for (const auto& T : ls->row[r]) fbytes += nwords64(T.num_bits) * 8;
    }
    for (const auto& ch : ls->chunks) cbytes += ch->buf.bytes;
    out[0] = ntab;
    out[1] = ls->inherited;
    out[2] = ls->up_bytes;
    out[3] = ls->up_copies;
    out[4] = cbytes;
    out[5] = fbytes;
    return LSMB_OK;
}

int lsmb_lset_seal(lsmb_lset* ls) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return LSMB_OK;
    // per row: sorted by min_key, ranges disjoint
    std::vector<uint32_t> order[kLsetMaxRows];
    uint64_t ntab = 0;
    for (uint32_t r = 0; r < ls->nrows; r++) {
        const auto& T = ls->row[r];
        std::vector<LsetRange> rg(T.size());
        for (size_t j = 0; j < T.size(); j++)
            rg[j] = LsetRange{T[j].lo.data(), T[j].lo.size(), T[j].hi.data(), T[j].hi.size(), T[j].id};
        LsetOrderError err;
        if (!lset_order_row(rg.data(), (uint32_t)rg.size(), &order[r], &err)) {
            if (err.inverted) return fail(LSMB_EINVAL, "level set row %u: table %u has min_key > max_key", r, err.id_a);
            return fail(LSMB_EINVAL, "level set row %u: tables %u and %u overlap (max_key of %u >= min_key of %u)", r,
                        err.id_a, err.id_b, err.id_a, err.id_b);
        }
        ntab += T.size();
    }
    // the bound keys' bytes, the descriptors and the search prefixes, each row's
    // tables in sorted order, rows back to back
    std::vector<uint8_t> blob;
    std::vector<LsetTable> d;
    std::vector<ulonglong2> px;
    d.reserve(ntab);
    px.reserve(ntab);
    for (uint32_t r = 0; r < ls->nrows; r++)
        for (uint32_t j : order[r]) {
            const auto& S = ls->row[r][j];
            LsetTable t;
            memset(&t, 0, sizeof t);
            t.words32 = S.words;
            t.lo = (const uint8_t*)(uintptr_t)blob.size();  // offsets until the blob has its address
            blob.insert(blob.end(), S.lo.begin(), S.lo.end());
            t.hi = (const uint8_t*)(uintptr_t)blob.size();
            blob.insert(blob.end(), S.hi.begin(), S.hi.end());
            const HostPfx16 pl = host_prefix16(S.lo.data(), S.lo.size()), ph = host_prefix16(S.hi.data(), S.hi.size());
            t.lo_w0 = pl.w0;
            t.lo_w1 = pl.w1;
            t.md = Mod32::make(S.num_bits ? S.num_bits : 1);
            t.lo_len = (uint32_t)S.lo.size();
            t.hi_len = (uint32_t)S.hi.size();
            t.num_bits = S.num_bits;
            t.k = S.k;
            t.id = S.id;
            d.push_back(t);
            ulonglong2 q;
            q.x = ph.w0;
            q.y = ph.w1;
            px.push_back(q);
        }
    DevGuard g(ls->c->dev);
    HIP_TRY(ls->bounds.ensure(blob.size() + 16));
    HIP_TRY(ls->desc.ensure(std::max<size_t>(d.size(), 1) * sizeof(LsetTable)));
    HIP_TRY(ls->pfx.ensure(std::max<size_t>(px.size(), 1) * sizeof(ulonglong2)));
    const uint8_t* base = (const uint8_t*)ls->bounds.p;
    for (auto& t : d) {
        t.lo = base + (uintptr_t)t.lo;
        t.hi = base + (uintptr_t)t.hi;
    }
    if (!blob.empty()) HIP_TRY(hipMemcpyAsync(ls->bounds.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ls->ust));
    if (!d.empty()) {
        HIP_TRY(hipMemcpyAsync(ls->desc.p, d.data(), d.size() * sizeof(LsetTable), hipMemcpyHostToDevice, ls->ust));
        HIP_TRY(hipMemcpyAsync(ls->pfx.p, px.data(), px.size() * sizeof(ulonglong2), hipMemcpyHostToDevice, ls->ust));
    }
    HIP_TRY(hipStreamSynchronize(ls->ust));  // blob, d and px are host temporaries
    memset(&ls->rows, 0, sizeof ls->rows);
    ls->rows.nrows = ls->nrows;
    uint64_t at = 0;
    for (uint32_t r = 0; r < ls->nrows; r++) {
        const uint32_t m = (uint32_t)ls->row[r].size();
        if (m) {
            ls->rows.row[r].hi_pfx = (const ulonglong2*)ls->pfx.p + at;
            ls->rows.row[r].tab = (const LsetTable*)ls->desc.p + at;
        }
        ls->rows.row[r].ntab = m;
        ls->base[r] = at;
        at += m;
    }
    for (uint32_t r = ls->nrows; r <= kLsetMaxRows; r++) ls->base[r] = at;
    ls->ids.resize(d.size());
    for (size_t g = 0; g < d.size(); g++) ls->ids[g] = d[g].id;
    ls->sealed = true;
    return LSMB_OK;
}

int lsmb_lset_rows(const lsmb_lset* ls) { return ls ? (int)ls->nrows : 0; }

uint64_t lsmb_lset_tables(const lsmb_lset* ls, uint32_t row) {
    return ls && row < kLsetMaxRows ? (uint64_t)ls->row[row].size() : 0;
}

int lsmb_lset_probe_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                        void* d_out, void* stream) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n == 0 || ls->nrows == 0) return LSMB_OK;
    if (!d_out || !d_data) return fail(LSMB_EINVAL, "null keys or output");
    DevGuard g(ls->c->dev);
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    HIP_TRY(launch_lset_probe(kb, ls->rows, (uint32_t*)d_out, ls->c->num_cus, pick_stream(ls->c, stream)));
    return LSMB_OK;
}

int lsmb_lset_probe(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                    uint32_t* out) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n == 0 || ls->nrows == 0) return LSMB_OK;
    if (!out || (!data && (offsets ? offsets[n] > offsets[0] : key_len > 0)))
        return fail(LSMB_EINVAL, "null keys or output");
    lsmb_ctx* c = ls->c;
    DevGuard g(c->dev);
    const uint64_t obytes = (uint64_t)ls->nrows * n * 4;
    HIP_TRY(c->out.ensure(obytes));
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    HIP_TRY(launch_lset_probe(kb, ls->rows, (uint32_t*)c->out.p, c->num_cus, c->st));
    HIP_TRY(hipMemcpyAsync(out, c->out.p, obytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

uint64_t lsmb_lset_total_tables(const lsmb_lset* ls) { return ls && ls->sealed ? ls->base[ls->nrows] : 0; }

int lsmb_lset_table_order(const lsmb_lset* ls, uint32_t* ids, uint64_t* row_base) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (ids && !ls->ids.empty()) memcpy(ids, ls->ids.data(), ls->ids.size() * sizeof(uint32_t));
    if (row_base) memcpy(row_base, ls->base, ((size_t)ls->nrows + 1) * sizeof(uint64_t));
    return LSMB_OK;
}

uint64_t lsmb_lset_lists_work_bytes(const lsmb_lset* ls, uint64_t n) {
    if (!ls || !ls->sealed || n > UINT32_MAX) return 0;
    return lset_lists_plan(n, ls->nrows, ls->base[ls->nrows]).work_bytes;
}

// The argument checks shared by both lists entry points; G = all tables.
static int lset_lists_check(const lsmb_lset* ls, uint64_t n, const void* starts, const void* index, uint64_t cap) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n > UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-1 keys (the lists hold 32-bit indices)");
    if (ls->base[ls->nrows] > UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-1 tables");
    if (!starts || (cap && !index)) return fail(LSMB_EINVAL, "null output");
    return LSMB_OK;
}

int lsmb_lset_probe_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                              void* d_starts, void* d_index, uint64_t cap, void* d_work, uint64_t work_bytes,
                              void* stream) {
    if (int rc = lset_lists_check(ls, n, d_starts, d_index, cap)) return rc;
    const uint64_t G = ls->base[ls->nrows];
    if (n && G) {
        if (!d_data) return fail(LSMB_EINVAL, "null keys");
        if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15))
            return fail(LSMB_EINVAL, "null or misaligned workspace (16-byte alignment)");
        const uint64_t need = lset_lists_plan(n, ls->nrows, G).work_bytes;
        if (work_bytes < need)
            return fail(LSMB_EINVAL, "workspace of %llu bytes, lsmb_lset_lists_work_bytes asks for %llu",
                        (unsigned long long)work_bytes, (unsigned long long)need);
    }
    DevGuard g(ls->c->dev);
    const hipStream_t st = pick_stream(ls->c, stream);
    if (n == 0 || G == 0) {
        HIP_TRY(hipMemsetAsync(d_starts, 0, (G + 1) * 8, st));
        return LSMB_OK;
    }
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    HIP_TRY(launch_lset_lists(kb, ls->rows, G, (uint64_t*)d_starts, (uint32_t*)d_index, cap, d_work, work_bytes,
                              ls->c->num_cus, st));
    return LSMB_OK;
}

int lsmb_lset_probe_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                          uint64_t* starts, uint32_t* index, uint64_t cap) {
    if (int rc = lset_lists_check(ls, n, starts, index, cap)) return rc;
    if (n && !data && (offsets ? offsets[n] > offsets[0] : key_len > 0)) return fail(LSMB_EINVAL, "null keys");
    const uint64_t G = ls->base[ls->nrows];
    memset(starts, 0, (G + 1) * 8);
    if (n == 0 || G == 0) return LSMB_OK;
    lsmb_ctx* c = ls->c;
    DevGuard g(c->dev);
    // the context's output scratch, carved: workspace | starts | index (no
    // list entry beyond one per row and key)
    const LsetListsPlan pl = lset_lists_plan(n, ls->nrows, G);
    const uint64_t dcap = std::min<uint64_t>(cap, pl.pairs);
    const uint64_t sbytes = ((G + 1) * 8 + kLlAlign - 1) / kLlAlign * kLlAlign;
    HIP_TRY(c->out.ensure(pl.work_bytes + sbytes + std::max<uint64_t>(dcap, 1) * 4));
    uint8_t* w = (uint8_t*)c->out.p;
    uint64_t* d_starts = (uint64_t*)(w + pl.work_bytes);
    uint32_t* d_index = (uint32_t*)(w + pl.work_bytes + sbytes);
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    HIP_TRY(launch_lset_lists(kb, ls->rows, G, d_starts, d_index, dcap, w, pl.work_bytes, c->num_cus, c->st));
    HIP_TRY(hipMemcpyAsync(starts, d_starts, (G + 1) * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    const uint64_t got = std::min<uint64_t>(starts[G], dcap);
    if (got) {
        HIP_TRY(hipMemcpyAsync(index, d_index, got * 4, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    return LSMB_OK;
}

}  // extern "C"

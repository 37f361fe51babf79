// partition_stage_test.hip — the partitioned build, stage by stage.
//
// The suite checks the partitioned build through whole builds: keys in, filter
// words compared with the oracle.  At the ~52 % fill of those filters a
// position pass A drops is hidden half the time by another key's bit, nothing
// shows that the overflow tiers are reached, and the edges of the pass A ->
// pass B contract cannot be steered to through
// hashing.  This program runs the two passes apart:
//
//   pass A   k_bin over the harness's own buffers (garbage in regions, counts,
//            lists and a fresh build's words; guards behind every buffer),
//            then every region, count, list and overflow word is decoded and
//            compared, as multisets per slice, with the positions the keys
//            must produce; then pass B (+ k_ovf_apply) and every word against
//            the oracle's build (filters up to 1e9 bits);
//   records  hash_records' (r, s, c) against literal arithmetic;
//   pass B   synthetic regions and counts at the contract's edges through
//            launch_pass_b, every word against a host OR;
//   selftest (--selftest, host only) the pass A checker on a host binning of
//            the expected positions: accepted as it is, rejected after each of
//            nine single mutations.
//
// bloom_build.hip is included, so its kernels and launch helpers inside
// `namespace lsmb { namespace {` are this translation unit's own.  Expected
// values never pass through xxh3.hpp or bloom_math.hpp: hashes come from the
// oracle, positions are the literal (h1 + i*h2 mod 2^64) % num_bits.  Only the
// layout constants and PassA's field meanings are shared with the product;
// decode_segment is the one place that knows the segment format.
//
// Exit 0: every case good; 1: a case failed; 2: a HIP call failed (nothing is
// launched after it).
#include "../../storage-engine_amd/csrc/bloom_build.hip"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <iterator>
#include <random>
#include <string>
#include <utility>

extern "C" {
void oracle_xxh3_128(const uint8_t* in, size_t len, uint64_t* lo, uint64_t* hi);
void oracle_bloom_build_fixed(const uint8_t* keys, uint32_t key_len, uint64_t n, uint32_t num_bits, uint32_t k,
                              uint64_t* words);
void oracle_bloom_build_var(const uint8_t* data, const uint64_t* offsets, uint64_t n, uint32_t num_bits, uint32_t k,
                            uint64_t* words);
void oracle_gen_key16(uint64_t seed, uint64_t first, uint64_t n, uint8_t* out);
}

namespace lsmb {
namespace {

constexpr int kCus = 4;  // plan_partition's num_cus: small grids and regions
constexpr uint32_t kBitsC2 = 100u * (1u << 20) + 12345u;
constexpr uint32_t kBits21 = 1200u * (1u << 20) + 77u;
constexpr size_t kGuard = 4096;
constexpr uint8_t kGuardByte = 0xC3, kGarbage = 0xA5;
constexpr uint32_t kGarbage32 = 0xA5A5A5A5u;

// ---------------------------------------------------------------- the segment format
// Entry e of a 64-byte segment: bits sl * (e >> 3) of u64 word e & 7.  False
// when a word has bits above its three offsets (an offset >= 2^sl).
bool decode_segment(const uint64_t* seg, uint32_t sl, uint32_t out[kSegEntries]) {
    const uint64_t mask = (1ull << sl) - 1;
    bool ok = true;
    for (int e = 0; e < kSegEntries; e++) out[e] = (uint32_t)((seg[e & 7] >> (sl * (uint32_t)(e >> 3))) & mask);
    for (int w = 0; w < kSegWords; w++)
        if (seg[w] >> (3 * sl)) ok = false;
    return ok;
}
// (the selftest's host binning and pass B's synthetic regions)
void encode_segment(const uint32_t in[kSegEntries], uint32_t sl, uint64_t* seg) {
    for (int w = 0; w < kSegWords; w++)
        seg[w] = (uint64_t)in[w] | ((uint64_t)in[w + 8] << sl) | ((uint64_t)in[w + 16] << (2 * sl));
}

// ---------------------------------------------------------------- the pass A checker
// What one k_bin launch left behind, on the host.
struct PassAView {
    uint32_t num_bits, sl, nbins, grid, cap, b0, nb;
    bool fresh;                   // the LIST form
    const uint64_t* regions;      // [grid][nbins][cap][kSegSlotWords]
    const uint32_t* counts;       // [nbins][grid]
    const uint32_t* ovl;          // fresh: this sweep's lists [grid][kOvfListCap]
    const uint32_t* ovn;          //        and their lengths [grid]
    std::vector<uint32_t> side;   // positions this launch set in ovf (fresh) or the words, sorted
    uint32_t unit0;               // fresh: dirty marks of the 2^20-bit units
    std::vector<uint32_t> dirty;  //        [unit0, unit0 + size) that hold the sweep's slices
    uint64_t words_touched;       // fresh: filter words that no longer hold the garbage
    bool guards_ok;
};
struct Tiers {
    uint64_t region = 0, pad = 0, list = 0, side = 0, at_cap = 0, full_lists = 0;
    int64_t culprit = -1;  // a failed check: the position it is about (run_pass_a names its key and workgroup)
};

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// E: the sweep's expected positions, sorted, one entry per (key, i).
bool check_pass_a(const PassAView& v, const uint32_t* E, size_t nE, Tiers& t, std::string& why) {
    const uint64_t lo = (uint64_t)v.b0 << v.sl;
    const uint64_t hi = std::min((uint64_t)(v.b0 + v.nb) << v.sl, (uint64_t)v.num_bits);
    for (uint32_t b = v.b0; b < v.b0 + v.nb; b++)
        for (uint32_t w = 0; w < v.grid; w++) {
            const uint32_t c = v.counts[(uint64_t)b * v.grid + w];
            if (c > v.cap) {
                why = fmt("counts[slice %u][workgroup %u] = %u > cap_segs %u (never stored?)", b, w, c, v.cap);
                return false;
            }
        }
    if (v.fresh)
        for (uint32_t w = 0; w < v.grid; w++)
            if (v.ovn[w] > kOvfListCap) {
                why = fmt("ovn[workgroup %u] = %u > kOvfListCap", w, v.ovn[w]);
                return false;
            }
    std::vector<uint32_t> D;
    D.reserve(nE + (size_t)v.nb * v.grid * kSegEntries);
    std::vector<std::pair<uint32_t, uint32_t>> pads;  // (entry 0's position, trailing copies of it) per region
    for (uint32_t b = v.b0; b < v.b0 + v.nb; b++)
        for (uint32_t w = 0; w < v.grid; w++) {
            const uint32_t c = v.counts[(uint64_t)b * v.grid + w];
            if (c == v.cap) t.at_cap++;
            const uint64_t* r = v.regions + ((uint64_t)w * v.nbins + b) * v.cap * kSegSlotWords;
            for (uint32_t s = 0; s < c; s++) {
                uint32_t off[kSegEntries];
                if (!decode_segment(r + (uint64_t)s * kSegSlotWords, v.sl, off)) {
                    why = fmt("region (slice %u, workgroup %u) segment %u: an offset >= 2^%u", b, w, s, v.sl);
                    return false;
                }
                for (int e = 0; e < kSegEntries; e++) {
                    const uint64_t p = ((uint64_t)b << v.sl) | off[e];
                    if (p >= v.num_bits) {
                        why = fmt("region (slice %u, workgroup %u) segment %u entry %d: position %llu >= num_bits", b, w,
                                  s, e, (unsigned long long)p);
                        return false;
                    }
                    D.push_back((uint32_t)p);
                }
                if (s + 1 == c) {
                    uint32_t npad = 0;
                    while (npad < kSegEntries - 1 && off[kSegEntries - 1 - npad] == off[0]) npad++;
                    if (npad) pads.push_back({(uint32_t)(((uint64_t)b << v.sl) | off[0]), npad});
                }
            }
            t.region += (uint64_t)c * kSegEntries;
        }
    if (v.fresh)
        for (uint32_t w = 0; w < v.grid; w++) {
            for (uint32_t i = 0; i < v.ovn[w]; i++) {
                const uint32_t p = v.ovl[(uint64_t)w * kOvfListCap + i];
                if (p < lo || p >= hi) {
                    why = fmt("list of workgroup %u entry %u: position %u (slice %u) outside the sweep's slices [%u, %u)",
                              w, i, p, p >> v.sl, v.b0, v.b0 + v.nb);
                    return false;
                }
                D.push_back(p);
            }
            t.list += v.ovn[w];
            if (v.ovn[w] == kOvfListCap) t.full_lists++;
        }
    std::sort(D.begin(), D.end());
    std::sort(pads.begin(), pads.end());
    // D - E (runs) and E - D (as a set)
    std::vector<uint32_t> deficit;
    size_t i = 0, j = 0;
    while (i < D.size() || j < nE) {
        const uint32_t p = (j >= nE || (i < D.size() && D[i] < E[j])) ? D[i] : E[j];
        size_t nd = 0, ne = 0;
        while (i < D.size() && D[i] == p) i++, nd++;
        while (j < nE && E[j] == p) j++, ne++;
        if (nd < ne) deficit.push_back(p);
        if (nd > ne) {
            // only pad copies may be in excess: trailing copies of entry 0 in a region's last segment
            size_t credit = 0;
            for (auto it = std::lower_bound(pads.begin(), pads.end(), std::make_pair(p, 0u));
                 it != pads.end() && it->first == p; ++it)
                credit += it->second;
            if (nd - ne > credit) {
                t.culprit = p;
                why = fmt("position %u (slice %u, offset %u): %zu stored, %zu expected, %zu of them pad copies at the most "
                          "(spurious or duplicated)",
                          p, p >> v.sl, p & ((1u << v.sl) - 1), nd, ne, credit);
                return false;
            }
            t.pad += nd - ne;
        }
    }
    t.region -= t.pad;
    if (v.fresh && !deficit.empty() && t.full_lists == 0) {
        const uint32_t p = deficit[0];
        t.culprit = p;
        why = fmt("position %u (slice %u, offset %u) is in no region and no list, and no list is full (dropped; %zu such)",
                  p, p >> v.sl, p & ((1u << v.sl) - 1), deficit.size());
        return false;
    }
    // the overflow bits are exactly the positions stored nowhere else
    for (size_t a = 0, b = 0; a < deficit.size() || b < v.side.size();) {
        if (b >= v.side.size() || (a < deficit.size() && deficit[a] < v.side[b])) {
            const uint32_t p = deficit[a];
            t.culprit = p;
            why = fmt("position %u (slice %u, offset %u) is in no region, no list and not set in %s (dropped)", p,
                      p >> v.sl, p & ((1u << v.sl) - 1), v.fresh ? "ovf" : "the words");
            return false;
        }
        if (a >= deficit.size() || v.side[b] < deficit[a]) {
            const uint32_t p = v.side[b];
            why = fmt("bit %u (slice %u) is set in %s but its position is stored elsewhere or expected nowhere (spurious)",
                      p, p >> v.sl, v.fresh ? "ovf" : "the words");
            return false;
        }
        a++, b++;
    }
    t.side = v.side.size();
    if (v.fresh) {
        for (size_t u = 0; u < v.dirty.size(); u++) {
            const uint64_t ulo = (uint64_t)(v.unit0 + u) << kSliceLog2, uhi = ulo + (1ull << kSliceLog2);
            auto it = std::lower_bound(v.side.begin(), v.side.end(), (uint32_t)ulo);
            const bool want = it != v.side.end() && *it < uhi;
            if ((v.dirty[u] != 0) != want) {
                why = fmt("dirty[unit %zu] = %u, but the unit holds %s overflow bit", v.unit0 + u, v.dirty[u],
                          want ? "an" : "no");
                return false;
            }
        }
        if (v.words_touched) {
            why = fmt("pass A touched %llu filter words of a fresh build", (unsigned long long)v.words_touched);
            return false;
        }
    }
    if (!v.guards_ok) {
        why = "a guard strip behind a buffer was written";
        return false;
    }
    return true;
}

void print_tiers(const char* name, uint32_t sweep, const Tiers& t) {
    printf("tiers %s sweep %u: region_entries=%llu pad_entries=%llu list_entries=%llu side_positions=%llu "
           "regions_at_cap=%llu full_lists=%llu\n",
           name, sweep, (unsigned long long)t.region, (unsigned long long)t.pad, (unsigned long long)t.list,
           (unsigned long long)t.side, (unsigned long long)t.at_cap, (unsigned long long)t.full_lists);
}

// ---------------------------------------------------------------- keys and expected values
struct Keys {
    std::vector<uint8_t> data;      // the keys' bytes, from `skew` on
    std::vector<uint64_t> offsets;  // var-len: n + 1 offsets into data + skew
    uint32_t key_len = 16;
    uint64_t n = 0;
    size_t skew = 0;  // 1: a fixed-length batch on an unaligned base
    const uint8_t* key(uint64_t i, size_t* len) const {
        if (!offsets.empty()) {
            *len = (size_t)(offsets[i + 1] - offsets[i]);
            return data.data() + skew + offsets[i];
        }
        *len = key_len;
        return data.data() + skew + i * key_len;
    }
};

Keys keys16(uint64_t seed, uint64_t n) {
    Keys ks;
    ks.n = n;
    ks.data.resize(16 * n);
    oracle_gen_key16(seed, 0, n, ks.data.data());
    return ks;
}
Keys keys_fixed(uint64_t seed, uint64_t n, uint32_t len, size_t skew) {
    Keys ks;
    ks.n = n, ks.key_len = len, ks.skew = skew;
    ks.data.resize(skew + (size_t)len * n);
    std::mt19937_64 rng(seed);
    for (auto& b : ks.data) b = (uint8_t)rng();
    return ks;
}
Keys keys_var(uint64_t seed, uint64_t n) {  // 0 .. 300 bytes, every XXH3 length class
    Keys ks;
    ks.n = n;
    ks.offsets.resize(n + 1);
    std::mt19937_64 rng(seed);
    uint64_t o = 0;
    for (uint64_t i = 0; i < n; i++) {
        ks.offsets[i] = o;
        o += rng() % 301;
    }
    ks.offsets[n] = o;
    ks.data.resize(o);
    for (auto& b : ks.data) b = (uint8_t)rng();
    return ks;
}

struct Hashes {
    std::vector<uint64_t> h1, h2;
};
Hashes hash_keys(const Keys& ks) {
    Hashes h;
    h.h1.resize(ks.n), h.h2.resize(ks.n);
    for (uint64_t i = 0; i < ks.n; i++) {
        size_t len;
        const uint8_t* p = ks.key(i, &len);
        oracle_xxh3_128(p, len, &h.h1[i], &h.h2[i]);
    }
    return h;
}
uint32_t position(uint64_t h1, uint64_t h2, uint32_t i, uint32_t num_bits) {
    const uint64_t x = (uint64_t)((unsigned __int128)h1 + (unsigned __int128)i * h2);  // wraps at 2^64
    return (uint32_t)(x % num_bits);
}
// every (key, i) position, sorted
std::vector<uint32_t> all_positions(const Hashes& h, uint32_t num_bits, uint32_t k) {
    std::vector<uint32_t> p;
    p.reserve(h.h1.size() * k);
    for (size_t i = 0; i < h.h1.size(); i++)
        for (uint32_t q = 0; q < k; q++) p.push_back(position(h.h1[i], h.h2[i], q, num_bits));
    std::sort(p.begin(), p.end());
    return p;
}
// the part of sorted positions inside slices [b0, b0 + nb)
std::pair<const uint32_t*, size_t> sweep_range(const std::vector<uint32_t>& pos, uint32_t sl, uint32_t b0, uint32_t nb) {
    const uint64_t lo = (uint64_t)b0 << sl, hi = (uint64_t)(b0 + nb) << sl;
    const auto a = std::lower_bound(pos.begin(), pos.end(), (uint32_t)std::min<uint64_t>(lo, 0xFFFFFFFFull));
    const auto b = hi > 0xFFFFFFFFull ? pos.end() : std::lower_bound(pos.begin(), pos.end(), (uint32_t)hi);
    return {pos.data() + (a - pos.begin()), (size_t)(b - a)};
}

int g_cases = 0, g_bad = 0;
void verdict(const char* group, const std::string& name, bool ok, const std::string& why) {
    g_cases++;
    if (ok) {
        printf("case %s/%s: ok\n", group, name.c_str());
    } else {
        g_bad++;
        printf("FAIL %s/%s: %s\n", group, name.c_str(), why.c_str());
    }
    fflush(stdout);
}

// ---------------------------------------------------------------- device plumbing
#define HIP_OK(call)                                                                               \
    do {                                                                                           \
        const hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            fflush(stdout);                                                                        \
            fflush(stderr);                                                                        \
            _exit(2); /* the first HIP error ends the run: nothing is launched after it */        \
        }                                                                                          \
    } while (0)

// A device buffer with a guard strip behind it.
struct DBuf {
    uint8_t* p = nullptr;
    size_t bytes = 0;
    void alloc(size_t n, int fill) {
        bytes = n;
        HIP_OK(hipMalloc((void**)&p, n + kGuard));
        if (n) HIP_OK(hipMemset(p, fill, n));
        HIP_OK(hipMemset(p + n, kGuardByte, kGuard));
    }
    bool guard_ok() const {
        std::vector<uint8_t> g(kGuard);
        HIP_OK(hipMemcpy(g.data(), p + bytes, kGuard, hipMemcpyDeviceToHost));
        for (uint8_t b : g)
            if (b != kGuardByte) return false;
        return true;
    }
    void free() {
        if (p) HIP_OK(hipFree(p));
        p = nullptr;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// unit_ne[u] += the words of 2^20-bit unit u that differ from pat (the harness's
// own kernel: which units of a 512 MiB buffer are worth copying back)
__global__ __launch_bounds__(256) void k_count_ne(const uint32_t* __restrict__ w, uint64_t n32, uint32_t pat,
                                                  uint32_t* __restrict__ unit_ne) {
    const uint64_t base = (uint64_t)blockIdx.x * kSliceWords32;
    uint32_t cnt = 0;
    for (uint32_t i = threadIdx.x; i < kSliceWords32 && base + i < n32; i += 256) cnt += w[base + i] != pat;
    if (cnt) atomicAdd(unit_ne + blockIdx.x, cnt);
}

std::vector<uint32_t> count_ne(const uint32_t* d_w, uint64_t n32, uint32_t units, uint32_t pat) {
    std::vector<uint32_t> ne(units, 0);
    if (!units) return ne;
    uint32_t* d_ne = nullptr;
    HIP_OK(hipMalloc((void**)&d_ne, units * 4));
    HIP_OK(hipMemset(d_ne, 0, units * 4));
    k_count_ne<<<dim3(units), dim3(256)>>>(d_w, n32, pat, d_ne);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(ne.data(), d_ne, units * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_ne));
    return ne;
}
// the set bits of a device word buffer, ascending (only the units that hold one are copied back)
std::vector<uint32_t> set_bits(const uint32_t* d_w, uint64_t n32, uint32_t units) {
    const std::vector<uint32_t> ne = count_ne(d_w, n32, units, 0u);
    std::vector<uint32_t> bits, buf(kSliceWords32);
    for (uint32_t u = 0; u < units; u++) {
        if (!ne[u]) continue;
        const uint64_t base = (uint64_t)u * kSliceWords32;
        const size_t nw = (size_t)std::min<uint64_t>(kSliceWords32, n32 - base);
        HIP_OK(hipMemcpy(buf.data(), d_w + base, nw * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nw; i++)
            for (uint32_t v = buf[i]; v; v &= v - 1)
                bits.push_back((uint32_t)((base + i) * 32 + (uint32_t)__builtin_ctz(v)));
    }
    return bits;
}

// ---------------------------------------------------------------- pass A on the device
enum class KeyKind { Fixed16, Records };
struct ACase {
    std::string name;
    uint32_t num_bits, k;
    bool fresh;
    bool pass_b;          // run pass B afterwards and compare with the oracle
    uint32_t want_sl, want_sweeps;  // the plan this case is meant to reach (0: not pinned)
    bool tiers;           // the first ceil(n / grid) keys are one key: every overflow tier must engage
};

struct Buffers {
    DBuf keys, offsets, hashes, regions, counts, words, ovf, dirty, ovl, ovn;
    bool guards_ok() const {
        return keys.guard_ok() && offsets.guard_ok() && hashes.guard_ok() && regions.guard_ok() && counts.guard_ok() &&
               words.guard_ok() && ovf.guard_ok() && dirty.guard_ok() && ovl.guard_ok() && ovn.guard_ok();
    }
    void free() {
        for (DBuf* b : {&keys, &offsets, &hashes, &regions, &counts, &words, &ovf, &dirty, &ovl, &ovn}) b->free();
    }
};

// hash_records' output against the record's definition, computed literally
bool check_records(const Buffers& B, const Hashes& h, uint32_t d, uint32_t k, std::string& why) {
    const size_t n = h.h1.size();
    std::vector<uint32_t> rec(3 * n);
    HIP_OK(hipMemcpy(rec.data(), B.hashes.p, rec.size() * 4, hipMemcpyDeviceToHost));
    const uint32_t steps = k < 2 ? 0 : (k - 1 < 31 ? k - 1 : 31);
    uint32_t c_or = 0, c_and = ~0u;
    for (size_t i = 0; i < n; i++) {
        uint32_t carries = 0;
        unsigned __int128 x = h.h1[i];
        for (uint32_t s = 0; s < steps; s++) {
            x += h.h2[i];
            if (x >> 64) carries |= 1u << s;
            x = (uint64_t)x;
        }
        const uint32_t want[3] = {(uint32_t)(h.h1[i] % d), (uint32_t)(h.h2[i] % d), carries};
        c_or |= carries, c_and &= carries;
        for (int f = 0; f < 3; f++)
            if (rec[3 * i + f] != want[f]) {
                why = fmt("record of key %zu field %c: got %u want %u", i, "rsc"[f], rec[3 * i + f], want[f]);
                return false;
            }
    }
    const uint32_t all = steps ? (steps == 32 ? ~0u : (1u << steps) - 1) : 0;
    if (n > 1000 && (c_or != all || c_and != 0)) {  // every carry bit seen set and clear
        why = fmt("the keys do not exercise every carry bit (or %08x and %08x)", c_or, c_and);
        return false;
    }
    return true;
}

void run_pass_a(const char* group, const ACase& c, Keys keys, KeyKind kind) {
    const uint64_t n = keys.n;
    const PartitionPlan pl = plan_partition(c.num_bits, c.k, n, kCus);
    const uint32_t sl = pl.slice_log2;
    const uint64_t nw32 = 2 * (((uint64_t)c.num_bits + 63) / 64);
    const uint32_t units = (uint32_t)((nw32 + kSliceWords32 - 1) / kSliceWords32);
    const bool list = c.fresh && c.k == 7;
    printf("plan %s: n=%llu bits=%u k=%u %s slice_log2=%u nbins=%u sweeps=%u bins_per_sweep=%u ring=%u grid=%u "
           "cap_segs=%u keys_per_lane=%u\n",
           c.name.c_str(), (unsigned long long)n, c.num_bits, c.k, list ? "fresh" : "accumulate", sl, pl.nbins, pl.sweeps,
           pl.bins_per_sweep, pl.ring, pl.grid, pl.cap_segs, pl.keys_per_lane);
    if ((c.want_sl && sl != c.want_sl) || (c.want_sweeps && pl.sweeps != c.want_sweeps)) {
        verdict(group, c.name, false, fmt("the plan no longer has the shape this case is for (slice_log2 %u, %u sweeps)",
                                          c.want_sl, c.want_sweeps));
        return;
    }
    if (c.fresh != list) {
        verdict(group, c.name, false, "a fresh pass A exists for k = 7 only");
        return;
    }
    if (c.tiers) {
        // the first workgroup's whole key range is key 0
        const uint64_t m = (n + pl.grid - 1) / pl.grid;
        for (uint64_t i = 1; i < m; i++) memcpy(&keys.data[16 * i], &keys.data[0], 16);
    }
    const Hashes h = hash_keys(keys);
    if (c.tiers) {
        // From the plan alone: workgroup 0 must overfill one slice's region and
        // ring, and leave more than a full list over.
        const uint64_t m = (n + pl.grid - 1) / pl.grid;
        std::vector<uint32_t> sl_of;
        for (uint32_t q = 0; q < c.k; q++) sl_of.push_back(position(h.h1[0], h.h2[0], q, c.num_bits) >> sl);
        uint64_t most = 0;
        for (uint32_t s : sl_of) most = std::max<uint64_t>(most, (uint64_t)std::count(sl_of.begin(), sl_of.end(), s) * m);
        const uint64_t held = (uint64_t)pl.cap_segs * kSegEntries + pl.ring;
        printf("tiers %s precondition: workgroup 0 sends %llu positions to one slice, region + ring hold %llu, "
               "kOvfListCap %u\n",
               c.name.c_str(), (unsigned long long)most, (unsigned long long)held, kOvfListCap);
        if (!(most > held && most - held > kOvfListCap)) {
            verdict(group, c.name, false, "the plan no longer forces this input through every overflow tier");
            return;
        }
    }
    const std::vector<uint32_t> pos = all_positions(h, c.num_bits, c.k);

    const bool aligned16 = kind == KeyKind::Fixed16;
    const WorkspaceBytes need = workspace_bytes(BuildStrategy::Partition, pl, TiledPlan{}, c.num_bits, c.k, n, aligned16, c.fresh);
    Buffers B;
    B.keys.alloc(keys.data.size(), 0);
    if (!keys.data.empty()) HIP_OK(hipMemcpy(B.keys.p, keys.data.data(), keys.data.size(), hipMemcpyHostToDevice));
    B.offsets.alloc(keys.offsets.size() * 8, 0);
    if (!keys.offsets.empty()) HIP_OK(hipMemcpy(B.offsets.p, keys.offsets.data(), keys.offsets.size() * 8, hipMemcpyHostToDevice));
    B.hashes.alloc(need.hashes, kGarbage);
    B.regions.alloc(need.regions, kGarbage);
    B.counts.alloc(need.counts, kGarbage);
    B.words.alloc(nw32 * 4, list ? kGarbage : 0);  // a fresh build's words are output-only
    B.ovf.alloc(need.ovf, 0);                      // all-zero between builds (their contract)
    B.dirty.alloc(need.dirty, 0);
    B.ovl.alloc(need.ovl, kGarbage);
    B.ovn.alloc(need.ovn, kGarbage);
    PartitionWorkspace ws;
    ws.hashes = B.hashes.as<uint4>(), ws.regions = B.regions.as<uint64_t>(), ws.counts = B.counts.as<uint32_t>();
    ws.ovf = B.ovf.as<uint32_t>(), ws.dirty = B.dirty.as<uint32_t>(), ws.ovl = B.ovl.as<uint32_t>();
    ws.ovn = B.ovn.as<uint32_t>(), ws.have = need;
    const Launch L{n,  c.num_bits, c.k,     (uint32_t)nw32, Mod32::make(c.num_bits), B.words.as<uint32_t>(), ws, kCus,
                   nullptr, nullptr, nullptr, pl, TiledPlan{}};

    bool ok = true;
    std::string why;
    if (kind == KeyKind::Records) {
        const KeyBatch kb{B.keys.p + keys.skew, keys.offsets.empty() ? nullptr : B.offsets.as<uint64_t>(), keys.key_len, n};
        HIP_OK(hash_records(kb, L));
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        ok = check_records(B, h, c.num_bits, c.k, why);
    }

    // launch_partition's choice of kernel
    const bool rec = kind == KeyKind::Records;
    const WalkKind walk = fits_walk32(c.num_bits)                 ? WalkKind::W32
                          : !rec && c.num_bits == kMersenneBits   ? WalkKind::Fold
                                                                  : WalkKind::W64;
    std::vector<uint64_t> regions(need.regions / 8);
    std::vector<uint32_t> counts(need.counts / 4), ovl, ovn, dirty(units, 0), dirty_prev(units, 0), side_prev;
    for (uint32_t sw = 0; ok && sw < pl.sweeps; sw++) {
        const PassA a = pass_a_args(L, sw);
        if ((size_t)(a.nb + 1) * (4 * a.ring + kBinExtraBytes) + kBinJobBytes > kLdsBytes) {
            ok = false, why = "the plan's rings do not fit the LDS";
            break;
        }
        if (rec)
            pick_k_bin<ks::Recs>(c.k, walk, pl.sweeps == 1, pl.keys_per_lane == 2, sl, list)<<<dim3(pl.grid), dim3(kBinBlock)>>>(
                ks::Recs{reinterpret_cast<const uint32_t*>(B.hashes.p)}, n, L.md, c.k, a);
        else
            pick_k_bin<Fixed16>(c.k, walk, pl.sweeps == 1, pl.keys_per_lane == 2, sl, list)<<<dim3(pl.grid), dim3(kBinBlock)>>>(
                Fixed16{B.keys.as<uint4>()}, n, L.md, c.k, a);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());

        PassAView v;
        v.num_bits = c.num_bits, v.sl = sl, v.nbins = pl.nbins, v.grid = pl.grid, v.cap = pl.cap_segs;
        v.b0 = a.b0, v.nb = a.nb, v.fresh = list;
        HIP_OK(hipMemcpy(regions.data(), B.regions.p, need.regions, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(counts.data(), B.counts.p, need.counts, hipMemcpyDeviceToHost));
        v.regions = regions.data(), v.counts = counts.data(), v.ovl = nullptr, v.ovn = nullptr;
        v.unit0 = 0, v.words_touched = 0;
        if (list) {
            ovl.resize((size_t)pl.grid * kOvfListCap), ovn.resize(pl.grid);
            HIP_OK(hipMemcpy(ovl.data(), a.ovl, ovl.size() * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(ovn.data(), a.ovn, ovn.size() * 4, hipMemcpyDeviceToHost));
            v.ovl = ovl.data(), v.ovn = ovn.data();
            for (uint32_t x : count_ne(B.words.as<uint32_t>(), nw32, units, kGarbage32)) v.words_touched += x;
            HIP_OK(hipMemcpy(dirty.data(), B.dirty.p, units * 4, hipMemcpyDeviceToHost));
            // the sweep's units; every other unit's mark is what it was
            const uint32_t u0 = a.b0 << (sl - kSliceLog2), u1 = std::min(units, (a.b0 + a.nb) << (sl - kSliceLog2));
            v.unit0 = u0;
            v.dirty.assign(dirty.begin() + u0, dirty.begin() + u1);
            for (uint32_t u = 0; ok && u < units; u++)
                if ((u < u0 || u >= u1) && dirty[u] != dirty_prev[u])
                    ok = false, why = fmt("sweep %u changed dirty[unit %u], outside its slices", sw, u);
            dirty_prev = dirty;
        }
        // this sweep's overflow bits: what is set now and was not before it
        const std::vector<uint32_t> side_now = set_bits(list ? B.ovf.as<uint32_t>() : B.words.as<uint32_t>(), nw32, units);
        if (!std::includes(side_now.begin(), side_now.end(), side_prev.begin(), side_prev.end()))
            ok = false, why = fmt("sweep %u cleared an overflow bit of an earlier sweep", sw);
        std::set_difference(side_now.begin(), side_now.end(), side_prev.begin(), side_prev.end(), std::back_inserter(v.side));
        side_prev = side_now;
        v.guards_ok = B.guards_ok();
        if (!ok) break;
        const auto E = sweep_range(pos, sl, a.b0, a.nb);
        Tiers t;
        ok = check_pass_a(v, E.first, E.second, t, why);
        if (!ok) why = fmt("sweep %u: ", sw) + why;
        if (!ok && t.culprit >= 0) {  // whose position it is
            const uint64_t per = (n + pl.grid - 1) / pl.grid;
            bool found = false;
            for (uint64_t i = 0; i < n && !found; i++)
                for (uint32_t q = 0; q < c.k && !found; q++)
                    if (position(h.h1[i], h.h2[i], q, c.num_bits) == (uint32_t)t.culprit) {
                        why += fmt("; position %u of key %llu, pass A workgroup %llu", q, (unsigned long long)i,
                                   (unsigned long long)(i / per));
                        found = true;
                    }
            if (!found) why += "; no key produces it";
        }
        print_tiers(c.name.c_str(), sw, t);
        // (an accumulate build has no lists: past its ring or region a position goes to the words)
        if (ok && c.tiers && !(t.side && t.at_cap && (!list || (t.list && t.full_lists))))
            ok = false, why = "a tier was not reached (list entries, a full list, overflow bits, a region at cap_segs)";
    }
    if (ok && c.pass_b) {
        HIP_OK(launch_pass_b(L, 0, pl.nbins, -1, list));
        HIP_OK(hipDeviceSynchronize());
        std::vector<uint64_t> got(nw32 / 2), want(nw32 / 2, 0);
        HIP_OK(hipMemcpy(got.data(), B.words.p, nw32 * 4, hipMemcpyDeviceToHost));
        if (keys.offsets.empty())
            oracle_bloom_build_fixed(keys.data.data() + keys.skew, keys.key_len, n, c.num_bits, c.k, want.data());
        else
            oracle_bloom_build_var(keys.data.data(), keys.offsets.data(), n, c.num_bits, c.k, want.data());
        for (size_t i = 0; ok && i < got.size(); i++)
            if (got[i] != want[i])
                ok = false, why = fmt("after pass B word %zu (slice %zu): got %016llx want %016llx", i, (i * 64) >> sl,
                                      (unsigned long long)got[i], (unsigned long long)want[i]);
        if (ok && list) {  // pass B clears what it consumes
            uint64_t left = 0;
            for (uint32_t x : count_ne(B.ovf.as<uint32_t>(), nw32, units, 0u)) left += x;
            for (uint32_t x : count_ne(B.dirty.as<uint32_t>(), units, 1, 0u)) left += x;
            if (left) ok = false, why = "pass B left overflow words or dirty marks behind";
        }
        if (ok && !B.guards_ok()) ok = false, why = "pass B wrote a guard strip";
    }
    B.free();
    verdict(group, c.name, ok, why);
}

// ---------------------------------------------------------------- pass B on synthetic regions
struct BCase {
    std::string name;
    uint32_t sl, num_bits, grid, cap;
    bool fresh, zero_counts;
    uint32_t bfirst, bend;  // bend 0: every bin
    bool dirty, lists;      // fresh only
};

void run_pass_b(const char* group, const BCase& c, uint64_t seed) {
    std::mt19937_64 rng(seed);
    const uint32_t sl = c.sl, nbins = (uint32_t)(((uint64_t)c.num_bits + (1ull << sl) - 1) >> sl);
    const uint32_t bfirst = c.bfirst, bend = c.bend ? c.bend : nbins;
    const uint64_t nw32 = 2 * (((uint64_t)c.num_bits + 63) / 64);
    const uint32_t units = (uint32_t)((nw32 + kSliceWords32 - 1) / kSliceWords32);
    std::vector<uint64_t> regions((size_t)nbins * c.grid * c.cap * kSegSlotWords);
    std::vector<uint32_t> counts((size_t)nbins * c.grid, kGarbage32);  // other slices' counts: never read
    memset(regions.data(), kGarbage, regions.size() * 8);              // past each count, other slices: never read
    std::vector<uint32_t> words(nw32), expect;
    if (c.fresh) {
        memset(words.data(), kGarbage, nw32 * 4);
        expect = words;
        const uint64_t wlo = (uint64_t)bfirst << (sl - 5), whi = std::min<uint64_t>(nw32, (uint64_t)bend << (sl - 5));
        for (uint64_t i = wlo; i < whi; i++) expect[i] = 0;
    } else {
        for (auto& w : words) w = (uint32_t)(rng() & rng() & rng());
        expect = words;
    }
    auto set = [&](uint64_t p) { expect[p >> 5] |= 1u << (p & 31); };
    for (uint32_t b = bfirst; b < bend; b++) {
        const uint32_t lim = (uint32_t)std::min<uint64_t>(1ull << sl, c.num_bits - ((uint64_t)b << sl));
        for (uint32_t w = 0; w < c.grid; w++) {
            // region (b, 0) is exactly full; the rest anything from empty to full
            const uint32_t cnt = c.zero_counts ? 0 : (w == 0 ? c.cap : (uint32_t)(rng() % (c.cap + 1)));
            counts[(size_t)b * c.grid + w] = cnt;
            uint64_t* r = regions.data() + ((size_t)w * nbins + b) * c.cap * kSegSlotWords;
            for (uint32_t s = 0; s < cnt; s++) {
                uint32_t off[kSegEntries];
                for (auto& o : off) o = (uint32_t)(rng() % lim);
                if (w == 0 && s == 0)  // 24 equal offsets
                    for (auto& o : off) o = off[0];
                if (w == 0 && s == 1) {  // the offset range's ends, and both sides of bit 20
                    off[0] = 0, off[23] = lim - 1, off[7] = 0, off[8] = lim - 1;
                    if (lim > (1u << kSliceLog2)) off[3] = (1u << kSliceLog2) - 1, off[16] = 1u << kSliceLog2;
                }
                encode_segment(off, sl, r + (size_t)s * kSegSlotWords);
                for (uint32_t o : off) set(((uint64_t)b << sl) | o);
            }
        }
    }
    std::vector<uint32_t> ovf((size_t)units * kSliceWords32, 0), ovf_after, dirty(units, 0);
    std::vector<uint32_t> ovl((size_t)c.grid * kOvfListCap, kGarbage32), ovn(c.grid, 0);
    if (c.dirty) {
        // unit uA is marked: folded in and cleared; unit uB holds bits without a mark: ignored, left alone
        const uint32_t uA = bfirst << (sl - kSliceLog2) | (sl > kSliceLog2 ? 1u : 0u), uB = uA + 1;
        for (uint32_t u : {uA, uB}) {
            const uint64_t base = (uint64_t)u * kSliceWords32;
            for (uint64_t i = base; i < std::min<uint64_t>(nw32, base + kSliceWords32); i++) ovf[i] = (uint32_t)(rng() & rng());
        }
        dirty[uA] = 1;
        ovf_after = ovf;
        for (uint64_t i = (uint64_t)uA * kSliceWords32; i < std::min<uint64_t>(nw32, (uint64_t)(uA + 1) * kSliceWords32); i++)
            expect[i] |= ovf[i], ovf_after[i] = 0;
    } else {
        ovf_after = ovf;
    }
    if (c.lists) {  // lengths 0, 1 and kOvfListCap, the rest 0
        const uint32_t len[3] = {0, 1, kOvfListCap};
        for (uint32_t w = 0; w < 3 && w < c.grid; w++) {
            ovn[w] = len[w];
            for (uint32_t i = 0; i < len[w]; i++) {
                const uint32_t p = (uint32_t)(rng() % c.num_bits);
                ovl[(size_t)w * kOvfListCap + i] = p;
                set(p);
            }
        }
    }
    Buffers B;
    B.keys.alloc(0, 0), B.offsets.alloc(0, 0), B.hashes.alloc(0, 0);
    B.regions.alloc(regions.size() * 8, 0), B.counts.alloc(counts.size() * 4, 0), B.words.alloc(nw32 * 4, 0);
    B.ovf.alloc(c.fresh ? ovf.size() * 4 : 0, 0), B.dirty.alloc(c.fresh ? units * 4 : 0, 0);
    B.ovl.alloc(c.fresh ? ovl.size() * 4 : 0, 0), B.ovn.alloc(c.fresh ? ovn.size() * 4 : 0, 0);
    HIP_OK(hipMemcpy(B.regions.p, regions.data(), regions.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(B.counts.p, counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(B.words.p, words.data(), nw32 * 4, hipMemcpyHostToDevice));
    if (c.fresh) {
        HIP_OK(hipMemcpy(B.ovf.p, ovf.data(), ovf.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(B.dirty.p, dirty.data(), units * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(B.ovl.p, ovl.data(), ovl.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(B.ovn.p, ovn.data(), ovn.size() * 4, hipMemcpyHostToDevice));
    }
    PartitionPlan pl;
    pl.slice_log2 = sl, pl.nbins = nbins, pl.grid = c.grid, pl.cap_segs = c.cap, pl.bins_per_sweep = nbins, pl.sweeps = 1;
    PartitionWorkspace ws;
    ws.regions = B.regions.as<uint64_t>(), ws.counts = B.counts.as<uint32_t>(), ws.ovf = B.ovf.as<uint32_t>();
    ws.dirty = B.dirty.as<uint32_t>(), ws.ovl = B.ovl.as<uint32_t>(), ws.ovn = B.ovn.as<uint32_t>();
    const Launch L{0,       c.num_bits, 7,       (uint32_t)nw32, Mod32::make(c.num_bits), B.words.as<uint32_t>(), ws, kCus,
                   nullptr, nullptr,    nullptr, pl,             TiledPlan{}};
    HIP_OK(launch_pass_b(L, bfirst, bend, -1, c.fresh));
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> got(nw32);
    HIP_OK(hipMemcpy(got.data(), B.words.p, nw32 * 4, hipMemcpyDeviceToHost));
    bool ok = true;
    std::string why;
    for (size_t i = 0; ok && i < nw32; i++)
        if (got[i] != expect[i])
            ok = false, why = fmt("u32 word %zu (bin %zu): got %08x want %08x", i, (i * 32) >> sl, got[i], expect[i]);
    if (ok && c.fresh) {
        std::vector<uint32_t> o(ovf.size()), d(units);
        HIP_OK(hipMemcpy(o.data(), B.ovf.p, o.size() * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(d.data(), B.dirty.p, units * 4, hipMemcpyDeviceToHost));
        if (o != ovf_after) ok = false, why = "ovf: a marked unit's words must be cleared, an unmarked unit's left alone";
        for (uint32_t u = 0; ok && u < units; u++)
            if (d[u]) ok = false, why = fmt("dirty[unit %u] was not cleared", u);
    }
    if (ok && !B.guards_ok()) ok = false, why = "a guard strip behind a buffer was written";
    B.free();
    verdict(group, c.name, ok, why);
}

// ---------------------------------------------------------------- the groups
void group_c2(const char* g) {
    for (bool fresh : {false, true}) {
        const char* f = fresh ? "fresh" : "accumulate";
        run_pass_a(g, {fmt("c2-kernel-%s", f), kBitsC2, 7, fresh, true, 20, 1, false}, keys16(0xA001, 200001), KeyKind::Fixed16);
        run_pass_a(g, {fmt("tightest-ring-%s", f), 1000000000u, 7, fresh, true, 20, 1, false}, keys16(0xA002, 300001),
                   KeyKind::Fixed16);
        for (uint64_t n : {1ull, 1023ull, 1024ull, 1025ull, 32768ull, 32769ull})
            run_pass_a(g, {fmt("keys-%llu-%s", (unsigned long long)n, f), kBitsC2, 7, fresh, true, 20, 1, false},
                       keys16(0xA100 + n, n), KeyKind::Fixed16);
    }
}
void group_k(const char* g) {
    const uint32_t ks[] = {1, 8, 9, 16, 17, 32};
    const uint64_t ns[] = {200001, 200001, 100001, 100001, 50001, 200001};
    for (int i = 0; i < 6; i++)
        run_pass_a(g, {fmt("k-%u", ks[i]), kBitsC2, ks[i], false, true, 20, ks[i] == 32 ? 2u : 1u, false},
                   keys16(0xB000 + ks[i], ns[i]), KeyKind::Fixed16);
}
void group_wide(const char* g) {
    for (bool fresh : {false, true}) {
        const char* f = fresh ? "fresh" : "accumulate";
        run_pass_a(g, {fmt("bins21-one-sweep-%s", f), kBits21, 7, fresh, false, 21, 1, false}, keys16(0xC001, 150001),
                   KeyKind::Fixed16);
        run_pass_a(g, {fmt("2^31+1-%s", f), 0x80000001u, 7, fresh, false, 21, 2, false}, keys16(0xC002, 150001),
                   KeyKind::Fixed16);
        run_pass_a(g, {fmt("2^32-1-%s", f), 0xFFFFFFFFu, 7, fresh, false, 21, 2, false}, keys16(0xC003, 150001),
                   KeyKind::Fixed16);
        run_pass_a(g, {fmt("2^32-2-%s", f), 0xFFFFFFFEu, 7, fresh, false, 21, 2, false}, keys16(0xC004, 150001),
                   KeyKind::Fixed16);
    }
}
void group_records(const char* g) {
    const uint64_t n = 100003;
    for (uint32_t bits : {kBitsC2, 0x80000001u})
        for (uint32_t k : {7u, 32u}) {
            const bool small = bits == kBitsC2;
            const char* bn = small ? "c2" : "2^31+1";
            run_pass_a(g, {fmt("var-%s-k%u", bn, k), bits, k, false, small, 0, 0, false}, keys_var(0xD001 + k, n), KeyKind::Records);
            run_pass_a(g, {fmt("fixed24-%s-k%u", bn, k), bits, k, false, small, 0, 0, false}, keys_fixed(0xD002 + k, n, 24, 0),
                       KeyKind::Records);
            run_pass_a(g, {fmt("unaligned16-%s-k%u", bn, k), bits, k, false, small, 0, 0, false}, keys_fixed(0xD003 + k, n, 16, 1),
                       KeyKind::Records);
        }
    run_pass_a(g, {"var-c2-k7-fresh", kBitsC2, 7, true, true, 0, 0, false}, keys_var(0xD004, n), KeyKind::Records);
}
void group_tiers(const char* g) {
    run_pass_a(g, {"tiers20-fresh", kBitsC2, 7, true, true, 20, 1, true}, keys16(0xE001, 200001), KeyKind::Fixed16);
    run_pass_a(g, {"tiers20-accumulate", kBitsC2, 7, false, true, 20, 1, true}, keys16(0xE001, 200001), KeyKind::Fixed16);
    run_pass_a(g, {"tiers21-fresh", kBits21, 7, true, false, 21, 1, true}, keys16(0xE002, 150001), KeyKind::Fixed16);
}
void group_passb(const char* g) {
    // 3 bins each: the last 2^20-bit slice is 4 u32 words; the last 2^21-bit bin lacks its upper half
    const uint32_t bits20 = 2u * (1u << 20) + 65u, bits21 = 2u * (1u << 21) + 1000u;
    uint64_t seed = 0xF000;
    for (uint32_t sl : {20u, 21u}) {
        const uint32_t bits = sl == 20 ? bits20 : bits21;
        for (uint32_t grid : {1u, 15u, 16u, 17u, 512u, 1024u})
            run_pass_b(g, {fmt("sl%u-grid%u-accumulate", sl, grid), sl, bits, grid, 3, false, false, 0, 0, false, false}, seed++);
        for (uint32_t grid : {1u, 17u})
            run_pass_b(g, {fmt("sl%u-grid%u-fresh", sl, grid), sl, bits, grid, 3, true, false, 0, 0, false, false}, seed++);
        for (bool fresh : {false, true}) {
            const char* f = fresh ? "fresh" : "accumulate";
            run_pass_b(g, {fmt("sl%u-zero-counts-%s", sl, f), sl, bits, 17, 3, fresh, true, 0, 0, false, false}, seed++);
            run_pass_b(g, {fmt("sl%u-subrange-%s", sl, f), sl, bits, 17, 3, fresh, false, 1, 2, false, false}, seed++);
        }
        run_pass_b(g, {fmt("sl%u-dirty", sl), sl, bits, 16, 3, true, false, 0, 0, true, false}, seed++);
        run_pass_b(g, {fmt("sl%u-lists", sl), sl, bits, 17, 3, true, false, 0, 0, false, true}, seed++);
    }
}

// ---------------------------------------------------------------- the checker's self-test (host only)
// A pass A output made from the expected positions by a plain host binning:
// workgroup w's keys in order, each slice's offsets appended to its region,
// then to the workgroup's list, then to the side bits.
struct HostPassA {
    PassAView v;
    std::vector<uint64_t> regions;
    std::vector<uint32_t> counts, ovl, ovn, E;
    void bind() { v.regions = regions.data(), v.counts = counts.data(), v.ovl = ovl.data(), v.ovn = ovn.data(); }
};

HostPassA host_bin(const Hashes& h, uint32_t num_bits, uint32_t k, const PartitionPlan& pl, uint32_t sw, bool fresh) {
    HostPassA o;
    PassAView& v = o.v;
    const uint32_t sl = pl.slice_log2;
    v.num_bits = num_bits, v.sl = sl, v.nbins = pl.nbins, v.grid = pl.grid, v.cap = pl.cap_segs;
    v.b0 = sw * pl.bins_per_sweep, v.nb = std::min(pl.bins_per_sweep, pl.nbins - v.b0), v.fresh = fresh;
    v.words_touched = 0, v.guards_ok = true;
    o.regions.assign((size_t)pl.nbins * pl.grid * pl.cap_segs * kSegSlotWords, 0xA5A5A5A5A5A5A5A5ull);
    o.counts.assign((size_t)pl.nbins * pl.grid, kGarbage32);
    o.ovl.assign((size_t)pl.grid * kOvfListCap, kGarbage32);
    o.ovn.assign(pl.grid, 0);
    const uint64_t n = h.h1.size(), per = (n + pl.grid - 1) / pl.grid;
    std::vector<uint32_t> side;
    for (uint32_t w = 0; w < pl.grid; w++) {
        std::vector<std::vector<uint32_t>> bin(v.nb);
        for (uint64_t i = w * per; i < std::min(n, (w + 1) * per); i++)
            for (uint32_t q = 0; q < k; q++) {
                const uint32_t p = position(h.h1[i], h.h2[i], q, num_bits), b = p >> sl;
                if (b >= v.b0 && b < v.b0 + v.nb) bin[b - v.b0].push_back(p);
            }
        for (uint32_t b = v.b0; b < v.b0 + v.nb; b++) {
            const std::vector<uint32_t>& ps = bin[b - v.b0];
            uint64_t* r = o.regions.data() + ((size_t)w * pl.nbins + b) * pl.cap_segs * kSegSlotWords;
            uint32_t segs = 0;
            size_t i = 0;
            for (; i < ps.size() && segs < pl.cap_segs; segs++) {
                uint32_t off[kSegEntries];
                const size_t m = std::min<size_t>(kSegEntries, ps.size() - i);
                for (size_t t = 0; t < (size_t)kSegEntries; t++) off[t] = ps[i + (t < m ? t : 0)] & ((1u << sl) - 1);
                encode_segment(off, sl, r + (size_t)segs * kSegSlotWords);
                i += m;
            }
            o.counts[(size_t)b * pl.grid + w] = segs;
            for (; i < ps.size(); i++) {
                if (fresh && o.ovn[w] < kOvfListCap)
                    o.ovl[(size_t)w * kOvfListCap + o.ovn[w]++] = ps[i];
                else
                    side.push_back(ps[i]);
            }
        }
    }
    std::sort(side.begin(), side.end());
    side.erase(std::unique(side.begin(), side.end()), side.end());
    v.side = side;
    v.unit0 = v.b0 << (sl - kSliceLog2);
    const uint64_t nw32 = 2 * (((uint64_t)num_bits + 63) / 64);
    const uint32_t units = (uint32_t)((nw32 + kSliceWords32 - 1) / kSliceWords32);
    v.dirty.assign(std::min(units, (v.b0 + v.nb) << (sl - kSliceLog2)) - v.unit0, 0);
    if (fresh)
        for (uint32_t p : side) v.dirty[(p >> kSliceLog2) - v.unit0] = 1;
    const std::vector<uint32_t> pos = all_positions(h, num_bits, k);
    const auto E = sweep_range(pos, sl, v.b0, v.nb);
    o.E.assign(E.first, E.first + E.second);
    o.bind();
    return o;
}

int selftest() {
    const char* g = "selftest";
    const uint64_t n = 200001;
    const Hashes h = hash_keys(keys16(0x5E1F, n));
    auto run = [&](HostPassA& o, std::string& why) {
        o.bind();
        Tiers t;
        return check_pass_a(o.v, o.E.data(), o.E.size(), t, why);
    };
    auto accept = [&](const char* name, HostPassA o) {
        std::string why;
        const bool ok = run(o, why);
        verdict(g, name, ok, why);
    };
    auto reject = [&](const std::string& name, HostPassA& o) {
        std::string why;
        const bool ok = run(o, why);
        if (!ok) printf("  (%s rejected: %s)\n", name.c_str(), why.c_str());
        verdict(g, name, !ok, "the checker accepted the mutated output");
    };
    // the C2 kernel's plan as it is: nothing overflows
    const PartitionPlan real = plan_partition(kBitsC2, 7, n, kCus);
    accept("accept-plan-accumulate", host_bin(h, kBitsC2, 7, real, 0, false));
    accept("accept-plan-fresh", host_bin(h, kBitsC2, 7, real, 0, true));
    // two sweeps and regions of two segments: lists fill and overflow bits appear
    PartitionPlan tight = real;
    tight.cap_segs = 2, tight.sweeps = 2, tight.bins_per_sweep = (real.nbins + 1) / 2;
    const HostPassA base = host_bin(h, kBitsC2, 7, tight, 0, true);
    accept("accept-tight-fresh", base);
    accept("accept-tight-fresh-sweep1", host_bin(h, kBitsC2, 7, tight, 1, true));
    accept("accept-tight-accumulate", host_bin(h, kBitsC2, 7, tight, 0, false));
    {
        Tiers t;
        std::string why;
        HostPassA o = base;
        o.bind();
        check_pass_a(o.v, o.E.data(), o.E.size(), t, why);
        print_tiers("selftest-tight-fresh", 0, t);
        verdict(g, "tight-reaches-every-tier", t.list && t.full_lists && t.side && t.at_cap, "a tier is empty");
    }
    const uint32_t sl = tight.slice_log2, grid = tight.grid;
    auto region = [&](HostPassA& o, uint32_t b, uint32_t w) {
        return o.regions.data() + ((size_t)w * tight.nbins + b) * tight.cap_segs * kSegSlotWords;
    };
    auto edit = [&](HostPassA& o, uint32_t b, uint32_t w, uint32_t s, auto&& f) {
        uint32_t off[kSegEntries];
        decode_segment(region(o, b, w) + (size_t)s * kSegSlotWords, sl, off);
        f(off);
        encode_segment(off, sl, region(o, b, w) + (size_t)s * kSegSlotWords);
    };
    // an offset of slice b that no key produces
    auto unexpected = [&](const HostPassA& o, uint32_t b) {
        for (uint32_t off = 1;; off++) {
            const uint32_t p = (b << sl) | off;
            if (!std::binary_search(o.E.begin(), o.E.end(), p)) return off;
        }
    };
    // the uniform plan's regions end in an open, padded segment
    const HostPassA open = host_bin(h, kBitsC2, 7, real, 0, true);
    auto open_edit = [&](HostPassA& o, uint32_t b, uint32_t w, auto&& f) {
        uint32_t off[kSegEntries];
        const uint32_t s = o.counts[(size_t)b * real.grid + w] - 1;
        uint64_t* seg = o.regions.data() + (((size_t)w * real.nbins + b) * real.cap_segs + s) * kSegSlotWords;
        decode_segment(seg, sl, off);
        f(off);
        encode_segment(off, sl, seg);
    };
    {  // a drop: an entry replaced by its neighbour
        HostPassA o = base;
        edit(o, 3, 1, 0, [](uint32_t* off) { off[5] = off[6]; });
        reject("drop-entry-replaced-by-neighbour", o);
        HostPassA p = open;
        open_edit(p, 3, 1, [](uint32_t* off) { off[1] = off[2]; });
        reject("drop-entry-replaced-by-neighbour-open-segment", p);
    }
    {  // a spurious offset, in a pad slot: nothing is dropped
        HostPassA o = open;
        const uint32_t x = unexpected(o, 4);
        bool had_pad = false;
        open_edit(o, 4, 2, [&](uint32_t* off) { had_pad = off[23] == off[0], off[23] = x; });
        if (!had_pad) verdict(g, "spurious-offset", false, "the self-test's region has no pad slot");
        else reject("spurious-offset", o);
    }
    {  // a count one too high: the segment past it is garbage
        HostPassA o = open;
        o.counts[(size_t)5 * real.grid + 0]++;
        reject("count-one-too-high-over-garbage", o);
    }
    {  // a count one too low
        HostPassA o = base;
        o.counts[(size_t)5 * grid + 0]--;
        reject("count-one-too-low", o);
    }
    {  // an entry filed under the wrong slice: two regions of one workgroup swap an entry
        HostPassA o = base;
        uint32_t x = 0;
        edit(o, 6, 0, 0, [&](uint32_t* off) { x = off[2]; });
        edit(o, 7, 0, 0, [&](uint32_t* off) { std::swap(x, off[2]); });
        edit(o, 6, 0, 0, [&](uint32_t* off) { off[2] = x; });
        reject("entry-under-wrong-slice", o);
    }
    {  // a pad that is not a copy of entry 0 (but of entry 1: a position the keys do produce)
        HostPassA o = open;
        bool had_pad = false;
        open_edit(o, 8, 3, [&](uint32_t* off) { had_pad = off[23] == off[0] && off[1] != off[0], off[23] = off[1]; });
        if (!had_pad) verdict(g, "pad-not-a-copy-of-entry-0", false, "the self-test's region has no pad slot");
        else reject("pad-not-a-copy-of-entry-0", o);
    }
    {  // a list entry outside the sweep (sweep 0 holds slices [0, bins_per_sweep))
        HostPassA o = base;
        o.ovl[0] = ((tight.bins_per_sweep + 3) << sl) | 17;
        reject("list-entry-outside-sweep", o);
    }
    {  // an extra ovf bit
        HostPassA o = base;
        const uint32_t p = (2u << sl) | unexpected(o, 2);
        o.v.side.insert(std::lower_bound(o.v.side.begin(), o.v.side.end(), p), p);
        o.v.dirty[p >> kSliceLog2] = 1;
        reject("extra-ovf-bit", o);
    }
    {  // a missing dirty mark
        HostPassA o = base;
        o.v.dirty[o.v.side[0] >> kSliceLog2] = 0;
        reject("missing-dirty-mark", o);
    }
    {  // (beyond the list) a filter word touched by a fresh pass A, a guard written
        HostPassA o = base;
        o.v.words_touched = 1;
        reject("fresh-words-touched", o);
        HostPassA p = base;
        p.v.guards_ok = false;
        reject("guard-written", p);
    }
    return 0;
}

int stage_main(int argc, char** argv) {
    struct Group {
        const char* name;
        void (*run)(const char*);
    };
    const Group groups[] = {{"passa-c2", group_c2},       {"passa-k", group_k},     {"passa-wide", group_wide},
                            {"records", group_records},   {"tiers", group_tiers},   {"passb", group_passb}};
    const char* name = nullptr;
    if (argc == 2 && strcmp(argv[1], "--selftest") == 0) {
        name = "selftest";
        selftest();
    } else if (argc == 3 && strcmp(argv[1], "--group") == 0) {
        for (const Group& g : groups)
            if (strcmp(argv[2], g.name) == 0) {
                name = g.name;
                g.run(g.name);
            }
    }
    if (!name) {
        fprintf(stderr, "usage: %s --selftest | --group {passa-c2|passa-k|passa-wide|records|tiers|passb}\n", argv[0]);
        return 2;
    }
    printf("partition_stage_test (%s): %d cases, %d bad\n", name, g_cases, g_bad);
    return g_bad ? 1 : 0;
}

}  // namespace
}  // namespace lsmb

int main(int argc, char** argv) { return lsmb::stage_main(argc, argv); }

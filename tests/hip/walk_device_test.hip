// walk_device_test.hip — the DEVICE compile of bloom_math.hpp at its arithmetic
// edges.  tests/cpp/reduce_test.cpp and walkrec_test.cpp prove the reductions
// and walks on the host build of the header, but three of its branches exist
// only under __HIP_DEVICE_COMPILE__ (the v_cvt_f64_u32 of f64_of_u64, __umul24
// in Mod14, the add-with-carry chain that builds WalkRec::c), and on the GPU
// the product's kernels feed them hashes of random keys, which never land on
// x = q*d + (d-1), r + s == d, s0 + dt == d or a 31-carry chain.
//
// One kernel evaluates, per case (kind, d, k, a, b):
//   Mod32::reduce(a), Mod32::reduce31(a) (d <= 2^31), Mod14::reduce(a) (d < 2^14),
//   the k positions of Walk32 / Walk14 / Walk64 / WalkM from (h1, h2) = (a, b),
//   WalkRec::make (r, s, c) and the k positions RecWalk32 / RecWalk64 replay.
// The expectation is a literal % on uint64_t / unsigned __int128 computed here,
// never through bloom_math.hpp.  Exit 0: every value equal; 1: mismatches (the
// first 20 printed); 2: a HIP call failed.  `--host` runs the same case list
// through the host compile of the same eval() (no device needed).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../storage-engine_amd/csrc/bloom_math.hpp"

using namespace lsmb;

enum Kind : uint32_t { kReduce, kReduce31, kMod14, kWalk32, kWalk14, kWalk64, kWalkM, kRec32, kRec64, kKinds };
static const char* const kKindName[kKinds] = {"reduce", "reduce31", "mod14", "walk32", "walk14",
                                              "walk64", "walkM", "rec32", "rec64"};

struct Case {
    uint32_t kind, mod, k, off;  // mod: index of the modulus; off: first output value
    uint64_t a, b;               // x (reductions) or h1, h2 (walks)
};

static bool is_reduce(uint32_t kind) { return kind <= kMod14; }
static bool is_rec(uint32_t kind) { return kind == kRec32 || kind == kRec64; }
static uint32_t outputs(const Case& c) { return is_reduce(c.kind) ? 1u : (is_rec(c.kind) ? 3u : 0u) + c.k; }

template <class W>
LSMB_HD void walk_out(const typename W::Mod& md, uint64_t h1, uint64_t h2, uint32_t k, uint32_t* out) {
    W w(md, h1, h2);
    for (uint32_t i = 0; i < k; i++) {
        out[i] = w.pos();
        w.next(md);
    }
}

template <class RW>
LSMB_HD void rec_out(const Mod32& md, uint64_t h1, uint64_t h2, uint32_t k, uint32_t* out) {
    const WalkRec q = WalkRec::make(md, H128{h1, h2}, k);
    out[0] = q.r, out[1] = q.s, out[2] = q.c;
    RW w(md, q);
    for (uint32_t i = 0; i < k; i++) {
        out[3 + i] = w.pos();
        w.next(md);
    }
}

// The code under test: compiled for the device (k_eval) and for the host (--host).
LSMB_HD void eval(const Case& c, const Mod32& md, const Mod14& m14, uint32_t* out) {
    switch (c.kind) {
        case kReduce: out[0] = md.reduce(c.a); break;
        case kReduce31: out[0] = md.reduce31(c.a); break;
        case kMod14: out[0] = m14.reduce(c.a); break;
        case kWalk32: walk_out<Walk32>(md, c.a, c.b, c.k, out); break;
        case kWalk14: walk_out<Walk14>(m14, c.a, c.b, c.k, out); break;
        case kWalk64: walk_out<Walk64>(md, c.a, c.b, c.k, out); break;
        case kWalkM: walk_out<WalkM>(md, c.a, c.b, c.k, out); break;
        case kRec32: rec_out<RecWalk32>(md, c.a, c.b, c.k, out); break;
        case kRec64: rec_out<RecWalk64>(md, c.a, c.b, c.k, out); break;
    }
}

__global__ void __launch_bounds__(256) k_eval(const Case* cases, uint32_t n, const Mod32* m32, const Mod14* m14,
                                              uint32_t* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Case c = cases[i];
    eval(c, m32[c.mod], m14[c.mod], out + c.off);  // writes outputs(c) values: [c.off, next case's off)
}

// ---------------------------------------------------------------- the reference
// Literal arithmetic of src/bloom/mod.rs:192-197 and of the record's definition.
static void expect(const Case& c, uint32_t d, uint32_t* out) {
    if (is_reduce(c.kind)) {
        out[0] = (uint32_t)(c.a % d);
        return;
    }
    uint32_t* pos = out;
    if (is_rec(c.kind)) {
        out[0] = (uint32_t)(c.a % d);
        out[1] = (uint32_t)(c.b % d);
        uint32_t carries = 0;
        const uint32_t steps = c.k < 2 ? 0 : (c.k - 1 < 31 ? c.k - 1 : 31);
        unsigned __int128 x = c.a;
        for (uint32_t i = 0; i < steps; i++) {
            x += c.b;
            if (x >> 64) carries |= 1u << i;  // carry out of x_i + h2
            x = (uint64_t)x;
        }
        out[2] = carries;
        pos = out + 3;
    }
    for (uint32_t i = 0; i < c.k; i++) {
        const uint64_t x = (uint64_t)((unsigned __int128)c.a + (unsigned __int128)i * c.b);  // wraps at 2^64
        pos[i] = (uint32_t)(x % d);
    }
}

// How many cases sit on each edge the list is built for (literal arithmetic
// again), so a change to the generator cannot quietly lose one.
struct EdgeCounts {
    long below_multiple = 0;  // reductions of x = q*d + (d - 1), d > 1
    long s0_dt_is_d = 0;      // walks with h2 = 2^64 (mod d): s0 + dt == d
    long r_s_is_d = 0;        // walks with a step whose sum r + s is exactly d
    long carries_all = 0;     // k = 32 walks whose 31 steps all carry
    long carries_none = 0;    // k = 32 walks with h2 > 0 and no carry
};

static void count_edges(const Case& c, uint32_t d32, EdgeCounts& e) {
    const uint64_t d = d32;
    if (is_reduce(c.kind)) {
        if (d > 1 && c.a % d == d - 1) e.below_multiple++;
        return;
    }
    const uint64_t t64 = (uint64_t)((((unsigned __int128)1) << 64) % d);
    const uint64_t s0 = c.b % d, s1 = (s0 + d - t64) % d;
    if (s0 == t64) e.s0_dt_is_d++;
    bool sum_d = false;
    uint32_t ncarry = 0;
    uint64_t x = c.a;
    for (uint32_t i = 1; i < c.k; i++) {
        const bool carry = (((unsigned __int128)x + c.b) >> 64) != 0;
        if (d > 1 && x % d + (carry ? s1 : s0) == d) sum_d = true;
        ncarry += carry;
        x += c.b;
    }
    if (sum_d) e.r_s_is_d++;
    if (c.k == 32 && ncarry == 31) e.carries_all++;
    if (c.k == 32 && ncarry == 0 && c.b) e.carries_none++;
}

// ---------------------------------------------------------------- the case list
struct Cases {
    std::vector<uint32_t> d;
    std::vector<Mod32> m32;
    std::vector<Mod14> m14;
    std::vector<Case> cases;
    uint64_t nout = 0;

    uint32_t modulus(uint32_t dv) {
        d.push_back(dv);
        m32.push_back(Mod32::make(dv));
        Mod14 z;
        memset(&z, 0, sizeof z);
        m14.push_back(Mod14::fits(dv) ? Mod14::make(dv) : z);
        return (uint32_t)d.size() - 1;
    }
    void add(uint32_t kind, uint32_t mod, uint32_t k, uint64_t a, uint64_t b) {
        Case c{kind, mod, k, (uint32_t)nout, a, b};
        nout += outputs(c);
        cases.push_back(c);
    }
    // every reduction that serves this modulus (only14: Mod14's alone)
    void reduce_all(uint32_t mod, uint64_t x, bool only14) {
        const uint32_t dv = d[mod];
        if (!only14) add(kReduce, mod, 0, x, 0);
        if (!only14 && dv <= 0x80000000u) add(kReduce31, mod, 0, x, 0);
        if (Mod14::fits(dv)) add(kMod14, mod, 0, x, 0);
    }
    // every walk that serves this modulus; the record walks hold 31 carries (k <= 32)
    void walk_all(uint32_t mod, uint32_t k, uint64_t h1, uint64_t h2) {
        const uint32_t dv = d[mod];
        add(kWalk64, mod, k, h1, h2);
        if (k <= 32) add(kRec64, mod, k, h1, h2);
        if (dv <= 0x80000000u) {
            add(kWalk32, mod, k, h1, h2);
            if (k <= 32) add(kRec32, mod, k, h1, h2);
        }
        if (Mod14::fits(dv)) add(kWalk14, mod, k, h1, h2);
        if (dv == 0xFFFFFFFFu) add(kWalkM, mod, k, h1, h2);
    }
};

// tests/cpp/reduce_test.cpp's grid: x = q*d + {0, 1, d-1} at the extreme q, x
// near 0 and near 2^64, then random x, every second one a multiple of d and
// every sixth one just below a multiple.
static void reduce_grid(Cases& cs, uint32_t mod, std::mt19937_64& rng, int nrand, bool only14 = false) {
    const uint32_t d = cs.d[mod];
    const uint64_t qmax = ~0ull / d;
    const uint64_t qs[] = {0, 1, 2, qmax, qmax - 1, qmax / 2, qmax >> 32, (qmax >> 32) + 1, 1ull << 32};
    for (uint64_t q : qs) {
        if (q > qmax) continue;
        for (uint64_t r : {(uint64_t)0, (uint64_t)1, (uint64_t)d - 1}) {
            if (r >= d) continue;
            const unsigned __int128 x = (unsigned __int128)q * d + r;
            if (x <= ~0ull) cs.reduce_all(mod, (uint64_t)x, only14);
        }
    }
    for (unsigned long long x : {0ull, 1ull, ~0ull, ~0ull - 1, 1ull << 32, (1ull << 32) - 1, 1ull << 63, (1ull << 63) - 1})
        cs.reduce_all(mod, x, only14);
    for (int t = 0; t < nrand; t++) {
        uint64_t x = rng();
        if (t & 1) x -= x % d;
        else if (t % 3 == 0) x = x - x % d + d - 1;  // (may wrap: still a valid input)
        cs.reduce_all(mod, x, only14);
    }
}

static const uint32_t kKs[] = {1, 2, 7, 8, 16, 32, 40};

static void walk_grid(Cases& cs, uint32_t mod, std::mt19937_64& rng, int nrand) {
    const uint64_t d = cs.d[mod];
    const uint64_t top = ~0ull, p32 = 1ull << 32, p63 = 1ull << 63;
    const uint64_t t64 = (uint64_t)((((unsigned __int128)1) << 64) % d);
    const uint64_t edge[] = {0, 1, d - 1, d, d + 1, 2 * d, p32 - 1, p32, p63, 0 - d, top};
    for (uint32_t k : kKs)
        for (uint64_t h1 : edge)
            for (uint64_t h2 : edge) cs.walk_all(mod, k, h1, h2);
    // the largest value <= 2^64 - 1 with residue r (>= 2^64 - d: it carries with any h2 >= d)
    auto top_with_residue = [&](uint64_t r) { return top - (top % d + d - r) % d; };
    for (uint32_t k : kKs) {
        // h2 = 2^64 (mod d): s0 + dt == d, the carrying increment s1 is 0.  From
        // a low and a high multiplier, with h1 that carries at once and never.
        const uint64_t hi_mult = t64 + (top - t64) / d * d;
        for (uint64_t h2 : {t64, t64 + d, hi_mult})
            for (uint64_t h1 : {top, top - 1, (uint64_t)0, d - 1}) cs.walk_all(mod, k, h1, h2);
        if (d >= 2) {
            // r + s0 == d at step 1 without a carry (h1 + h2 = d), for a small,
            // a middle and the largest increment
            for (uint64_t a : {(uint64_t)1, d / 2 + 1, d - 1}) cs.walk_all(mod, k, d - a, a);
            // r + s1 == d at step 1 with a carry: h2 >= 2^63, h1 the top value
            // whose residue is d - s1
            for (uint64_t h2 : {p63, p63 + d / 3, top - 1, top - d}) {
                const uint64_t s1 = (h2 % d + d - t64) % d;
                if (s1) cs.walk_all(mod, k, top_with_residue(d - s1), h2);
            }
        }
        // every step carries (x + 2^64 - 1 = x - 1 + 2^64 while x >= 1), and none does
        for (uint64_t h1 : {p63, top, (uint64_t)1000}) cs.walk_all(mod, k, h1, top);
        for (uint64_t h1 : {(uint64_t)0, d - 1, p32}) {
            cs.walk_all(mod, k, h1, 0);
            cs.walk_all(mod, k, h1, 1);
            cs.walk_all(mod, k, h1, d);
        }
    }
    for (int t = 0; t < nrand; t++) {
        uint64_t h1 = rng(), h2 = rng();
        if (t % 7 == 0) h2 = top - rng() % 1000;  // carries at every step
        if (t % 11 == 0) h1 = top - rng() % 1000;
        if (t % 13 == 0) h2 = rng() % (2 * d);    // no carry for a long while
        cs.walk_all(mod, kKs[rng() % 7], h1, h2);
    }
}

static Cases make_cases() {
    Cases cs;
    std::mt19937_64 rng(20);
    // reduce_test.cpp's fixed_d, and the build tests' wide moduli (tests/test_gpu_wide_moduli.py
    // NB): 2^31, 2^31 + 1, new(3e8, .01) = 2 870 145 874 bits and 2^32 - 2
    const uint32_t big[] = {1, 2, 3, 5, 7, 64, 957, 9568, 9569, 16383, 65535, 65536, 65537, 956716,
                            956715292, 1000000000, 0x3FFFFFFFu, 0x40000000u, 0x40000001u, 0x7FFFFFFFu,
                            0x80000000u, 0x80000001u, 2870145874u, 3000000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t dv : big) {
        const uint32_t m = cs.modulus(dv);
        reduce_grid(cs, m, rng, 4000);
        walk_grid(cs, m, rng, 2500);
    }
    // every Mod14 modulus: the x grid through Mod14::reduce, and Walk14 over a
    // few carrying and edge pairs
    for (uint32_t dv = 1; dv < (1u << 14); dv++) {
        const uint32_t m = cs.modulus(dv);
        reduce_grid(cs, m, rng, 10, true);
        const uint64_t top = ~0ull;
        cs.add(kWalk14, m, 7, rng(), rng());
        cs.add(kWalk14, m, 7, top, top - rng() % 1000);
        cs.add(kWalk14, m, 8, dv - 1, 1);
        cs.add(kWalk14, m, 2, top, (uint64_t)((((unsigned __int128)1) << 64) % dv));
    }
    // random moduli of every width
    for (int t = 0; t < 400; t++) {
        uint32_t dv = (uint32_t)(rng() >> (32 + rng() % 32));
        if (dv == 0) dv = 1;
        const uint32_t m = cs.modulus(dv);
        reduce_grid(cs, m, rng, 20);
        for (int j = 0; j < 20; j++) cs.walk_all(m, kKs[rng() % 7], rng(), j % 5 == 0 ? ~0ull - rng() % 1000 : rng());
    }
    return cs;
}

#define HIP_OK(call)                                                                              \
    do {                                                                                          \
        const hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 2;                                                                             \
        }                                                                                         \
    } while (0)

static int run_device(const Cases& cs, std::vector<uint32_t>& got) {
    Case* d_cases = nullptr;
    Mod32* d_m32 = nullptr;
    Mod14* d_m14 = nullptr;
    uint32_t* d_out = nullptr;
    const uint32_t n = (uint32_t)cs.cases.size();
    HIP_OK(hipMalloc(&d_cases, cs.cases.size() * sizeof(Case)));
    HIP_OK(hipMalloc(&d_m32, cs.m32.size() * sizeof(Mod32)));
    HIP_OK(hipMalloc(&d_m14, cs.m14.size() * sizeof(Mod14)));
    HIP_OK(hipMalloc(&d_out, got.size() * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(d_cases, cs.cases.data(), cs.cases.size() * sizeof(Case), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_m32, cs.m32.data(), cs.m32.size() * sizeof(Mod32), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_m14, cs.m14.data(), cs.m14.size() * sizeof(Mod14), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xA5, got.size() * sizeof(uint32_t)));
    k_eval<<<dim3((n + 255) / 256), dim3(256)>>>(d_cases, n, d_m32, d_m14, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(got.data(), d_out, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_cases));
    HIP_OK(hipFree(d_m32));
    HIP_OK(hipFree(d_m14));
    HIP_OK(hipFree(d_out));
    return 0;
}

int main(int argc, char** argv) {
    const bool host = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc > 1 && !host) {
        fprintf(stderr, "usage: %s [--host]\n", argv[0]);
        return 2;
    }
    const Cases cs = make_cases();
    if (cs.nout >= (1ull << 32)) {
        fprintf(stderr, "too many outputs\n");
        return 2;
    }
    std::vector<uint32_t> want(cs.nout), got(cs.nout, 0xA5A5A5A5u);
    for (const Case& c : cs.cases) expect(c, cs.d[c.mod], &want[c.off]);
    if (host) {
        for (const Case& c : cs.cases) eval(c, cs.m32[c.mod], cs.m14[c.mod], &got[c.off]);
    } else {
        const int rc = run_device(cs, got);
        if (rc) return rc;
    }
    long bad = 0, per_kind[kKinds] = {}, bad_kind[kKinds] = {};
    for (const Case& c : cs.cases) {
        const uint32_t no = outputs(c);
        per_kind[c.kind]++;
        if (memcmp(&got[c.off], &want[c.off], no * sizeof(uint32_t)) == 0) continue;
        bad_kind[c.kind]++;
        if (bad++ >= 20) continue;
        uint32_t j = 0;
        while (got[c.off + j] == want[c.off + j]) j++;
        printf("FAIL %s d=%u k=%u a=%llu b=%llu value %u%s: got=%u want=%u\n", kKindName[c.kind], cs.d[c.mod], c.k,
               (unsigned long long)c.a, (unsigned long long)c.b, j, is_rec(c.kind) ? " (r, s, c, then positions)" : "",
               got[c.off + j], want[c.off + j]);
    }
    for (uint32_t kd = 0; kd < kKinds; kd++) printf("%-9s %8ld cases, %ld bad\n", kKindName[kd], per_kind[kd], bad_kind[kd]);
    EdgeCounts e;
    for (const Case& c : cs.cases) count_edges(c, cs.d[c.mod], e);
    printf("edges: below_multiple=%ld s0_dt_is_d=%ld r_s_is_d=%ld carries_all=%ld carries_none=%ld\n", e.below_multiple,
           e.s0_dt_is_d, e.r_s_is_d, e.carries_all, e.carries_none);
    printf("walk_device_test (%s): %zu cases, %llu values, %ld bad\n", host ? "host" : "device", cs.cases.size(),
           (unsigned long long)cs.nout, bad);
    return bad ? 1 : 0;
}

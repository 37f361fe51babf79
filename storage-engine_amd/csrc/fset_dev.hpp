// fset_dev.hpp — the device pieces shared by the kernels that probe a set of
// ranged filters (internal): the filter-set kernels of bloom_probe.hip and the
// fused Version probe of lset_version.hip.  The boundary points and region
// masks staged in LDS, the region lookup, the bit-sliced class tables and the
// per-key walk over them, and the answer rows' store policy.
#pragma once

#include <type_traits>

#include "kernels.hpp"
#include "keyorder.hpp"
#include "keysrc.hpp"

namespace lsmb {

// A filter set's answer rows: row i = the u64 mask's low rb bytes (rb = 1, 2,
// 4 or 8: the caller's row width, covering the highest live slot), stored
// non-temporal (nothing in the call reads them; tools/archive/r04_out_nt.sh).
// rb is uniform, so the width select is scalar.
struct MaskOut {
    uint8_t* p;
    uint32_t rb;
    __device__ __forceinline__ void put(uint64_t i, uint64_t o) const {
        if (rb == 8) __builtin_nontemporal_store(o, reinterpret_cast<uint64_t*>(p) + i);
        else if (rb == 4) __builtin_nontemporal_store((uint32_t)o, reinterpret_cast<uint32_t*>(p) + i);
        else if (rb == 2) __builtin_nontemporal_store((uint16_t)o, reinterpret_cast<uint16_t*>(p) + i);
        else __builtin_nontemporal_store((uint8_t)o, p + i);
    }
};

// Per workgroup: the set's boundary points and region masks into LDS.
struct FsetLds {
    uint64_t w0[kFsetMaxPoints], w1[kFsetMaxPoints];
    const uint8_t* p[kFsetMaxPoints];
    uint32_t len[kFsetMaxPoints];
    uint64_t regmask[2 * kFsetMaxPoints + 1];
};

__device__ __forceinline__ void stage_ranges(const FsetRanges& rg, FsetLds& L) {
    for (uint32_t j = threadIdx.x; j < rg.npts; j += blockDim.x) {
        const FsetPoint q = rg.pts[j];
        L.w0[j] = q.w0;
        L.w1[j] = q.w1;
        L.p[j] = q.p;
        L.len[j] = q.len;
    }
    for (uint32_t j = threadIdx.x; j < 2 * rg.npts + 1; j += blockDim.x) L.regmask[j] = rg.regmask[j];
}

// The key's region among the sorted points: a branch-free binary search on
// the 16-byte prefixes (a uniform loop of ceil(log2(npts + 1)) steps), then
// exact compares over the run of points whose prefix equals the key's (rare:
// keys or bounds longer than 16 bytes sharing their first 16).
__device__ __forceinline__ uint32_t key_region(const Pfx16& kx, const uint8_t* kp, uint64_t kl, const FsetLds& L,
                                               uint32_t m) {
    uint32_t lo = 0;
    for (uint32_t step = m ? 1u << (31 - __builtin_clz(m)) : 0u; step; step >>= 1) {
        const uint32_t j = lo + step - 1;
        if (j < m) {
            const uint64_t a = L.w0[j], b = L.w1[j];
            if (a < kx.w0 || (a == kx.w0 && b < kx.w1)) lo += step;
        }
    }
    uint32_t e = 0;
    while (lo < m && L.w0[lo] == kx.w0 && L.w1[lo] == kx.w1) {
        const uint32_t pl = L.len[lo];
        const int c = (kl <= 16 && pl <= 16) ? (kl < pl ? -1 : (kl > pl ? 1 : 0)) : key_cmp(kp, kl, L.p[lo], pl);
        if (c > 0) {
            lo++;
            continue;
        }
        e = c == 0;
        break;
    }
    return 2 * lo + e;
}

// The size classes' LDS state besides the tables themselves.
struct FsetClassLds {
    RangedFilter fl[64];
    uint8_t mem[kFsetMaxClasses][64];  // member j -> descriptor (per-lane indexed)
};

// Per workgroup: the descriptors and the member maps into LDS (a barrier must
// follow before build_class_tables reads them).
__device__ __forceinline__ void stage_classes(const RangedFilter* __restrict__ filters, uint32_t nfilt,
                                              const FsetClasses& cl, FsetClassLds& S) {
    for (uint32_t f = threadIdx.x; f < nfilt; f += blockDim.x) S.fl[f] = filters[f];
    for (uint32_t i = threadIdx.x; i < cl.ncls * 64; i += blockDim.x) S.mem[i / 64][i % 64] = cl.cls[i / 64].mem[i % 64];
}

// A one-byte bit-sliced table of up to 8 filters at `table` (LDS, 32 * nw32
// bytes): entry p bit f = bit p of filter f's words wp[f], under the byte mask
// vm[f] (0xFF, or 0 for an absent slot, whose wp re-reads a live filter).  Each
// (word, byte) item is an 8x8 bit transpose of the filters' bytes, spread over
// all threads of the workgroup (a per-word loop of 32 x 8 bit extracts ran on
// 299 threads of 1024: ~900 VALU each).  A barrier must follow.
__device__ __forceinline__ void build_table8(const uint32_t* const (&wp)[8], const uint32_t (&vm)[8], uint32_t nw32,
                                             uint8_t* table) {
    for (uint32_t it = threadIdx.x; it < 4 * nw32; it += blockDim.x) {
        const uint32_t w = it >> 2, sh = 8 * (it & 3);
        uint64_t x = 0;
#pragma unroll
        for (uint32_t f = 0; f < 8; f++) x |= (uint64_t)((wp[f][w] >> sh) & vm[f]) << (8 * f);
        // row f, column i (filter f's bit 8 (it&3) + i) -> row i, column f
        *reinterpret_cast<uint64_t*>(table + 8 * it) = transpose8x8(x);
    }
}

// Class tables at `tables` (LDS, cl.table_bytes): thread w builds the 32
// entries of word w, 32 members a pass.  A barrier must follow.
__device__ __forceinline__ void build_class_tables(const FsetClasses& cl, const FsetClassLds& S, uint8_t* tables) {
    const FsetClass* C = cl.cls;  // uniform: scalar loads of the kernel arguments
    for (uint32_t c = 0; c < cl.ncls; c++) {
        const uint32_t nw32 = (C[c].num_bits + 31) / 32, nm = C[c].nmem, width = C[c].width;
        uint8_t* t = tables + C[c].off;
        if (width == 1) {  // (uniform) <= 8 members: 8x8 bit transposes over all threads
            const uint32_t* wp[8];
            uint32_t vm[8];
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                wp[j] = S.fl[S.mem[c][j < nm ? j : 0]].f.words32;
                vm[j] = j < nm ? 0xFFu : 0u;
            }
            build_table8(wp, vm, nw32, t);
            continue;
        }
        for (uint32_t w = threadIdx.x; w < nw32; w += blockDim.x) {
            for (uint32_t j0 = 0; j0 < nm; j0 += 32) {
                uint32_t acc[32];
#pragma unroll
                for (int b = 0; b < 32; b++) acc[b] = 0;
                for (uint32_t j = j0; j < nm && j < j0 + 32; j++) {
                    const uint32_t x = S.fl[S.mem[c][j]].f.words32[w];
#pragma unroll
                    for (int b = 0; b < 32; b++) acc[b] |= ((x >> b) & 1u) << (j - j0);
                }
#pragma unroll
                for (int b = 0; b < 32; b++) {
                    const uint32_t e = w * 32 + b;
                    if (width == 1) t[e] = (uint8_t)acc[b];
                    else if (width == 2) reinterpret_cast<uint16_t*>(t)[e] = (uint16_t)acc[b];
                    else if (width == 4) reinterpret_cast<uint32_t*>(t)[e] = acc[b];
                    else reinterpret_cast<uint32_t*>(t)[2 * e + (j0 >> 5)] = acc[b];
                }
            }
        }
    }
}

// Geometry of the kernels that hold the class tables: 1024-thread workgroups,
// two per CU for 16-B keys (registers capped at 64 for 8 waves per SIMD), one
// for the var-len / odd-length sources, which would spill at that cap.
constexpr uint32_t kClassBlock = 1024;
template <class Src>
constexpr uint32_t class_wgs_per_cu() { return std::is_same<Src, ks::Fixed16>::value ? 2u : 1u; }

// One key against the set: rm = its region's in-range mask; returns the
// descriptors (bit d = descriptor d) that are in range and may contain the
// key.  Per class with an in-range member: one walk (Walk14 below 2^14 bits),
// k table reads ANDed over the class's members, the class's hits mapped back
// to descriptor bits.  The descriptors of cl.walk_mask (classes that did not
// fit, k = 0) are walked from L2 with early exit.
__device__ __forceinline__ uint64_t classes_answer(const H128& h, uint64_t rm, const FsetClasses& cl,
                                                   const FsetClassLds& S, const uint8_t* tables) {
    const FsetClass* C = cl.cls;
    const uint32_t ncls = cl.ncls;
    uint64_t o = 0;  // descriptor bits
    for (uint32_t c = 0; c < ncls; c++) {
        if (!(rm & C[c].mask)) continue;
        const uint8_t* t = tables + C[c].off;
        const uint32_t width = C[c].width, kc = C[c].k;
        uint64_t acc = ~0ull;
        // entry type and walk (Walk14 below 2^14 bits): uniform per class
        auto walk = [&](auto tag, auto pw, const auto& md) {
            using E = decltype(tag);
            const E* te = reinterpret_cast<const E*>(t);
            if (kc == 7) acc = table_and<7>(te, pw, md, kc, (E)~(E)0);
            else acc = table_and<0>(te, pw, md, kc, (E)~(E)0);
        };
        auto walk_w = [&](auto pw, const auto& md) {
            if (width == 1) walk(uint8_t{}, pw, md);
            else if (width == 2) walk(uint16_t{}, pw, md);
            else if (width == 4) walk(uint32_t{}, pw, md);
            else walk(uint64_t{}, pw, md);
        };
        if (Mod14::fits(C[c].num_bits)) {
            const Mod14 md = C[c].md14;
            walk_w(Walk14(md, h.lo, h.hi), md);
        } else {
            const Mod32 md = C[c].md;
            walk_w(Walk32(md, h.lo, h.hi), md);
        }
        if (C[c].nmem < 64) acc &= (1ull << C[c].nmem) - 1;
        while (acc) {
            const uint32_t j = (uint32_t)__builtin_ctzll(acc);
            acc &= acc - 1;
            o |= 1ull << S.mem[c][j];
        }
    }
    uint64_t wm = rm & cl.walk_mask;
    while (wm) {
        const uint32_t f = (uint32_t)__builtin_ctzll(wm);
        wm &= wm - 1;
        const RangedFilter& R = S.fl[f];
        if (words_may_contain(R.f.words32, R.f.md, R.f.k, h)) o |= 1ull << f;
    }
    return o & rm;
}

}  // namespace lsmb

// lset_walk.hpp — one key's walk over the rows of a level set (device side,
// internal), with the hash and the 16-byte prefix already in hand: the loop
// of lset.hip's probes and of the fused Version probe (lset_version.hip).
// Steps 1-4 are described at the top of lset.hip; csrc/lset_order.hpp states
// steps 1-3 in plain C++ (lset_find).  lset_row_find is one row of it, for the
// walk probe (lset_walk_first.hip).
#pragma once

#include "kernels.hpp"
#include "keyorder.hpp"

namespace lsmb {

// <0, 0, >0: the bound (prefix bw0:bw1, bytes bp[0..bl)) against the key.
// Different prefixes decide; equal ones order by length when both strings fit
// 16 bytes (they differ in trailing zero bytes at most), else by the bytes.
__device__ __forceinline__ int bound_cmp(uint64_t bw0, uint64_t bw1, const uint8_t* bp, uint32_t bl, const Pfx16& kx,
                                         const uint8_t* kp, uint64_t kl) {
    if (bw0 != kx.w0) return bw0 < kx.w0 ? -1 : 1;
    if (bw1 != kx.w1) return bw1 < kx.w1 ? -1 : 1;
    if (bl <= 16 && kl <= 16) return bl < kl ? -1 : (bl > kl ? 1 : 0);
    return -key_cmp(kp, kl, bp, bl);
}

// Key i (hash h, prefix kx, bytes kp[0..kl)) over every row: kOrdinal = false
// stores the hit's table id at out[r * stride + i]; kOrdinal = true its
// ordinal (the tables of rows 0 .. r-1, then its place in row r's sealed
// order), for the lists probe (lset_lists.hip).
template <bool kOrdinal>
__device__ __forceinline__ void lset_rows_walk(const H128& h, const Pfx16& kx, const uint8_t* kp, uint64_t kl,
                                               const LsetRows& rows, uint32_t* __restrict__ out, uint64_t stride,
                                               uint64_t i) {
    uint32_t base = 0;  // ordinal of the row's first table
    for (uint32_t r = 0; r < rows.nrows; r++) {
        const LsetRow& R = rows.row[r];
        const uint32_t m = R.ntab;
        // branch-free lower bound: a uniform loop of ceil(log2(m + 1)) steps
        uint32_t lo = 0;
        for (uint32_t step = m ? 1u << (31 - __builtin_clz(m)) : 0u; step; step >>= 1) {
            const uint32_t j = lo + step - 1;
            if (j < m) {
                const ulonglong2 q = R.hi_pfx[j];
                if (q.x < kx.w0 || (q.x == kx.w0 && q.y < kx.w1)) lo += step;
            }
        }
        while (lo < m) {
            const ulonglong2 q = R.hi_pfx[lo];
            if (q.x != kx.w0 || q.y != kx.w1) break;  // max_key's prefix above the key's: max_key > key
            const LsetTable& T = R.tab[lo];
            if (bound_cmp(q.x, q.y, T.hi, T.hi_len, kx, kp, kl) >= 0) break;
            lo++;
        }
        uint32_t ans = kLsetNone;
        if (lo < m) {
            const LsetTable& T = R.tab[lo];
            if (bound_cmp(T.lo_w0, T.lo_w1, T.lo, T.lo_len, kx, kp, kl) <= 0) {
                // words_may_contain, written out: called here, the lists probe measured 0.3 % slower (AB_LOG.md)
                bool hit = true;
                const uint32_t k = T.k;
                if (k) {
                    const Mod32 md = T.md;
                    const uint32_t* __restrict__ w = T.words32;
                    PosWalk pw(md, h.lo, h.hi);
                    for (uint32_t j = 0; j < k; j++) {
                        const uint32_t p = pw.pos();
                        if (!((w[p >> 5] >> (p & 31)) & 1u)) {
                            hit = false;
                            break;
                        }
                        pw.next(md);
                    }
                }
                if (hit) ans = kOrdinal ? base + lo : T.id;
            }
        }
        out[(uint64_t)r * stride + i] = ans;
        base += m;
    }
}

// One row of that walk on its own, for the walk probe (lset_walk_first.hip),
// which stops at a key's first hit: the place in R's sealed order of the one
// table that answers the key, else kLsetNone.  The row search above the
// filter walk is stated twice on purpose: as one function called from
// lset_rows_walk it costs k_lset_version<VarLen, ordinal> 95 -> 106 VGPRs
// (occupancy 5 -> 4) and the FixedN forms of k_lset_probe, k_lset_probe_ord
// and k_lset_version two more SGPR spills each.  The filter walk is
// words_may_contain here; lset_rows_walk writes the same loop out, where the
// call moves no register but measured slower in the lists probe.
__device__ __forceinline__ uint32_t lset_row_find(const H128& h, const Pfx16& kx, const uint8_t* kp, uint64_t kl,
                                                  const LsetRow& R) {
    const uint32_t m = R.ntab;
    uint32_t lo = 0;
    for (uint32_t step = m ? 1u << (31 - __builtin_clz(m)) : 0u; step; step >>= 1) {
        const uint32_t j = lo + step - 1;
        if (j < m) {
            const ulonglong2 q = R.hi_pfx[j];
            if (q.x < kx.w0 || (q.x == kx.w0 && q.y < kx.w1)) lo += step;
        }
    }
    while (lo < m) {
        const ulonglong2 q = R.hi_pfx[lo];
        if (q.x != kx.w0 || q.y != kx.w1) break;
        const LsetTable& T = R.tab[lo];
        if (bound_cmp(q.x, q.y, T.hi, T.hi_len, kx, kp, kl) >= 0) break;
        lo++;
    }
    if (lo >= m) return kLsetNone;
    const LsetTable& T = R.tab[lo];
    if (bound_cmp(T.lo_w0, T.lo_w1, T.lo, T.lo_len, kx, kp, kl) > 0) return kLsetNone;
    return words_may_contain(T.words32, T.md, T.k, h) ? lo : kLsetNone;
}

}  // namespace lsmb

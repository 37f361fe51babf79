// fset_plan.hpp — the host side of a set of up to 64 ranged filters whose key
// ranges may overlap in any way: a filter set (lsmb_fset, capi_fset.hip) and
// the L0 part of a level set (lsmb_lset, capi_lset.hip) plan their probes
// here.  From the tables' ranges and filter geometries:
//   * the sorted distinct boundary points with one in-range mask per region
//     (FsetRanges, fset_types.hpp),
//   * the RangedFilter descriptors,
//   * the (num_bits, k) size classes with their LDS offsets (FsetClasses),
// and a plain statement of the answer the kernels (bloom_probe.hip,
// lset_version.hip) give per key: a region lookup, then a literal may_contain
// per in-range table (src/sstable/reader.rs:192-199, src/bloom/mod.rs:82-94).
// Plain C++: nothing here touches a device, so tests/cpp/fset_plan_test.cpp
// drives it on a CPU.  Internal.
#pragma once

#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fset_types.hpp"
#include "lset_order.hpp"

namespace lsmb {

// One table of the set, descriptor d = its index: the range [lo, hi] and the
// filter's geometry.
struct FsetPlanTable {
    const uint8_t* lo;
    uint64_t lo_len;
    const uint8_t* hi;
    uint64_t hi_len;
    uint32_t num_bits, k;
};

struct FsetPlan {
    // the distinct bounds, sorted as Rust's [u8] Ord (std::vector<uint8_t> <
    // is the same unsigned lexicographic order, a proper prefix first)
    std::vector<std::vector<uint8_t>> pts;
    // region 2r = (P[r-1], P[r]), region 2r+1 = {P[r]}: bit d = descriptor d's
    // range holds every key of the region
    std::vector<uint64_t> regmask;  // 2 * pts.size() + 1
    std::vector<uint8_t> blob;      // the points' bytes back to back
    std::vector<FsetPoint> points;  // p = the point's OFFSET in blob, until the blob has a device address
    FsetClasses cl;
    uint32_t shared_nb = 0, shared_k = 0;  // (num_bits, k) of every table, or 0 when they differ
};

inline void fset_plan(const FsetPlanTable* t, uint32_t n, FsetPlan* pl) {
    pl->pts.clear();
    for (uint32_t d = 0; d < n; d++) {
        pl->pts.emplace_back(t[d].lo, t[d].lo + t[d].lo_len);
        pl->pts.emplace_back(t[d].hi, t[d].hi + t[d].hi_len);
    }
    auto& pts = pl->pts;
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    const uint32_t m = (uint32_t)pts.size();
    pl->regmask.assign(2 * (size_t)m + 1, 0);
    for (uint32_t d = 0; d < n; d++) {
        const std::vector<uint8_t> lo(t[d].lo, t[d].lo + t[d].lo_len), hi(t[d].hi, t[d].hi + t[d].hi_len);
        if (hi < lo) continue;  // an empty range holds no key
        const uint32_t a = (uint32_t)(std::lower_bound(pts.begin(), pts.end(), lo) - pts.begin());
        const uint32_t b = (uint32_t)(std::lower_bound(pts.begin(), pts.end(), hi) - pts.begin());
        for (uint32_t reg = 2 * a + 1; reg <= 2 * b + 1; reg++) pl->regmask[reg] |= 1ull << d;
    }
    pl->blob.clear();
    pl->points.resize(m);
    for (uint32_t j = 0; j < m; j++) {
        const auto& p = pts[j];
        const HostPfx16 px = host_prefix16(p.data(), p.size());
        FsetPoint& fp = pl->points[j];
        fp.w0 = px.w0;
        fp.w1 = px.w1;
        fp.p = (const uint8_t*)(uintptr_t)pl->blob.size();
        fp.len = (uint32_t)p.size();
        fp.pad = 0;
        pl->blob.insert(pl->blob.end(), p.begin(), p.end());
    }
    // size classes: descriptors grouped by (num_bits, k); the classes with the
    // smallest tables go to LDS first (most filters per byte), the rest and
    // k = 0 filters are walked from L2
    memset(&pl->cl, 0, sizeof pl->cl);
    std::vector<std::pair<uint64_t, uint32_t>> keyd;  // (num_bits << 32 | k, descriptor)
    for (uint32_t j = 0; j < n; j++)
        if (t[j].k) keyd.push_back({((uint64_t)t[j].num_bits << 32) | t[j].k, j});
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
    std::stable_sort(all.begin(), all.end(), [&](const FsetClass& x, const FsetClass& y) { return tbytes(x) < tbytes(y); });
    uint64_t off = 0, in_lds = 0;
    uint32_t ncls = 0;
    for (auto& c : all) {
        const uint64_t tb = (tbytes(c) + 15) & ~15ull;
        if (ncls < kFsetMaxClasses && off + tb <= kFsetTableBytes) {
            c.off = (uint32_t)off;
            off += tb;
            in_lds |= c.mask;
            pl->cl.cls[ncls++] = c;
        }
    }
    const uint64_t all_desc = n == 64 ? ~0ull : (1ull << n) - 1;
    pl->cl.ncls = ncls;
    pl->cl.table_bytes = (uint32_t)off;
    pl->cl.walk_mask = all_desc & ~in_lds;
    pl->shared_nb = n ? t[0].num_bits : 0;
    pl->shared_k = n ? t[0].k : 0;
    for (uint32_t j = 0; j < n; j++)
        if (t[j].num_bits != pl->shared_nb || t[j].k != pl->shared_k) pl->shared_nb = pl->shared_k = 0;
}

// Descriptor of a table whose filter words are at words32 (device memory);
// out_bit = the bit of the answer mask it reports on.
inline RangedFilter fset_plan_desc(const uint32_t* words32, uint32_t num_bits, uint32_t k, uint32_t out_bit) {
    RangedFilter r;
    memset(&r, 0, sizeof r);
    r.f.words32 = words32;
    r.f.md = Mod32::make(num_bits ? num_bits : 1);
    r.f.num_bits = num_bits;
    r.f.k = k;
    r.f.out_bit = out_bit;
    r.f.group = out_bit;
    return r;
}

// The key's region among the plan's points, as the kernels find it
// (key_region): the first point whose prefix is not below the key's, exact
// compares over the points that share the key's prefix, then 2 * rank + (the
// key equals that point).
inline uint32_t fset_plan_region(const FsetPlan& pl, const uint8_t* key, uint64_t len) {
    const uint32_t m = (uint32_t)pl.points.size();
    const HostPfx16 kx = host_prefix16(key, len);
    auto pfx = [&](uint32_t j) {
        HostPfx16 q;
        q.w0 = pl.points[j].w0;
        q.w1 = pl.points[j].w1;
        return q;
    };
    uint32_t lo = 0;
    for (uint32_t step = m ? 1u << (31 - __builtin_clz(m)) : 0u; step; step >>= 1) {
        const uint32_t j = lo + step - 1;
        if (j < m && pfx(j) < kx) lo += step;
    }
    uint32_t e = 0;
    while (lo < m && pfx(lo) == kx) {
        const int c = bytes_cmp(key, len, pl.pts[lo].data(), pl.pts[lo].size());
        if (c > 0) {
            lo++;
            continue;
        }
        e = c == 0;
        break;
    }
    return 2 * lo + e;
}

// BloomFilter::may_contain as the reference states it (src/bloom/mod.rs:82-94,
// 192-197): (h1 + i * h2) % num_bits with wrapping sums and a plain `%`.
inline bool fset_plan_may_contain(const uint64_t* words, uint32_t num_bits, uint32_t k, const uint8_t* key,
                                  uint64_t len) {
    const H128 h = xxh3_128(key, len);
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t p = (h.lo + (uint64_t)i * h.hi) % num_bits;
        if (!((words[p >> 6] >> (p & 63)) & 1)) return false;
    }
    return true;
}

// The answer for one key: bit d = (lo_d <= key <= hi_d) && may_contain(filter
// d, key), words[d] = table d's u64 words (host memory).
inline uint64_t fset_plan_answer(const FsetPlan& pl, const FsetPlanTable* t, const uint64_t* const* words,
                                 const uint8_t* key, uint64_t len) {
    uint64_t in = pl.regmask[fset_plan_region(pl, key, len)], m = 0;
    while (in) {
        const uint32_t d = (uint32_t)__builtin_ctzll(in);
        in &= in - 1;
        if (fset_plan_may_contain(words[d], t[d].num_bits, t[d].k, key, len)) m |= 1ull << d;
    }
    return m;
}

}  // namespace lsmb

// lset_order.hpp — the host side of a level set's rows (lsmb_lset), free of
// HIP so that tests/cpp/lset_order_test.cpp can drive it on a CPU: the order
// of a row's tables, the disjointness check lsmb_lset_seal makes, the 16-byte
// search prefixes it uploads, and a plain statement of the search the kernel
// (lset.hip) runs per key and row.  Internal.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace lsmb {

// Byte-string order as Rust's `[u8]` Ord (a proper prefix sorts first): <0, 0, >0.
inline int bytes_cmp(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const uint64_t m = la < lb ? la : lb;
    const int c = m ? memcmp(a, b, m) : 0;
    if (c) return c < 0 ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// The first 16 bytes, zero-padded, as two big-endian words (prefix16 of the
// kernels).  a <= b in byte order implies prefix(a) <= prefix(b); the converse
// fails only between strings of equal prefix.
struct HostPfx16 {
    uint64_t w0 = 0, w1 = 0;
    bool operator<(const HostPfx16& o) const { return w0 < o.w0 || (w0 == o.w0 && w1 < o.w1); }
    bool operator==(const HostPfx16& o) const { return w0 == o.w0 && w1 == o.w1; }
};
inline HostPfx16 host_prefix16(const uint8_t* p, uint64_t len) {
    HostPfx16 r;
    for (uint64_t i = 0; i < len && i < 16; i++) {
        const uint64_t b = p[i];
        if (i < 8) r.w0 |= b << (56 - 8 * i);
        else r.w1 |= b << (56 - 8 * (i - 8));
    }
    return r;
}

// One table of a row: its key range [lo, hi] and the caller's id.
struct LsetRange {
    const uint8_t* lo;
    uint64_t lo_len;
    const uint8_t* hi;
    uint64_t hi_len;
    uint32_t id;
};

// Why a row cannot be sealed: tables a and b (ids; a == b for a table whose
// own min_key exceeds its max_key).
struct LsetOrderError {
    uint32_t id_a = 0, id_b = 0;
    bool inverted = false;  // min_key > max_key of table id_a
};

// order = the row's tables sorted by min_key.  True when every table has
// min <= max and each max is strictly below the next table's min (so the
// ranges are pairwise disjoint and the max keys ascend strictly too);
// otherwise false with the first offending pair in sorted order.
inline bool lset_order_row(const LsetRange* t, uint32_t n, std::vector<uint32_t>* order, LsetOrderError* err) {
    order->resize(n);
    for (uint32_t j = 0; j < n; j++) (*order)[j] = j;
    std::stable_sort(order->begin(), order->end(), [&](uint32_t x, uint32_t y) {
        return bytes_cmp(t[x].lo, t[x].lo_len, t[y].lo, t[y].lo_len) < 0;
    });
    for (uint32_t j = 0; j < n; j++) {
        const LsetRange& a = t[(*order)[j]];
        if (bytes_cmp(a.lo, a.lo_len, a.hi, a.hi_len) > 0) {
            *err = LsetOrderError{a.id, a.id, true};
            return false;
        }
        if (j + 1 < n) {
            const LsetRange& b = t[(*order)[j + 1]];
            if (bytes_cmp(a.hi, a.hi_len, b.lo, b.lo_len) >= 0) {
                *err = LsetOrderError{a.id, b.id, false};
                return false;
            }
        }
    }
    return true;
}

constexpr uint32_t kLsetNoTable = 0xFFFFFFFFu;

// The search, over a sealed row (t sorted as lset_order_row leaves it, hi_pfx[j]
// = host_prefix16 of t[j].hi): the index of the one table whose range holds
// the key, or kLsetNoTable.
//   1. lower bound on the prefixes: the first j with hi_pfx[j] >= prefix(key).
//      Every table before it has max < key;
//   2. tie-break: tables whose max prefix EQUALS the key's may still sort
//      below the key (bounds or keys longer than 16 bytes sharing their first
//      16, or differing in trailing zero bytes): step over them by full compares;
//   3. j is now the first table with max >= key, the only candidate since the
//      ranges are disjoint: it holds the key iff min_j <= key.
inline uint32_t lset_find(const LsetRange* t, const HostPfx16* hi_pfx, uint32_t n, const uint8_t* key, uint64_t len) {
    const HostPfx16 kx = host_prefix16(key, len);
    uint32_t lo = 0;
    for (uint32_t step = n ? 1u << (31 - __builtin_clz(n)) : 0u; step; step >>= 1) {
        const uint32_t j = lo + step - 1;
        if (j < n && hi_pfx[j] < kx) lo += step;
    }
    while (lo < n && hi_pfx[lo] == kx && bytes_cmp(t[lo].hi, t[lo].hi_len, key, len) < 0) lo++;
    if (lo == n) return kLsetNoTable;
    return bytes_cmp(t[lo].lo, t[lo].lo_len, key, len) <= 0 ? lo : kLsetNoTable;
}

}  // namespace lsmb

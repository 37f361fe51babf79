// keyorder.hpp — byte-string order of keys on the device (internal): the
// compare and the 16-byte search prefix shared by the filter-set kernels
// (bloom_probe.hip) and the level-set kernel (lset.hip).
#pragma once

#include "xxh3.hpp"

namespace lsmb {

// Lexicographic byte-string order, as Rust's `[u8]` Ord (a proper prefix
// sorts first): <0, 0, >0.  Eight bytes per step as big-endian u64 (unaligned
// dwordx2 loads), the tail byte by byte.
__device__ __forceinline__ int key_cmp(const uint8_t* a, uint64_t la, const uint8_t* b, uint32_t lb) {
    const uint64_t m = la < lb ? la : lb;
    uint64_t i = 0;
    for (; i + 8 <= m; i += 8) {
        const uint64_t x = __builtin_bswap64(xx::ld64(a + i)), y = __builtin_bswap64(xx::ld64(b + i));
        if (x != y) return x < y ? -1 : 1;
    }
    for (; i < m; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// A byte string's first 16 bytes, zero-padded, as two big-endian words.  Two
// strings whose padded prefixes differ order as the prefixes do (a difference
// inside the padding means the shorter one is a proper prefix of the other);
// equal prefixes order by length when both fit 16 bytes, else by key_cmp.
struct Pfx16 {
    uint64_t w0, w1;
    uint32_t len;
};

__device__ __forceinline__ Pfx16 prefix16(const uint8_t* p, uint64_t len) {
    Pfx16 r;
    r.len = len > 0xffffffffull ? 0xffffffffu : (uint32_t)len;
    if (len >= 16) {
        r.w0 = __builtin_bswap64(xx::ld64(p));
        r.w1 = __builtin_bswap64(xx::ld64(p + 8));
    } else {
        r.w0 = r.w1 = 0;
        for (uint32_t i = 0; i < (uint32_t)len; i++) {
            const uint64_t b = p[i];
            if (i < 8) r.w0 |= b << (56 - 8 * i);
            else r.w1 |= b << (56 - 8 * (i - 8));
        }
    }
    return r;
}

}  // namespace lsmb

// popcount_seg.hpp — the host side of a level set's fill census
// (lsmb_lset_census, capi_lset.hip; the kernel is k_popcount_segs,
// lset_census.hip), free of HIP so that tests/cpp/popcount_seg_test.cpp can
// drive it on a CPU: the items a Version's tables are cut into
// (popcount_items), the sum of the item counts back per table (popcount_fold)
// and a serial statement of the kernel (popcount_segs_ref).  Internal.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace lsmb {

// One segment of k_popcount_segs (the ABI of lsmb_popcount_segs_dev): the set
// bits among bits 0 .. nbits-1 of the LE u64 words at `words`, 16-byte
// aligned.  ceil(nbits / 64) words are read and not a byte more; bits at or
// above nbits in the last of them do not count (0: nothing is read).
struct PopSeg {
    const void* words;
    uint64_t nbits;
};
static_assert(sizeof(PopSeg) == 16, "the ABI's (words, bits) pairs");

// k_popcount_segs: one wave per item, four items per workgroup; each lane
// keeps kPopSegInFlight 16-byte loads in flight before it counts them, so one
// iteration of a wave reads kPopSegIterBytes.
constexpr uint32_t kPopSegLanes = 64;
constexpr uint32_t kPopSegPerBlock = 4;
constexpr uint32_t kPopSegInFlight = 4;
constexpr uint64_t kPopSegIterBytes = (uint64_t)kPopSegLanes * kPopSegInFlight * 16;  // 4096

// A table's words are cut into items of at most this many bytes (the cut of
// kRepackItemBytes, lset_repack.hpp), so that a filter of hundreds of
// megabytes spreads over many waves.
constexpr uint64_t kPopItemBytes = 64u << 10;
constexpr uint64_t kPopItemBits = kPopItemBytes * 8;

inline uint64_t popcount_words(uint64_t nbits) { return nbits / 64 + (nbits % 64 != 0); }

// The items of tables 0 .. ntab-1, table t's filter being nbits[t] bits at
// words[t] (16-byte aligned): every item but a table's last covers
// kPopItemBits bits, whole words, and the last the rest, so the items of a
// table tile its bits exactly and each starts 16-byte aligned.  A table of no
// bits has no item.  table_of[i] = the table of item i.
inline void popcount_items(const void* const* words, const uint64_t* nbits, uint64_t ntab, std::vector<PopSeg>* items,
                           std::vector<uint32_t>* table_of) {
    items->clear();
    table_of->clear();
    for (uint64_t t = 0; t < ntab; t++)
        for (uint64_t at = 0; at < nbits[t]; at += kPopItemBits) {
            items->push_back(PopSeg{(const void*)((uintptr_t)words[t] + at / 8), std::min(kPopItemBits, nbits[t] - at)});
            table_of->push_back((uint32_t)t);
        }
}

// out[t] = the sum of the counts of table t's items (0 for a table without).
inline void popcount_fold(const uint64_t* counts, const uint32_t* table_of, uint64_t nitems, uint64_t ntab,
                          uint64_t* out) {
    std::fill(out, out + ntab, (uint64_t)0);
    for (uint64_t i = 0; i < nitems; i++) out[table_of[i]] += counts[i];
}

// k_popcount_segs, serially.
inline void popcount_segs_ref(const PopSeg* segs, uint64_t nseg, uint64_t* out) {
    for (uint64_t s = 0; s < nseg; s++) {
        const uint8_t* p = (const uint8_t*)segs[s].words;
        const uint64_t full = segs[s].nbits / 64;  // words wholly below nbits
        const uint32_t rem = (uint32_t)(segs[s].nbits % 64);
        uint64_t cnt = 0, w;
        for (uint64_t i = 0; i < full; i++) {
            memcpy(&w, p + 8 * i, 8);
            cnt += (uint64_t)__builtin_popcountll(w);
        }
        if (rem) {
            memcpy(&w, p + 8 * full, 8);
            cnt += (uint64_t)__builtin_popcountll(w & ((1ull << rem) - 1));
        }
        out[s] = cnt;
    }
}

}  // namespace lsmb

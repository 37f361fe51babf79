// lset_arena.hpp — where a level set's filters go in its device arena
// (lsmb_lset_add*, capi_lset.hip), as a pure function of the arena's bump state
// and the filters' word counts.  No HIP calls and no lsmb_lset here, so that
// tests/cpp/lset_arena_test.cpp can drive it on a CPU: an add plans its whole
// placement first, allocates and copies next, and touches the set only once
// everything has succeeded.  It is also the one statement of the 16-byte slot
// rule, shared with the batched build's packed layout (build_batch_plan.hpp).
// Internal.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace lsmb {

constexpr size_t kLsetChunkBytes = 4u << 20;

// 16-B-aligned device memory for one filter's nw u64 words (a filter larger
// than a chunk gets a chunk of its own).
inline size_t lset_slot_bytes(uint64_t nw) { return (std::max<size_t>(nw * 8, 8) + 15) & ~(size_t)15; }

// The bump state of one set's arena.  Slots are handed out only in a chunk the
// set allocated itself (own_tail), never in the tail of an inherited one.
struct LsetArenaState {
    size_t chunks = 0;      // chunks held, inherited ones first
    bool own_tail = false;  // the last chunk is this set's own: the bump pointer may advance in it
    size_t used = 0;        // bytes handed out in the tail
    size_t cap = 0;         // the tail's capacity
};

struct LsetSlot {
    uint32_t chunk;  // index among the set's chunks, this placement's new ones counted on
    size_t off;      // byte offset in that chunk
};

// A maximal run of consecutive tables in one chunk: one copy.  src is the run's
// offset in a packed source, slot after slot from 0: the pinned staging of
// lsmb_lset_add_batch, and word_off[t] * 8 of lsmb_build_batch_layout.
struct LsetSpan {
    uint32_t chunk;
    size_t off, bytes, src;
};

struct LsetPlacement {
    std::vector<LsetSlot> slot;      // per table
    std::vector<size_t> new_chunks;  // capacities of the chunks to allocate, in order: max(slot, kLsetChunkBytes)
    std::vector<LsetSpan> spans;
    LsetArenaState after;
    size_t packed_bytes() const { return spans.empty() ? 0 : spans.back().src + spans.back().bytes; }
};

// Places filters of nw[0 .. ntab) words, in order.  A new chunk starts when the
// tail is not the set's own or the slot does not fit in it (a slot ending
// exactly at the chunk's end fits).  False, *out of no use, when that would be
// chunk number 2^32-1 or later.  Reads s, changes nothing but *out, whose
// vectors keep their capacity from an earlier call (s is not out->after).
inline bool lset_place(const LsetArenaState& s, const uint64_t* nw, uint64_t ntab, LsetPlacement* out) {
    LsetPlacement& pl = *out;
    pl.slot.clear();
    pl.new_chunks.clear();
    pl.spans.clear();
    LsetArenaState& a = pl.after = s;
    pl.slot.reserve(ntab);
    size_t packed = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        const size_t slot = lset_slot_bytes(nw[t]);
        if (!a.own_tail || a.used + slot > a.cap) {
            if (a.chunks >= UINT32_MAX) return false;
            pl.new_chunks.push_back(std::max(slot, kLsetChunkBytes));
            a.chunks++;
            a.own_tail = true;
            a.used = 0;
            a.cap = pl.new_chunks.back();
        }
        const uint32_t chunk = (uint32_t)(a.chunks - 1);
        pl.slot.push_back(LsetSlot{chunk, a.used});
        if (pl.spans.empty() || pl.spans.back().chunk != chunk) pl.spans.push_back(LsetSpan{chunk, a.used, 0, packed});
        pl.spans.back().bytes += slot;
        a.used += slot;
        packed += slot;
    }
    return true;
}

}  // namespace lsmb

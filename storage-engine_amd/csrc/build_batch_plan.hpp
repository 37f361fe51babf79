// build_batch_plan.hpp — the host side of the batched build (lsmb_build_batch_*,
// kernels in build_batch.hip): many SSTable filters from one key run in one
// launch per geometry class.  No HIP calls and no kernels here, so that
// tests/cpp/build_batch_plan_test.cpp can drive it on a CPU.  It is the one
// statement of the packed output layout (shared with the level set's arena),
// of the work list the kernels run, and of the whole transform as plain C++
// (build_batch_ref: the same items walked serially with the host compile of
// xxh3.hpp / bloom_math.hpp).  Internal.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bloom_math.hpp"
#include "lset_arena.hpp"

namespace lsmb {

// ---- the packed layout -------------------------------------------------------
// Table t's u64 words start at word_off[t]; its slot is max(ceil(num_bits/64), 1)
// words rounded up to an even count: 16-byte-aligned slots, the arena's own rule
// (lset_slot_bytes in lset_arena.hpp), so a packed buffer and the arena agree slot
// for slot and a run of slots moves into a chunk as one copy.
inline uint64_t bb_slot_words(uint32_t num_bits) { return lset_slot_bytes(((uint64_t)num_bits + 63) / 64) / 8; }

// word_off[0 .. ntab]; word_off[ntab] = the words of the whole buffer.
inline void bb_layout(uint64_t ntab, const uint32_t* num_bits, uint64_t* word_off) {
    uint64_t at = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        word_off[t] = at;
        at += bb_slot_words(num_bits[t]);
    }
    word_off[ntab] = at;
}

// ---- geometry classes ----------------------------------------------------------
// wave   one wave per item, kBbWavesPerGroup items per 256-lane workgroup, each
//        wave owning a private LDS region and meeting no workgroup barrier (as
//        k_crc32_seg per segment): thousands of ~1 KB filters.  A region is at
//        most 8 KiB, so a workgroup asks for at most 32 KiB and five of them
//        share a CU.
// group  one 1 024-lane workgroup per item with up to the whole 160 KiB of LDS,
//        as k_build_lds.
// A table with more keys than its class gives one item is split into parts over
// contiguous key sub-ranges; the parts OR their non-zero words into a slot that
// a zero pass cleared.
constexpr uint32_t kBbMaxWords32 = 40 * 1024;            // kLdsFilterMaxWords32: the largest filter
constexpr uint32_t kBbMaxBits = kBbMaxWords32 * 32;      // 1 310 720
constexpr uint32_t kBbLdsBytes = 160 * 1024;
constexpr uint32_t kBbWaveLanes = 64;
constexpr uint32_t kBbWavesPerGroup = 4;
constexpr uint32_t kBbWaveMaxBits = 65536;               // 8 KiB region
constexpr uint32_t kBbWaveKeys = 4096;                   // keys per wave item: 64 per lane
constexpr uint32_t kBbGroupLanes = 1024;
constexpr uint32_t kBbGroupKeys = 65536;                 // keys per group item: 64 per lane
constexpr uint32_t kBbMaxParts = 1u << 16;               // huge tables: longer parts, not more

// wave_max_bits below kBbWaveMaxBits (a measurement knob, LSMB_BB_WAVE_MAX_BITS)
// sends smaller filters to the group class too; the words never depend on it.
inline bool bb_is_wave(uint32_t num_bits, uint32_t wave_max_bits = kBbWaveMaxBits) { return num_bits <= wave_max_bits; }

// Items the plan gives one table of this shape (>= 1, non-decreasing in keys).
inline uint32_t bb_parts(uint64_t keys, uint32_t num_bits, uint32_t wave_max_bits = kBbWaveMaxBits) {
    const uint64_t per = bb_is_wave(num_bits, wave_max_bits) ? kBbWaveKeys : kBbGroupKeys;
    const uint64_t p = keys / per + (keys % per != 0);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(p, 1), kBbMaxParts);
}

// One unit of work, read by the kernel as it stands (64 bytes).
struct BbItem {
    uint64_t dst;             // u64 index of the table's slot in the packed buffer
    uint64_t key_lo, key_hi;  // this part's keys [key_lo, key_hi) of the run
    Mod32 md;                 // of num_bits (of 1 for a k = 0 filter of no bits)
    uint32_t k;
    uint32_t nw32;            // u32 words of the slot (a multiple of 4): zeroed in LDS, built, written out
    uint32_t table;
    uint32_t parts;           // items of this table; 1: every word stored once, plain; else atomicOr of non-zero words
};
static_assert(sizeof(BbItem) == 64, "BbItem is the device descriptor");

struct BbPlan {
    std::vector<uint64_t> word_off;  // ntab + 1
    std::vector<BbItem> wave, group; // one launch each (when non-empty)
    std::vector<BbItem> zero;        // the first part of every multi-part table: slots cleared before the launches
    uint32_t wave_region32 = 0;      // u32 words of a wave's LDS region: the largest wave item's nw32
    uint32_t group_region32 = 0;     // the same for the group launch
};

// The work list of ntab tables, table t built from the units [seg[t], seg[t+1])
// of a run (keys here; data blocks in sst_blocks.hpp) into (num_bits[t],
// num_hashes[t]), split into parts_of(t) >= 1 parts of equal unit counts.
template <class PartsOf>
inline BbPlan bb_plan_by(uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes,
                         uint32_t wave_max_bits, PartsOf&& parts_of) {
    BbPlan pl;
    pl.word_off.resize(ntab + 1);
    bb_layout(ntab, num_bits, pl.word_off.data());
    for (uint64_t t = 0; t < ntab; t++) {
        const uint64_t keys = seg[t + 1] - seg[t];
        const uint32_t parts = parts_of(t);
        const uint64_t per = keys / parts + (keys % parts != 0);
        const bool wave = bb_is_wave(num_bits[t], wave_max_bits);
        BbItem it;
        it.dst = pl.word_off[t];
        it.md = Mod32::make(num_bits[t] ? num_bits[t] : 1);
        it.k = num_hashes[t];
        it.nw32 = (uint32_t)(2 * bb_slot_words(num_bits[t]));
        it.table = (uint32_t)t;
        it.parts = parts;
        uint32_t& region = wave ? pl.wave_region32 : pl.group_region32;
        region = std::max(region, it.nw32);
        for (uint32_t p = 0; p < parts; p++) {
            it.key_lo = std::min(seg[t + 1], seg[t] + (uint64_t)p * per);
            it.key_hi = std::min(seg[t + 1], it.key_lo + per);
            (wave ? pl.wave : pl.group).push_back(it);
            if (parts > 1 && p == 0) pl.zero.push_back(it);
        }
    }
    return pl;
}

// The work list of ntab tables, table t built from keys [seg[t], seg[t+1]) into
// (num_bits[t], num_hashes[t]).  The arguments are the caller's to validate
// (seg non-decreasing, num_bits <= kBbMaxBits, num_bits > 0 unless k == 0).
inline BbPlan bb_plan(uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes,
                      uint32_t wave_max_bits = kBbWaveMaxBits) {
    return bb_plan_by(ntab, seg, num_bits, num_hashes, wave_max_bits,
                      [&](uint64_t t) { return bb_parts(seg[t + 1] - seg[t], num_bits[t], wave_max_bits); });
}

// ---- the transform, serially ---------------------------------------------------
// What one item does, lane order aside: a zeroed private image of the slot, the
// k positions of each of its keys set in it, then the image into the buffer.
inline void bb_item_ref(const BbItem& it, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                        uint64_t* words) {
    std::vector<uint32_t> img(it.nw32, 0);
    for (uint64_t i = it.key_lo; i < it.key_hi; i++) {
        const uint8_t* key = offsets ? data + offsets[i] : data + i * (uint64_t)key_len;
        const uint64_t len = offsets ? offsets[i + 1] - offsets[i] : key_len;
        const H128 h = xxh3_128(key, len);
        Walk32 w(it.md, h.lo, h.hi);
        for (uint32_t j = 0; j < it.k; j++) {
            const uint32_t p = w.pos();
            img[p >> 5] |= 1u << (p & 31);
            w.next(it.md);
        }
    }
    uint64_t* dst = words + it.dst;
    for (uint32_t q = 0; q < it.nw32 / 2; q++) {
        const uint64_t v = (uint64_t)img[2 * q] | ((uint64_t)img[2 * q + 1] << 32);
        if (it.parts == 1)
            dst[q] = v;
        else
            dst[q] |= v;
    }
}

// The launches in their order: the zero pass, the wave items, the group items.
// Every word of [0, word_off[ntab]) is written, pad words as zero.
inline void build_batch_ref(const BbPlan& pl, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                            uint64_t* words) {
    for (const BbItem& z : pl.zero)
        for (uint32_t q = 0; q < z.nw32 / 2; q++) words[z.dst + q] = 0;
    for (const BbItem& it : pl.wave) bb_item_ref(it, data, offsets, key_len, words);
    for (const BbItem& it : pl.group) bb_item_ref(it, data, offsets, key_len, words);
}

}  // namespace lsmb

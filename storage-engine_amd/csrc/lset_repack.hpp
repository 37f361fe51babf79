// lset_repack.hpp — the host side of a repacking derive
// (lsmb_lset_derive_packed, capi_lset.hip; the kernel is k_copy_segs,
// lset_repack.hip), free of HIP so that tests/cpp/lset_repack_test.cpp can drive
// it on a CPU: which surviving tables leave their parent's chunks
// (lset_repack_plan), the copy items that move them into the slots lset_place
// gave them (lset_repack_items), and a serial statement of the copy
// (copy_segs_ref).  Internal.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "lset_arena.hpp"

namespace lsmb {

// One device-to-device move of k_copy_segs (the ABI of lsmb_copy_segs_dev):
// src and dst 16-byte aligned, len a multiple of 16 (0: nothing moves), the
// two ranges disjoint.
struct CopySeg {
    const void* src;
    void* dst;
    uint64_t len;
};
static_assert(sizeof(CopySeg) == 24, "the ABI's (source, destination, length) triples");

// k_copy_segs: one wave per item, four items per workgroup; each lane keeps
// kCopySegInFlight 16-byte loads in flight before it stores them, so one
// iteration of a wave moves kCopySegIterBytes.
constexpr uint32_t kCopySegLanes = 64;
constexpr uint32_t kCopySegPerBlock = 4;
constexpr uint32_t kCopySegInFlight = 4;
constexpr uint64_t kCopySegIterBytes = (uint64_t)kCopySegLanes * kCopySegInFlight * 16;  // 4096

// A moved slot is cut into items of at most this many bytes, so that a filter
// of several megabytes spreads over many waves.
constexpr size_t kRepackItemBytes = 64u << 10;

constexpr uint32_t kLsetRepackAll = 1000001;  // LSMB_LSET_REPACK_ALL: every survivor moves

// A surviving table as the plan sees it: the parent's chunk it lives in and
// its slot there (lset_slot_bytes).
struct RepackTable {
    uint32_t chunk;
    size_t slot;
};

// Which survivors move: tab[0 .. ntab) in derive order, cap[c] the capacity of
// the parent's chunk c.  live[c] = the survivors' slot bytes in chunk c; the
// chunk is evacuated iff live[c] > 0 and live[c] * 1e6 < min_ppm * cap[c]
// (128-bit), under kLsetRepackAll iff live[c] > 0.  move[t] = 1 for every
// survivor of an evacuated chunk, 0 for the others; evac[c] likewise per chunk.
// So min_ppm == 0 moves nothing, and a filter alone in a chunk of its own
// (live == cap) moves only under kLsetRepackAll.  False, the outputs of no use,
// for min_ppm > kLsetRepackAll.
inline bool lset_repack_plan(const RepackTable* tab, uint64_t ntab, const size_t* cap, size_t nchunks,
                             uint32_t min_ppm, std::vector<uint8_t>* move, std::vector<uint8_t>* evac) {
    if (min_ppm > kLsetRepackAll) return false;
    std::vector<uint64_t> live(nchunks, 0);
    for (uint64_t t = 0; t < ntab; t++) live[tab[t].chunk] += tab[t].slot;
    evac->assign(nchunks, 0);
    for (size_t c = 0; c < nchunks; c++) {
        if (live[c] == 0) continue;
        if (min_ppm == kLsetRepackAll)
            (*evac)[c] = 1;
        else
            (*evac)[c] = (unsigned __int128)live[c] * 1000000u < (unsigned __int128)min_ppm * cap[c];
    }
    move->resize(ntab);
    for (uint64_t t = 0; t < ntab; t++) (*move)[t] = (*evac)[tab[t].chunk];
    return true;
}

// The copy items of the moved tables: table m (of pl.slot.size()) goes from
// src[m] to its slot pl.slot[m], chunk `held + j` of the placement being the
// j-th new chunk, at fresh[j]; its slot bytes are lset_slot_bytes(nw[m]), cut
// into items of at most kRepackItemBytes.  pl is lset_place's answer for nw on
// a state of `held` chunks.
inline void lset_repack_items(const LsetPlacement& pl, size_t held, uint8_t* const* fresh, const uint8_t* const* src,
                              const uint64_t* nw, std::vector<CopySeg>* items) {
    items->clear();
    for (size_t m = 0; m < pl.slot.size(); m++) {
        uint8_t* dst = fresh[pl.slot[m].chunk - held] + pl.slot[m].off;
        const size_t bytes = lset_slot_bytes(nw[m]);
        for (size_t at = 0; at < bytes; at += kRepackItemBytes)
            items->push_back(CopySeg{src[m] + at, dst + at, std::min(kRepackItemBytes, bytes - at)});
    }
}

// k_copy_segs, serially.
inline void copy_segs_ref(const CopySeg* segs, uint64_t nseg) {
    for (uint64_t s = 0; s < nseg; s++)
        if (segs[s].len) memcpy(segs[s].dst, segs[s].src, segs[s].len);
}

}  // namespace lsmb

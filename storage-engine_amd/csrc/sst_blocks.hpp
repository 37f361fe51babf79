// sst_blocks.hpp — the store's data blocks as a key source of the batched build
// (lsmb_build_batch_sst_*, kernels in build_batch_sst.hip).  The one statement
// of the block format for the host and the device, the check of a caller's
// claimed blocks, the host plan and the transform as plain C++ (sst_check_claim,
// sst_plan, build_batch_sst_ref).  No HIP
// calls and no kernels here, so that tests/cpp/sst_blocks_test.cpp can drive it
// on a CPU.  Internal.
//
// A data block as BlockBuilder::build leaves it (src/sstable/block/builder.rs:
// 40-76; read back by Block::decode / key_at, src/sstable/block/reader.rs:18-44):
//   [klen u16][vlen u16][key][value] ... [off u16 ...][n u16]
// all little-endian, `off` from the block's start.  A block of len bytes is
// well-formed when
//   len >= 2, n = the u16 at len - 2;
//   2 + 2n <= len, data_end = len - 2 - 2n;
//   for every i < n, with off = the u16 at data_end + 2i, klen = the u16 at off
//   and vlen = the u16 at off + 2:  off + 4 <= data_end  and
//   off + 4 + klen + vlen <= data_end.
// Nothing else is asked: offsets need not ascend, entries may overlap, an empty
// key is a key, and so is the key of an empty value (a tombstone:
// src/sstable/builder.rs:93 adds the key before it looks at the value).  A
// single-entry block may be longer than 65 535 bytes (block/builder.rs:45: the
// first entry is always accepted), so every length here is 32 bits wide.
//
// No function reads a byte outside [blk, blk + len), whatever the bytes are:
// each bound is checked before the load that depends on it, and blocks sit at
// any byte offset (every multi-byte read is a memcpy-style load, as xxh3.hpp's).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "build_batch_plan.hpp"

namespace lsmb {

constexpr uint32_t kSstBadBlock = 0xFFFFFFFFu;  // LSMB_SST_BAD_BLOCK of include/lsmbloom.h

LSMB_HD uint32_t sst_ld16(const uint8_t* p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// ---- block head ------------------------------------------------------------------
struct SstHead {
    uint32_t n;         // entries
    uint32_t data_end;  // the entries' bytes are [0, data_end), the offset array starts there
    bool ok;
};

// The head in two steps, so that a kernel can have a block's count in flight
// while it works on another block: the raw u16 at len - 2 (0, nothing read, for
// a block too short to hold it), then the checks.
LSMB_HD uint32_t sst_head_fetch(const uint8_t* blk, uint32_t len) { return len >= 2 ? sst_ld16(blk + (len - 2)) : 0u; }
LSMB_HD SstHead sst_head_of(uint32_t raw_n, uint32_t len) {
    if (len < 2 || 2 + 2 * raw_n > len) return SstHead{0, 0, false};  // raw_n <= 65 535: no overflow
    return SstHead{raw_n, len - 2 - 2 * raw_n, true};
}
LSMB_HD SstHead sst_block_head(const uint8_t* blk, uint32_t len) { return sst_head_of(sst_head_fetch(blk, len), len); }

// ---- entry -------------------------------------------------------------------------
struct SstKey {
    uint32_t at;   // the key's bytes are blk[at .. at + len)
    uint32_t len;
    bool ok;
};

// Entry i < n of a block whose head passed.  Again in two steps: the entry's
// offset (inside the offset array: data_end + 2i + 2 <= len - 2), then the
// entry it names.
LSMB_HD uint32_t sst_entry_fetch(const uint8_t* blk, uint32_t data_end, uint32_t i) {
    return sst_ld16(blk + data_end + 2 * i);
}
LSMB_HD SstKey sst_entry_at(const uint8_t* blk, uint32_t data_end, uint32_t off) {
    if (off + 4 > data_end) return SstKey{0, 0, false};  // klen and vlen would leave the entries' bytes
    const uint32_t klen = sst_ld16(blk + off), vlen = sst_ld16(blk + off + 2);
    if (off + 4 + klen + vlen > data_end) return SstKey{0, 0, false};  // at most 4 + 3 * 65 535: no overflow
    return SstKey{off + 4, klen, true};
}
LSMB_HD SstKey sst_block_entry(const uint8_t* blk, uint32_t data_end, uint32_t n, uint32_t i) {
    if (i >= n) return SstKey{0, 0, false};
    return sst_entry_at(blk, data_end, sst_entry_fetch(blk, data_end, i));
}

// Insert of one key into a u32 image of a filter: the XXH3-128 split and the
// wrapping double-hash walk of every other build.  Or = what sets a bit (a plain
// |= on the host, ds_or in a kernel).
template <class Or>
LSMB_HD void sst_insert_key(const uint8_t* key, uint32_t len, const Mod32& md, uint32_t k, Or&& set_bit) {
    const H128 h = xxh3_128(key, len);
    Walk32 w(md, h.lo, h.hi);  // num_bits <= 1 310 720 < 2^31
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t p = w.pos();
        set_bit(p >> 5, 1u << (p & 31));
        w.next(md);
    }
}

// ---- the host plan -------------------------------------------------------------------
// One block as the kernels read it: where it starts in the byte buffer and how
// long it is.  Staged for the claimed blocks [bseg[0], bseg[ntab]) only.
struct SstBlk {
    uint64_t off;
    uint32_t len;
    uint32_t pad;
};
static_assert(sizeof(SstBlk) == 16, "SstBlk is the device descriptor");

// The work list is build_batch_plan.hpp's (bb_plan_by): a BbItem whose key_lo /
// key_hi are block_lo / block_hi, a run of the caller's blocks.  Classes by
// num_bits as bb_is_wave.  A table is split into parts by a bound on the block
// bytes an item walks.  Both bounds are what tools/mb_build_batch_sst.py
// measured on the card (profiles/AB_LOG.md): a wave item
// walks 256 KiB (64 blocks of 4 KiB, about 2 200 keys: near the 4 096 keys of a
// packed-key wave item; 64 KiB is faster while the batch leaves wave slots idle
// and slower from a few thousand tables on, 1 MiB slower on split tables), a
// group item 1 MiB spread over its 16 waves (4 MiB and 16 MiB are equal on
// SSTable-sized batches and 7 % slower on split tables).  No test pins them.
constexpr uint64_t kSstWaveBytes = 256u << 10;
constexpr uint64_t kSstGroupBytes = 1u << 20;

// The bounds as a pair, so that a measurement can move them (LSMB_SST_WAVE_BYTES /
// LSMB_SST_GROUP_BYTES, capi_build_batch.hip); the words never depend on them.
struct SstBounds {
    uint64_t wave_bytes = kSstWaveBytes, group_bytes = kSstGroupBytes;
    uint32_t wave_max_bits = kBbWaveMaxBits;
};

// Items the plan gives a table of `blocks` blocks holding `bytes` bytes: >= 1,
// non-decreasing in bytes, never more than its blocks (a block has one owner).
inline uint32_t sst_parts(uint64_t blocks, uint64_t bytes, uint32_t num_bits, const SstBounds& bd = SstBounds()) {
    const uint64_t per = std::max<uint64_t>(bb_is_wave(num_bits, bd.wave_max_bits) ? bd.wave_bytes : bd.group_bytes, 1);
    const uint64_t p = bytes / per + (bytes % per != 0);
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>({p, blocks, (uint64_t)kBbMaxParts}), 1);
}

// The work list of ntab tables, table t built from the blocks [bseg[t],
// bseg[t+1]) of (blk_len) into (num_bits[t], num_hashes[t]): bb_plan's items with
// key_lo / key_hi counting blocks.  The arguments are the caller's to validate,
// as bb_plan's.
inline BbPlan sst_plan(const uint32_t* blk_len, uint64_t ntab, const uint64_t* bseg, const uint32_t* num_bits,
                       const uint32_t* num_hashes, const SstBounds& bd = SstBounds()) {
    return bb_plan_by(ntab, bseg, num_bits, num_hashes, bd.wave_max_bits, [&](uint64_t t) {
        uint64_t bytes = 0;
        for (uint64_t b = bseg[t]; b < bseg[t + 1]; b++) bytes += blk_len[b];
        return sst_parts(bseg[t + 1] - bseg[t], bytes, num_bits[t], bd);
    });
}

// ---- the caller's claim ------------------------------------------------------------------
// What a call on blocks hands over: nblk blocks (blk_off, blk_len) of a buffer of
// nbytes bytes, and seg[0 .. ngroups], which cuts the claimed blocks [seg[0],
// seg[ngroups]) into groups (the build's tables, the compaction's sources).
struct SstClaim {
    const void* bytes;  // only ever compared with NULL here
    uint64_t nbytes, nblk;
    const uint64_t* blk_off;
    const uint32_t* blk_len;
    uint64_t ngroups;
    const uint64_t* seg;
};

// The first rule a claim breaks, in the order of the checks, and what broke it:
// `group`, seg_end = seg[ngroups], `block` with its (off, len), or the hook_rc
// that the caller's own check of `group` gave.
enum SstClaimRule { kClaimOk, kClaimNullSeg, kClaimNullBlocks, kClaimGroups, kClaimSegDescends, kClaimSegPast,
                    kClaimBlocks, kClaimGroupHook, kClaimBlockLeaves, kClaimNullBytes };
struct SstClaimFault {
    SstClaimRule rule = kClaimOk;
    uint64_t group = 0, block = 0, off = 0, seg_end = 0;
    uint32_t len = 0;
    int hook_rc = 0;
};

// The check behind every "no lane reads outside its block": after it, each
// claimed block lies inside the nbytes and there are fewer than 2^31 groups and
// claimed blocks.  Nothing is read before the rule that makes the read safe has
// passed, and no block outside the claimed run is looked at.  per_group(g) -> int,
// the caller's own rules, runs in front of g's blocks; non-zero ends the check.
template <class PerGroup>
inline SstClaimFault sst_check_claim(const SstClaim& cl, PerGroup&& per_group) {
    SstClaimFault f;
    const auto broke = [&f](SstClaimRule r) { return f.rule = r, f; };
    if (!cl.seg) return broke(kClaimNullSeg);
    if (cl.nblk && (!cl.blk_off || !cl.blk_len)) return broke(kClaimNullBlocks);
    if (cl.ngroups >= (1ull << 31)) return broke(kClaimGroups);
    for (f.group = 0; f.group < cl.ngroups; f.group++)
        if (cl.seg[f.group + 1] < cl.seg[f.group]) return broke(kClaimSegDescends);
    f.seg_end = cl.seg[cl.ngroups];
    if (f.seg_end > cl.nblk) return broke(kClaimSegPast);
    if (f.seg_end - cl.seg[0] >= (1ull << 31)) return broke(kClaimBlocks);
    for (f.group = 0; f.group < cl.ngroups; f.group++) {
        if ((f.hook_rc = per_group(f.group)) != 0) return broke(kClaimGroupHook);
        for (f.block = cl.seg[f.group]; f.block < cl.seg[f.group + 1]; f.block++) {
            f.off = cl.blk_off[f.block];
            f.len = cl.blk_len[f.block];
            if (f.off > cl.nbytes || f.len > cl.nbytes - f.off) return broke(kClaimBlockLeaves);
            if (f.len && !cl.bytes) return broke(kClaimNullBytes);
        }
    }
    return SstClaimFault();
}

// The bytes [lo, hi) that the non-empty claimed blocks of a checked claim span,
// (0, 0) when there is none; `lo` is the `origin` of bbs_work / cs_plan.
struct SstSpan {
    uint64_t lo, hi;
};
inline SstSpan sst_claim_span(const SstClaim& cl) {
    SstSpan sp{cl.nbytes, 0};
    for (uint64_t b = cl.seg[0]; b < cl.seg[cl.ngroups]; b++)
        if (cl.blk_len[b]) {
            sp.lo = std::min(sp.lo, cl.blk_off[b]);
            sp.hi = std::max(sp.hi, cl.blk_off[b] + cl.blk_len[b]);
        }
    return sp.hi < sp.lo ? SstSpan{0, 0} : sp;
}

// ---- the transform, serially ----------------------------------------------------------
// What the owner of one block does, lane order aside: the block's keys into the
// image, and the block's entry count or LSMB_SST_BAD_BLOCK.  A malformed entry
// is skipped; the well-formed entries of such a block still set their bits
// (the table's words are unspecified then, and only its own).
template <class Or>
LSMB_HD uint32_t sst_block_ref(const uint8_t* blk, uint32_t len, const Mod32& md, uint32_t k, Or&& set_bit) {
    const SstHead hd = sst_block_head(blk, len);
    if (!hd.ok) return kSstBadBlock;
    bool bad = false;
    for (uint32_t i = 0; i < hd.n; i++) {
        const SstKey e = sst_block_entry(blk, hd.data_end, hd.n, i);
        if (!e.ok) {
            bad = true;
            continue;
        }
        sst_insert_key(blk + e.at, e.len, md, k, set_bit);
    }
    return bad ? kSstBadBlock : hd.n;
}

// One item: a zeroed private image of the slot, the keys of its blocks set in
// it, then the image into the buffer (bb_item_ref's rule: a single part stores
// every word, several OR theirs in).  blk_entries may be null.
inline void sst_item_ref(const BbItem& it, const uint8_t* bytes, const uint64_t* blk_off, const uint32_t* blk_len,
                         uint64_t* words, uint32_t* blk_entries) {
    std::vector<uint32_t> img(it.nw32, 0);
    for (uint64_t b = it.key_lo; b < it.key_hi; b++) {
        const uint32_t got = sst_block_ref(bytes + blk_off[b], blk_len[b], it.md, it.k,
                                           [&](uint32_t w, uint32_t m) { img[w] |= m; });
        if (blk_entries) blk_entries[b] = got;
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
inline void build_batch_sst_ref(const BbPlan& pl, const uint8_t* bytes, const uint64_t* blk_off,
                                const uint32_t* blk_len, uint64_t* words, uint32_t* blk_entries) {
    for (const BbItem& z : pl.zero)
        for (uint32_t q = 0; q < z.nw32 / 2; q++) words[z.dst + q] = 0;
    for (const BbItem& it : pl.wave) sst_item_ref(it, bytes, blk_off, blk_len, words, blk_entries);
    for (const BbItem& it : pl.group) sst_item_ref(it, bytes, blk_off, blk_len, words, blk_entries);
}

}  // namespace lsmb

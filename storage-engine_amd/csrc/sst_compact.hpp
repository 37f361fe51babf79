// sst_compact.hpp — the surviving keys of a compaction's merged data blocks
// (lsmb_compact_sst_*, kernels in compact_sst.hip).  The one statement, for the
// host and the device, of the key order, the block descriptor, the two binary
// searches and the survivor predicate, the layout of the work buffer, and the
// whole transform as plain C++ (compact_sst_ref).  No HIP calls and no kernels
// here, so that tests/cpp/sst_compact_test.cpp can drive it on a CPU.  Internal.
//
// The blocks are sst_blocks.hpp's, format and well-formed rule unchanged.  The
// claimed blocks are cut into sources: source s is the blocks [seg[s],
// seg[s+1]), source 0 the newest (src/compaction/scheduler.rs:92-103 pushes
// task.inputs in that order; src/iterator/merge.rs:15 "lower index = newer
// source").  A source is meant to be one SSTable: keys strictly ascending in
// unsigned byte order (Vec<u8>'s cmp: a proper prefix is smaller) across its
// entries and its blocks.
//
// An entry e of source s SURVIVES when
//   1. no source s' < s holds an entry with a byte-equal key, and
//   2. drop_tombstones == 0, or e's vlen > 0.
// For ascending sources that is the set run_compaction hands to builder.add
// (scheduler.rs:152-158: MergeIterator keeps the lowest source index of equal
// keys, merge.rs:55-56,98-121; a bottommost compaction drops the keys whose
// newest version is a tombstone, scheduler.rs:147-158).  Survivors are reported
// in (block index, entry index) order.
//
// The lookup in a newer source is SSTable::get's: a binary search of the
// source's blocks by each block's last key, then a binary search inside that one
// block through its offset array.  Every "shadowed" verdict rests on a
// byte-equal key actually found (cs_block_has returns true only from a compare
// that gave 0): for sources that are not ascending a search may miss and can
// never hit falsely, so the survivor set is then a superset of the right one —
// extra filter bits, no false negative.
//
// A claimed block is BAD when it is malformed (any entry of it) or holds no
// entries (the store never writes one, src/sstable/builder.rs:112-115, and the
// search needs a last key).  A bad block holds no keys for any search — the
// block search steps over it as if it were absent — and contributes no
// survivors.  No function reads a byte outside a claimed block, whatever the
// bytes are: every load goes through sst_blocks.hpp's checked steps or is
// bounded by the two key lengths those steps returned.  Every search
// terminates on any input: each step strictly shrinks its interval.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sst_blocks.hpp"

namespace lsmb {

// ---- key order ------------------------------------------------------------------------
// Unsigned byte-lexicographic order in 8-byte steps (a memcpy-style load, byte
// swapped so that integer order is byte order) with a byte tail; reads
// min(alen, blen) bytes of each key, at any alignment.  < 0, 0, > 0.
LSMB_HD uint64_t cs_ld64be(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}
LSMB_HD int cs_key_cmp(const uint8_t* a, uint32_t alen, const uint8_t* b, uint32_t blen) {
    const uint32_t m = alen < blen ? alen : blen;
    uint32_t i = 0;
    for (; i + 8 <= m; i += 8) {
        const uint64_t x = cs_ld64be(a + i), y = cs_ld64be(b + i);
        if (x != y) return x < y ? -1 : 1;
    }
    for (; i < m; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return alen < blen ? -1 : (alen > blen ? 1 : 0);
}

// ---- the staged input and the work buffer ---------------------------------------------
// One claimed block as the kernels read it (staged by the host, renumbered from
// the first claimed block): where it lies, which source owns it and where its
// survivor bitmap starts in the work buffer's flag words.
struct CsBlk {
    uint64_t off;      // the block is bytes[off .. off + len)
    uint64_t flag_at;  // first u64 flag word of the block
    uint32_t len;
    uint32_t src;
};
static_assert(sizeof(CsBlk) == 24, "CsBlk is the device descriptor");

// What the index pass leaves for the searches: the absolute position and the
// length of the block's last key, its count and data_end, and whether it is good.
struct CsDesc {
    uint64_t last_at;
    uint32_t last_len;
    uint32_t n;
    uint32_t data_end;
    uint32_t ok;
};
static_assert(sizeof(CsDesc) == 24, "CsDesc is the work buffer's record");

constexpr uint32_t kCsNone = 0xFFFFFFFFu;  // no block
constexpr uint64_t kCsWorkAlign = 16;

// The entries a well-formed block of len bytes can hold.  Entries may overlap
// (sst_blocks.hpp), so only the offset array bounds them: 2 + 2n <= len.
LSMB_HD uint32_t cs_max_entries(uint32_t len) { return len < 2 ? 0u : ((len - 2) / 2 < 65535u ? (len - 2) / 2 : 65535u); }
LSMB_HD uint32_t cs_flag_words(uint32_t len) { return (cs_max_entries(len) + 63) / 64; }

// The work buffer of B claimed blocks holding `flag_words` flag words in all:
// the descriptors, per block the survivor count and the survivors' key bytes,
// the exclusive scans of both, the flag words.  Every part is 8-byte aligned.
struct CsLayout {
    uint64_t desc_at, cnt_at, kb_at, cnt_ex_at, kb_ex_at, flags_at, bytes;
};
LSMB_HD CsLayout cs_layout(uint64_t B, uint64_t flag_words) {
    CsLayout l;
    l.desc_at = 0;
    l.cnt_at = l.desc_at + B * sizeof(CsDesc);
    l.kb_at = l.cnt_at + B * 8;
    l.cnt_ex_at = l.kb_at + B * 8;
    l.kb_ex_at = l.cnt_ex_at + B * 8;
    l.flags_at = l.kb_ex_at + B * 8;
    l.bytes = l.flags_at + flag_words * 8;
    return l;
}

// Host-side sizing: the bytes a work buffer needs for any choice of sources over
// these nblk blocks (the claimed blocks are a sub-run of them).
inline uint64_t cs_work_bytes(uint64_t nblk, const uint32_t* blk_len) {
    uint64_t fw = 0;
    for (uint64_t b = 0; b < nblk; b++) fw += cs_flag_words(blk_len[b]);
    return cs_layout(nblk, fw).bytes;
}

// The typed views of a work buffer.
struct CsWork {
    CsDesc* desc;
    uint64_t *cnt, *kb, *cnt_ex, *kb_ex, *flags;
};
LSMB_HD CsWork cs_work_of(uint8_t* work, const CsLayout& l) {
    return CsWork{(CsDesc*)(work + l.desc_at),     (uint64_t*)(work + l.cnt_at),   (uint64_t*)(work + l.kb_at),
                  (uint64_t*)(work + l.cnt_ex_at), (uint64_t*)(work + l.kb_ex_at), (uint64_t*)(work + l.flags_at)};
}

// The host plan: the claimed blocks [sseg[0], sseg[nsrc]) renumbered from 0
// (offsets less `origin`), the sources' bounds in that numbering, the layout.
// The arguments are the caller's to validate.
struct CsPlan {
    std::vector<CsBlk> blks;
    std::vector<uint32_t> seg;  // nsrc + 1
    CsLayout lay;
};
inline CsPlan cs_plan(const uint64_t* blk_off, const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg,
                      uint64_t origin) {
    CsPlan p;
    const uint64_t b0 = sseg[0], B = sseg[nsrc] - b0;
    p.blks.resize(B);
    p.seg.resize(nsrc + 1);
    uint64_t fw = 0;
    for (uint64_t s = 0; s < nsrc; s++) {
        p.seg[s] = (uint32_t)(sseg[s] - b0);
        for (uint64_t b = sseg[s]; b < sseg[s + 1]; b++) {
            p.blks[b - b0] = CsBlk{blk_off[b] - origin, fw, blk_len[b], (uint32_t)s};
            fw += cs_flag_words(blk_len[b]);
        }
    }
    p.seg[nsrc] = (uint32_t)B;
    p.lay = cs_layout(B, fw);
    return p;
}

// ---- the index pass ---------------------------------------------------------------------
// The descriptor of a block whose head is hd, whose entries were all checked
// (`bad`: one of them failed) and whose last entry is `last`.
LSMB_HD CsDesc cs_desc_of(uint64_t off, const SstHead& hd, bool bad, const SstKey& last) {
    if (!hd.ok || hd.n == 0 || bad || !last.ok) return CsDesc{0, 0, 0, 0, 0};
    return CsDesc{off + last.at, last.len, hd.n, hd.data_end, 1};
}
// Serially: what the wave that owns the block does, lane order aside.
LSMB_HD CsDesc cs_index_block(const uint8_t* bytes, const CsBlk& bk) {
    const uint8_t* blk = bytes + bk.off;
    const SstHead hd = sst_block_head(blk, bk.len);
    if (!hd.ok || hd.n == 0) return CsDesc{0, 0, 0, 0, 0};
    bool bad = false;
    for (uint32_t i = 0; i < hd.n && !bad; i++) bad = !sst_block_entry(blk, hd.data_end, hd.n, i).ok;
    return cs_desc_of(bk.off, hd, bad, sst_block_entry(blk, hd.data_end, hd.n, hd.n - 1));
}
LSMB_HD uint32_t cs_blk_entries(const CsDesc& d) { return d.ok ? d.n : kSstBadBlock; }

// An entry's vlen: the u16 in front of the key of an entry that passed sst_entry_at.
LSMB_HD uint32_t cs_vlen(const uint8_t* blk, const SstKey& e) { return sst_ld16(blk + e.at - 2); }

// ---- the two searches --------------------------------------------------------------------
// The first good block of [lo, hi) whose last key is >= key, kCsNone when there
// is none: SSTable::get's search of the index, bad blocks stepped over as if
// absent.  [lo, hi) shrinks at every step, whatever the keys are.
LSMB_HD uint32_t cs_find_block(const uint8_t* bytes, const CsDesc* desc, uint32_t lo, uint32_t hi, const uint8_t* key,
                               uint32_t klen) {
    uint32_t ans = kCsNone;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        uint32_t m = mid;
        while (m < hi && !desc[m].ok) m++;  // the next good block at or after mid
        if (m == hi) {
            hi = mid;
            continue;
        }
        if (cs_key_cmp(bytes + desc[m].last_at, desc[m].last_len, key, klen) < 0) {
            lo = m + 1;
        } else {
            ans = m;
            hi = mid;
        }
    }
    return ans;
}

// Whether the good block d at blk holds a byte-equal key: a binary search
// through the offset array; true only from a compare that gave 0.
LSMB_HD bool cs_block_has(const uint8_t* blk, const CsDesc& d, const uint8_t* key, uint32_t klen) {
    uint32_t lo = 0, hi = d.n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const SstKey e = sst_block_entry(blk, d.data_end, d.n, mid);
        if (!e.ok) return false;  // (a good block has none)
        const int c = cs_key_cmp(blk + e.at, e.len, key, klen);
        if (c == 0) return true;
        if (c < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

// Whether a source newer than s holds the key.
LSMB_HD bool cs_shadowed(const uint8_t* bytes, const CsBlk* blks, const CsDesc* desc, const uint32_t* seg, uint32_t s,
                         const uint8_t* key, uint32_t klen) {
    for (uint32_t t = 0; t < s; t++) {
        const uint32_t m = cs_find_block(bytes, desc, seg[t], seg[t + 1], key, klen);
        if (m != kCsNone && cs_block_has(bytes + blks[m].off, desc[m], key, klen)) return true;
    }
    return false;
}

// The survivor predicate of entry e (it passed sst_entry_at) of block blk of source s.
LSMB_HD bool cs_survives(const uint8_t* bytes, const CsBlk* blks, const CsDesc* desc, const uint32_t* seg, uint32_t s,
                         int drop_tombstones, const uint8_t* blk, const SstKey& e) {
    if (drop_tombstones && cs_vlen(blk, e) == 0) return false;
    return !cs_shadowed(bytes, blks, desc, seg, s, blk + e.at, e.len);  // (source 0: no search at all)
}

// ---- the transform, serially -------------------------------------------------------------
// The mark: index every claimed block, then per block the flags, the survivor
// count and key bytes, then the scans and the four totals (survivors, survivor
// key bytes, entries seen, bad blocks).  blk_entries (of the claimed blocks,
// renumbered) may be null.
inline void compact_sst_mark_ref(const uint8_t* bytes, const CsPlan& pl, int drop_tombstones, uint8_t* work,
                                 uint32_t* blk_entries, uint64_t totals[4]) {
    const uint32_t B = (uint32_t)pl.blks.size();
    const CsWork w = cs_work_of(work, pl.lay);
    for (uint32_t b = 0; b < B; b++) {
        w.desc[b] = cs_index_block(bytes, pl.blks[b]);
        if (blk_entries) blk_entries[b] = cs_blk_entries(w.desc[b]);
    }
    for (uint32_t b = 0; b < B; b++) {
        const CsBlk& bk = pl.blks[b];
        const CsDesc d = w.desc[b];
        const uint8_t* blk = bytes + bk.off;
        uint64_t cnt = 0, kb = 0;
        for (uint32_t r = 0; d.ok && r * 64 < d.n; r++) {
            uint64_t word = 0;
            for (uint32_t i = r * 64; i < d.n && i < r * 64 + 64; i++) {
                const SstKey e = sst_block_entry(blk, d.data_end, d.n, i);
                if (!e.ok || !cs_survives(bytes, pl.blks.data(), w.desc, pl.seg.data(), bk.src, drop_tombstones, blk, e))
                    continue;
                word |= 1ull << (i & 63);
                cnt++;
                kb += e.len;
            }
            w.flags[bk.flag_at + r] = word;
        }
        w.cnt[b] = cnt;
        w.kb[b] = kb;
    }
    uint64_t t[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < B; b++) {
        w.cnt_ex[b] = t[0];
        w.kb_ex[b] = t[1];
        t[0] += w.cnt[b];
        t[1] += w.kb[b];
        t[2] += w.desc[b].ok ? w.desc[b].n : 0;
        t[3] += !w.desc[b].ok;
    }
    for (int j = 0; j < 4; j++) totals[j] = t[j];
}

// The gather after a mark of the same plan: the flagged keys back to back into
// key_data and survivors + 1 offsets, offsets[0] = 0; nothing is written at or
// past either capacity.  The head is read again from the block itself, so the
// reads stay inside the block whatever the work buffer holds.
inline void compact_sst_gather_ref(const uint8_t* bytes, const CsPlan& pl, uint8_t* work, uint8_t* key_data,
                                   uint64_t data_cap, uint64_t* key_offsets, uint64_t offs_cap) {
    const uint32_t B = (uint32_t)pl.blks.size();
    const CsWork w = cs_work_of(work, pl.lay);
    if (offs_cap) key_offsets[0] = 0;
    for (uint32_t b = 0; b < B; b++) {
        const CsBlk& bk = pl.blks[b];
        const uint8_t* blk = bytes + bk.off;
        const SstHead hd = sst_block_head(blk, bk.len);
        if (!w.desc[b].ok || !hd.ok) continue;
        uint64_t idx = w.cnt_ex[b], at = w.kb_ex[b];
        for (uint32_t i = 0; i < hd.n; i++) {
            if (!(w.flags[bk.flag_at + i / 64] >> (i & 63) & 1)) continue;
            const SstKey e = sst_block_entry(blk, hd.data_end, hd.n, i);
            const uint32_t klen = e.ok ? e.len : 0;
            for (uint32_t j = 0; j < klen; j++)
                if (at + j < data_cap) key_data[at + j] = blk[e.at + j];
            at += klen;
            idx++;
            if (idx < offs_cap) key_offsets[idx] = at;
        }
    }
}

// The whole transform: the mark, then the gather.
inline void compact_sst_ref(const uint8_t* bytes, const CsPlan& pl, int drop_tombstones, uint8_t* work,
                            uint32_t* blk_entries, uint64_t totals[4], uint8_t* key_data, uint64_t data_cap,
                            uint64_t* key_offsets, uint64_t offs_cap) {
    compact_sst_mark_ref(bytes, pl, drop_tombstones, work, blk_entries, totals);
    compact_sst_gather_ref(bytes, pl, work, key_data, data_cap, key_offsets, offs_cap);
}

}  // namespace lsmb

// build_batch_sst.hip — many SSTable filters straight from the tables' data
// blocks in one launch per geometry class (gfx950): the sibling of
// build_batch.hip for tables written long ago, whose only copy of the keys is
// interleaved with the values inside the blocks
//   [klen u16][vlen u16][key][value] ... [off u16 ...][n u16]
// (src/sstable/block/builder.rs:40-76).  The work list, the LDS image, the
// write-out and the zero pass are the batched build's (build_batch_plan.hpp,
// build_batch_dev.hpp); an item is a run of blocks instead of a run of keys, and
// the unit of work is a wave per block:
//   wave   the item's wave walks its blocks one after another;
//   group  the workgroup's waves take the item's blocks wave-strided.
// Within a block lane j takes the entries j, j + 64, ...: the entry's offset,
// its klen / vlen, then the key bytes through xxh3_128 and the double-hash walk
// into the image with ds_or.  Every step of the parse is a function of
// sst_blocks.hpp, which checks each bound before the load that depends on it:
// no lane reads outside its block, whatever the bytes are (the host has checked
// that every block lies inside the buffer).  The chain n -> off -> klen -> key
// is three round trips; the next block's n (and the descriptor of the block
// after it) is in flight while this block is hashed.
// The wave that owns a block reports it with one plain store: the entry count,
// or LSMB_SST_BAD_BLOCK.  A block has exactly one owner, so global memory sees
// no atomic beyond the multi-part word OR and equal inputs give equal bytes.
#include "build_batch_dev.hpp"
#include "sst_blocks.hpp"

namespace lsmb {
namespace {

template <bool kGroup>
__global__ __launch_bounds__(kGroup ? kBbGroupLanes : kBbWaveLanes * kBbWavesPerGroup) void k_build_batch_sst(
    const uint8_t* __restrict__ bytes, const SstBlk* __restrict__ blks, const BbItem* __restrict__ items,
    uint32_t nitems, uint32_t region32, uint32_t* __restrict__ gw, uint32_t* __restrict__ blk_entries) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bbs_lds[];
    const uint32_t L = kGroup ? blockDim.x : kBbWaveLanes;  // the lanes that share the item
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kBbWaveLanes);
    const uint32_t idx = kGroup ? blockIdx.x : blockIdx.x * kBbWavesPerGroup + wave;
    if (idx >= nitems) return;  // whole waves; the wave class meets no workgroup barrier
    const uint32_t lane = kGroup ? threadIdx.x : threadIdx.x % kBbWaveLanes;
    const uint32_t wlane = threadIdx.x % kBbWaveLanes;
    uint32_t* f = bbs_lds + (kGroup ? 0u : wave * region32);  // region32 is a multiple of 4: 16-byte aligned
    const BbItem it = items[idx];  // nw32 <= region32; key_lo / key_hi = block_lo / block_hi (sst_plan)
    const uint64_t stride = kGroup ? blockDim.x / kBbWaveLanes : 1;  // the waves that share the item's blocks

    bb_image_clear(f, it, lane, L);
    bb_sync<kGroup>();

    const auto set_bit = [f](uint32_t w, uint32_t m) { atomicOr(&f[w], m); };
    const auto desc = [&](uint64_t b) { return b < it.key_hi ? blks[b] : SstBlk{0, 0, 0}; };
    // block b's count was fetched while block b - stride was hashed, and its descriptor one block earlier
    uint64_t b = it.key_lo + (kGroup ? wave : 0u);
    SstBlk cur = desc(b), nxt = desc(b + stride);
    uint32_t raw = sst_head_fetch(bytes + cur.off, cur.len);  // (nothing is read for the empty descriptor)
    for (; b < it.key_hi; b += stride) {
        const SstBlk nn = desc(b + 2 * stride);
        const uint32_t nraw = sst_head_fetch(bytes + nxt.off, nxt.len);
        const uint8_t* blk = bytes + cur.off;
        const SstHead hd = sst_head_of(raw, cur.len);
        bool bad = !hd.ok;
        if (hd.ok) {
            // the lane's next entry offset is in flight while this entry is hashed and walked
            uint32_t i = wlane;
            uint32_t off = i < hd.n ? sst_entry_fetch(blk, hd.data_end, i) : 0u;
            for (; i < hd.n; i += kBbWaveLanes) {
                const uint32_t noff = i + kBbWaveLanes < hd.n ? sst_entry_fetch(blk, hd.data_end, i + kBbWaveLanes) : 0u;
                const SstKey e = sst_entry_at(blk, hd.data_end, off);
                if (e.ok)
                    sst_insert_key(blk + e.at, e.len, it.md, it.k, set_bit);
                else
                    bad = true;  // the entry is skipped: nothing outside the block is read
                off = noff;
            }
        }
        bad = __any(bad);  // one malformed entry in any lane
        if (blk_entries && wlane == 0) blk_entries[b] = bad ? kSstBadBlock : hd.n;
        cur = nxt;
        nxt = nn;
        raw = nraw;
    }
    bb_sync<kGroup>();

    bb_image_out(f, it, gw, lane, L);
}

}  // namespace

hipError_t launch_build_batch_sst(const uint8_t* d_bytes, const SstBlk* d_blks, const BbItem* d_items,
                                  uint32_t nzero, uint32_t nwave, uint32_t ngroup, uint32_t wave_region32,
                                  uint32_t group_region32, uint32_t group_lanes, uint64_t* d_words,
                                  uint32_t* d_blk_entries, hipStream_t st, hipEvent_t done) {
    if (group_lanes < kBbWaveLanes || group_lanes > kBbGroupLanes || group_lanes % kBbWaveLanes) return hipErrorInvalidValue;
    if (wave_region32 % 4 || group_region32 % 4 || wave_region32 * 4 * kBbWavesPerGroup > kLdsBytes ||
        group_region32 * 4 > kLdsBytes)
        return hipErrorInvalidValue;
    // (one-time attributes: function-local statics are initialised once, thread-safely)
    static const hipError_t attr_w = hipFuncSetAttribute((const void*)k_build_batch_sst<false>,
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    static const hipError_t attr_g = hipFuncSetAttribute((const void*)k_build_batch_sst<true>,
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (attr_w != hipSuccess) return attr_w;
    if (attr_g != hipSuccess) return attr_g;
    uint32_t* gw = reinterpret_cast<uint32_t*>(d_words);
    if (nwave + ngroup == 0) return done ? hipEventRecord(done, st) : hipSuccess;
    hipError_t e = hipSuccess;
    if (nzero) {
        k_bb_zero<<<dim3(nzero), dim3(256), 0, st>>>(d_items, gw);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the last launch completes `done` itself (launch_done)
    if (nwave) {
        const uint32_t nwg = (nwave + kBbWavesPerGroup - 1) / kBbWavesPerGroup;
        e = launch_done(k_build_batch_sst<false>, dim3(nwg), dim3(kBbWaveLanes * kBbWavesPerGroup),
                        wave_region32 * 4 * kBbWavesPerGroup, st, ngroup ? nullptr : done, d_bytes, d_blks, d_items + nzero,
                        nwave, wave_region32, gw, d_blk_entries);
        if (e != hipSuccess) return e;
    }
    if (ngroup)
        e = launch_done(k_build_batch_sst<true>, dim3(ngroup), dim3(group_lanes), group_region32 * 4, st, done, d_bytes,
                        d_blks, d_items + nzero + nwave, ngroup, group_region32, gw, d_blk_entries);
    return e;
}

}  // namespace lsmb

// compact_sst.hip — the surviving keys of a compaction's merged data blocks,
// resolved on the device (gfx950): which entries of the input tables' blocks
// MergeIterator would hand to the output table's builder
// (src/iterator/merge.rs:15,55-56,98-121; src/compaction/scheduler.rs:147-158),
// and those keys as a device key run.  Every step of the parse, the key order,
// the searches and the predicate are sst_blocks.hpp's and sst_compact.hpp's; the
// kernels only give them lanes.  A wave owns a block in every pass:
//   index   lane j checks the entries j, j + 64, ...; the wave writes the block's
//           descriptor (its last key, n, data_end, good or bad) and its
//           d_blk_entries value;
//   mark    rounds of 64 entries, a lane per entry: the entry's key is searched
//           in every newer source (the descriptors' last keys, then the one
//           candidate block's offset array); the round's ballot is the flag
//           word, stored by lane 0 with the block's survivor count and key bytes;
//   scan    one workgroup: the exclusive scans of the counts and the key bytes
//           over the blocks, and the four totals;
//   gather  rounds of 64 again: a flagged lane's rank among the round's flags and
//           the prefix of the round's key lengths place its key and its offset.
// Every store has one owner decided by the block and entry index, so no atomic
// decides a layout and equal inputs give equal bytes.  The lanes of a round
// diverge in the searches (their keys differ); the loads they make are the
// descriptors' last keys, shared by the whole launch and cache-resident, and
// one block per newer source.  No LDS but the scan's sixteen partial sums.
#include "sst_compact.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace lsmb {
namespace {

constexpr uint32_t kCsWaves = 4;  // waves (blocks) per workgroup of the index, mark and gather kernels
constexpr uint32_t kCsLanes = 64 * kCsWaves;
constexpr uint32_t kCsScanLanes = 1024;

// The block a wave owns, kCsNone past the end (whole waves leave together).
__device__ __forceinline__ uint32_t cs_wave_block(uint32_t B) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    const uint64_t b = (uint64_t)blockIdx.x * kCsWaves + wave;
    return b < B ? (uint32_t)b : kCsNone;
}

__global__ __launch_bounds__(kCsLanes) void k_cs_index(const uint8_t* __restrict__ bytes,
                                                       const CsBlk* __restrict__ blks, uint32_t B,
                                                       CsDesc* __restrict__ desc, uint32_t* __restrict__ blk_entries) {
    const uint32_t b = cs_wave_block(B);
    if (b == kCsNone) return;
    const uint32_t lane = threadIdx.x % 64;
    const CsBlk bk = blks[b];
    const uint8_t* blk = bytes + bk.off;
    const SstHead hd = sst_block_head(blk, bk.len);
    bool bad = !hd.ok || hd.n == 0;
    if (!bad)
        for (uint32_t r = 0; r * 64 < hd.n; r++) {  // (a uniform loop: the wave leaves at its first bad round)
            const uint32_t i = r * 64 + lane;
            if (i < hd.n && !sst_block_entry(blk, hd.data_end, hd.n, i).ok) bad = true;
            if (__any(bad)) break;
        }
    bad = __any(bad);
    const SstKey last = bad ? SstKey{0, 0, false} : sst_block_entry(blk, hd.data_end, hd.n, hd.n - 1);
    const CsDesc d = cs_desc_of(bk.off, hd, bad, last);
    if (lane == 0) {
        desc[b] = d;
        if (blk_entries) blk_entries[b] = cs_blk_entries(d);
    }
}

__global__ __launch_bounds__(kCsLanes) void k_cs_mark(const uint8_t* __restrict__ bytes, const CsBlk* __restrict__ blks,
                                                      const uint32_t* __restrict__ seg, uint32_t B, int drop_tombstones,
                                                      const CsDesc* __restrict__ desc, uint64_t* __restrict__ cnt,
                                                      uint64_t* __restrict__ kb, uint64_t* __restrict__ flags) {
    const uint32_t b = cs_wave_block(B);
    if (b == kCsNone) return;
    const uint32_t lane = threadIdx.x % 64;
    const CsBlk bk = blks[b];
    const CsDesc d = desc[b];
    const uint8_t* blk = bytes + bk.off;
    uint64_t n_live = 0, bytes_live = 0;
    for (uint32_t r = 0; d.ok && r * 64 < d.n; r++) {  // d.n <= cs_max_entries(bk.len): the flag words are the block's
        const uint32_t i = r * 64 + lane;
        bool live = false;
        uint32_t klen = 0;
        if (i < d.n) {
            const SstKey e = sst_block_entry(blk, d.data_end, d.n, i);
            live = e.ok && cs_survives(bytes, blks, desc, seg, bk.src, drop_tombstones, blk, e);
            klen = e.len;
        }
        const uint64_t word = __ballot(live);
        if (lane == 0) flags[bk.flag_at + r] = word;
        n_live += __popcll(word);
        bytes_live += live ? klen : 0u;
    }
    bytes_live = __shfl(wave_incl_scan(bytes_live, lane), 63);
    if (lane == 0) {
        cnt[b] = n_live;
        kb[b] = bytes_live;
    }
}

// One workgroup: the exclusive scans of cnt and kb over the B blocks in chunks
// of its lanes, and the totals {survivors, survivor key bytes, entries seen,
// bad blocks}, each written in full.
__global__ __launch_bounds__(kCsScanLanes) void k_cs_scan(uint32_t B, const CsDesc* __restrict__ desc,
                                                          const uint64_t* __restrict__ cnt,
                                                          const uint64_t* __restrict__ kb, uint64_t* __restrict__ cnt_ex,
                                                          uint64_t* __restrict__ kb_ex, uint64_t* __restrict__ totals) {
    __shared__ uint64_t part[kCsScanLanes / 64][4];
    const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    uint64_t carry[4] = {0, 0, 0, 0};
    for (uint64_t base = 0; base < B; base += kCsScanLanes) {
        const uint64_t b = base + threadIdx.x;
        uint64_t v[4] = {0, 0, 0, 0};
        if (b < B) {
            const CsDesc d = desc[b];
            v[0] = cnt[b];
            v[1] = kb[b];
            v[2] = d.ok ? d.n : 0u;
            v[3] = d.ok ? 0u : 1u;
        }
        uint64_t incl[4];
        for (int j = 0; j < 4; j++) incl[j] = wave_incl_scan(v[j], lane);
        if (lane == 63)
            for (int j = 0; j < 4; j++) part[wave][j] = incl[j];
        __syncthreads();
        uint64_t before[4] = {0, 0, 0, 0}, all[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (uint32_t w = 0; w < kCsScanLanes / 64; w++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (w < wave) before[j] += part[w][j];
                all[j] += part[w][j];
            }
        if (b < B) {
            cnt_ex[b] = carry[0] + before[0] + incl[0] - v[0];
            kb_ex[b] = carry[1] + before[1] + incl[1] - v[1];
        }
        for (int j = 0; j < 4; j++) carry[j] += all[j];
        __syncthreads();  // part is rewritten by the next chunk
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < 4; j++) totals[j] = carry[j];
}

__global__ __launch_bounds__(kCsLanes) void k_cs_gather(const uint8_t* __restrict__ bytes,
                                                        const CsBlk* __restrict__ blks, uint32_t B,
                                                        const CsDesc* __restrict__ desc,
                                                        const uint64_t* __restrict__ cnt_ex,
                                                        const uint64_t* __restrict__ kb_ex,
                                                        const uint64_t* __restrict__ flags, uint8_t* __restrict__ key_data,
                                                        uint64_t data_cap, uint64_t* __restrict__ key_offsets,
                                                        uint64_t offs_cap) {
    const uint32_t b = cs_wave_block(B);
    if (b == kCsNone) return;
    const uint32_t lane = threadIdx.x % 64;
    const CsBlk bk = blks[b];
    const uint8_t* blk = bytes + bk.off;
    // the head from the block itself: the reads stay inside it whatever the work buffer holds
    const SstHead hd = sst_block_head(blk, bk.len);
    if (!desc[b].ok || !hd.ok) return;
    uint64_t idx0 = cnt_ex[b], at0 = kb_ex[b];
    for (uint32_t r = 0; r * 64 < hd.n; r++) {
        const uint64_t word = flags[bk.flag_at + r];
        if (word == 0) continue;
        const bool live = word >> lane & 1;
        SstKey e{0, 0, false};
        if (live) e = sst_block_entry(blk, hd.data_end, hd.n, r * 64 + lane);
        const uint64_t klen = e.ok ? e.len : 0u;
        const uint64_t incl = wave_incl_scan(klen, lane);
        if (live) {
            const uint64_t at = at0 + incl - klen;
            const uint64_t idx = idx0 + __popcll(word & ((1ull << lane) - 1)) + 1;
            if (idx < offs_cap) key_offsets[idx] = at + klen;
            const uint8_t* src = blk + e.at;
            if (at + klen <= data_cap && at + klen >= at) {
                uint64_t j = 0;
                for (; j + 8 <= klen; j += 8) __builtin_memcpy(key_data + at + j, src + j, 8);
                for (; j < klen; j++) key_data[at + j] = src[j];
            } else {
                for (uint64_t j = 0; j < klen && at + j < data_cap; j++) key_data[at + j] = src[j];
            }
        }
        at0 += __shfl(incl, 63);
        idx0 += __popcll(word);
    }
}

inline uint32_t cs_grid(uint32_t B) { return (B + kCsWaves - 1) / kCsWaves; }

}  // namespace

hipError_t launch_compact_sst_mark(const uint8_t* d_bytes, const CsBlk* d_blks, const uint32_t* d_seg, uint32_t B,
                                   const CsLayout& lay, int drop_tombstones, uint8_t* d_work, uint32_t* d_blk_entries,
                                   uint64_t* d_totals, hipStream_t st, hipEvent_t done, int stages) {
    const CsWork w = cs_work_of(d_work, lay);
    hipError_t e = hipSuccess;
    if (B) {
        // (stages < 3, a measurement's: the passes up to that one; the event is then recorded behind them)
        k_cs_index<<<dim3(cs_grid(B)), dim3(kCsLanes), 0, st>>>(d_bytes, d_blks, B, w.desc, d_blk_entries);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (stages < 2) return done ? hipEventRecord(done, st) : hipSuccess;
        k_cs_mark<<<dim3(cs_grid(B)), dim3(kCsLanes), 0, st>>>(d_bytes, d_blks, d_seg, B, drop_tombstones, w.desc, w.cnt,
                                                              w.kb, w.flags);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (stages < 3) return done ? hipEventRecord(done, st) : hipSuccess;
    }
    // the last launch completes `done` itself (launch_done)
    return launch_done(k_cs_scan, dim3(1), dim3(kCsScanLanes), 0, st, done, B, (const CsDesc*)w.desc,
                       (const uint64_t*)w.cnt, (const uint64_t*)w.kb, w.cnt_ex, w.kb_ex, d_totals);
}

hipError_t launch_compact_sst_gather(const uint8_t* d_bytes, const CsBlk* d_blks, uint32_t B, const CsLayout& lay,
                                     const uint8_t* d_work, uint8_t* d_key_data, uint64_t data_cap,
                                     uint64_t* d_key_offsets, uint64_t offs_cap, hipStream_t st, hipEvent_t done) {
    const CsWork w = cs_work_of(const_cast<uint8_t*>(d_work), lay);
    hipError_t e = hipSuccess;
    if (offs_cap && (e = hipMemsetAsync(d_key_offsets, 0, 8, st)) != hipSuccess) return e;  // offsets[0] = 0
    if (!B) return done ? hipEventRecord(done, st) : hipSuccess;
    return launch_done(k_cs_gather, dim3(cs_grid(B)), dim3(kCsLanes), 0, st, done, d_bytes, d_blks, B,
                       (const CsDesc*)w.desc, (const uint64_t*)w.cnt_ex, (const uint64_t*)w.kb_ex,
                       (const uint64_t*)w.flags, d_key_data, data_cap, d_key_offsets, offs_cap);
}

}  // namespace lsmb

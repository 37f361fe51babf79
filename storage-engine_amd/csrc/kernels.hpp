// kernels.hpp — launchers for the Bloom build / probe kernels (internal).
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom_math.hpp"
#include "fset_lists_plan.hpp"
#include "fset_types.hpp"

namespace lsmb {

// Geometry of the partitioned build (see DESIGN.md "Build kernels").
constexpr int kSliceLog2 = 20;                        // 2^20 bits = 128 KiB LDS slice
constexpr uint32_t kSliceWords32 = 1u << (kSliceLog2 - 5);
constexpr uint32_t kSliceMask = (1u << kSliceLog2) - 1;
constexpr int kSegEntries = 24;                       // 20-bit offsets per 64-B segment
constexpr int kSegWords = 8;                          // 3 offsets per u64 word
#ifndef LSMB_SEG_STRIDE
#define LSMB_SEG_STRIDE 64  // bytes between a region's segments (measurement knob: 128 = one segment per line)
#endif
constexpr uint32_t kSegSlotBytes = LSMB_SEG_STRIDE;
constexpr uint32_t kSegSlotWords = kSegSlotBytes / 8;
constexpr int kBinBlock = 1024;                       // pass A workgroup
constexpr int kApplyBlock = 1024;                     // pass B workgroup
constexpr uint32_t kLdsFilterMaxWords32 = 40 * 1024;  // 160 KiB: whole filter in LDS
constexpr uint32_t kLdsBytes = 160 * 1024;            // LDS per CU (gfx950)
// pass A flush: segments per wave per phase posted to the cooperative stores
// (2 rounds of up to 16; C2 averages ~19).  28, not 32: the 1 KiB saved lets
// a 1e9-bit filter (954 slices, C2's exact 10 bits/key) keep 40-entry rings
// in one sweep.
constexpr uint32_t kBinJobsPerWave = 28;
constexpr uint32_t kBinJobBytes = (kBinBlock / 64) * kBinJobsPerWave * 16 + 16;  // job tables (+ alignment)
constexpr uint32_t kBinLdsBudget = kLdsBytes - kBinJobBytes;  // pass A: rings + fill words
constexpr uint32_t kBinExtraBytes = 4;                // per slice besides its ring: fill word
constexpr uint32_t kMaxBinsPerSweep = 1024;           // one owner lane per slice: <= 64 slices per wave
constexpr uint32_t kMaxRing = 1024;                   // ring entries per slice
constexpr uint32_t kMaxRegionSegs = 1u << 24;         // region capacity bound (segments)
constexpr uint32_t kOvfListCap = 16384;               // fresh builds: overflow positions listed per pass A workgroup

// How a key batch is presented to the kernels.
struct KeyBatch {
    const uint8_t* data;      // fixed: key i at data + i*key_len; var: data + offsets[i]
    const uint64_t* offsets;  // NULL for fixed-length keys
    uint32_t key_len;
    uint64_t n;
};

enum class BuildStrategy { None, Lds, Partition, Atomic, Tiled };

BuildStrategy pick_build_strategy(uint32_t num_bits, uint32_t k, uint64_t n);
const char* strategy_name(BuildStrategy s);

// Partitioned build layout for one chunk of keys.  Pass A workgroup w writes
// the 20-bit slice offsets of its keys' positions that fall in slice b into
// its private region (b, w) as 64-B segments; pass B reads every region of
// slice b.  No global atomics: each region has one writer.
struct PartitionPlan {
    uint32_t slice_log2 = kSliceLog2;  // bin width: 2^20 bits, or 2^21 where that saves sweeps
    uint32_t nbins = 0;           // ceil(num_bits / 2^slice_log2)
    uint32_t grid = 0;            // pass A workgroups = regions per slice
    uint32_t cap_segs = 0;        // region capacity, segments
    uint32_t bins_per_sweep = 0;  // slices buffered in LDS per pass A launch
    uint32_t ring = 0;            // pass A ring entries per slice (multiple of 4, >= kSegEntries)
    uint32_t sweeps = 0;
    uint32_t keys_per_lane = 1;   // pass A keys per lane per phase (2: k = 7 sweeps)
    uint64_t region_bytes = 0;    // nbins * grid * cap_segs * 64
    uint64_t counts_bytes = 0;    // nbins * grid * 4
};

// The plan in two steps (build_plan.hip).  The layout — slice_log2, nbins,
// bins_per_sweep, ring, sweeps, keys_per_lane — is a function of (num_bits, k)
// alone, so build_sweeps / sweep_words answer without a device; the capacity
// — grid, cap_segs and the byte sizes — of (layout, n, num_cus).
PartitionPlan partition_layout(uint32_t num_bits, uint32_t k);
PartitionPlan partition_capacity(PartitionPlan layout, uint32_t num_bits, uint32_t k, uint64_t n, int num_cus);
PartitionPlan plan_partition(uint32_t num_bits, uint32_t k, uint64_t n, int num_cus);

// Tiled strategy (filters of 2..kTiledMaxSlices slices): workgroup (c, s)
// builds slice s from key chunk c in LDS and stores it to scratch tile
// [c][s]; k_or_reduce then ORs the chunk tiles into the filter.
constexpr uint32_t kTiledMaxSlices = 32;
struct TiledPlan {
    uint32_t nslices = 0, chunks = 0;
    uint64_t stride32 = 0;       // u32 words per chunk tile row (nslices * 2^15)
    uint64_t scratch_bytes = 0;  // chunks * stride32 * 4
};
TiledPlan plan_tiled(uint32_t num_bits, uint64_t n, int num_cus);

// Largest key count whose plan fits `max_bytes` of workspace.
uint64_t partition_chunk_keys(uint32_t num_bits, uint32_t k, uint64_t max_bytes, int num_cus);

// Bytes per workspace buffer: what a build needs (workspace_bytes) and what
// it was handed (PartitionWorkspace::have).
struct WorkspaceBytes {
    uint64_t regions = 0;  // partition: the regions; tiled: the scratch tiles
    uint64_t counts = 0;   // partition: segments written per region
    uint64_t hashes = 0;   // 16 B per key (partition builds store 12-B walk records in them)
    uint64_t ovf = 0;      // fresh k = 7 partition builds: overflow words of the whole filter,
    uint64_t dirty = 0;    //   one mark per 2^20-bit unit of them,
    uint64_t ovl = 0;      //   kOvfListCap overflow positions per pass A workgroup per sweep
    uint64_t ovn = 0;      //   and each list's length
    bool covers(const WorkspaceBytes& need) const {
        return regions >= need.regions && counts >= need.counts && hashes >= need.hashes && ovf >= need.ovf &&
               dirty >= need.dirty && ovl >= need.ovl && ovn >= need.ovn;
    }
};

// The one workspace contract: build_dev.hip allocates by it, launch_build
// validates by it.  n = the keys of one launch_build call (a chunk); aligned16
// = 16-B keys on a 16-B-aligned base (pass A hashes them inline).
WorkspaceBytes workspace_bytes(BuildStrategy s, const PartitionPlan& pl, const TiledPlan& tp, uint32_t num_bits,
                               uint32_t k, uint64_t n, bool aligned16, bool fresh);

struct PartitionWorkspace {
    uint4* hashes = nullptr;  // k_hash output for var-len / odd-length keys
    uint64_t* regions = nullptr;
    uint32_t* counts = nullptr;
    uint32_t* err = nullptr;  // device flag, see PassA::err
    // Pass A's overflow bits (ring / region overflow, adversarial inputs) and
    // per-2^20-bit-unit marks, both all-zero between builds (pass B clears
    // what it consumes)
    uint32_t* ovf = nullptr;
    uint32_t* dirty = nullptr;
    // fresh builds: the overflow position lists and their lengths
    uint32_t* ovl = nullptr;
    uint32_t* ovn = nullptr;
    WorkspaceBytes have;  // bytes behind each pointer above
};

struct BuildTimers {
    hipEvent_t t0, t1, t2;
    bool valid = false;
};

// Builds into d_words32 (OR-accumulate; fresh: BloomFilter::new + inserts,
// the words are output-only and every word of the build's range is written).
// The workspace must cover workspace_bytes() of this call (the tiled hash
// records are optional: without them the tiles hash the keys).  Records
// t0/t1/t2 (start / pass A done / end) when timers != NULL.  sweep >= 0
// builds only the bits of that partition sweep's slices (sweep 0 = the whole
// build for the other strategies; see build_sweeps / sweep_words).
hipError_t launch_build(const KeyBatch& kb, uint32_t num_bits, uint32_t k, uint32_t* d_words32,
                        BuildStrategy s, const PartitionWorkspace& ws, int num_cus,
                        hipStream_t st, BuildTimers* timers, int sweep = -1, bool fresh = false,
                        hipEvent_t done = nullptr);  // done: completed by the build's last kernel (launch_done)

// The batched build (build_batch.hip; plan, layout and item format in
// build_batch_plan.hpp): d_items holds nzero zero-pass items, then nwave wave
// items, then ngroup group items (device memory, read by the launches on st);
// *_region32 = the u32 words of the largest slot of each class, group_lanes =
// the group class's workgroup (kBbGroupLanes; fewer only to measure).  Writes the
// slots those items name inside d_words (16-byte aligned) and nothing else.
// done (optional): completed by the last launch.  No host synchronisation.
struct BbItem;
hipError_t launch_build_batch(const KeyBatch& kb, const BbItem* d_items, uint32_t nzero, uint32_t nwave,
                              uint32_t ngroup, uint32_t wave_region32, uint32_t group_region32, uint32_t group_lanes,
                              uint64_t* d_words, hipStream_t st, hipEvent_t done = nullptr);

// The batched build over data blocks (build_batch_sst.hip; block format, plan
// and descriptors in sst_blocks.hpp): the same item list, an item's key_lo /
// key_hi naming the blocks [block_lo, block_hi) of d_blks, every one of them
// inside d_bytes (the caller has checked).  Writes the slots the items name inside d_words and, when
// d_blk_entries is non-null, d_blk_entries[b] = block b's entry count or
// LSMB_SST_BAD_BLOCK for every block of an item; nothing else.
struct SstBlk;
hipError_t launch_build_batch_sst(const uint8_t* d_bytes, const SstBlk* d_blks, const BbItem* d_items,
                                  uint32_t nzero, uint32_t nwave, uint32_t ngroup, uint32_t wave_region32,
                                  uint32_t group_region32, uint32_t group_lanes, uint64_t* d_words,
                                  uint32_t* d_blk_entries, hipStream_t st, hipEvent_t done = nullptr);

// The surviving keys of a compaction's merged data blocks (compact_sst.hip; the
// contract, the descriptors and the work buffer's layout in sst_compact.hpp).
// d_blks: the B claimed blocks, every one of them inside d_bytes (the caller
// has checked); d_seg: the nsrc + 1 source bounds over them; d_work: 16-byte
// aligned, lay.bytes long.  The mark writes the work buffer, d_totals[0 .. 4)
// and, when d_blk_entries is non-null, d_blk_entries[b] for every claimed block;
// the gather, after a mark of the same blocks on the same stream, writes
// d_key_offsets[0 .. min(survivors + 1, offs_cap)) and the keys' bytes below
// data_cap.  Nothing else is written; no host synchronisation.  stages (a
// measurement's, tools/mb_compact_sst.py): 1 = the index pass alone, 2 = index
// and mark, neither scans nor totals; 3 = the whole mark.
struct CsBlk;
struct CsLayout;
hipError_t launch_compact_sst_mark(const uint8_t* d_bytes, const CsBlk* d_blks, const uint32_t* d_seg, uint32_t B,
                                   const CsLayout& lay, int drop_tombstones, uint8_t* d_work, uint32_t* d_blk_entries,
                                   uint64_t* d_totals, hipStream_t st, hipEvent_t done = nullptr, int stages = 3);
hipError_t launch_compact_sst_gather(const uint8_t* d_bytes, const CsBlk* d_blks, uint32_t B, const CsLayout& lay,
                                     const uint8_t* d_work, uint8_t* d_key_data, uint64_t data_cap,
                                     uint64_t* d_key_offsets, uint64_t offs_cap, hipStream_t st,
                                     hipEvent_t done = nullptr);

// out[i] bit s = (lo_s <= key i <= hi_s) && may_contain(filter s, key i), for
// the nfilt (<= 64) descriptors at d_filters (device memory).  One class
// holding every descriptor takes the bit-sliced kernel with a compile-time
// entry width; several classes the per-class tables; none the L2 walk.
// done (optional): an event the dispatch itself completes (see launch_done).
hipError_t launch_fset_probe(const KeyBatch& kb, const RangedFilter* d_filters, uint32_t nfilt, const FsetRanges& rg,
                             const FsetClasses& cl, uint32_t shared_nb, uint32_t shared_k, uint8_t* d_out_rows,
                             uint32_t row_bytes, int num_cus, hipStream_t st, hipEvent_t done = nullptr);

// The probe's answer transposed (fset_lists.hip): from the n mask rows of
// launch_fset_probe (row_bytes each, every slot of `live` within them), for
// every slot s < 64, d_index[d_starts[s] .. d_starts[s+1]) = the ascending
// indices of the rows with bit s set; d_starts[65] is always exact, the entry
// at position p is stored iff p < cap.  d_tiles: fset_lists_tile_bytes(n,
// live) bytes of scratch (per-tile counts, then offsets), 16-B aligned.
// 1 <= n <= 2^32-1, live != 0.  done: completed by the last kernel.
// (kListTile and fset_lists_tile_bytes: fset_lists_plan.hpp)
hipError_t launch_fset_lists(const uint8_t* d_rows, uint32_t row_bytes, uint64_t n, uint64_t live, uint32_t* d_tiles,
                             uint64_t* d_starts, uint32_t* d_index, uint64_t cap, hipStream_t st,
                             hipEvent_t done = nullptr);

// A level set (lsmb_lset): up to kLsetMaxRows rows (the store's levels below
// L0), each any number of tables with pairwise disjoint key ranges, sorted by
// min_key — so the max keys ascend too, and at most one table of a row holds a
// given key.  hi_pfx[j] = the zero-padded 16-byte prefix of table j's max_key
// as two big-endian words (FsetPoint's w0, w1): the array the kernel searches.
constexpr uint32_t kLsetMaxRows = 8;
constexpr uint32_t kLsetNone = 0xFFFFFFFFu;
struct LsetTable {
    const uint32_t* words32;
    const uint8_t* lo;  // min_key, max_key: the full bytes (device memory)
    const uint8_t* hi;
    uint64_t lo_w0, lo_w1;  // min_key's 16-byte prefix
    Mod32 md;
    uint32_t lo_len, hi_len;
    uint32_t num_bits, k;
    uint32_t id, pad;  // the caller's table id: the answer
};
struct LsetRow {
    const ulonglong2* hi_pfx;  // ntab entries (x = w0, y = w1), ascending
    const LsetTable* tab;      // ntab, in the same order
    uint32_t ntab, pad;
};
struct LsetRows {
    LsetRow row[kLsetMaxRows];  // by value: uniform kernel arguments
    uint32_t nrows;
};

// d_out[r * n + i] = the id of the one table t of row r with lo_t <= key i <=
// hi_t && may_contain(filter t, key i), else kLsetNone; r < rows.nrows.  A
// sealed set is read-only: the launch needs no scratch.
hipError_t launch_lset_probe(const KeyBatch& kb, const LsetRows& rows, uint32_t* d_out, int num_cus, hipStream_t st);

// The same walk answering by ordinal: d_out[r * stride + i] = (the tables of
// rows 0 .. r-1) + the hit's place in row r's sealed order, else kLsetNone;
// stride >= kb.n.  Ids are the caller's and need not be unique; ordinals are.
hipError_t launch_lset_probe_ordinals(const KeyBatch& kb, const LsetRows& rows, uint32_t* d_out, uint64_t stride,
                                      int num_cus, hipStream_t st);

// A whole Version from one hash per key (lset_version.hip): the rows as
// launch_lset_probe answers them (d_out, may be null when rows.nrows == 0),
// and d_l0_mask[i] bit j = (lo_j <= key i <= hi_j) && may_contain(filter j,
// key i) for the set's nl0 (1 .. 64) L0 tables, descriptor j = the table at
// position j with out_bit j (d_l0, rg and cl as fset_plan.hpp plans them,
// cl.table_bytes <= kFsetTableBytes).  Read-only, no scratch.
hipError_t launch_lset_version(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                               const FsetRanges& rg, const FsetClasses& cl, uint64_t* d_l0_mask, uint32_t* d_out,
                               int num_cus, hipStream_t st);

// The same kernel feeding the Version lists probe: the L0 masks in n rows of
// row_bytes (1, 2, 4 or 8, covering nl0) at d_mask_rows, as launch_fset_probe
// leaves them for launch_fset_lists, and the rows answered by ordinal at
// d_out[r * stride + i] as launch_lset_probe_ordinals does; stride >= kb.n.
hipError_t launch_lset_version_ordinals(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0,
                                        uint32_t nl0, const FsetRanges& rg, const FsetClasses& cl, uint8_t* d_mask_rows,
                                        uint32_t row_bytes, uint32_t* d_out, uint64_t stride, int num_cus,
                                        hipStream_t st);

// The level set's answer per table (lset_lists.hip): with G = the tables of
// all rows, for every ordinal g < G, d_index[d_starts[g] .. d_starts[g+1]) =
// the ascending key indices i whose row answers table g; d_starts[G + 1] is
// always exact, the entry at position p is stored iff p < cap.  All scratch is
// d_work (16-B aligned, at least lset_lists_plan(kb.n, rows.nrows, G)
// .work_bytes, see lset_lists_plan.hpp): the set is only read.  1 <= kb.n <=
// 2^32-1, 1 <= G <= 2^32-1.  No host synchronisation.
hipError_t launch_lset_lists(const KeyBatch& kb, const LsetRows& rows, uint64_t G, uint64_t* d_starts,
                             uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, int num_cus,
                             hipStream_t st);

// launch_lset_lists after its ordinal probe: splits the answers already in the
// kAns region of d_work (laid out by pl = lset_lists_plan(n, R, G), n * R * G
// > 0) into lists that begin at *d_base (device memory, read by the kernels;
// NULL = 0) and at d_starts[ord_off]: d_starts[ord_off + g] = *d_base + the
// start of ordinal g's list, g <= G, and the entry at position p of the lists
// goes to d_index[*d_base + p] iff *d_base + p < cap.  With a null base and
// ord_off = 0 this is the second half of launch_lset_lists exactly.
struct LsetListsPlan;
hipError_t launch_lset_lists_split(const LsetListsPlan& pl, void* d_work, const uint64_t* d_base, uint64_t ord_off,
                                   uint64_t* d_starts, uint32_t* d_index, uint64_t cap, int num_cus, hipStream_t st);

// A whole Version per table (lset_version_lists.hip): Version ordinal v < nl0
// is the L0 table at position v, v >= nl0 the rows' ordinal v - nl0, V = nl0 +
// G.  d_index[d_starts[v] .. d_starts[v+1]) = the ascending key indices that
// table v answers, from one hash per key; d_starts[V + 1] is always exact, the
// entry at position p is stored iff p < cap.  All scratch is d_work (16-B
// aligned, at least lset_vlists_plan(kb.n, nl0, rows.nrows, G).work_bytes, see
// lset_vlists_plan.hpp).  1 <= kb.n <= 2^32-1, 1 <= nl0 <= 64, G <= 2^32-1.
// No host synchronisation.
hipError_t launch_lset_version_lists(const KeyBatch& kb, const LsetRows& rows, uint64_t G, const RangedFilter* d_l0,
                                     uint32_t nl0, const FsetRanges& rg, const FsetClasses& cl, uint64_t* d_starts,
                                     uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, int num_cus,
                                     hipStream_t st);

// The walk probe (lset_walk_first.hip; steps and ordinals in
// lset_walk_plan.hpp): with W = nl0 + rows.nrows walk steps, d_step[i] = the
// smallest step w >= d_from[i] at which key i has a candidate (step w < nl0:
// bit nl0-1-w of launch_lset_version's mask; step nl0 + r: launch_lset_probe
// answers a table in row r), d_ord[i] = that candidate's Version ordinal, both
// kLsetNone when there is none or d_from[i] >= W (such a key is not hashed).
// d_from null = all zero, d_step null = not wanted, and the two may be one
// buffer.  nl0 == 0 is allowed (nothing staged, d_l0 / rg / cl unread), and
// rows.nrows == 0.  Read-only, no scratch.
hipError_t launch_lset_walk_first(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                                  const FsetRanges& rg, const FsetClasses& cl, const uint32_t* d_from, uint32_t* d_step,
                                  uint32_t* d_ord, int num_cus, hipStream_t st);

// The walk probe per table: d_index[d_starts[v] .. d_starts[v+1]) = the
// ascending key indices whose d_ord is v, over the V = nl0 + G Version
// ordinals; a key is in at most one list.  d_starts[V + 1] is always exact, the
// entry at position p is stored iff p < cap.  All scratch is d_work (16-B
// aligned, at least lset_walk_lists_plan(kb.n, V).work_bytes).  1 <= kb.n <=
// 2^32-1, 1 <= V <= 2^32-1.  No host synchronisation.
hipError_t launch_lset_walk_lists(const KeyBatch& kb, const LsetRows& rows, uint64_t G, const RangedFilter* d_l0,
                                  uint32_t nl0, const FsetRanges& rg, const FsetClasses& cl, const uint32_t* d_from,
                                  uint32_t* d_step, uint64_t* d_starts, uint32_t* d_index, uint64_t cap, void* d_work,
                                  uint64_t work_bytes, int num_cus, hipStream_t st);

// A kernel launch whose completion also completes `done` (when non-null):
// hipExtLaunchKernelGGL tracks the event with the dispatch's own completion
// signal, where hipEventRecord after the launch would put a marker packet in
// the stream — ~6 us between back-to-back kernels (rocprofv3, the C3 probe).
template <typename K, typename... Args>
hipError_t launch_done(K kern, dim3 grid, dim3 block, uint32_t smem, hipStream_t st, hipEvent_t done, Args... args) {
    if (done)
        hipExtLaunchKernelGGL(kern, grid, block, smem, st, nullptr, done, 0, args...);
    else
        kern<<<grid, block, smem, st>>>(args...);
    return hipGetLastError();
}

// Workgroups for n grid-strided items at `block` items per workgroup (its
// lanes, for most kernels): ceil(n / block) within [1, max_wgs] (max_wgs = the
// device's CUs times the kernel's workgroups per CU).
inline uint32_t grid_for(uint64_t n, uint32_t block, uint64_t max_wgs) {
    uint64_t g = (n + block - 1) / block;
    if (g > max_wgs) g = max_wgs;
    return (uint32_t)(g < 1 ? 1 : g);
}

// True when launch_probe walks these filters with k_probe_generic, the one
// probe kernel that reads the device descriptor copy (the bit-sliced kernels
// take the filters in their arguments).
bool probe_reads_descriptors(const ProbeFilter* h_filters, uint32_t nfilt);

hipError_t launch_probe(const KeyBatch& kb, const ProbeFilter* h_filters, uint32_t nfilt,
                        ProbeFilter* d_filters_scratch, uint8_t* d_out, int num_cus,
                        hipStream_t st, hipEvent_t done = nullptr);

hipError_t launch_or_reduce(uint32_t* dst, const uint32_t* src, uint64_t nwords32, uint32_t nsrc,
                            uint64_t stride32, hipStream_t st, hipEvent_t done = nullptr);

hipError_t launch_gen_splitmix(uint64_t seed, uint64_t first, uint64_t n, uint32_t mod, uint32_t add,
                               uint64_t* d_out, hipStream_t st);
hipError_t launch_gen_key16(uint64_t seed, uint64_t first, uint64_t n, uint8_t* d_keys,
                            hipStream_t st);

}  // namespace lsmb

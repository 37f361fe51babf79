// lset_version_lists.hip — a whole Version's answer per table
// (lsmb_lset_probe_version_lists*) for gfx950 (MI355X): the lists a reader
// that works table by table over DB::get's walk wants (src/db/mod.rs:238-267,
// src/db/snapshot.rs:40-69, each entry past src/sstable/reader.rs:192-199's
// range-and-bloom check), L0 included, from ONE hash per key.
//
// Version ordinal v < T0 is the L0 table at position v, v >= T0 the rows'
// ordinal v - T0.  On one stream, all scratch in the caller's workspace
// (lset_vlists_plan.hpp):
//   1. k_lset_version's ordinal form (lset_version.hip): per key one hash, the
//      L0 mask into a row of rb bytes, the rows' ordinals into the tile-padded
//      answer rows of the rows' split;
//   2. launch_fset_lists (fset_lists.hip) over the mask rows, live = the low
//      T0 bits: the L0 lists into d_index from position 0, their 65 starts into
//      the workspace; starts65[64] = E0, the L0 entries, known here only;
//   3. launch_lset_lists_split (lset_lists.hip) over the answer rows with
//      base = &starts65[64]: the rows' lists behind the L0 lists, their starts
//      at d_starts[T0 ..];
//   4. k_vl_stitch: d_starts[0 .. T0) from starts65 (and d_starts[T0] = E0
//      where step 3 did not run: no row, or rows without a table).
// Every position follows from counts (no atomic anywhere), so d_starts and
// d_index are the same bytes on every run.
#include "kernels.hpp"
#include "lset_vlists_plan.hpp"

namespace lsmb {

namespace {

// d_starts[v] = starts65[v] for v < count (count <= kVlStarts)
__global__ __launch_bounds__(128) void k_vl_stitch(const uint64_t* __restrict__ starts65, uint32_t count,
                                                  uint64_t* __restrict__ d_starts) {
    if (threadIdx.x < count) d_starts[threadIdx.x] = starts65[threadIdx.x];
}

}  // namespace

hipError_t launch_lset_version_lists(const KeyBatch& kb, const LsetRows& rows, uint64_t G, const RangedFilter* d_l0,
                                     uint32_t nl0, const FsetRanges& rg, const FsetClasses& cl, uint64_t* d_starts,
                                     uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, int num_cus,
                                     hipStream_t st) {
    if (kb.n == 0 || kb.n > 0xFFFFFFFFull || G > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (nl0 == 0 || nl0 > 64 || rows.nrows > kLsetMaxRows) return hipErrorInvalidValue;
    if (!d_starts || (cap && !d_index)) return hipErrorInvalidValue;
    const LsetVlistsPlan pl = lset_vlists_plan(kb.n, nl0, rows.nrows, G);
    if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15) || work_bytes < pl.work_bytes) return hipErrorInvalidValue;
    uint8_t* w = (uint8_t*)d_work;
    uint8_t* mask = w + pl.reg[LsetVlistsPlan::kMask].off;
    uint32_t* tiles = (uint32_t*)(w + pl.reg[LsetVlistsPlan::kTiles].off);
    uint64_t* starts65 = (uint64_t*)(w + pl.reg[LsetVlistsPlan::kStarts].off);
    const bool has_rows = pl.rows.work_bytes != 0;  // rows emptied by derive have no answer rows to write

    LsetRows walked = rows;
    if (!has_rows) walked.nrows = 0;
    uint32_t* ans = has_rows ? (uint32_t*)(w + pl.rows.reg[LsetListsPlan::kAns].off) : nullptr;
    if (hipError_t e = launch_lset_version_ordinals(kb, walked, d_l0, nl0, rg, cl, mask, pl.rb, ans,
                                                    has_rows ? pl.rows.row_stride : kb.n, num_cus, st);
        e != hipSuccess)
        return e;
    if (hipError_t e = launch_fset_lists(mask, pl.rb, kb.n, pl.live, tiles, starts65, d_index, cap, st, nullptr);
        e != hipSuccess)
        return e;
    if (has_rows)
        if (hipError_t e = launch_lset_lists_split(pl.rows, d_work, starts65 + 64, nl0, d_starts, d_index, cap, num_cus,
                                                   st);
            e != hipSuccess)
            return e;
    // starts65[nl0] = E0 for every nl0 <= 64: the slots past the live ones are empty
    static_assert(kVlStarts <= 128, "one lane per start");
    k_vl_stitch<<<1, 128, 0, st>>>(starts65, has_rows ? nl0 : nl0 + 1, d_starts);
    return hipGetLastError();
}

}  // namespace lsmb

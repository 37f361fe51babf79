// lset_walk_first.hip — the walk probe of a level set (lsmb_lset_probe_walk*)
// for gfx950 (MI355X): the batched form of DB::get's walk itself
// (src/db/mod.rs:243-267, Snapshot::get src/db/snapshot.rs:40-69), which stops
// at the first table that holds the key.  Per key, from ONE hash: the first
// walk step at or after the key's resume point whose table passes the
// range-and-bloom check of src/sstable/reader.rs:192-199, and that table's
// Version ordinal.  Steps, positions and ordinals: lset_walk_plan.hpp, whose
// constexpr mapping this kernel calls and whose lset_walk_ref states the
// answer in plain C++.
//
// A sibling of k_lset_version (lset_version.hip): the same workgroup geometry,
// the same staging of the L0 descriptors, ranges and class tables in LDS, the
// same three key sources.  Per key (one lane per key, grid-stride):
//   from >= W   no hash, no key read: NONE / NONE (a retired key)
//   from <  T0  the region's in-range mask ANDed with the positions the resume
//               point still allows BEFORE classes_answer, so classes and
//               generic filters with no allowed member are not walked; the
//               highest set bit of the answer is the newest hit
//   no L0 hit   the rows from max(from, T0) - T0, one lset_row_find each, up
//               to the first hit
// The row loop is uniform (r is scalar, so the row descriptors stay scalar
// loads of the kernel arguments) with the lanes that still search as its
// predicate: a wave leaves the loop as soon as none of its lanes searches, and
// skips a row's search when none of them is at that row yet.  Lanes of a wave
// finish at different rows, so a wave pays for the rows of its slowest lane —
// never for more than k_lset_version, which searches every row for every lane.
// Read-only, no scratch, no atomics: the same inputs give the same bytes.
//
// launch_lset_walk_lists: the kernel writes the ordinals into the answer row
// of lset_walk_lists_plan(n, V) and launch_lset_lists_split (lset_lists.hip)
// transposes that one row over the V Version ordinals, null base, offset 0.
#include <type_traits>

#include "fset_dev.hpp"
#include "kernels.hpp"
#include "keyorder.hpp"
#include "keysrc.hpp"
#include "lset_walk.hpp"
#include "lset_walk_plan.hpp"

namespace lsmb {
namespace {

static_assert(kWalkNone == kLsetNone, "the plan header restates the probe's 'no table'");

// d_from (null: all zero) and d_step (null: not wanted) may be one buffer:
// lane i reads from[i] before it writes step[i], and no other lane touches
// either, so neither is __restrict__.
template <class Src>
__global__ __launch_bounds__(kClassBlock, 4 * class_wgs_per_cu<Src>()) void k_lset_walk_first(
    Src src, uint64_t n, LsetRows rows, const RangedFilter* __restrict__ l0, uint32_t nl0, FsetRanges rg, FsetClasses cl,
    const uint32_t* d_from, uint32_t* d_step, uint32_t* __restrict__ d_ord) {
    extern __shared__ __align__(16) uint8_t smem_raw[];
    __shared__ FsetClassLds S;
    __shared__ FsetLds L;
    if (nl0) {  // uniform; a set without L0 tables stages nothing
        stage_classes(l0, nl0, cl, S);
        stage_ranges(rg, L);
        __syncthreads();
        build_class_tables(cl, S, smem_raw);
        __syncthreads();
    }
    const uint32_t npts = rg.npts;
    const uint32_t nrows = rows.nrows;
    const uint32_t W = lset_walk_steps(nl0, nrows);
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
        const uint32_t from = d_from ? d_from[i] : 0u;
        uint32_t step = kLsetNone, ord = kLsetNone;
        if (from < W) {
            const H128 h = src.hash(i);
            const uint8_t* kp = src.bytes(i);
            const uint64_t kl = src.key_len(i);
            const Pfx16 kx = prefix16(kp, kl);
            if (from < nl0) {
                const uint64_t rm = L.regmask[key_region(kx, kp, kl, L, npts)] & lset_walk_allowed(nl0, from);
                const uint64_t o = classes_answer(h, rm, cl, S, smem_raw);
                if (o) {
                    ord = 63u - (uint32_t)__builtin_clzll(o);  // descriptor d is the L0 table at position d
                    step = lset_walk_l0_step(nl0, ord);
                }
            }
            const uint32_t r0 = lset_walk_first_row(nl0, from);
            uint32_t base = 0;  // rows' ordinal of the row's first table
            for (uint32_t r = 0; r < nrows; r++) {
                const bool live = step == kLsetNone;
                if (!__any(live)) break;  // uniform: every lane of the wave has its answer
                if (live && r >= r0) {
                    const uint32_t j = lset_row_find(h, kx, kp, kl, rows.row[r]);
                    if (j != kLsetNone) {
                        step = lset_walk_row_step(nl0, r);
                        ord = nl0 + base + j;
                    }
                }
                base += rows.row[r].ntab;
            }
        }
        if (d_step) d_step[i] = step;
        d_ord[i] = ord;
    }
}

template <class Src>
hipError_t lset_walk_with(const Src& src, uint64_t n, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                          const FsetRanges& rg, const FsetClasses& cl, const uint32_t* d_from, uint32_t* d_step,
                          uint32_t* d_ord, int num_cus, hipStream_t st) {
    const uint32_t g = grid_for(n, kClassBlock, (uint64_t)num_cus * class_wgs_per_cu<Src>());
    const size_t smem = nl0 ? cl.table_bytes : 0;
    hipFuncSetAttribute((const void*)k_lset_walk_first<Src>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    k_lset_walk_first<Src><<<dim3(g), dim3(kClassBlock), smem, st>>>(src, n, rows, d_l0, nl0, rg, cl, d_from, d_step,
                                                                    d_ord);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lset_walk_first(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                                  const FsetRanges& rg, const FsetClasses& cl, const uint32_t* d_from, uint32_t* d_step,
                                  uint32_t* d_ord, int num_cus, hipStream_t st) {
    if (kb.n == 0) return hipSuccess;
    if (rows.nrows > kLsetMaxRows || nl0 > 64 || !d_ord) return hipErrorInvalidValue;
    if (nl0 && (!d_l0 || rg.npts > kFsetMaxPoints || cl.ncls > kFsetMaxClasses || cl.table_bytes > kFsetTableBytes))
        return hipErrorInvalidValue;
    return with_key_source(kb, [&](auto src) {
        return lset_walk_with(src, kb.n, rows, d_l0, nl0, rg, cl, d_from, d_step, d_ord, num_cus, st);
    });
}

hipError_t launch_lset_walk_lists(const KeyBatch& kb, const LsetRows& rows, uint64_t G, const RangedFilter* d_l0,
                                  uint32_t nl0, const FsetRanges& rg, const FsetClasses& cl, const uint32_t* d_from,
                                  uint32_t* d_step, uint64_t* d_starts, uint32_t* d_index, uint64_t cap, void* d_work,
                                  uint64_t work_bytes, int num_cus, hipStream_t st) {
    const uint64_t V = (uint64_t)nl0 + G;
    if (kb.n == 0 || kb.n > 0xFFFFFFFFull || V == 0 || V > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (!d_starts || (cap && !d_index)) return hipErrorInvalidValue;
    const LsetListsPlan pl = lset_walk_lists_plan(kb.n, V);
    if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15) || work_bytes < pl.work_bytes) return hipErrorInvalidValue;
    uint32_t* ans = (uint32_t*)((uint8_t*)d_work + pl.reg[LsetListsPlan::kAns].off);
    if (hipError_t e = launch_lset_walk_first(kb, rows, d_l0, nl0, rg, cl, d_from, d_step, ans, num_cus, st);
        e != hipSuccess)
        return e;
    return launch_lset_lists_split(pl, d_work, nullptr, 0, d_starts, d_index, cap, num_cus, st);
}

}  // namespace lsmb

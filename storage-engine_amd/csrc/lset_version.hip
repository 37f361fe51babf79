// lset_version.hip — the fused Version probe of a level set for gfx950
// (MI355X): the batched form of DB::get's whole walk (src/db/mod.rs:238-267,
// Snapshot::get src/db/snapshot.rs:40-69) — L0 newest first, where tables
// overlap, then one table per level below — from ONE hash per key.
//
// Per workgroup, once: the L0 descriptors, the boundary points and region
// masks of the L0 ranges, and the bit-sliced class tables of the L0 filters
// into LDS, exactly as k_fset_classes stages them (fset_dev.hpp).
// Per key (one lane per key, grid-stride): the hash and the 16-byte prefix
// once; then
//   L0    one region lookup for the in-range mask, one walk and k LDS reads
//         per class with an in-range member, an L2 walk with early exit for
//         the filters outside the classes (classes_answer): bit j of the mask
//         = (min_j <= key <= max_j) && may_contain(filter j, key) for the L0
//         table at position j, so a reader visits set bits from the highest
//         down (version.level(0).iter().rev());
//   rows  the walk of lset.hip (lset_rows_walk), ids stored as k_lset_probe
//         stores them (or ordinals, as k_lset_probe's ordinal form does, for
//         the Version lists probe).
// csrc/fset_plan.hpp states the L0 answer in plain C++ (fset_plan_answer),
// csrc/lset_order.hpp the rows' search (lset_find).
#include <type_traits>

#include "fset_dev.hpp"
#include "kernels.hpp"
#include "keyorder.hpp"
#include "keysrc.hpp"
#include "lset_walk.hpp"

namespace lsmb {
namespace {

// k_fset_classes' geometry (fset_dev.hpp): 1024-thread workgroups, two per CU
// for 16-B keys, one for the other key sources, so a CU builds the class
// tables at most twice.  The row search adds no register beyond that cap's 64
// (16-B keys) and 128: no scratch in any instantiation (DESIGN.md section 4.4
// records the compiled figures).
//
// kOrdinal = false: the Version probe itself, 8-byte masks and table ids at
// out[r * n + i].  kOrdinal = true, for the Version lists probe
// (lset_version_lists.hip): masks in rows of rb bytes (1, 2, 4 or 8, covering
// nl0; a wave-uniform choice inside MaskOut::put, so one instantiation per key
// source serves every width) and the rows' ordinals at out[r * stride + i].
template <class Src, bool kOrdinal>
__global__ __launch_bounds__(kClassBlock, 4 * class_wgs_per_cu<Src>()) void k_lset_version(
    Src src, uint64_t n, LsetRows rows, const RangedFilter* __restrict__ l0, uint32_t nl0, FsetRanges rg,
    FsetClasses cl, uint8_t* __restrict__ mask, uint32_t rb, uint32_t* __restrict__ out, uint64_t stride) {
    extern __shared__ __align__(16) uint8_t smem_raw[];
    __shared__ FsetClassLds S;
    __shared__ FsetLds L;
    stage_classes(l0, nl0, cl, S);
    stage_ranges(rg, L);
    __syncthreads();
    build_class_tables(cl, S, smem_raw);
    __syncthreads();
    const MaskOut mo{mask, kOrdinal ? rb : 8u};
    const uint32_t npts = rg.npts;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
        const H128 h = src.hash(i);
        const uint8_t* kp = src.bytes(i);
        const uint64_t kl = src.key_len(i);
        const Pfx16 kx = prefix16(kp, kl);
        const uint64_t rm = L.regmask[key_region(kx, kp, kl, L, npts)];
        // descriptor d is the L0 table at position d: the descriptor bits are the answer
        mo.put(i, classes_answer(h, rm, cl, S, smem_raw));
        lset_rows_walk<kOrdinal>(h, kx, kp, kl, rows, out, kOrdinal ? stride : n, i);
    }
}

template <class Src, bool kOrdinal>
hipError_t lset_version_with(const Src& src, uint64_t n, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                             const FsetRanges& rg, const FsetClasses& cl, uint8_t* d_mask, uint32_t rb, uint32_t* d_out,
                             uint64_t stride, int num_cus, hipStream_t st) {
    const uint32_t g = grid_for(n, kClassBlock, (uint64_t)num_cus * class_wgs_per_cu<Src>());
    const size_t smem = cl.table_bytes;
    hipFuncSetAttribute((const void*)k_lset_version<Src, kOrdinal>, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)smem);
    k_lset_version<Src, kOrdinal><<<dim3(g), dim3(kClassBlock), smem, st>>>(src, n, rows, d_l0, nl0, rg, cl, d_mask, rb,
                                                                              d_out, stride);
    return hipGetLastError();
}

// The argument checks and the choice of key source both forms share.
template <bool kOrdinal>
hipError_t lset_version_any(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                            const FsetRanges& rg, const FsetClasses& cl, uint8_t* d_mask, uint32_t rb, uint32_t* d_out,
                            uint64_t stride, int num_cus, hipStream_t st) {
    if (kb.n == 0) return hipSuccess;
    if (rows.nrows > kLsetMaxRows || nl0 == 0 || nl0 > 64 || rg.npts > kFsetMaxPoints || cl.ncls > kFsetMaxClasses ||
        cl.table_bytes > kFsetTableBytes)
        return hipErrorInvalidValue;
    if (!d_mask || (rows.nrows && !d_out)) return hipErrorInvalidValue;
    return with_key_source(kb, [&](auto src) {
        return lset_version_with<decltype(src), kOrdinal>(src, kb.n, rows, d_l0, nl0, rg, cl, d_mask, rb, d_out, stride,
                                                          num_cus, st);
    });
}

}  // namespace

hipError_t launch_lset_version(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0, uint32_t nl0,
                               const FsetRanges& rg, const FsetClasses& cl, uint64_t* d_l0_mask, uint32_t* d_out,
                               int num_cus, hipStream_t st) {
    return lset_version_any<false>(kb, rows, d_l0, nl0, rg, cl, reinterpret_cast<uint8_t*>(d_l0_mask), 8, d_out, kb.n,
                                   num_cus, st);
}

hipError_t launch_lset_version_ordinals(const KeyBatch& kb, const LsetRows& rows, const RangedFilter* d_l0,
                                        uint32_t nl0, const FsetRanges& rg, const FsetClasses& cl, uint8_t* d_mask_rows,
                                        uint32_t row_bytes, uint32_t* d_out, uint64_t stride, int num_cus,
                                        hipStream_t st) {
    if (row_bytes != 1 && row_bytes != 2 && row_bytes != 4 && row_bytes != 8) return hipErrorInvalidValue;
    if (row_bytes < 8 && nl0 > 8 * row_bytes) return hipErrorInvalidValue;
    if (stride < kb.n) return hipErrorInvalidValue;
    return lset_version_any<true>(kb, rows, d_l0, nl0, rg, cl, d_mask_rows, row_bytes, d_out, stride, num_cus, st);
}

}  // namespace lsmb

// lset.hip — level-set probe for gfx950 (MI355X): the batched form of DB::get's
// walk over L1 and below (src/db/mod.rs:255-267, "L1+: no overlaps, at most
// one SSTable contains the key").  Per key and per row (level) the answer is
// one table id or none, so a row of thousands of tables costs one binary
// search, one range check and at most one filter walk — not a mask bit per
// table as in a filter set (bloom_probe.hip).
//
// One lane per key, grid-stride.  The key is hashed once and its 16-byte
// prefix taken once; then per row:
//   1. a lower bound over the row's max-key prefixes (global memory: a
//      thousand-table row does not fit LDS; the top of the search tree stays
//      in L1/L2) for the first table whose max_key >= key;
//   2. full compares over the tables whose prefix equals the key's (bounds or
//      keys longer than 16 bytes sharing their first 16);
//   3. min_key <= key;
//   4. the table's own filter walked from L2, out at the first clear bit
//      (src/bloom/mod.rs:88-90).
// csrc/lset_order.hpp states steps 1-3 in plain C++ (lset_find) for the CPU
// tests.  Output out[r * n + i]: a row's answers are contiguous, so the stores
// of a wave coalesce.  The lists probe (lset_lists.hip) runs the same walk
// and takes the hit's ordinal instead of its id, rows a padded stride apart.
#include "kernels.hpp"
#include "keyorder.hpp"
#include "keysrc.hpp"
#include "lset_walk.hpp"

namespace lsmb {
namespace {

// The walk of one key batch over every row, shared by both forms of the
// answer: kOrdinal = false stores the hit's table id at out[r * n + i];
// kOrdinal = true its ordinal (the tables of rows 0 .. r-1, then its place in
// row r's sealed order) at out[r * stride + i], for the lists probe
// (lset_lists.hip).  The per-key loop is lset_rows_walk (lset_walk.hpp), which
// the Version probe (lset_version.hip) runs too.
template <class Src, bool kOrdinal>
__device__ __forceinline__ void lset_probe_body(const Src& src, uint64_t n, const LsetRows& rows,
                                                uint32_t* __restrict__ out, uint64_t stride_arg, uint64_t gs) {
    const uint64_t stride = kOrdinal ? stride_arg : n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
        const H128 h = src.hash(i);
        const uint8_t* kp = src.bytes(i);
        const uint64_t kl = src.key_len(i);
        lset_rows_walk<kOrdinal>(h, prefix16(kp, kl), kp, kl, rows, out, stride, i);
    }
}

template <class Src>
__global__ __launch_bounds__(256) void k_lset_probe(Src src, uint64_t n, LsetRows rows, uint32_t* __restrict__ out) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    lset_probe_body<Src, false>(src, n, rows, out, n, gs);
}

template <class Src>
__global__ __launch_bounds__(256) void k_lset_probe_ord(Src src, uint64_t n, LsetRows rows, uint32_t* __restrict__ out,
                                                        uint64_t stride) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    lset_probe_body<Src, true>(src, n, rows, out, stride, gs);
}

// Both forms behind one host path: the grid, then the id kernel (rows n apart)
// or the ordinal kernel (rows `stride` apart).
template <bool kOrdinal>
hipError_t lset_probe_any(const KeyBatch& kb, const LsetRows& rows, uint32_t* d_out, uint64_t stride, int num_cus,
                          hipStream_t st) {
    if (kb.n == 0 || rows.nrows == 0) return hipSuccess;
    if (rows.nrows > kLsetMaxRows || (kOrdinal && stride < kb.n)) return hipErrorInvalidValue;
    return with_key_source(kb, [&](auto src) {
        using Src = decltype(src);
        const dim3 g(grid_for(kb.n, 256, (uint64_t)num_cus * 8));
        if constexpr (kOrdinal)
            k_lset_probe_ord<Src><<<g, dim3(256), 0, st>>>(src, kb.n, rows, d_out, stride);
        else
            k_lset_probe<Src><<<g, dim3(256), 0, st>>>(src, kb.n, rows, d_out);
        return hipGetLastError();
    });
}

}  // namespace

hipError_t launch_lset_probe(const KeyBatch& kb, const LsetRows& rows, uint32_t* d_out, int num_cus, hipStream_t st) {
    return lset_probe_any<false>(kb, rows, d_out, kb.n, num_cus, st);
}

hipError_t launch_lset_probe_ordinals(const KeyBatch& kb, const LsetRows& rows, uint32_t* d_out, uint64_t stride,
                                      int num_cus, hipStream_t st) {
    return lset_probe_any<true>(kb, rows, d_out, stride, num_cus, st);
}

}  // namespace lsmb

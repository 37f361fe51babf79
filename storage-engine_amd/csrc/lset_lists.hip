// lset_lists.hip — the level set's answer transposed: per-table lists of key
// indices (lsmb_lset_probe_lists*), a deterministic, stable multisplit over
// any number of tables, for gfx950 (MI355X).
//
// The ordinal probe (lset.hip) leaves ans[r][i] = the ordinal of the table of
// row r that answers key i, or none.  A list per ordinal is those (ordinal,
// key index) pairs sorted by ordinal, stably: 8-bit LSD radix passes, the
// first of which reads the answer rows themselves and drops the misses, so it
// is the compaction too.  Rows are walked in order and keys ascending within
// each, an ordinal belongs to one row and every pass is stable: each list
// comes out ascending.  Per pass, over tiles of kLlTile elements (one
// workgroup each, chunk c of a tile = its elements [64c, 64c + 64)):
//   k_ll_hist     per tile and digit, the tile's elements with that digit
//   k_ll_rowsum   per digit, its total over the tiles
//   k_ll_rowscan  digit-major exclusive scan: counts[d][t] becomes the first
//                 output position of digit d in tile t (the digits before d,
//                 then the tiles before t)
//   k_ll_scatter  an element's position = that + the tile's earlier chunks
//                 with its digit + its rank among the chunk's lanes with its
//                 digit (one ballot per digit bit, mbcnt)
// then k_ll_bounds turns the sorted ordinals into d_starts.  Positions follow
// from counts alone — no atomic anywhere — so d_starts and d_index are the
// same bytes on every run.  From the second pass on the element count E is
// known to the device only: the grid is sized for R * n and tiles past E leave
// at once.  Geometry and workspace layout: lset_lists_plan.hpp.
//
// launch_lset_lists = the ordinal probe, then launch_lset_lists_split (the
// passes and the bounds).  The Version lists probe (lset_version_lists.hip)
// fills the answer rows from its own fused kernel and enters at the split,
// with the lists based behind its L0 lists: a base for the last scatter and
// for the bounds, read from device memory (null = 0, the rows' own probe).
#include "kernels.hpp"
#include "lset_lists_plan.hpp"
#include "wave.hpp"

namespace lsmb {

namespace {

static_assert(kLlBlock == kLlDigits, "thread t of a workgroup owns digit t");
static_assert(kLlNone == kLsetNone, "the plan header restates the probe's 'no table'");
static_assert(kLlChunks * 64 <= (1u << 23), "packed (earlier + rank) field");

// What a pass reads.  First pass: the answer rows (element = row r, key i;
// value = i; a miss is no element).  Later passes: the E pairs of the pass
// before, E read from device memory.
struct LlSrc {
    const uint32_t* keys;
    const uint32_t* vals;
    const uint64_t* count;
    uint64_t n, row_stride;
    uint32_t tiles_per_row;
};

// The lane's kLlChunks elements of `tile` and where each goes inside the
// tile.  pk[k] = digit | valid << 8 | (elements of the same digit in the
// wave's earlier chunks + the lane's rank among the chunk's lanes of that
// digit) << 9.  On return (after a barrier) wcnt[w][d] = wave w's elements
// with digit d.  Every loop is uniform over the workgroup.
template <bool kFirst>
__device__ __forceinline__ void ll_tile_rank(const LlSrc& s, uint32_t tile, uint64_t count, uint32_t shift,
                                             uint32_t (&key)[kLlChunks], uint32_t (&val)[kLlChunks],
                                             uint32_t (&pk)[kLlChunks], uint32_t (*wcnt)[kLlDigits]) {
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t j = 0; j < kLlWaves; j++) (&wcnt[0][0])[threadIdx.x + j * kLlBlock] = 0;
    bool valid[kLlChunks];
    const uint32_t o0 = wave * (kLlChunks * 64) + lane;
    if (kFirst) {
        const uint32_t r = tile / s.tiles_per_row;
        const uint64_t i0 = (uint64_t)(tile - r * s.tiles_per_row) * kLlTile + o0;
        const uint32_t* __restrict__ row = s.keys + (uint64_t)r * s.row_stride;
#pragma unroll
        for (uint32_t k = 0; k < kLlChunks; k++) {
            const uint64_t i = i0 + k * 64;
            const uint32_t g = i < s.n ? row[i] : kLlNone;
            key[k] = g;
            val[k] = (uint32_t)i;
            valid[k] = g != kLlNone;
        }
    } else {
        const uint64_t e0 = (uint64_t)tile * kLlTile + o0;
#pragma unroll
        for (uint32_t k = 0; k < kLlChunks; k++) {
            const uint64_t e = e0 + k * 64;
            valid[k] = e < count;
            key[k] = valid[k] ? s.keys[e] : 0;
            val[k] = valid[k] ? s.vals[e] : 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kLlChunks; k++) {
        const uint32_t d = (key[k] >> shift) & (kLlDigits - 1);
        uint64_t same = __ballot(valid[k]);  // the chunk's lanes holding an element with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < kLlRadixBits; b++) {
            const bool bit = (d >> b) & 1;
            const uint64_t bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        const uint32_t pre = valid[k] ? wcnt[wave][d] : 0;
        __syncthreads();
        if (valid[k] && rank == 0) wcnt[wave][d] = pre + (uint32_t)__popcll(same);  // one lane per digit
        __syncthreads();
        pk[k] = d | ((uint32_t)valid[k] << 8) | ((pre + rank) << 9);
    }
}

template <bool kFirst>
__global__ __launch_bounds__(kLlBlock) void k_ll_hist(LlSrc s, uint32_t shift, uint32_t ntiles,
                                                      uint64_t* __restrict__ counts) {
    __shared__ uint32_t wcnt[kLlWaves][kLlDigits];
    const uint32_t tile = blockIdx.x;
    uint64_t count = 0;
    if (!kFirst) {
        count = *s.count;
        if ((uint64_t)tile * kLlTile >= count) {  // uniform
            counts[(uint64_t)threadIdx.x * ntiles + tile] = 0;
            return;
        }
    }
    uint32_t key[kLlChunks], val[kLlChunks], pk[kLlChunks];
    ll_tile_rank<kFirst>(s, tile, count, shift, key, val, pk, wcnt);
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kLlWaves; w++) t += wcnt[w][threadIdx.x];
    counts[(uint64_t)threadIdx.x * ntiles + tile] = t;
}

__device__ __forceinline__ uint64_t ll_block_sum(uint64_t v, uint64_t* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = kLlBlock / 2; d; d >>= 1) {
        if (threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    const uint64_t r = part[0];
    __syncthreads();
    return r;
}

// Workgroup d: totals[d] = the sum of counts[d][0 .. ntiles)
__global__ __launch_bounds__(kLlBlock) void k_ll_rowsum(const uint64_t* __restrict__ counts, uint32_t ntiles,
                                                        uint64_t* __restrict__ totals) {
    __shared__ uint64_t part[kLlBlock];
    const uint64_t* row = counts + (uint64_t)blockIdx.x * ntiles;
    uint64_t v = 0;
    for (uint32_t t = threadIdx.x; t < ntiles; t += kLlBlock) v += row[t];
    v = ll_block_sum(v, part);
    if (threadIdx.x == 0) totals[blockIdx.x] = v;
}

// Workgroup d: counts[d][t] becomes (the totals of the digits below d) + (the
// counts of d's tiles before t), 256 tiles a step.  The last digit's
// workgroup ends on the number of elements: *total_out when asked for.
__global__ __launch_bounds__(kLlBlock) void k_ll_rowscan(uint64_t* __restrict__ counts, uint32_t ntiles,
                                                         const uint64_t* __restrict__ totals,
                                                         uint64_t* __restrict__ total_out) {
    __shared__ uint64_t part[kLlBlock];
    __shared__ uint64_t wtot[kLlWaves];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t carry = ll_block_sum(threadIdx.x < blockIdx.x ? totals[threadIdx.x] : 0, part);
    uint64_t* row = counts + (uint64_t)blockIdx.x * ntiles;
    for (uint32_t t0 = 0; t0 < ntiles; t0 += kLlBlock) {
        const uint32_t t = t0 + threadIdx.x;
        const uint64_t v = t < ntiles ? row[t] : 0;
        // (wave_incl_scan written out: with the call this kernel compiles to other code, and the lists
        // probe it belongs to measured 0.3 % slower, AB_LOG.md)
        uint64_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kLlWaves; w++) {
            if (w < wave) before += wtot[w];
            all += wtot[w];
        }
        if (t < ntiles) row[t] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (total_out && blockIdx.x == kLlDigits - 1 && threadIdx.x == 0) *total_out = carry;
}

// out_keys[p] = key, out_vals[p] = value for every element of the tile, p as
// the file comment states it.  The last pass stores the values (key indices)
// into the caller's index under its capacity, the lists beginning at *base
// there (null: 0; the Version lists probe puts them behind the L0 lists);
// `limit` (R * n, the buffers' size) bounds every other store.
template <bool kFirst, bool kLast>
__global__ __launch_bounds__(kLlBlock) void k_ll_scatter(LlSrc s, uint32_t shift, uint32_t ntiles,
                                                         const uint64_t* __restrict__ offs,
                                                         uint32_t* __restrict__ out_keys,
                                                         uint32_t* __restrict__ out_vals, uint64_t limit, uint64_t cap,
                                                         const uint64_t* __restrict__ base) {
    __shared__ uint32_t wcnt[kLlWaves][kLlDigits];
    __shared__ uint64_t wbase[kLlWaves][kLlDigits];
    const uint32_t tile = blockIdx.x, wave = threadIdx.x >> 6;
    uint64_t count = 0;
    if (!kFirst) {
        count = *s.count;
        if ((uint64_t)tile * kLlTile >= count) return;  // uniform
    }
    uint32_t key[kLlChunks], val[kLlChunks], pk[kLlChunks];
    ll_tile_rank<kFirst>(s, tile, count, shift, key, val, pk, wcnt);
    uint64_t b = offs[(uint64_t)threadIdx.x * ntiles + tile];
#pragma unroll
    for (uint32_t w = 0; w < kLlWaves; w++) {
        wbase[w][threadIdx.x] = b;
        b += wcnt[w][threadIdx.x];
    }
    __syncthreads();
    const uint64_t b0 = kLast && base ? *base : 0;  // uniform
    const uint64_t vcap = kLast ? cap : ~0ull;
#pragma unroll
    for (uint32_t k = 0; k < kLlChunks; k++) {
        if ((pk[k] >> 8) & 1) {
            const uint64_t p = wbase[wave][pk[k] & (kLlDigits - 1)] + (pk[k] >> 9);
            if (p < limit) {
                out_keys[p] = key[k];
                if (b0 + p < vcap) out_vals[b0 + p] = val[k];
            }
        }
    }
}

// starts[g] = the first position whose ordinal is >= g: position q fills every
// g in (skeys[q-1], skeys[q]] (from 0 at q = 0, to G at q = E), so the tables
// of a gap — empty ones — get equal starts.  The lists begin at *base (null:
// 0) of the index and at `off` of starts: starts[off + g] = *base + q.
__global__ __launch_bounds__(256) void k_ll_bounds(const uint32_t* __restrict__ skeys, const uint64_t* __restrict__ count,
                                                   uint64_t G, uint64_t* __restrict__ starts,
                                                   const uint64_t* __restrict__ base, uint64_t off) {
    const uint64_t E = *count;
    const uint64_t b0 = base ? *base : 0;
    starts += off;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= E; q += gs) {
        const uint64_t lo = q ? (uint64_t)skeys[q - 1] + 1 : 0;
        uint64_t hi = q < E ? skeys[q] : G;
        if (hi > G) hi = G;
        for (uint64_t g = lo; g <= hi; g++) starts[g] = b0 + q;
    }
}

template <bool kFirst, bool kLast>
hipError_t ll_pass(const LlSrc& s, uint32_t shift, uint32_t ntiles, uint64_t* counts, uint64_t* meta,
                   uint32_t* out_keys, uint32_t* out_vals, uint64_t limit, uint64_t cap, const uint64_t* base,
                   hipStream_t st) {
    k_ll_hist<kFirst><<<ntiles, kLlBlock, 0, st>>>(s, shift, ntiles, counts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    k_ll_rowsum<<<kLlDigits, kLlBlock, 0, st>>>(counts, ntiles, meta);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    k_ll_rowscan<<<kLlDigits, kLlBlock, 0, st>>>(counts, ntiles, meta, kFirst ? meta + kLlDigits : nullptr);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    k_ll_scatter<kFirst, kLast><<<ntiles, kLlBlock, 0, st>>>(s, shift, ntiles, counts, out_keys, out_vals, limit, cap,
                                                             base);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lset_lists(const KeyBatch& kb, const LsetRows& rows, uint64_t G, uint64_t* d_starts,
                             uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, int num_cus,
                             hipStream_t st) {
    if (kb.n == 0 || kb.n > 0xFFFFFFFFull || G == 0 || G > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (rows.nrows == 0 || rows.nrows > kLsetMaxRows) return hipErrorInvalidValue;
    if (!d_starts || (cap && !d_index)) return hipErrorInvalidValue;
    const LsetListsPlan pl = lset_lists_plan(kb.n, rows.nrows, G);
    if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15) || work_bytes < pl.work_bytes) return hipErrorInvalidValue;
    uint32_t* ans = (uint32_t*)((uint8_t*)d_work + pl.reg[LsetListsPlan::kAns].off);
    if (hipError_t e = launch_lset_probe_ordinals(kb, rows, ans, pl.row_stride, num_cus, st); e != hipSuccess) return e;
    return launch_lset_lists_split(pl, d_work, nullptr, 0, d_starts, d_index, cap, num_cus, st);
}

hipError_t launch_lset_lists_split(const LsetListsPlan& pl, void* d_work, const uint64_t* d_base, uint64_t ord_off,
                                   uint64_t* d_starts, uint32_t* d_index, uint64_t cap, int num_cus, hipStream_t st) {
    if (pl.work_bytes == 0 || !d_work || (reinterpret_cast<uintptr_t>(d_work) & 15)) return hipErrorInvalidValue;
    if (!d_starts || (cap && !d_index)) return hipErrorInvalidValue;
    const uint64_t G = pl.G;
    uint8_t* w = (uint8_t*)d_work;
    uint64_t* meta = (uint64_t*)(w + pl.reg[LsetListsPlan::kMeta].off);
    uint64_t* counts = (uint64_t*)(w + pl.reg[LsetListsPlan::kCounts].off);
    uint32_t* ans = (uint32_t*)(w + pl.reg[LsetListsPlan::kAns].off);
    uint32_t* key_a = (uint32_t*)(w + pl.reg[LsetListsPlan::kKeyA].off);
    uint32_t* val_a = (uint32_t*)(w + pl.reg[LsetListsPlan::kValA].off);
    uint32_t* val_b = (uint32_t*)(w + pl.reg[LsetListsPlan::kValB].off);
    const uint32_t ntiles = (uint32_t)pl.ntiles;  // <= 8 * 2^21

    const uint64_t* count = meta + kLlDigits;
    // pass 0 reads the answers and writes buffer a; then a -> b (b's keys take
    // the answers' place) -> a ...; the last pass's values are the index
    LlSrc s{ans, nullptr, count, pl.n, pl.row_stride, (uint32_t)pl.tiles_per_row};
    uint32_t* sorted = nullptr;
    for (uint32_t p = 0; p < pl.passes; p++) {
        const bool first = p == 0, last = p + 1 == pl.passes, to_a = (p & 1) == 0;
        uint32_t* ok = to_a ? key_a : ans;
        uint32_t* ov = last ? d_index : (to_a ? val_a : val_b);
        const uint32_t shift = p * kLlRadixBits;
        hipError_t e;
        if (first && last) e = ll_pass<true, true>(s, shift, ntiles, counts, meta, ok, ov, pl.pairs, cap, d_base, st);
        else if (first) e = ll_pass<true, false>(s, shift, ntiles, counts, meta, ok, ov, pl.pairs, cap, d_base, st);
        else if (last) e = ll_pass<false, true>(s, shift, ntiles, counts, meta, ok, ov, pl.pairs, cap, d_base, st);
        else e = ll_pass<false, false>(s, shift, ntiles, counts, meta, ok, ov, pl.pairs, cap, d_base, st);
        if (e != hipSuccess) return e;
        s.keys = ok;
        s.vals = ov;
        sorted = ok;
    }
    k_ll_bounds<<<dim3(grid_for(pl.pairs + 1, 256, (uint64_t)num_cus * 8)), dim3(256), 0, st>>>(sorted, count, G, d_starts,
                                                                                             d_base, ord_off);
    return hipGetLastError();
}

}  // namespace lsmb

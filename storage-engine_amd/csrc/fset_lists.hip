// fset_lists.hip — the filter set's answer transposed: per-slot lists of key
// indices from the probe's mask rows (lsmb_fset_probe_lists*).
//
// A stream compaction in three kernels over contiguous tiles of kListTile
// keys, one workgroup per tile, chunk c of a tile = its keys [64c, 64c + 64):
//   k_lists_count    per tile and live slot, the rows with the slot's bit set
//                    (one wave ballot + popcount per chunk and slot)
//   k_lists_scan     exclusive scan of those counts over tiles per slot, then
//                    over slots: d_starts[65] and each (slot, tile) offset
//   k_lists_scatter  the ballots again; a key's position = start of its slot
//                    + its tile's offset + the chunks before it in the tile
//                    + its rank among the wave's set lanes (mbcnt)
// Positions follow from counts alone (no atomics), tiles and chunks are
// contiguous and ranks ordered, so every slot's list is ascending and the
// output is the same on every run.  Tile size and scratch bytes:
// fset_lists_plan.hpp.
#include "fset_lists_plan.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace lsmb {

namespace {

constexpr int kListBlock = 256;                                 // 4 waves
constexpr int kListWaves = kListBlock / 64;
constexpr int kListChunks = (int)kListTile / kListBlock;        // chunks (rows) per lane
static_assert(kListTile % kListBlock == 0, "a tile is a whole number of chunks per wave");
constexpr int kScanBlock = 1024;                                // 16 waves, one live slot each per round

// The lane's rows of tile `tile`: row k is key tile * kListTile + (wave *
// kListChunks + k) * 64 + lane; rows past n read as 0 (no bit set).
template <class Row>
__device__ __forceinline__ void load_rows(const Row* __restrict__ rows, uint64_t n, uint64_t tile, uint32_t wave,
                                          uint32_t lane, uint64_t (&r)[kListChunks]) {
    const uint64_t base = tile * kListTile + (uint64_t)wave * (kListChunks * 64) + lane;
#pragma unroll
    for (int k = 0; k < kListChunks; k++) {
        const uint64_t i = base + (uint64_t)k * 64;
        r[k] = i < n ? (uint64_t)rows[i] : 0;
    }
}

// cnt[k] in lane j = the set bits of the j-th live slot among the wave's
// chunk k (j counts the set bits of `live` from the low end).
__device__ __forceinline__ void count_chunks(const uint64_t (&r)[kListChunks], uint64_t live, uint32_t lane,
                                             uint32_t (&cnt)[kListChunks]) {
#pragma unroll
    for (int k = 0; k < kListChunks; k++) cnt[k] = 0;
    uint32_t j = 0;
    for (uint64_t m = live; m; m &= m - 1, j++) {  // wave-uniform: the live slots only
        const uint32_t s = (uint32_t)__builtin_ctzll(m);
#pragma unroll
        for (int k = 0; k < kListChunks; k++) {
            const uint32_t c = (uint32_t)__popcll(__ballot((r[k] >> s) & 1));
            if (lane == j) cnt[k] = c;
        }
    }
}

// counts[j * tpad + tile] = keys of the tile with the j-th live slot's bit set
template <class Row>
__global__ __launch_bounds__(kListBlock) void k_lists_count(const Row* __restrict__ rows, uint64_t n, uint64_t live,
                                                            uint32_t nlive, uint32_t tpad,
                                                            uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[kListWaves][64];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t r[kListChunks];
    uint32_t cnt[kListChunks];
    load_rows(rows, n, blockIdx.x, wave, lane, r);
    count_chunks(r, live, lane, cnt);
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < kListChunks; k++) tot += cnt[k];
    wsum[wave][lane] = tot;
    __syncthreads();
    if (threadIdx.x < nlive) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kListWaves; w++) t += wsum[w][threadIdx.x];
        counts[(uint64_t)threadIdx.x * tpad + blockIdx.x] = t;
    }
}

// One workgroup.  Wave w takes the live slots j = w, w + 16, ...: it replaces
// counts[j][0 .. ntiles) by their exclusive scan (each tile's offset inside the
// slot's list, < 2^32 as n is) 256 tiles a step, and leaves the slot's total
// in LDS; wave 0 then scans the totals over the 64 slots in 64 bits.
__global__ __launch_bounds__(kScanBlock) void k_lists_scan(uint32_t* __restrict__ counts, uint32_t ntiles,
                                                           uint32_t tpad, uint64_t live, uint32_t nlive,
                                                           uint64_t* __restrict__ starts) {
    __shared__ uint32_t total[64];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t j = wave; j < nlive; j += kScanBlock / 64) {
        uint4* row = reinterpret_cast<uint4*>(counts + (uint64_t)j * tpad);  // tpad % 4 == 0
        uint32_t carry = 0;
        uint32_t t = lane * 4;
        uint4 v = t < ntiles ? row[t / 4] : make_uint4(0, 0, 0, 0);
        for (uint32_t t0 = 0; t0 < ntiles; t0 += 256) {
            const uint32_t tn = t0 + 256 + lane * 4;  // the next step's load, issued before this step's scan
            const uint4 vn = tn < ntiles ? row[tn / 4] : make_uint4(0, 0, 0, 0);
            t = t0 + lane * 4;
            // entries at and past ntiles (the padding of the last uint4) hold nothing
            const uint32_t a = t < ntiles ? v.x : 0, b = t + 1 < ntiles ? v.y : 0, c = t + 2 < ntiles ? v.z : 0,
                           d = t + 3 < ntiles ? v.w : 0;
            const uint32_t sum = a + b + c + d;
            const uint32_t incl = wave_incl_scan(sum, lane);
            const uint32_t ex = carry + incl - sum;
            if (t < ntiles) row[t / 4] = make_uint4(ex, ex + a, ex + a + b, ex + a + b + c);
            carry += __shfl(incl, 63);
            v = vn;
        }
        if (lane == 0) total[j] = carry;
    }
    __syncthreads();
    if (wave == 0) {
        // lane = slot; its live index = the live slots below it
        const bool is_live = (live >> lane) & 1;
        const uint32_t j = (uint32_t)__popcll(live & ((1ull << lane) - 1));
        const uint64_t cnt = is_live ? total[j] : 0;
        const uint64_t v = wave_incl_scan(cnt, lane);
        starts[lane] = v - cnt;
        if (lane == 63) starts[64] = v;
    }
}

// index[starts[s] + offs[j][tile] + (set bits of slot s before key i in the
// tile)] = i for every key i of the tile with bit s set, where that position
// is below cap.
template <class Row>
__global__ __launch_bounds__(kListBlock) void k_lists_scatter(const Row* __restrict__ rows, uint64_t n, uint64_t live,
                                                              uint32_t nlive, uint32_t tpad,
                                                              const uint32_t* __restrict__ offs,
                                                              const uint64_t* __restrict__ starts,
                                                              uint32_t* __restrict__ index, uint64_t cap) {
    __shared__ uint32_t wsum[kListWaves][64];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t r[kListChunks];
    uint32_t cnt[kListChunks];
    load_rows(rows, n, blockIdx.x, wave, lane, r);
    count_chunks(r, live, lane, cnt);
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < kListChunks; k++) tot += cnt[k];
    wsum[wave][lane] = tot;
    __syncthreads();
    // lane j: where the j-th live slot's entries of this wave begin
    uint64_t base = 0;
    if (lane < nlive) {
        // slot of live index `lane`: clear the lane lowest set bits of live
        uint64_t m = live;
        for (uint32_t q = 0; q < lane; q++) m &= m - 1;
        const uint32_t s = (uint32_t)__builtin_ctzll(m);
        base = starts[s] + offs[(uint64_t)lane * tpad + blockIdx.x];
        for (uint32_t w = 0; w < wave; w++) base += wsum[w][lane];
    }
    const uint32_t i0 = (uint32_t)((uint64_t)blockIdx.x * kListTile) + wave * (kListChunks * 64) + lane;
    uint32_t j = 0;
    for (uint64_t m = live; m; m &= m - 1, j++) {
        const uint32_t s = (uint32_t)__builtin_ctzll(m);
        // the wave's first position of slot s: lane j's base, made uniform
        uint64_t pos = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base >> 32), (int)j) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, (int)j);
#pragma unroll
        for (int k = 0; k < kListChunks; k++) {
            const bool hit = (r[k] >> s) & 1;
            const uint64_t b = __ballot(hit);
            const uint32_t rank =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            const uint64_t p = pos + rank;
            if (hit && p < cap) index[p] = i0 + (uint32_t)k * 64;
            pos += (uint32_t)__popcll(b);
        }
    }
}

template <class Row>
hipError_t lists_with(const Row* rows, uint64_t n, uint64_t live, uint32_t nlive, uint32_t ntiles, uint32_t tpad,
                      uint32_t* tiles, uint64_t* starts, uint32_t* index, uint64_t cap, hipStream_t st,
                      hipEvent_t done) {
    k_lists_count<Row><<<ntiles, kListBlock, 0, st>>>(rows, n, live, nlive, tpad, tiles);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    k_lists_scan<<<1, kScanBlock, 0, st>>>(tiles, ntiles, tpad, live, nlive, starts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return launch_done(k_lists_scatter<Row>, dim3(ntiles), dim3(kListBlock), 0, st, done, rows, n, live, nlive, tpad,
                       (const uint32_t*)tiles, (const uint64_t*)starts, index, cap);
}

}  // namespace

hipError_t launch_fset_lists(const uint8_t* d_rows, uint32_t row_bytes, uint64_t n, uint64_t live, uint32_t* d_tiles,
                             uint64_t* d_starts, uint32_t* d_index, uint64_t cap, hipStream_t st, hipEvent_t done) {
    if (n == 0 || live == 0 || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (row_bytes < 8 && (live >> (8 * row_bytes)) != 0) return hipErrorInvalidValue;
    const uint32_t nlive = (uint32_t)__builtin_popcountll(live);
    const uint32_t ntiles = (uint32_t)((n + kListTile - 1) / kListTile);
    const uint32_t tpad = (ntiles + 3) & ~3u;
    switch (row_bytes) {
        case 1: return lists_with((const uint8_t*)d_rows, n, live, nlive, ntiles, tpad, d_tiles, d_starts, d_index, cap, st, done);
        case 2: return lists_with((const uint16_t*)d_rows, n, live, nlive, ntiles, tpad, d_tiles, d_starts, d_index, cap, st, done);
        case 4: return lists_with((const uint32_t*)d_rows, n, live, nlive, ntiles, tpad, d_tiles, d_starts, d_index, cap, st, done);
        case 8: return lists_with((const uint64_t*)d_rows, n, live, nlive, ntiles, tpad, d_tiles, d_starts, d_index, cap, st, done);
    }
    return hipErrorInvalidValue;
}

}  // namespace lsmb

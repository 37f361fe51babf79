// build_plan.hip — the host planner of the Bloom build: which strategy a build
// takes, the partitioned and tiled plans, the key chunk a workspace limit
// allows, and the bytes every workspace buffer must hold (the one contract
// build_dev.hip allocates by and bloom_build.hip's launchers validate by).
//
// Host-only arithmetic over the geometry constants of kernels.hpp: no HIP call,
// so tests/cpp/plan_test.cpp links this file and checks it against
// tests/golden/plan_table.json without a GPU.
#include <math.h>
#include <stdlib.h>

#include "kernels.hpp"

namespace lsmb {

const char* strategy_name(BuildStrategy s) {
    switch (s) {
        case BuildStrategy::None: return "none";
        case BuildStrategy::Lds: return "lds";
        case BuildStrategy::Partition: return "partition";
        case BuildStrategy::Atomic: return "atomic";
        case BuildStrategy::Tiled: return "tiled";
    }
    return "?";
}

BuildStrategy pick_build_strategy(uint32_t num_bits, uint32_t k, uint64_t n) {
    if (n == 0 || k == 0 || num_bits == 0) return BuildStrategy::None;
    const uint64_t nw32 = 2 * (((uint64_t)num_bits + 63) / 64);
    if (nw32 <= kLdsFilterMaxWords32) return BuildStrategy::Lds;
    if (k > 32) return BuildStrategy::Atomic;
    // Few keys into a big filter: scattered atomics beat a full-slice RMW.
    if (n * (uint64_t)k < nw32 / 16) return BuildStrategy::Atomic;
    // Fewer than 64 slices (< 8 MiB filters): too few LDS buffers to spread
    // a workgroup's claims; memory-side atomics on the small filter instead.
    if (nw32 <= (uint64_t)kTiledMaxSlices * kSliceWords32 && k <= 32) return BuildStrategy::Tiled;
    if (nw32 < 64ull * kSliceWords32) return BuildStrategy::Atomic;
    return BuildStrategy::Partition;
}

namespace {
// The layout with bins of 2^sl bits.
PartitionPlan layout_sl(uint32_t num_bits, uint32_t k, uint32_t sl) {
    PartitionPlan pl;
    pl.slice_log2 = sl;
    pl.nbins = (uint32_t)(((uint64_t)num_bits + (1ull << sl) - 1) >> sl);
    // Entries a slice's ring receives per pass A phase (1024 keys), and the
    // ring that holds a segment's worth of leftovers plus a phase's arrivals
    // with margin.  Claims past the ring fall back to exact global atomics.
    const double lambda = (double)kBinBlock * k * fmin(1.0, (double)(1u << sl) / (double)num_bits);
    uint32_t need = kSegEntries + (uint32_t)ceil(lambda + 2.0 * sqrt(lambda));
    need = (need + 7) & ~7u;
    if (need > kMaxRing) need = kMaxRing;
    // Fewest sweeps whose slices fit LDS with that ring; each sweep re-reads
    // and re-hashes the keys and keeps only its own slices' positions.
    pl.sweeps = (pl.nbins + kMaxBinsPerSweep - 1) / kMaxBinsPerSweep;
    for (;; pl.sweeps++) {
        pl.bins_per_sweep = (pl.nbins + pl.sweeps - 1) / pl.sweeps;
        uint32_t r = (kBinLdsBudget / (pl.bins_per_sweep + 1) - kBinExtraBytes) / 4;  // + the sink slice
        r &= ~7u;
        if (r > kMaxRing) r = kMaxRing;
        if (r >= need || pl.bins_per_sweep == 1) {
            pl.ring = r;
            break;
        }
    }
    // k = 7 sweeps take two keys per lane per phase when the ring holds a
    // phase's doubled arrivals to within one 8-entry group: C5's 32-entry
    // rings (2^21-bit bins, 1024 per sweep; need2 = 40) then send ~0.45 % of
    // the positions to the exact global-atomic path, and pass A still gains
    // (C5 shard: 2.38 -> 2.33 ms).  Single-sweep filters keep one even where
    // the rings would hold two: it is slower there (4.97e8 bits, 100 M keys:
    // 0.995 -> 1.026 ms).  LSMB_SWEEP_PER=1 / =2 forces one / two
    // (measurement knob).
    if (k == 7) {
        const char* e = getenv("LSMB_SWEEP_PER");
        const uint32_t need2 = (kSegEntries + (uint32_t)ceil(2 * lambda + 2.0 * sqrt(2 * lambda)) + 7) & ~7u;
        // Not for the saturated 2^32-1-bit filter: with its fold walk (WalkM)
        // the doubled phase is slower (C5 shard, accumulate: pass A 2.074 ->
        // 2.136 ms; tools/r04_c5per.sh).
        const bool auto2 = pl.sweeps > 1 && pl.ring + 8 >= need2 && num_bits != kMersenneBits;
        if ((auto2 && !(e && atoi(e) == 1)) || (e && atoi(e) == 2)) pl.keys_per_lane = 2;
    }
    return pl;
}
}  // namespace

// Bins of 2^20 bits (one pass B workgroup's LDS) unless the filter needs
// several sweeps: then 2^21-bit bins halve the sweeps (each re-reads and
// re-hashes every key) for a second read of each bin's regions in pass B.
// k = 7 only (the kernels instantiated for it); LSMB_SLICE_LOG2=20 pins 2^20,
// =21 forces 2^21 (measurement knobs).
PartitionPlan partition_layout(uint32_t num_bits, uint32_t k) {
    const PartitionPlan p20 = layout_sl(num_bits, k, kSliceLog2);
    const char* e = getenv("LSMB_SLICE_LOG2");
    if (k == 7 && e && atoi(e) == 21 && num_bits > (1u << 21))  // measurement: force 2^21-bit bins
        return layout_sl(num_bits, k, 21);
    if (p20.sweeps < 2 || k != 7) return p20;
    if (e && atoi(e) == 20) return p20;
    const PartitionPlan p21 = layout_sl(num_bits, k, 21);
    return p21.sweeps < p20.sweeps ? p21 : p20;
}

PartitionPlan partition_capacity(PartitionPlan pl, uint32_t num_bits, uint32_t k, uint64_t n, int num_cus) {
    // 1024-thread workgroups (one resident per CU), at least ~kBinBlock keys
    // each: two per CU for 2^20-bit bins — pass B then streams twice as many,
    // half-size regions per slice (C2: pass B 0.448 -> 0.411 ms, pass A
    // unchanged) — one for 2^21-bit bins, whose two half-bin workgroups each
    // read every region (C5 shard: pass B 0.843 -> 0.986 ms at two).
    // LSMB_BIN_WGS_PER_CU overrides (measurement knob, tools/bin_wgs.sh).
    const uint64_t gmax = (n + kBinBlock - 1) / kBinBlock;
    static const long wenv = [] {
        const char* e = getenv("LSMB_BIN_WGS_PER_CU");
        return e ? atol(e) : 0L;
    }();
    const uint64_t wpc = wenv >= 1 && wenv <= 4 ? (uint64_t)wenv : (pl.slice_log2 == kSliceLog2 ? 2 : 1);
    uint64_t g = (uint64_t)num_cus * wpc;
    if (g > gmax) g = gmax;
    if (g < 1) g = 1;
    pl.grid = (uint32_t)g;
    const uint64_t keys_w = (n + g - 1) / g;  // workgroup w hashes keys [w*keys_w, (w+1)*keys_w)
    double p = (double)(1u << pl.slice_log2) / (double)num_bits;
    if (p > 1.0) p = 1.0;
    const double mu = (double)keys_w * k * p;
    const double cap_e = mu + 8.0 * sqrt(mu) + 2.0 * kSegEntries;
    pl.cap_segs = (uint32_t)ceil(cap_e / kSegEntries);
    // A region holds at most kMaxRegionSegs segments (and a workgroup's regions
    // stay within pass A's 2^31-byte buffer range): a bigger plan is reported
    // as unbounded so callers chunk the keys.
    const bool fits = pl.cap_segs <= kMaxRegionSegs && (uint64_t)pl.nbins * pl.cap_segs * kSegSlotBytes < (1ull << 31);
    pl.region_bytes = fits ? (uint64_t)pl.nbins * pl.grid * pl.cap_segs * kSegSlotBytes : ~0ull >> 2;
    pl.counts_bytes = (uint64_t)pl.nbins * pl.grid * 4;
    return pl;
}

PartitionPlan plan_partition(uint32_t num_bits, uint32_t k, uint64_t n, int num_cus) {
    return partition_capacity(partition_layout(num_bits, k), num_bits, k, n, num_cus);
}

TiledPlan plan_tiled(uint32_t num_bits, uint64_t n, int num_cus) {
    TiledPlan tp;
    const uint64_t nw32 = 2 * (((uint64_t)num_bits + 63) / 64);
    tp.nslices = (uint32_t)((nw32 + kSliceWords32 - 1) / kSliceWords32);
    // ~2 workgroups per CU in all, at least 4 Ki keys per chunk
    uint64_t ch = (2ull * (uint64_t)num_cus + tp.nslices - 1) / tp.nslices;
    const uint64_t by_keys = (n + 4095) / 4096;
    if (ch > by_keys) ch = by_keys;
    if (ch < 1) ch = 1;
    tp.chunks = (uint32_t)ch;
    tp.stride32 = (uint64_t)tp.nslices * kSliceWords32;
    tp.scratch_bytes = (uint64_t)tp.chunks * tp.stride32 * 4;
    return tp;
}

uint64_t partition_chunk_keys(uint32_t num_bits, uint32_t k, uint64_t max_bytes, int num_cus) {
    const PartitionPlan layout = partition_layout(num_bits, k);
    uint64_t lo = 0, hi = (1ull << 40);
    while (lo + 1 < hi) {  // largest n whose plan fits
        const uint64_t mid = lo + (hi - lo) / 2;
        const PartitionPlan pl = partition_capacity(layout, num_bits, k, mid, num_cus);
        if (pl.region_bytes + pl.counts_bytes <= max_bytes) lo = mid; else hi = mid;
    }
    return lo;
}

WorkspaceBytes workspace_bytes(BuildStrategy s, const PartitionPlan& pl, const TiledPlan& tp, uint32_t num_bits,
                               uint32_t k, uint64_t n, bool aligned16, bool fresh) {
    WorkspaceBytes b;
    if (s == BuildStrategy::Tiled) {
        b.regions = tp.scratch_bytes;
        b.hashes = n * 16;  // every slice's workgroups read the keys' 16-B hash records
    } else if (s == BuildStrategy::Partition) {
        b.regions = pl.region_bytes;
        b.counts = pl.counts_bytes;
        // Keys that pass A does not hash inline are hashed first.  16 B per
        // key; partition builds store 12-B walk records in them.
        if (!aligned16) b.hashes = n * 16;
        if (fresh && k == 7) {
            // the LIST pass A: overflow words + one mark per 2^20-bit unit of
            // the whole filter, and a position list + length per workgroup
            // per sweep
            const uint64_t nw32 = 2 * (((uint64_t)num_bits + 63) / 64);
            const uint64_t units = (nw32 + kSliceWords32 - 1) / kSliceWords32;
            b.ovf = units * kSliceWords32 * 4;
            b.dirty = units * 4;
            b.ovl = (uint64_t)pl.grid * pl.sweeps * kOvfListCap * 4;
            b.ovn = (uint64_t)pl.grid * pl.sweeps * 4;
        }
    }
    return b;
}

}  // namespace lsmb

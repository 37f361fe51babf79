// build_batch.hip — many SSTable filters from one device-resident key run in
// one launch per geometry class (gfx950).
//
// The store sizes every SSTable's filter new(1000, 0.01) (SSTableBuilder::new,
// src/sstable/builder.rs:51,74: 9 586 bits, 1 212 bytes) and builds it key by
// key (builder.rs:93 add_key, builder.rs:177-182 build + serialize).  One such
// filter is too small to pay for a launch, but a bulk load, a level rewritten
// with another false-positive rate or several compactions finishing together
// (src/compaction/scheduler.rs:147-177) build thousands at once.  Here every
// table is one or more items of the work list in build_batch_plan.hpp:
//   wave   an item per wave, four per 256-lane workgroup, each wave with a
//          private LDS region and no workgroup barrier;
//   group  an item per 1 024-lane workgroup with up to the whole LDS.
// An item zeroes its LDS image of the table's slot, sets the k positions of
// each of its keys in it with ds_or (the same XXH3-128 split and wrapping
// double-hash walk as every other build: bit-identical words), and writes the
// image out.  A single-part table is output-only: each of its words, zero
// ones and the pad word included, is stored exactly once with plain 16-byte
// stores, so nothing is zeroed beforehand and no global atomic is used.  Only
// the parts of a table split over several items OR their non-zero words in
// with atomicOr, after k_bb_zero cleared just those slots.
#include "build_batch_dev.hpp"
#include "keysrc.hpp"

namespace lsmb {
namespace {

template <class Src, bool kGroup>
__global__ __launch_bounds__(kGroup ? kBbGroupLanes : kBbWaveLanes * kBbWavesPerGroup) void k_build_batch(
    Src src, const BbItem* __restrict__ items, uint32_t nitems, uint32_t region32, uint32_t* __restrict__ gw) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bb_lds[];
    const uint32_t L = kGroup ? blockDim.x : kBbWaveLanes;  // the lanes that share the item
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kBbWaveLanes);
    const uint32_t idx = kGroup ? blockIdx.x : blockIdx.x * kBbWavesPerGroup + wave;
    if (idx >= nitems) return;  // whole waves; the wave class meets no workgroup barrier
    const uint32_t lane = kGroup ? threadIdx.x : threadIdx.x % kBbWaveLanes;
    uint32_t* f = bb_lds + (kGroup ? 0u : wave * region32);  // region32 is a multiple of 4: 16-byte aligned
    const BbItem it = items[idx];  // nw32 <= region32 (host: region32 = the launch's largest nw32)

    bb_image_clear(f, it, lane, L);
    bb_sync<kGroup>();

    // the next key's load (its offsets, for var-len keys) is in flight while this one is hashed and walked
    uint64_t i = it.key_lo + lane;
    typename Src::Pre pre = src.fetch(i, i < it.key_hi);
    for (; i < it.key_hi; i += L) {
        const typename Src::Pre nxt = src.fetch(i + L, i + L < it.key_hi);
        const H128 h = src.hash_pre(pre, i);
        Walk32 pw(it.md, h.lo, h.hi);  // num_bits <= 1 310 720 < 2^31
        for (uint32_t j = 0; j < it.k; j++) {
            const uint32_t p = pw.pos();
            atomicOr(&f[p >> 5], 1u << (p & 31));
            pw.next(it.md);
        }
        pre = nxt;
    }
    bb_sync<kGroup>();

    bb_image_out(f, it, gw, lane, L);
}

template <class Src>
hipError_t launch_classes(const Src& src, const BbItem* d_items, uint32_t nzero, uint32_t nwave, uint32_t ngroup,
                          uint32_t wave_region32, uint32_t group_region32, uint32_t group_lanes, uint32_t* gw,
                          hipStream_t st, hipEvent_t done) {
    // (one-time attribute per instantiation: function-local statics are initialised once, thread-safely)
    static const hipError_t attr_w = hipFuncSetAttribute((const void*)k_build_batch<Src, false>,
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    static const hipError_t attr_g = hipFuncSetAttribute((const void*)k_build_batch<Src, true>,
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (attr_w != hipSuccess) return attr_w;
    if (attr_g != hipSuccess) return attr_g;
    hipError_t e = hipSuccess;
    if (nzero) {
        k_bb_zero<<<dim3(nzero), dim3(256), 0, st>>>(d_items, gw);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the last launch completes `done` itself (launch_done)
    if (nwave) {
        const uint32_t nwg = (nwave + kBbWavesPerGroup - 1) / kBbWavesPerGroup;
        e = launch_done(k_build_batch<Src, false>, dim3(nwg), dim3(kBbWaveLanes * kBbWavesPerGroup),
                        wave_region32 * 4 * kBbWavesPerGroup, st, ngroup ? nullptr : done, src, d_items + nzero, nwave,
                        wave_region32, gw);
        if (e != hipSuccess) return e;
    }
    if (ngroup)
        e = launch_done(k_build_batch<Src, true>, dim3(ngroup), dim3(group_lanes), group_region32 * 4, st, done, src,
                        d_items + nzero + nwave, ngroup, group_region32, gw);
    return e;
}

}  // namespace

hipError_t launch_build_batch(const KeyBatch& kb, const BbItem* d_items, uint32_t nzero, uint32_t nwave,
                              uint32_t ngroup, uint32_t wave_region32, uint32_t group_region32, uint32_t group_lanes,
                              uint64_t* d_words, hipStream_t st, hipEvent_t done) {
    if (group_lanes < kBbWaveLanes || group_lanes > kBbGroupLanes || group_lanes % kBbWaveLanes) return hipErrorInvalidValue;
    if (wave_region32 % 4 || group_region32 % 4 || wave_region32 * 4 * kBbWavesPerGroup > kLdsBytes ||
        group_region32 * 4 > kLdsBytes)
        return hipErrorInvalidValue;
    uint32_t* gw = reinterpret_cast<uint32_t*>(d_words);
    if (nwave + ngroup == 0) return done ? hipEventRecord(done, st) : hipSuccess;
    return with_key_source(kb, [&](auto src) {
        return launch_classes(src, d_items, nzero, nwave, ngroup, wave_region32, group_region32, group_lanes, gw, st,
                              done);
    });
}

}  // namespace lsmb

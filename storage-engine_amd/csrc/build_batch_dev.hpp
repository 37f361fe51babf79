// build_batch_dev.hpp — the device steps every batched build kernel shares
// (build_batch.hip over packed keys, build_batch_sst.hip over data blocks):
// the phase barrier of an item, its LDS image cleared and written out, and the
// zero pass of the multi-part tables.  Device side, internal.
#pragma once

#include "build_batch_plan.hpp"
#include "kernels.hpp"

namespace lsmb {
namespace {

static_assert(kBbMaxWords32 == kLdsFilterMaxWords32, "the batch accepts the LDS class");
static_assert(kBbLdsBytes == kLdsBytes, "LDS per CU");
static_assert(kBbMaxWords32 * 4 <= kBbLdsBytes, "a group item's image fits the LDS");
static_assert((kBbWaveMaxBits / 32) * 4 * kBbWavesPerGroup <= kBbLdsBytes, "four wave regions fit the LDS");

// Between an item's phases.  group: the workgroup's barrier.  wave: the 64
// lanes run in lock step and the LDS serves one wave's operations in order,
// so the compiler alone has to be kept from moving LDS accesses across.
template <bool kGroup>
__device__ __forceinline__ void bb_sync() {
    if constexpr (kGroup) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// The item's image f (16-byte aligned, it.nw32 / 4 quads) zeroed by the L lanes that share it.
__device__ __forceinline__ void bb_image_clear(uint32_t* f, const BbItem& it, uint32_t lane, uint32_t L) {
    uint4* f4 = reinterpret_cast<uint4*>(f);
    for (uint32_t q = lane; q < it.nw32 / 4; q += L) f4[q] = make_uint4(0, 0, 0, 0);
}

// The finished image into the table's slot: a single part stores every word
// once with plain 16-byte stores (the buffer and every slot are 16-byte
// aligned), the parts of a split table OR their non-zero words into the slot
// k_bb_zero cleared.
__device__ __forceinline__ void bb_image_out(const uint32_t* f, const BbItem& it, uint32_t* __restrict__ gw, uint32_t lane,
                                             uint32_t L) {
    uint32_t* dst = gw + 2 * it.dst;
    if (it.parts == 1) {
        const uint4* f4 = reinterpret_cast<const uint4*>(f);
        uint4* dst4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t q = lane; q < it.nw32 / 4; q += L) dst4[q] = f4[q];
    } else {
        for (uint32_t w = lane; w < it.nw32; w += L) {
            const uint32_t v = f[w];
            if (v) atomicOr(dst + w, v);
        }
    }
}

// The slots of the multi-part tables (one item each), cleared before their parts OR in.
__global__ __launch_bounds__(256) void k_bb_zero(const BbItem* __restrict__ items, uint32_t* __restrict__ gw) {
    const BbItem it = items[blockIdx.x];
    uint4* dst4 = reinterpret_cast<uint4*>(gw + 2 * it.dst);
    for (uint32_t q = threadIdx.x; q < it.nw32 / 4; q += 256) dst4[q] = make_uint4(0, 0, 0, 0);
}

}  // namespace
}  // namespace lsmb

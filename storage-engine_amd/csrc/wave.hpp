// wave.hpp — the 64-lane wave steps the lists kernels share (device side,
// internal): fset_lists.hip, lset_lists.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsmb {

__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Inclusive scan over the wave's 64 lanes: lane L returns the sum of v over
// lanes 0 .. L (lane = lane_id()).
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= (uint32_t)d) v += up;
    }
    return v;
}

}  // namespace lsmb

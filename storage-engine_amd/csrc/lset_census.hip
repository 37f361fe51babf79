// lset_census.hip — k_popcount_segs: the set bits of many small device
// segments in one launch, the count behind a level set's fill census
// (lsmb_lset_census, capi_lset.hip: every SSTable filter of a resident Version,
// ~1.2 KB each, counted where it lives).  The geometry is k_copy_segs'
// (lset_repack.hip) and k_crc32_seg's (crc32.hip): one wave per item, four
// items per workgroup, no workgroup barrier.  The items and their planner are
// in popcount_seg.hpp, where a CPU test drives them.
#include "ctx.hpp"
#include "keysrc.hpp"
#include "popcount_seg.hpp"

namespace lsmb {
namespace {

// Wave w of workgroup b counts item s = 4 b + w.  The words wholly below
// nbits, in pairs: lane-strided 16-byte units, kPopSegInFlight non-temporal
// loads per lane issued before their counts (the words are read once).  Whole
// iterations first, every lane taking part; then the rest, unit by unit, lanes
// past the end idle.  What the units leave, at most two words (an odd word of
// the whole ones, and the word nbits ends in), is one 8-byte load each on a
// lane of its own, the last masked to its bits below nbits: ceil(nbits / 64)
// words are read and nothing after them.  One shuffle tree, lane 0 stores.
__global__ __launch_bounds__(kPopSegLanes* kPopSegPerBlock) void k_popcount_segs(const PopSeg* __restrict__ segs,
                                                                                  uint64_t nseg,
                                                                                  uint64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x % kPopSegLanes;
    const uint64_t s = (uint64_t)blockIdx.x * kPopSegPerBlock + threadIdx.x / kPopSegLanes;
    if (s >= nseg) return;  // idle waves of the last workgroup
    const PopSeg sg = segs[s];
    // pointers read from memory are generic; these are device memory: global loads
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    typedef __attribute__((address_space(1))) uint64_t g_u64;
    const g_u32x4* __restrict__ src = (const g_u32x4*)sg.words;
    const uint64_t full = sg.nbits / 64;  // words wholly below nbits
    const uint32_t rem = (uint32_t)(sg.nbits % 64);
    const uint64_t n = full / 2;  // 16-byte units of whole words
    constexpr uint64_t kIter = (uint64_t)kPopSegLanes * kPopSegInFlight;
    const uint64_t whole = n / kIter * kIter;
    uint64_t cnt = 0;
    auto count = [&](const u32x4 v) {
        cnt += (uint64_t)__popcll((uint64_t)v.x | (uint64_t)v.y << 32) + (uint64_t)__popcll((uint64_t)v.z | (uint64_t)v.w << 32);
    };
    uint64_t i = lane;
    for (; i < whole; i += kIter) {
        u32x4 v[kPopSegInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kPopSegInFlight; j++) v[j] = __builtin_nontemporal_load(src + i + j * kPopSegLanes);
#pragma unroll
        for (uint32_t j = 0; j < kPopSegInFlight; j++) count(v[j]);
    }
    for (; i < n; i += kPopSegLanes) count(__builtin_nontemporal_load(src + i));
    // words 2 n .. last: word 2 n + lane on lane 0 and lane 1
    const uint64_t w = 2 * n + lane, last = full + (rem != 0);
    if (w < last) {
        uint64_t v = __builtin_nontemporal_load((const g_u64*)sg.words + w);
        if (w == full) v &= (1ull << rem) - 1;  // rem != 0 here: the bits at and above nbits do not count
        cnt += (uint64_t)__popcll(v);
    }
#pragma unroll
    for (uint32_t d = kPopSegLanes / 2; d; d >>= 1) cnt += __shfl_down(cnt, d);  // all 64 lanes take part
    if (lane == 0) out[s] = cnt;
}

}  // namespace

// d_out[s] = the set bits of segment d_segs[s] (both in device memory), one
// launch on st; nothing is synchronised.
int popcount_segs_dev(const PopSeg* d_segs, uint64_t nseg, uint64_t* d_out, hipStream_t st) {
    if (nseg == 0) return LSMB_OK;
    const uint64_t nwg = (nseg + kPopSegPerBlock - 1) / kPopSegPerBlock;
    if (nwg > 0x7FFFFFFFull) return fail(LSMB_EINVAL, "popcount: %llu segments are too many", (unsigned long long)nseg);
    k_popcount_segs<<<dim3((uint32_t)nwg), dim3(kPopSegLanes * kPopSegPerBlock), 0, st>>>(d_segs, nseg, d_out);
    HIP_TRY(hipGetLastError());
    return LSMB_OK;
}

}  // namespace lsmb

using namespace lsmb;

extern "C" {

int lsmb_popcount_segs_dev(lsmb_ctx* c, const void* d_segs, uint64_t nseg, void* d_out, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null argument");
    if (nseg && (!d_segs || !d_out)) return fail(LSMB_EINVAL, "null device pointer");
    DevGuard g(c->dev);
    return popcount_segs_dev((const PopSeg*)d_segs, nseg, (uint64_t*)d_out, stream ? (hipStream_t)stream : c->st);
}

}  // extern "C"

// lset_repack.hip — k_copy_segs: many small device-to-device moves in one
// launch, the copy behind a repacking derive (lsmb_lset_derive_packed,
// capi_lset.hip: the surviving SSTable filters of sparse arena chunks, ~1.2 KB
// each, moved into the child's own chunk).  The geometry is k_crc32_seg's
// (crc32.hip): one wave per item, four items per workgroup, no workgroup
// barrier.  The items and their planner are in lset_repack.hpp, where a CPU
// test drives them.
#include "ctx.hpp"
#include "keysrc.hpp"
#include "lset_repack.hpp"

namespace lsmb {
namespace {

// Wave w of workgroup b moves item s = 4 b + w: lane-strided 16-byte units,
// kCopySegInFlight loads per lane issued before their stores.  The loads are
// non-temporal (the parent's words are read once), the stores plain (the
// child's probes read them next).  Whole iterations first, every lane taking
// part; then the rest, unit by unit, lanes past the end idle.
__global__ __launch_bounds__(kCopySegLanes* kCopySegPerBlock) void k_copy_segs(const CopySeg* __restrict__ segs,
                                                                                uint64_t nseg) {
    const uint32_t lane = threadIdx.x % kCopySegLanes;
    const uint64_t s = (uint64_t)blockIdx.x * kCopySegPerBlock + threadIdx.x / kCopySegLanes;
    if (s >= nseg) return;  // idle waves of the last workgroup
    const CopySeg sg = segs[s];
    // pointers read from memory are generic; these are device memory: global loads and stores
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    const g_u32x4* __restrict__ src = (const g_u32x4*)sg.src;
    g_u32x4* __restrict__ dst = (g_u32x4*)sg.dst;
    const uint64_t n = sg.len / 16;  // 16-byte units
    constexpr uint64_t kIter = (uint64_t)kCopySegLanes * kCopySegInFlight;
    const uint64_t whole = n / kIter * kIter;
    uint64_t i = lane;
    for (; i < whole; i += kIter) {
        u32x4 v[kCopySegInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kCopySegInFlight; j++) v[j] = __builtin_nontemporal_load(src + i + j * kCopySegLanes);
#pragma unroll
        for (uint32_t j = 0; j < kCopySegInFlight; j++) dst[i + j * kCopySegLanes] = v[j];
    }
    for (; i < n; i += kCopySegLanes) dst[i] = __builtin_nontemporal_load(src + i);
}

}  // namespace

// Every item of d_segs (device memory) moved by one launch on st; nothing is
// synchronised.
int copy_segs_dev(const CopySeg* d_segs, uint64_t nseg, hipStream_t st) {
    if (nseg == 0) return LSMB_OK;
    const uint64_t nwg = (nseg + kCopySegPerBlock - 1) / kCopySegPerBlock;
    if (nwg > 0x7FFFFFFFull) return fail(LSMB_EINVAL, "copy: %llu segments are too many", (unsigned long long)nseg);
    k_copy_segs<<<dim3((uint32_t)nwg), dim3(kCopySegLanes * kCopySegPerBlock), 0, st>>>(d_segs, nseg);
    HIP_TRY(hipGetLastError());
    return LSMB_OK;
}

}  // namespace lsmb

using namespace lsmb;

extern "C" {

int lsmb_copy_segs_dev(lsmb_ctx* c, const void* d_segs, uint64_t nseg, void* stream) {
    if (!c) return fail(LSMB_EINVAL, "null argument");
    if (nseg && !d_segs) return fail(LSMB_EINVAL, "null device pointer");
    DevGuard g(c->dev);
    return copy_segs_dev((const CopySeg*)d_segs, nseg, stream ? (hipStream_t)stream : c->st);
}

}  // extern "C"

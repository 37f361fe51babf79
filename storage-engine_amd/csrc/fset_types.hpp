// fset_types.hpp — the plain structs a set of ranged filters is described by
// (internal): what the host plans (fset_plan.hpp, which a CPU-only test
// includes, so nothing here needs more of HIP than bloom_math.hpp does) and
// the probe kernels take (kernels.hpp).
#pragma once

#include <stdint.h>

#include "bloom_math.hpp"

namespace lsmb {

// Filter descriptor for the probe kernels (device-side array).
struct ProbeFilter {
    const uint32_t* words32;
    Mod32 md;
    uint32_t num_bits;
    uint32_t k;
    uint32_t out_bit;  // bit index in the output mask row
    uint32_t group;    // filters with equal (num_bits, k) share one position walk
};

// A filter of a filter set (lsmb_fset): the SSTable's filter plus its key
// range [lo, hi] (SSTable meta min_key/max_key, src/sstable/reader.rs:192).
struct RangedFilter {
    ProbeFilter f;  // f.out_bit = the slot
    const uint8_t* lo;
    const uint8_t* hi;
    uint32_t lo_len, hi_len;
};

// The key ranges of a filter set as sorted boundary points (built on the host
// per set): the distinct min/max keys of the live tables in Rust [u8] order.
// For a key, region 2r = strictly between points r-1 and r, region 2r+1 =
// equal to point r; regmask[region] = the descriptors (bit d = descriptor d)
// whose [min_key, max_key] holds every key of that region.  So the range
// pre-check of all F tables is one rank search over <= 2F points.
constexpr uint32_t kFsetMaxPoints = 128;
struct FsetPoint {
    uint64_t w0, w1;   // zero-padded 16-byte prefix as two big-endian words
    const uint8_t* p;  // the full key (device memory)
    uint32_t len, pad;
};
struct FsetRanges {
    const FsetPoint* pts;     // npts, sorted
    const uint64_t* regmask;  // 2 * npts + 1
    uint32_t npts;
};

// Size classes of a filter set: the live filters grouped by (num_bits, k),
// each class a bit-sliced LDS table (entry p = its members' bit p, `width`
// bytes), the classes together within kFsetTableBytes of LDS.  Filters of
// classes that do not fit (and k = 0 filters) are walked from L2.
constexpr uint32_t kFsetMaxClasses = 8;
constexpr uint32_t kFsetTableBytes = 64 * 1024;
struct FsetClass {
    Mod32 md;
    Mod14 md14;        // valid when num_bits < 2^14 (small): the walk's cheaper reduction
    uint32_t num_bits, k;
    uint32_t off;      // byte offset of the class table in the LDS tables
    uint32_t width;    // entry bytes: 1, 2, 4 or 8 (members <= 8, 16, 32, 64)
    uint32_t nmem, pad;
    uint64_t mask;     // the members' descriptor bits
    uint8_t mem[64];   // member j -> descriptor index
};
struct FsetClasses {
    FsetClass cls[kFsetMaxClasses];  // by value: the kernel reads them as uniform kernel arguments
    uint32_t ncls;
    uint32_t table_bytes;  // LDS bytes of all class tables
    uint64_t walk_mask;    // descriptors walked from L2
};

}  // namespace lsmb

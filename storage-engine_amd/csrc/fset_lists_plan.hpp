// fset_lists_plan.hpp — the tile geometry of the mask-row compaction
// (fset_lists.hip) and the size of its scratch, free of HIP so that the
// workspace plans of its callers (lset_vlists_plan.hpp) and their host tests
// state the formula once.  Internal.
#pragma once

#include <stdint.h>

namespace lsmb {

constexpr uint32_t kListTile = 1024;  // keys per workgroup

// Bytes of launch_fset_lists' d_tiles for n mask rows and the slots of `live`:
// one u32 per live slot and tile, every slot's row padded to whole uint4s.
inline uint64_t fset_lists_tile_bytes(uint64_t n, uint64_t live) {
    const uint64_t ntiles = (n + kListTile - 1) / kListTile;
    return (uint64_t)__builtin_popcountll(live) * ((ntiles + 3) & ~3ull) * 4;
}

}  // namespace lsmb

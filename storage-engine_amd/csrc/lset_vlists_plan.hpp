// lset_vlists_plan.hpp — the host side of a level set's Version lists probe
// (lsmb_lset_probe_version_lists*, launcher in lset_version_lists.hip), free
// of HIP so that tests/cpp/lset_vlists_plan_test.cpp can drive it on a CPU:
// the mask row width of the L0 part, the one statement of the workspace layout
// (the allocators size by it, the launcher validates and carves by it) and a
// plain C++ statement of the whole transform (lset_vlists_ref).  Internal.
//
// Version ordinals: v < T0 is the L0 table at position v (bit v of the Version
// probe's mask), v >= T0 the rows' ordinal g = v - T0 (lset_lists_plan.hpp);
// V = T0 + G.
#pragma once

#include <stdint.h>

#include <vector>

#include "fset_lists_plan.hpp"
#include "lset_lists_plan.hpp"

namespace lsmb {

constexpr uint32_t kVlStarts = 65;  // launch_fset_lists' starts: 64 slots and the total

// Bytes of one mask row: the narrowest of 1, 2, 4, 8 whose bits cover the T0
// L0 tables, as a filter-set lists probe chooses them.
inline uint32_t lset_vlists_row_bytes(uint32_t T0) { return T0 <= 8 ? 1 : T0 <= 16 ? 2 : T0 <= 32 ? 4 : 8; }

// The low T0 bits: the L0 positions as launch_fset_lists' live slots.
inline uint64_t lset_vlists_live(uint32_t T0) { return T0 >= 64 ? ~0ull : (1ull << T0) - 1; }

// The workspace of one Version lists probe of n keys over T0 L0 tables and R
// rows of G tables in all.
//   rows    the regions of lset_lists_plan(n, R, G), at their own offsets from
//           the start of the workspace; absent (rows.work_bytes == 0) when
//           R * G == 0
//   mask    n rows of rb bytes: the fused probe's L0 answers
//   tiles   fset_lists_tile_bytes(n, live): the compaction's per-tile counts
//   starts  u64[kVlStarts]: the L0 lists' starts; [64] = the L0 entries E0,
//           the base of the rows' lists
// the last three absent when T0 == 0: the plan is then the rows' alone.
struct LsetVlistsPlan {
    uint64_t n = 0, G = 0, V = 0;
    uint32_t T0 = 0, R = 0, rb = 1;
    uint64_t live = 0;
    LsetListsPlan rows;
    enum { kMask, kTiles, kStarts, kRegions };
    LsetListsRegion reg[kRegions];
    uint64_t entries = 0;     // T0 * n + R * n: the most list entries there can be
    uint64_t work_bytes = 0;  // 0: no workspace (n == 0 or V == 0)
};

inline LsetVlistsPlan lset_vlists_plan(uint64_t n, uint32_t T0, uint32_t R, uint64_t G) {
    LsetVlistsPlan p;
    p.n = n;
    p.G = G;
    p.V = (uint64_t)T0 + G;
    p.T0 = T0;
    p.R = R;
    p.rb = lset_vlists_row_bytes(T0);
    p.live = lset_vlists_live(T0);
    p.rows = lset_lists_plan(n, R, G);
    if (n == 0 || p.V == 0) return p;
    p.entries = (uint64_t)T0 * n + p.rows.pairs;
    uint64_t at = p.rows.work_bytes;  // a multiple of kLlAlign
    if (T0) {
        const uint64_t want[LsetVlistsPlan::kRegions] = {n * p.rb, fset_lists_tile_bytes(n, p.live),
                                                         (uint64_t)kVlStarts * 8};
        for (int i = 0; i < LsetVlistsPlan::kRegions; i++) {
            p.reg[i].off = at;
            p.reg[i].bytes = want[i];
            at += (want[i] + kLlAlign - 1) / kLlAlign * kLlAlign;
        }
    }
    p.work_bytes = at;
    return p;
}

// The transform the kernels compute after the fused ordinal probe.  mask[i]
// bit j (j < T0) = L0 table j answers key i; ord as lset_lists_ref takes it
// (ordinals below G, or kLlNone).  starts gets T0 + G + 1 entries, index every
// entry: the L0 lists by position, each ascending, then the rows' lists
// behind them.
inline void lset_vlists_ref(const uint64_t* mask, uint32_t T0, const uint32_t* ord, uint32_t R, uint64_t n,
                            uint64_t stride, uint64_t G, std::vector<uint64_t>* starts, std::vector<uint32_t>* index) {
    starts->assign((uint64_t)T0 + G + 1, 0);
    index->clear();
    for (uint32_t j = 0; j < T0; j++) {
        (*starts)[j] = index->size();
        for (uint64_t i = 0; i < n; i++)
            if ((mask[i] >> j) & 1) index->push_back((uint32_t)i);
    }
    const uint64_t e0 = index->size();
    std::vector<uint64_t> rs;
    std::vector<uint32_t> ri;
    lset_lists_ref(ord, R, n, stride, G, &rs, &ri);
    for (uint64_t g = 0; g <= G; g++) (*starts)[T0 + g] = e0 + rs[g];
    index->insert(index->end(), ri.begin(), ri.end());
}

}  // namespace lsmb

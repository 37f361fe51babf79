// lset_lists_plan.hpp — the host side of a level set's lists probe
// (lsmb_lset_probe_lists*, kernels in lset_lists.hip), free of HIP so that
// tests/cpp/lset_lists_plan_test.cpp can drive it on a CPU: the radix pass
// count, the tile geometry, the one statement of the workspace layout (the
// allocators size by it, the launcher validates and carves by it) and a plain
// C++ statement of the whole transform (lset_lists_ref).  Internal.
#pragma once

#include <stdint.h>

#include <vector>

namespace lsmb {

// Tile geometry of the split kernels: one workgroup of kLlBlock lanes per tile
// of kLlTile consecutive elements; wave w takes the tile's chunks
// [w * kLlChunks, (w + 1) * kLlChunks), chunk c = elements [64c, 64c + 64).
constexpr uint32_t kLlBlock = 256;
constexpr uint32_t kLlWaves = kLlBlock / 64;
constexpr uint32_t kLlChunks = 8;
constexpr uint32_t kLlTile = kLlBlock * kLlChunks;  // 2048
constexpr uint32_t kLlRadixBits = 8;
constexpr uint32_t kLlDigits = 1u << kLlRadixBits;
constexpr uint64_t kLlAlign = 256;                   // every workspace region starts on it
constexpr uint32_t kLlNone = 0xFFFFFFFFu;            // kLsetNone: "no table of this row"

// LSD passes that order the ordinals 0 .. G-1: ceil(bits(G-1) / 8), at least
// one (the first pass is also the compaction of the hits).
inline uint32_t lset_lists_passes(uint64_t G) {
    uint32_t bits = 0;
    for (uint64_t v = G ? G - 1 : 0; v; v >>= 1) bits++;
    const uint32_t p = (bits + kLlRadixBits - 1) / kLlRadixBits;
    return p ? p : 1;
}

// The workspace of one lists probe of n keys over R rows and G tables.
//   meta    kLlDigits digit totals of the running pass, then E (the hits), u64
//   counts  u64[kLlDigits][ntiles]: per digit and tile the tile's count, then
//           (scanned in place) the first output position of that digit and tile
//   ans     u32[R][row_stride]: the ordinal probe's answers, every row padded
//           to whole tiles so that a tile lies in one row; from the second
//           pass on the region is the pairs' second key buffer
//   key_a   u32[R * n]: ordinals of the hits (first key buffer)
//   val_a, val_b  u32[R * n] each: the key indices that travel with the
//           ordinals; absent when one pass sorts (it writes d_index itself)
struct LsetListsRegion {
    uint64_t off = 0, bytes = 0;
};
struct LsetListsPlan {
    uint64_t n = 0, G = 0;
    uint32_t R = 0, passes = 0;
    uint64_t tiles_per_row = 0;  // ceil(n / kLlTile)
    uint64_t row_stride = 0;     // tiles_per_row * kLlTile
    uint64_t ntiles = 0;         // R * tiles_per_row: the grid of every split kernel
    uint64_t pairs = 0;          // R * n: the most hits there can be
    enum { kMeta, kCounts, kAns, kKeyA, kValA, kValB, kRegions };
    LsetListsRegion reg[kRegions];
    uint64_t work_bytes = 0;     // 0: no workspace (n == 0, R == 0 or G == 0)
};

inline LsetListsPlan lset_lists_plan(uint64_t n, uint32_t R, uint64_t G) {
    LsetListsPlan p;
    p.n = n;
    p.R = R;
    p.G = G;
    p.passes = lset_lists_passes(G);
    if (n == 0 || R == 0 || G == 0) return p;
    p.tiles_per_row = (n + kLlTile - 1) / kLlTile;
    p.row_stride = p.tiles_per_row * kLlTile;
    p.ntiles = (uint64_t)R * p.tiles_per_row;
    p.pairs = (uint64_t)R * n;
    const uint64_t want[LsetListsPlan::kRegions] = {
        (uint64_t)(kLlDigits + 1) * 8,
        (uint64_t)kLlDigits * p.ntiles * 8,
        (uint64_t)R * p.row_stride * 4,
        p.pairs * 4,
        p.passes > 1 ? p.pairs * 4 : 0,
        p.passes > 1 ? p.pairs * 4 : 0,
    };
    uint64_t at = 0;
    for (int i = 0; i < LsetListsPlan::kRegions; i++) {
        p.reg[i].off = at;
        p.reg[i].bytes = want[i];
        at += (want[i] + kLlAlign - 1) / kLlAlign * kLlAlign;
    }
    p.work_bytes = at;
    return p;
}

// The transform the kernels compute after the ordinal probe.  ord[r * stride +
// i] = the ordinal (< G) of the table of row r that answers key i, or kLlNone.
// starts gets G + 1 entries, index every hit: index[starts[g] .. starts[g+1])
// = the ascending i with ord[.][i] == g (an ordinal belongs to one row, and
// the rows are walked in order, keys ascending within each: a stable counting
// sort by ordinal).
inline void lset_lists_ref(const uint32_t* ord, uint32_t R, uint64_t n, uint64_t stride, uint64_t G,
                           std::vector<uint64_t>* starts, std::vector<uint32_t>* index) {
    starts->assign(G + 1, 0);
    for (uint32_t r = 0; r < R; r++)
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t g = ord[(uint64_t)r * stride + i];
            if (g != kLlNone) (*starts)[(uint64_t)g + 1]++;
        }
    for (uint64_t g = 0; g < G; g++) (*starts)[g + 1] += (*starts)[g];
    index->assign((*starts)[G], 0);
    std::vector<uint64_t> at(starts->begin(), starts->end() - 1);
    for (uint32_t r = 0; r < R; r++)
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t g = ord[(uint64_t)r * stride + i];
            if (g != kLlNone) (*index)[at[g]++] = (uint32_t)i;
        }
}

// The same lists by the kernels' own route: lset_lists_passes(G) stable
// 8-bit LSD passes over the hits taken in (row, key) order.  Equal to
// lset_lists_ref whenever the pass count covers every bit of G - 1.
inline void lset_lists_radix_ref(const uint32_t* ord, uint32_t R, uint64_t n, uint64_t stride, uint64_t G,
                                 std::vector<uint64_t>* starts, std::vector<uint32_t>* index) {
    std::vector<uint32_t> key, val;
    for (uint32_t r = 0; r < R; r++)
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t g = ord[(uint64_t)r * stride + i];
            if (g != kLlNone) key.push_back(g), val.push_back((uint32_t)i);
        }
    const uint32_t passes = lset_lists_passes(G);
    std::vector<uint32_t> k2(key.size()), v2(val.size());
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = p * kLlRadixBits;
        uint64_t at[kLlDigits + 1] = {0};
        for (uint32_t g : key) at[((g >> shift) & (kLlDigits - 1)) + 1]++;
        for (uint32_t d = 0; d < kLlDigits; d++) at[d + 1] += at[d];
        for (size_t e = 0; e < key.size(); e++) {
            const uint64_t q = at[(key[e] >> shift) & (kLlDigits - 1)]++;
            k2[q] = key[e];
            v2[q] = val[e];
        }
        key.swap(k2);
        val.swap(v2);
    }
    // bounds: starts[g] = the first position whose ordinal is >= g
    starts->assign(G + 1, 0);
    const uint64_t E = key.size();
    for (uint64_t q = 0; q <= E; q++) {
        const uint64_t lo = q ? (uint64_t)key[q - 1] + 1 : 0, hi = q < E ? key[q] : G;
        for (uint64_t g = lo; g <= hi && g <= G; g++) (*starts)[g] = q;
    }
    *index = val;
}

}  // namespace lsmb

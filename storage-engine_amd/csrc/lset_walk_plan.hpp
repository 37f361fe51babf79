// lset_walk_plan.hpp — the host side of a level set's walk probe
// (lsmb_lset_probe_walk*, kernel and launchers in lset_walk_first.hip), free
// of HIP so that tests/cpp/lset_walk_plan_test.cpp can drive it on a CPU: the
// walk steps of DB::get's order (src/db/mod.rs:243-267, src/db/snapshot.rs:
// 40-69) and what each consults, the L0 positions a resume point still allows,
// the workspace of the lists form and a plain C++ statement of the per-key
// answer and the lists (lset_walk_ref).  The mapping functions are constexpr:
// the kernel calls the very same ones.  Internal.
//
// Walk steps of a set with T0 L0 tables and R rows: step w < T0 consults the
// L0 table at position T0-1-w (step 0 = the newest arrival,
// version.level(0).iter().rev()), step w = T0 + r row r; W = T0 + R steps.
// Version ordinals as lset_vlists_plan.hpp: v < T0 the L0 position v, v >= T0
// the rows' ordinal v - T0.
#pragma once

#include <stdint.h>

#include <vector>

#include "lset_lists_plan.hpp"

namespace lsmb {

constexpr uint32_t kWalkNone = kLlNone;  // kLsetNone: "no candidate", and a resume point that retires the key

constexpr uint32_t lset_walk_steps(uint32_t T0, uint32_t R) { return T0 + R; }

// Step w < T0 -> the L0 position it consults; position p < T0 -> its step.
constexpr uint32_t lset_walk_l0_pos(uint32_t T0, uint32_t w) { return T0 - 1 - w; }
constexpr uint32_t lset_walk_l0_step(uint32_t T0, uint32_t p) { return T0 - 1 - p; }

// The first row a walk resumed at step `from` (< W) still consults, and row
// r's step.
constexpr uint32_t lset_walk_first_row(uint32_t T0, uint32_t from) { return from > T0 ? from - T0 : 0; }
constexpr uint32_t lset_walk_row_step(uint32_t T0, uint32_t r) { return T0 + r; }

// The L0 positions a walk resumed at `from` may still consult: bits
// 0 .. T0-1-from, none when from >= T0.  T0 <= 64; T0 - from == 64 is every
// bit (a shift by 64 is undefined).
constexpr uint64_t lset_walk_allowed(uint32_t T0, uint32_t from) {
    return from >= T0 ? 0ull : (T0 - from >= 64 ? ~0ull : (1ull << (T0 - from)) - 1);
}

// The workspace of the lists form over n keys and V = T0 + G Version ordinals:
// one answer row of ordinals, split by the rows' own passes
// (launch_lset_lists_split with a null base).
inline LsetListsPlan lset_walk_lists_plan(uint64_t n, uint64_t V) { return lset_lists_plan(n, 1, V); }

// The per-key answer.  mask[i] bit j (j < T0) = L0 table j answers key i (the
// Version probe's mask); ord[r * stride + i] = the rows' ordinal of the table
// of row r that answers key i, or kWalkNone (a row emptied by derive never
// answers).  from == nullptr is all zero.  step[i] = the smallest w >= from[i]
// with a candidate, ordv[i] its Version ordinal, else kWalkNone both.
inline void lset_walk_ref(const uint64_t* mask, uint32_t T0, const uint32_t* ord, uint32_t R, uint64_t n,
                          uint64_t stride, const uint32_t* from, std::vector<uint32_t>* step,
                          std::vector<uint32_t>* ordv) {
    step->assign(n, kWalkNone);
    ordv->assign(n, kWalkNone);
    const uint32_t W = lset_walk_steps(T0, R);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t f = from ? from[i] : 0;
        if (f >= W) continue;
        const uint64_t m = (T0 ? mask[i] : 0) & lset_walk_allowed(T0, f);
        if (m) {
            const uint32_t p = 63 - (uint32_t)__builtin_clzll(m);  // the newest of them
            (*step)[i] = lset_walk_l0_step(T0, p);
            (*ordv)[i] = p;
            continue;
        }
        for (uint32_t r = lset_walk_first_row(T0, f); r < R; r++) {
            const uint32_t g = ord[(uint64_t)r * stride + i];
            if (g == kWalkNone) continue;
            (*step)[i] = lset_walk_row_step(T0, r);
            (*ordv)[i] = T0 + g;
            break;
        }
    }
}

// The lists of that answer over the V Version ordinals: starts gets V + 1
// entries, index one per key with a candidate; each list ascending.
inline void lset_walk_lists_ref(const std::vector<uint32_t>& ordv, uint64_t V, std::vector<uint64_t>* starts,
                                std::vector<uint32_t>* index) {
    lset_lists_ref(ordv.data(), 1, ordv.size(), ordv.size(), V, starts, index);
}

}  // namespace lsmb

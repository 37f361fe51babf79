// plan_test.cpp — the host build planner (csrc/build_plan.hip) against its
// recorded table, tests/golden/plan_table.json: strategy, partition / tiled
// plan and workspace-bounded chunk size over a grid of (num_bits, k, n, CUs).
// No HIP call: runs without a GPU (tests/test_capi_host.py compiles it with
// build_plan.hip and runs it with the LSMB_* plan knobs unset).
//
//   plan_test <plan_table.json>   recompute every row, compare, check the
//                                 plan's invariants; exit 1 on any difference
//   plan_test --dump <commit>     print the table (one record per line)
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../storage-engine_amd/csrc/kernels.hpp"

using namespace lsmb;

static const uint32_t kBits[] = {64,         kLdsFilterMaxWords32 * 32, 1310784,    1u << 25,   (1u << 25) + 64,
                                 (1u << 26) - 64, 1u << 26,             68883501,   956715292,  1000000000,
                                 1u << 30,   (1u << 30) + 1,            1u << 31,   3000000000u, 0xFFFFFFFFu};
static const uint32_t kK[] = {1, 5, 7, 8, 9, 16, 17, 32, 33};
static const uint64_t kN[] = {1, 1000, 4096, 1000000, 100000000, 125000000, 1000000000};
static const int kCus[] = {256, 64};
static const uint64_t kMiB16 = 16ull << 20, kGiB8 = 8ull << 30;

// "p" = PartitionPlan, "t" = TiledPlan, in the field order of kernels.hpp.
static const char* kHeaderFields =
    "\"p\": [\"slice_log2\", \"nbins\", \"grid\", \"cap_segs\", \"bins_per_sweep\", \"ring\", \"sweeps\", "
    "\"keys_per_lane\", \"region_bytes\", \"counts_bytes\"], "
    "\"t\": [\"nslices\", \"chunks\", \"stride32\", \"scratch_bytes\"], "
    "\"c16\": \"partition_chunk_keys at 16 MiB\", \"c8g\": \"partition_chunk_keys at 8 GiB\"";

static std::string row(uint32_t nb, uint32_t k, uint64_t n, int cus) {
    char b[512];
    const BuildStrategy s = pick_build_strategy(nb, k, n);
    int at = snprintf(b, sizeof b, "{\"nb\": %u, \"k\": %u, \"n\": %llu, \"cus\": %d, \"s\": \"%s\"", nb, k,
                      (unsigned long long)n, cus, strategy_name(s));
    if (s == BuildStrategy::Partition) {
        const PartitionPlan p = plan_partition(nb, k, n, cus);
        at += snprintf(b + at, sizeof b - at, ", \"p\": [%u, %u, %u, %u, %u, %u, %u, %u, %llu, %llu]", p.slice_log2,
                       p.nbins, p.grid, p.cap_segs, p.bins_per_sweep, p.ring, p.sweeps, p.keys_per_lane,
                       (unsigned long long)p.region_bytes, (unsigned long long)p.counts_bytes);
    } else if (s == BuildStrategy::Tiled) {
        const TiledPlan t = plan_tiled(nb, n, cus);
        at += snprintf(b + at, sizeof b - at, ", \"t\": [%u, %u, %llu, %llu]", t.nslices, t.chunks,
                       (unsigned long long)t.stride32, (unsigned long long)t.scratch_bytes);
    }
    snprintf(b + at, sizeof b - at, ", \"c16\": %llu, \"c8g\": %llu}",
             (unsigned long long)partition_chunk_keys(nb, k, kMiB16, cus),
             (unsigned long long)partition_chunk_keys(nb, k, kGiB8, cus));
    return b;
}

static std::vector<std::string> table() {
    std::vector<std::string> rows;
    for (uint32_t nb : kBits)
        for (uint32_t k : kK)
            for (uint64_t n : kN)
                for (int cus : kCus) rows.push_back(row(nb, k, n, cus));
    return rows;
}

// The plan's layout is a function of (num_bits, k) alone (lsmb_build_sweeps /
// lsmb_sweep_words answer without a device), and fits pass A's static LDS.
static int check_invariants() {
    int bad = 0;
    for (uint32_t nb : kBits)
        for (uint32_t k : kK) {
            const PartitionPlan a = plan_partition(nb, k, kN[0], kCus[0]);
            for (uint64_t n : kN)
                for (int cus : kCus) {
                    const PartitionPlan p = plan_partition(nb, k, n, cus);
                    if (p.slice_log2 != a.slice_log2 || p.nbins != a.nbins || p.bins_per_sweep != a.bins_per_sweep ||
                        p.ring != a.ring || p.sweeps != a.sweeps || p.keys_per_lane != a.keys_per_lane) {
                        printf("layout of (%u, %u) differs at n = %llu, %d CUs\n", nb, k, (unsigned long long)n, cus);
                        bad++;
                    }
                }
            if ((size_t)(a.bins_per_sweep + 1) * (4 * a.ring + kBinExtraBytes) + kBinJobBytes > kLdsBytes ||
                a.ring % 8 != 0) {
                printf("layout of (%u, %u) does not fit LDS: %u bins per sweep, ring %u\n", nb, k, a.bins_per_sweep,
                       a.ring);
                bad++;
            }
        }
    const uint64_t c = partition_chunk_keys(68883501, 7, kMiB16, 256);
    if (c != 367616) {
        printf("partition_chunk_keys(68883501, 7, 16 MiB, 256) = %llu, want 367616\n", (unsigned long long)c);
        bad++;
    }
    return bad;
}

int main(int argc, char** argv) {
    const std::vector<std::string> rows = table();
    if (argc == 3 && !strcmp(argv[1], "--dump")) {
        printf("{\"commit\": \"%s\", %s,\n\"rows\": [\n", argv[2], kHeaderFields);
        for (size_t i = 0; i < rows.size(); i++) printf("%s%s\n", rows[i].c_str(), i + 1 < rows.size() ? "," : "");
        printf("]}\n");
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: plan_test <plan_table.json> | plan_test --dump <commit>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    size_t i = 0;
    int bad = 0;
    while (std::getline(in, line)) {
        if (line.compare(0, 6, "{\"nb\":") != 0) continue;
        if (!line.empty() && line.back() == ',') line.pop_back();
        if (i >= rows.size() || line != rows[i]) {
            if (bad++ < 10) printf("row %zu\n  recorded %s\n  computed %s\n", i, line.c_str(), i < rows.size() ? rows[i].c_str() : "-");
        }
        i++;
    }
    if (i != rows.size()) {
        printf("%zu recorded rows, %zu computed\n", i, rows.size());
        bad++;
    }
    bad += check_invariants();
    printf("%zu rows, %d bad\n", rows.size(), bad);
    return bad ? 1 : 0;
}

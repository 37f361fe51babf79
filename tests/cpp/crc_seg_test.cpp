// crc_seg_test.cpp — the arithmetic of the CRC-32 kernels
// (storage-engine_amd/csrc/crc_seg.hpp): crc_seg_ref, the serial statement of
// k_crc32_seg's pieces and shuffle tree, against a bit-at-a-time CRC-32 written
// here, at every length of a small bloom block and at the piece, wave and
// 128 KiB boundaries; the piece geometry; the combine against the CRC of the
// concatenation.  No HIP: a stand-alone host program
// (tests/test_lset_versions.py builds it with -fsanitize=address,undefined and
// runs it, then holds the printed combine lines against lsmb_crc32_combine and
// zlib).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../storage-engine_amd/csrc/crc_seg.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

// CRC-32 by definition, one bit at a time (no tables shared with the header).
static uint32_t crc_bitwise(const uint8_t* p, uint64_t n, uint32_t crc = 0) {
    uint32_t c = ~crc;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int j = 0; j < 8; j++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
    }
    return ~c;
}

// n bytes at a 16-byte-aligned address + shift.
struct Buf {
    void* raw = nullptr;
    uint8_t* p = nullptr;
    Buf(uint64_t n, uint32_t shift, uint64_t seed) {
        raw = aligned_alloc(16, ((n + shift + 15) / 16 + 1) * 16);
        p = (uint8_t*)raw + shift;
        uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
        for (uint64_t i = 0; i < n; i++) {
            s ^= s << 13, s ^= s >> 7, s ^= s << 17;
            p[i] = (uint8_t)(s >> 32);
        }
    }
    ~Buf() { free(raw); }
};

static void test_known_values() {
    const uint8_t* s = (const uint8_t*)"123456789";
    CHECK(crc_bitwise(s, 9) == 0xCBF43926u);  // the CRC-32 check value
    CHECK(crc_piece(crc_tables().t, s, 9, false) == 0xCBF43926u);
    CHECK(crc_seg_ref(s, 9) == 0xCBF43926u);
    CHECK(crc_seg_ref(s, 0) == 0);
    CHECK(x8nmodp(0) == 0x80000000u);  // x^0
    CHECK(x8nmodp(1) == 0x00800000u);  // x^8
    CHECK(multmodp(0x80000000u, 0x12345678u) == 0x12345678u);
}

static void test_geometry() {
    CHECK(crc_seg_geom(0).P == 16 && crc_seg_geom(0).nfull == 0 && crc_seg_geom(0).tail == 0);
    CHECK(crc_seg_geom(1).P == 16 && crc_seg_geom(1).nfull == 0 && crc_seg_geom(1).tail == 1);
    CHECK(crc_seg_geom(1024).P == 16 && crc_seg_geom(1024).nfull == 64 && crc_seg_geom(1024).tail == 0);
    CHECK(crc_seg_geom(1025).P == 32 && crc_seg_geom(1025).nfull == 32 && crc_seg_geom(1025).tail == 1);
    CHECK(crc_seg_geom(1200).P == 32 && crc_seg_geom(1200).nfull == 37 && crc_seg_geom(1200).tail == 16);
    CHECK(crc_seg_geom(kCrcSegWaveMax).P == 2048 && crc_seg_geom(kCrcSegWaveMax).nfull == 64);
    CHECK(crc_seg_geom(kCrcSegWaveMax + 1).P == 2064);
    for (uint64_t len : {0ull, 1ull, 15ull, 16ull, 17ull, 1023ull, 1024ull, 1025ull, 1208ull, 131072ull, 262152ull}) {
        const CrcSegGeom g = crc_seg_geom(len);
        CHECK(g.P % 16 == 0 && g.P * kCrcSegLanes >= len && (g.P == 16 || (g.P - 16) * kCrcSegLanes < len));
        CHECK(g.nfull <= kCrcSegLanes && g.tail < g.P && g.nfull * g.P + g.tail == len);
        // the lanes' pieces tile the segment: empty lanes, the tail's lane, then the whole pieces in order
        uint64_t sum = 0, next = 0;
        uint32_t tails = 0;
        for (uint32_t l = 0; l < kCrcSegLanes; l++) {
            uint64_t off;
            const uint64_t n = crc_seg_lane(g, l, &off);
            sum += n;
            if (crc_seg_is_tail_lane(g, l)) {
                tails++;
                CHECK(n == g.tail && off == g.nfull * g.P && l + 1 + g.nfull == kCrcSegLanes);
            } else if (n) {
                CHECK(n == g.P && off == next && off % 16 == 0 && l + g.nfull >= kCrcSegLanes);
                next += g.P;
            }
        }
        CHECK(sum == len && next == g.nfull * g.P && tails == (g.tail ? 1u : 0u));
    }
}

static void check_len(uint64_t len, uint32_t shift) {
    Buf b(len, shift, len * 31 + shift);
    const uint32_t want = crc_bitwise(b.p, len);
    const uint32_t got = crc_seg_ref(b.p, len);
    if (got != want) {
        fprintf(stderr, "FAILED len %llu shift %u: crc_seg_ref %08x, bitwise %08x\n", (unsigned long long)len, shift, got,
                want);
        g_fail++;
    }
}

static void test_lengths() {
    for (uint64_t nw = 0; nw <= 600; nw++) check_len(8 * nw, 0);  // every small bloom block
    // one piece per lane of 16 B, the 128 KiB wave range, and past it
    for (uint64_t nw : {4095ull, 4096ull, 4097ull, 16383ull, 16384ull, 16385ull, 32769ull}) check_len(8 * nw, 0);
    // tails that are no multiple of 8, around one and several pieces per lane
    for (uint64_t base : {0ull, 16ull, 1008ull, 1024ull, 4800ull, 131056ull})
        for (uint64_t tail = 1; tail <= 15; tail++) check_len(base + tail, 0);
    // a segment that is not 16-byte aligned takes the byte loop
    for (uint32_t shift : {1u, 4u, 8u, 15u})
        for (uint64_t len : {0ull, 7ull, 64ull, 1208ull, 5000ull}) check_len(len, shift);
}

static void test_combine() {
    const uint64_t la[] = {0, 1, 12, 12, 12, 1000, 4096, 70000};
    const uint64_t lb[] = {0, 1, 0, 8, 1208, 12, 131072, 3};
    for (int i = 0; i < 8; i++) {
        Buf b(la[i] + lb[i], 0, 77 + i);
        const uint32_t ca = crc_bitwise(b.p, la[i]), cb = crc_bitwise(b.p + la[i], lb[i]);
        const uint32_t whole = crc_bitwise(b.p, la[i] + lb[i]);
        CHECK(crc_combine(ca, cb, lb[i]) == whole);
        CHECK(crc_bitwise(b.p + la[i], lb[i], ca) == whole);
        // for the caller: the same triples through the library's lsmb_crc32_combine
        printf("combine %08x %08x %llu %08x\n", ca, cb, (unsigned long long)lb[i], whole);
    }
    // x^(8n) against repeated multiplication by x^8
    uint32_t p = 0x80000000u;
    for (uint64_t n = 0; n < 300; n++) {
        CHECK(x8nmodp(n) == p);
        p = multmodp(p, 0x00800000u);
    }
    CHECK(multmodp(x8nmodp(123456), x8nmodp(654321)) == x8nmodp(123456 + 654321));
}

int main() {
    test_known_values();
    test_geometry();
    test_lengths();
    test_combine();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all passed\n");
    return 0;
}
